// deflate_kernels.hip -- gzip on the GPU for the lossy pipelines' rank arrays
// (SURVEY §8(f) row 3).  Reference: GZIPTransformer.forward / backward
// (kc_pipeline.py:128-156, skc_pipeline.py:201-230, stc_pipeline.py:185-215):
// gzip.compress(float32 ranks bytes), decoded by gzip.decompress.  Any valid
// gzip stream decodes to the same bytes, so the wire stays compatible.
//
// Two parts:
//  * TLZ (namespace gz::tlz): the encoder of the rank arrays -- an
//    optimal-parse token LZ over the whole 32 KiB window, one dynamic-Huffman
//    block per 512 KiB member, with per-segment entry points in an RFC 1952
//    extra subfield -- and its lane-parallel two-kernel inflate;
//  * a generic member inflate (k_inflate_members: stored, fixed and dynamic
//    blocks, any deflate data of a member-indexed stream), used for streams
//    that are not TLZ (e.g. BGZF-style members written by zlib) and as the
//    fallback of the TLZ inflate.
//
// This file is the host driver and the C API (include/ofl_codec.h); one
// translation unit with what it includes:
//   gz_format.h   host + device: status bits, the index record, the TLZ
//                 member format's constants and header offsets
//   gz_device.h   device: tables, bit / code / CRC helpers, Huffman, k_gzip_scan
//   gz_inflate.h  device: the generic inflate
//   tlz_encode.h  device: the TLZ encoder (the format is described there)
//   tlz_decode.h  device: k_tlz_ops, k_tlz_resolve, the pack kernels
//   gz_members.h  host, no HIP: the parser of a stream's member headers, the
//                 CRC matrices, the workspace layouts
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <thread>
#include <zlib.h>

#include "ofl_codec.h"
#include "ofl_util.h"

#include "gz_format.h"
#include "gz_device.h"
#include "gz_inflate.h"
#include "tlz_encode.h"
#include "tlz_decode.h"
#include "gz_members.h"

namespace {
thread_local std::string g_gzerr;
int gzfail(int code, const std::string& m) { g_gzerr = m; return code; }
#define GZHIP(x)                                                                                        \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) return gzfail(OFL_EHIP, std::string(#x " failed: ") + hipGetErrorString(e_)); \
    } while (0)

// Optional per-kernel timing (bench.py's KC line): while enabled, every
// gzip / inflate launch is bracketed by HIP events on its stream; collect
// synchronises them and sums the time per kernel name.
std::mutex g_prof_m;
bool g_prof_on = false;
struct ProfRec { const char* name; hipEvent_t a, b; };
std::vector<ProfRec> g_prof_pending;
thread_local hipEvent_t g_prof_a = nullptr;
void gzprof_begin(hipStream_t st) {
    if (!g_prof_on) return;
    if (hipEventCreate(&g_prof_a) != hipSuccess || hipEventRecord(g_prof_a, st) != hipSuccess) g_prof_a = nullptr;
}
void gzprof_end(hipStream_t st, const char* name) {
    if (!g_prof_on || !g_prof_a) return;
    hipEvent_t b;
    if (hipEventCreate(&b) != hipSuccess) return;
    if (hipEventRecord(b, st) != hipSuccess) { (void)hipEventDestroy(b); return; }
    std::lock_guard<std::mutex> g(g_prof_m);
    g_prof_pending.push_back({name, g_prof_a, b});
    g_prof_a = nullptr;
}

// the device's stream for the gzip's DMA (created once per device): the
// DMA of batch k overlaps the encode of batch k + 1 only from another HW
// queue.  HIP hands normal-priority streams the GPU_MAX_HW_QUEUES queues in
// turn, so a normal stream made late in a busy process can share the
// caller's queue (the DMA then waits behind the next encode: gzip phase
// 11.9 -> 14.9 ms per GiB); a high-priority stream comes from HIP's separate
// high-priority queues (profiles/r05_kc_hw_queues_ab.txt)
hipError_t gz_side_stream(hipStream_t* out) {
    static std::mutex m;
    static hipStream_t side[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> g(m);
    if (!side[dev]) {
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&side[dev], hipStreamNonBlocking, greatest);
    }
    *out = side[dev];
    return e;
}

// a small pinned host block per thread (the gzip's per-batch offsets, read by
// the host while the next batch encodes); allocated once, kept
hipError_t gz_pinned_info(uint64_t** out) {
    thread_local uint64_t* p = nullptr;
    if (!p) {
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), 64, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
    }
    *out = p;
    return hipSuccess;
}

// what every entry point that launches a kernel needs, once per device (the
// __constant__ tables and the kernel attributes are per-device state): the
// CRC advance matrices and the two dynamic-LDS sizes above 64 KiB
// (defined below the TLZ inflate's launches: kernel templates are emitted in
// the order of their first use, and this keeps the code object's order that
// of the launches)
hipError_t gz_device_setup();

// the inflate kernels' status word -> the call's result.  tlz: the TLZ
// decoder's verdict, where anything but a range error only means "not TLZ"
int inflate_status(int h, bool tlz) {
    if (h & gz::kInfRange) return gzfail(OFL_ESPACE, "inflate: a member's output falls outside out");
    if (h && tlz) return gzfail(OFL_EFORMAT, "inflate: the TLZ decoder refused a member (the generic inflate decides)");
    if (h & gz::kInfCorrupt) return gzfail(OFL_EINVAL, "inflate: corrupt deflate data");
    if (h & gz::kInfSize) return gzfail(OFL_EINVAL, "inflate: member size differs from its ISIZE");
    if (h & gz::kInfCrc) return gzfail(OFL_EINVAL, "inflate: CRC-32 mismatch");
    return OFL_OK;
}
// the status word read back on st (synchronises st)
int read_status(const void* ws, hipStream_t st, int* h) {
    *h = 0;
    GZHIP(hipMemcpyAsync(h, static_cast<const char*>(ws) + gz::inflate_ws(0).status, sizeof(int), hipMemcpyDeviceToHost, st));
    GZHIP(hipStreamSynchronize(st));
    return OFL_OK;
}

// a stream's members, parsed on up to 16 threads in pieces of 4 MiB or more
int parse_stream(const uint8_t* src, size_t n, std::vector<gz::GzMember>& mem, size_t& total) {
    const char* msg = "";
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int rc = gz::parse_members(src, n, std::min(hw, 16u), (size_t)4 << 20, mem, total, &msg);
    return rc ? gzfail(rc, msg) : OFL_OK;
}

// the TLZ decoder's two kernels over members [first, first + count)
struct LutDev { const float* tab; const int64_t* start; const int64_t* end; int32_t n; };
int inflate_tlz_enqueue(const uint8_t* src, const int64_t* index, int64_t first, int64_t count, uint8_t* out,
                        size_t out_cap, void* ws, size_t ws_bytes, void* stream, bool reset, const LutDev* lut = nullptr) {
    if (first < 0 || count < 0 || (count && (!src || !index || !out))) return gzfail(OFL_EINVAL, "inflate: null argument");
    const gz::InflateWs W = gz::inflate_ws(first + count);
    if (!ws || ws_bytes < W.end) return gzfail(OFL_ESPACE, "inflate: workspace too small");
    GZHIP(gz_device_setup());
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* status = reinterpret_cast<int*>(static_cast<char*>(ws) + W.status);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + W.counts) + first * gz::tlz::kMemSeg;
    if (reset) GZHIP(hipMemsetAsync(status, 0, sizeof(int), st));
    if (count == 0) return OFL_OK;
    static const int dbg = getenv("OFL_TLZ_DEC_STATS") != nullptr;
    gz::tlz::DecArgs a{src, index + gz::kIdxWords * first, count, out, (uint64_t)out_cap, cnt, status,
                       lut ? lut->tab : nullptr, lut ? lut->start : nullptr, lut ? lut->end : nullptr, lut ? lut->n : 0,
                       dbg};
    gzprof_begin(st);
    hipLaunchKernelGGL(gz::tlz::k_tlz_ops, dim3((unsigned)count), dim3(64), sizeof(gz::tlz::DecSmem), st, a);
    gzprof_end(st, "tlz::k_tlz_ops");
    gzprof_begin(st);
    if (lut)
        hipLaunchKernelGGL(gz::tlz::k_tlz_resolve<true>, dim3((unsigned)count), dim3(gz::tlz::kRNT), sizeof(gz::tlz::ResSmem),
                           st, a);
    else
        hipLaunchKernelGGL(gz::tlz::k_tlz_resolve<false>, dim3((unsigned)count), dim3(gz::tlz::kRNT),
                           sizeof(gz::tlz::ResSmem), st, a);
    gzprof_end(st, "tlz::k_tlz_resolve");
    GZHIP(hipGetLastError());
    return OFL_OK;
}

hipError_t gz_device_setup() {
    return ofl_util::per_device_once([] {
        uint32_t m[32][32];
        gz::crc_matrices(m);
        hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(gz::c_adv), m, sizeof(m));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)gz::tlz::k_tlz_encode, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sizeof(gz::tlz::EncSmem));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)gz::k_inflate_members<65536, false, false>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(gz::InfSmem<65536, false>));
        return e;
    });
}

// what the two paths of gzip_ranks_impl share: the call's arguments and the
// workspace's regions (gz::GzRanksWs) as pointers
struct GzRanksJob {
    const float* x;
    int64_t n;
    const ofl_label_rec* lab;
    int lab_n;
    uint8_t* out;
    size_t out_cap;
    uint8_t* host_dst;
    int nthreads;
    hipStream_t st;
    gz::TlzLayout L;
    uint8_t* slots[2];
    uint32_t* ops;
    uint32_t* sizes[2];
    uint64_t* off[2];
    uint64_t* running;
    int* bad;
    uint8_t* stage[2];
    int aligned;      // x is 16-byte aligned
    uint64_t* d_ph;   // diagnostics (OFL_GZ_PHASES), else null
    // members [c0, c0 + nb) into slots[b], sizes[b]
    void encode(int64_t c0, int nb, int b) const {
        gz::tlz::EncArgs a{x, n, c0, slots[b], ops, sizes[b], bad, (uint32_t)L.slot, (uint32_t)L.ops_stride, aligned,
                           c0 == 0 ? d_ph : nullptr, lab, lab ? lab_n : 0};
        gzprof_begin(st);
        hipLaunchKernelGGL(gz::tlz::k_tlz_encode, dim3(nb), dim3(gz::tlz::kNT), sizeof(gz::tlz::EncSmem), st, a);
        gzprof_end(st, "tlz::k_tlz_encode");
    }
};

// the pinned path's events.  Every exit of the path (the GZHIP error returns
// included) waits for the work queued on both streams -- scan, pack and D2H
// read ws and write out -- before the caller may reuse those buffers, then
// frees the events
struct PinnedEvents {
    static constexpr int kTailPieces = 4;
    hipStream_t st, sd;
    bool drained = false;
    hipEvent_t pack[2] = {}, scan[2] = {}, dma[2] = {}, tail[kTailPieces] = {};
    PinnedEvents(hipStream_t st_, hipStream_t sd_) : st(st_), sd(sd_) {}
    PinnedEvents(const PinnedEvents&) = delete;
    PinnedEvents& operator=(const PinnedEvents&) = delete;
    template <typename F>
    void each(F f) {
        for (hipEvent_t& e : pack) f(e);
        for (hipEvent_t& e : scan) f(e);
        for (hipEvent_t& e : dma) f(e);
        for (hipEvent_t& e : tail) f(e);
    }
    hipError_t create() {
        hipError_t r = hipSuccess;
        each([&](hipEvent_t& e) { if (r == hipSuccess) r = hipEventCreateWithFlags(&e, hipEventDisableTiming); });
        return r;
    }
    ~PinnedEvents() {
        if (!drained) { (void)hipStreamSynchronize(sd); (void)hipStreamSynchronize(st); }
        each([](hipEvent_t& e) { if (e) (void)hipEventDestroy(e); });
    }
};

// diagnostics: OFL_GZ_FILL_TRACE=1 prints the host's wait / copy times per call
struct FillTrace {
    bool on;
    double t_call;
    char text[512];
    int n = 0;
    static double now_us() {
        return (double)std::chrono::duration_cast<std::chrono::microseconds>(
                   std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    FillTrace() {
        static const bool env = getenv("OFL_GZ_FILL_TRACE") != nullptr;
        on = env;
        t_call = on ? now_us() : 0.0;
        text[0] = 0;
    }
    double begin() const { return on ? now_us() : 0.0; }
    void span(const char* what, double t0) {  // what@start+duration
        if (on && n < 400) n += snprintf(text + n, sizeof(text) - n, " %s@%.0f+%.0f", what, t0 - t_call, now_us() - t0);
    }
    void mark(const char* what) {
        if (on && n < 400) n += snprintf(text + n, sizeof(text) - n, " %s@%.0f", what, now_us() - t_call);
    }
    void print() const {
        if (on) fprintf(stderr, "gzip fill (us):%s end@%.0f\n", text, now_us() - t_call);
    }
};

// out is mapped pinned host memory (dout: its device address).
// Batch k on the caller's stream: encode, scan, pack -- the scan and the pack
// (tens of us with the whole chip free) run before the next batch's encode, so
// nothing of a batch waits for CUs behind the next one (on a side stream they
// queued behind its 80 KiB-LDS blocks for up to 2.3 ms).  The pack goes to
// device staging and the stream crosses PCIe by DMA (a kernel's stores into
// mapped host memory are one small PCIe write each: 8.5 GB/s); a batch larger
// than its staging (> 1 byte per value: nearly incompressible ranks) is packed
// straight into the mapped output.  Only the DMA of batch k (its size is
// known once the host has read the scan) goes on the side stream, beside the
// encode of batch k + 1, and the host copies batch k into host_dst meanwhile.
// The last batch crosses PCIe in pieces, each copied as it lands.
int gzip_ranks_pinned(const GzRanksJob& J, uint8_t* dout, size_t* total) {
    const gz::TlzLayout& L = J.L;
    const hipStream_t st = J.st;
    constexpr int kTailPieces = PinnedEvents::kTailPieces;
    hipStream_t sd = nullptr;
    GZHIP(gz_side_stream(&sd));
    uint64_t* hinfo = nullptr;
    GZHIP(gz_pinned_info(&hinfo));  // [2][2]: a batch's first offset and end
    const int64_t nbatch = (L.members + L.batch - 1) / L.batch;
    PinnedEvents ev(st, sd);
    GZHIP(ev.create());
    GZHIP(hipMemsetAsync(J.running, 0, sizeof(uint64_t), st));
    uint64_t copied = 0;  // host_dst holds out[0, copied)
    FillTrace trace;
    auto host_copy = [&](uint64_t upto) {  // out[copied, upto) -> host_dst (its DMA complete)
        if (J.host_dst && upto > copied) {
            const double t0 = trace.begin();
            void* d = J.host_dst + copied;
            const void* src = J.out + copied;
            const int64_t nb = (int64_t)(upto - copied);
            ofl_host_copy_many(1, &d, &src, &nb, J.nthreads);
            copied = upto;
            trace.span("copy", t0);
        }
    };
    auto wait_ev = [&](hipEvent_t e, const char* what) -> hipError_t {
        const double t0 = trace.begin();
        const hipError_t r = hipEventSynchronize(e);
        trace.span(what, t0);
        return r;
    };
    uint64_t bfirst[2] = {0, 0}, bend[2] = {0, 0};
    // batch k's DMA (after its scan result is on the host); pieces > 1 for the last batch
    auto issue_dma = [&](int64_t k, int pieces) -> int {
        const int b = (int)(k & 1);
        GZHIP(wait_ev(ev.scan[b], "scan"));
        const uint64_t first = hinfo[2 * b], end = hinfo[2 * b + 1];
        bfirst[b] = first == ~0ull ? 0 : first;
        bend[b] = first == ~0ull ? 0 : end;
        GZHIP(hipStreamWaitEvent(sd, ev.pack[b], 0));
        if (first != ~0ull && end > first && end - first <= L.stage) {
            const uint64_t n = end - first;
            for (int p = 0; p < pieces; ++p) {
                const uint64_t lo = n * (uint64_t)p / (uint64_t)pieces, hi = n * (uint64_t)(p + 1) / (uint64_t)pieces;
                gzprof_begin(sd);
                if (hi > lo) GZHIP(hipMemcpyAsync(J.out + first + lo, J.stage[b] + lo, hi - lo, hipMemcpyDeviceToHost, sd));
                gzprof_end(sd, "gzip D2H (DMA)");
                if (pieces > 1) GZHIP(hipEventRecord(ev.tail[p], sd));
            }
        }
        GZHIP(hipEventRecord(ev.dma[b], sd));
        return OFL_OK;
    };
    for (int64_t k = 0; k < nbatch; ++k) {
        const int64_t c0 = k * L.batch;
        const int b = (int)(k & 1);
        const int nb = (int)std::min<int64_t>(L.batch, L.members - c0);
        J.encode(c0, nb, b);
        gzprof_begin(st);
        hipLaunchKernelGGL(gz::k_gzip_scan, dim3(1), dim3(1024), 0, st, J.sizes[b], nb, J.off[b], J.running,
                           (uint64_t)J.out_cap, J.bad);
        gzprof_end(st, "k_gzip_scan");
        GZHIP(hipMemcpyAsync(hinfo + 2 * b, J.off[b], 8, hipMemcpyDeviceToHost, st));
        GZHIP(hipMemcpyAsync(hinfo + 2 * b + 1, J.off[b] + nb, 8, hipMemcpyDeviceToHost, st));
        GZHIP(hipEventRecord(ev.scan[b], st));
        if (k >= 2) GZHIP(hipStreamWaitEvent(st, ev.dma[b], 0));  // stage[b]'s previous DMA has read it
        gzprof_begin(st);
        hipLaunchKernelGGL(gz::k_gzip_pack_batch, dim3(nb), dim3(256), 0, st, J.slots[b], (uint64_t)L.slot, J.sizes[b],
                           J.off[b], nb, J.stage[b], (uint64_t)L.stage, dout);
        gzprof_end(st, "k_gzip_pack");
        GZHIP(hipEventRecord(ev.pack[b], st));
        if (hipGetLastError() != hipSuccess) return gzfail(OFL_EHIP, "gzip ranks: kernel launch failed");
        if (k >= 1) {  // batch k - 1: its DMA and its bytes to host_dst, beside this batch's encode
            if (int rc = issue_dma(k - 1, 1)) return rc;
            if (J.host_dst) {
                GZHIP(wait_ev(ev.dma[(k - 1) & 1], "dma"));
                host_copy(bend[(k - 1) & 1]);
            }
        }
    }
    if (int rc = issue_dma(nbatch - 1, J.host_dst ? kTailPieces : 1)) return rc;
    {  // the last batch, piece by piece as its DMA lands
        const int b = (int)((nbatch - 1) & 1);
        const uint64_t first = bfirst[b], end = bend[b];
        if (J.host_dst && end > first && end - first <= L.stage) {
            const uint64_t n = end - first;
            for (int p = 0; p < kTailPieces; ++p) {
                GZHIP(wait_ev(ev.tail[p], "tail"));
                host_copy(first + n * (uint64_t)(p + 1) / (uint64_t)kTailPieces);
            }
        }
    }
    GZHIP(hipEventRecord(ev.pack[0], sd));
    GZHIP(hipStreamWaitEvent(st, ev.pack[0], 0));  // the caller's stream sees every copy
    uint64_t tot = 0;
    int badh = 0;
    GZHIP(hipMemcpyAsync(&tot, J.running, 8, hipMemcpyDeviceToHost, st));
    GZHIP(hipMemcpyAsync(&badh, J.bad, sizeof(int), hipMemcpyDeviceToHost, st));
    GZHIP(hipStreamSynchronize(st));
    ev.drained = true;  // st waited for everything sd ran
    if (badh & 1) return gzfail(OFL_EINVAL, "gzip ranks: values must be float32 integers 0..31");
    if (badh & 2) return gzfail(OFL_ESPACE, "gzip ranks: output buffer too small");
    *total = tot;
    trace.mark("sync");
    host_copy(tot);
    trace.print();
    return OFL_OK;
}

// out is pageable: one synchronous D2H per batch, through the second slot buffer
int gzip_ranks_pageable(const GzRanksJob& J, size_t* total_out) {
    const gz::TlzLayout& L = J.L;
    const hipStream_t st = J.st;
    uint8_t* packed = J.slots[1];
    size_t total = 0;
    for (int64_t c0 = 0; c0 < L.members; c0 += L.batch) {
        const int nb = (int)std::min<int64_t>(L.batch, L.members - c0);
        J.encode(c0, nb, 0);
        hipLaunchKernelGGL(gz::k_gzip_scan, dim3(1), dim3(1024), 0, st, J.sizes[0], nb, J.off[0], (uint64_t*)nullptr,
                           ~0ull, J.bad);
        hipLaunchKernelGGL(gz::k_gzip_pack, dim3(nb), dim3(256), 0, st, J.slots[0], (uint64_t)L.slot, J.sizes[0],
                           J.off[0], packed);
        GZHIP(hipGetLastError());
        uint64_t tot = 0;
        int badh = 0;
        GZHIP(hipMemcpyAsync(&tot, J.off[0] + nb, 8, hipMemcpyDeviceToHost, st));
        GZHIP(hipMemcpyAsync(&badh, J.bad, sizeof(int), hipMemcpyDeviceToHost, st));
        GZHIP(hipStreamSynchronize(st));
        if (badh) return gzfail(OFL_EINVAL, "gzip ranks: values must be float32 integers 0..31");
        if (total + tot > J.out_cap) return gzfail(OFL_ESPACE, "gzip ranks: output buffer too small");
        GZHIP(hipMemcpyAsync(J.out + total, packed, tot, hipMemcpyDeviceToHost, st));
        GZHIP(hipStreamSynchronize(st));
        if (J.host_dst) memcpy(J.host_dst + total, J.out + total, tot);
        total += tot;
    }
    *total_out = total;
    return OFL_OK;
}

// host_dst (optional): a pageable buffer of host_cap bytes that receives the
// stream too, each batch copied on nthreads host threads while the next batch
// encodes (ofl_gzip_ranks_to)
// lab (optional, device): x holds values, labelled through lab_n records as they load
int gzip_ranks_impl(const float* x, int64_t n, const ofl_label_rec* lab, int lab_n, uint8_t* out, size_t out_cap,
                    uint8_t* host_dst, size_t host_cap, int nthreads, size_t* out_len, void* ws, size_t ws_bytes,
                    void* stream) {
    if (n < 1 || !x || !out || !out_len) return gzfail(OFL_EINVAL, "gzip ranks: empty input");
    if (lab && lab_n < 1) return gzfail(OFL_EINVAL, "gzip label: no label records");
    if (host_dst && host_cap < out_cap) return gzfail(OFL_EINVAL, "gzip ranks: host_cap < out_cap");
    char* w = static_cast<char*>(ws);
    const gz::GzRanksWs W = gz::gzip_ranks_ws(n, reinterpret_cast<uintptr_t>(w));
    if (!ws || ws_bytes < W.end) return gzfail(OFL_ESPACE, "gzip ranks: workspace too small");
    GZHIP(gz_device_setup());
    GzRanksJob J{x, n, lab, lab_n, out, out_cap, host_dst, nthreads, static_cast<hipStream_t>(stream), W.L};
    for (int i = 0; i < 2; ++i) {
        J.slots[i] = reinterpret_cast<uint8_t*>(w + W.slots[i]);
        J.sizes[i] = reinterpret_cast<uint32_t*>(w + W.sizes[i]);
        J.off[i] = reinterpret_cast<uint64_t*>(w + W.off[i]);
        J.stage[i] = reinterpret_cast<uint8_t*>(w + W.stage[i]);
    }
    J.ops = reinterpret_cast<uint32_t*>(w + W.ops);
    J.running = reinterpret_cast<uint64_t*>(w + W.running);
    J.bad = reinterpret_cast<int*>(w + W.bad);
    GZHIP(hipMemsetAsync(J.bad, 0, sizeof(int), J.st));
    // out is mapped pinned host memory (e.g. torch pin_memory): the pack
    // kernel's output goes straight towards it and the batches run back to
    // back with one synchronisation at the end; otherwise one D2H per batch
    uint8_t* dout = nullptr;
    {
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, out) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer)
            dout = static_cast<uint8_t*>(pa.devicePointer);
        (void)hipGetLastError();  // a pageable pointer is not an error here
    }
    J.aligned = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
    // diagnostics: OFL_GZ_PHASES=1 prints block 0's phase times (10 ns ticks,
    // summed over its segments; [11] = Jacobi rounds) of the first launch
    static const bool phases = getenv("OFL_GZ_PHASES") != nullptr;
    J.d_ph = nullptr;
    if (phases) {
        GZHIP(hipMalloc(&J.d_ph, 8 * gz::tlz::kEncPhases));
        GZHIP(hipMemsetAsync(J.d_ph, 0, 8 * gz::tlz::kEncPhases, J.st));
    }
    size_t total = 0;
    if (int rc = dout ? gzip_ranks_pinned(J, dout, &total) : gzip_ranks_pageable(J, &total)) return rc;
    if (J.d_ph) {
        uint64_t h[gz::tlz::kEncPhases];
        GZHIP(hipMemcpy(h, J.d_ph, sizeof(h), hipMemcpyDeviceToHost));
        GZHIP(hipFree(J.d_ph));
        fprintf(stderr, "tlz phases (block 0, 10 ns ticks): load %llu chains[B1 %llu rest %llu] frontier %llu dp %llu parse %llu "
                "ops[walk %llu scan %llu rec %llu] model %llu code %llu bits %llu | jacobi rounds %llu\n",
                (unsigned long long)h[1], (unsigned long long)h[12], (unsigned long long)h[2], (unsigned long long)h[3],
                (unsigned long long)h[4], (unsigned long long)h[5], (unsigned long long)h[13], (unsigned long long)h[14],
                (unsigned long long)h[6], (unsigned long long)h[7], (unsigned long long)h[8], (unsigned long long)h[9],
                (unsigned long long)h[11]);
    }
    *out_len = total;
    return OFL_OK;
}
}  // namespace

extern "C" {

const char* ofl_gzip_last_error(void) { return g_gzerr.c_str(); }

size_t ofl_gzip_ranks_workspace_bytes(int64_t n) { return gz::gzip_ranks_ws(n, 0).end; }

size_t ofl_gzip_ranks_bound(int64_t n) { return gz::gzip_ranks_bound(n); }

int ofl_gzip_ranks(const float* x, int64_t n, uint8_t* out, size_t out_cap, size_t* out_len, void* ws,
                   size_t ws_bytes, void* stream) {
    return gzip_ranks_impl(x, n, nullptr, 0, out, out_cap, nullptr, 0, 1, out_len, ws, ws_bytes, stream);
}

int ofl_gzip_ranks_to(const float* x, int64_t n, uint8_t* out, size_t out_cap, uint8_t* host_dst, size_t host_cap,
                      int nthreads, size_t* out_len, void* ws, size_t ws_bytes, void* stream) {
    if (!host_dst) return gzfail(OFL_EINVAL, "gzip ranks to: null host_dst");
    return gzip_ranks_impl(x, n, nullptr, 0, out, out_cap, host_dst, host_cap, std::max(1, nthreads), out_len, ws,
                           ws_bytes, stream);
}

int ofl_gzip_label_to(const float* x, int64_t n, const ofl_label_rec* label_tab, int ntensors, uint8_t* out,
                      size_t out_cap, uint8_t* host_dst, size_t host_cap, int nthreads, size_t* out_len, void* ws,
                      size_t ws_bytes, void* stream) {
    if (!label_tab) return gzfail(OFL_EINVAL, "gzip label: null label_tab");
    return gzip_ranks_impl(x, n, label_tab, ntensors, out, out_cap, host_dst, host_cap, std::max(1, nthreads), out_len,
                           ws, ws_bytes, stream);
}

// Host inflate of a member-indexed gzip stream (every member carries the
// 'BC' extra field that k_gzip_members writes): the members are found from
// their headers alone and inflated on nthreads host threads straight into
// dst (each member's ISIZE gives its output offset).  Streams without the
// field (e.g. gzip.compress output) return OFL_EFORMAT so the caller can use
// gzip.decompress instead; dst == nullptr only measures.
int ofl_gunzip_members(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, int nthreads) {
    if (!src || !out_len) return gzfail(OFL_EINVAL, "gunzip: null argument");
    std::vector<gz::GzMember> mem;
    size_t total = 0;
    if (int rc = parse_stream(src, n, mem, total)) return rc;
    using M = gz::GzMember;
    *out_len = total;
    if (!dst) return OFL_OK;
    if (total > cap) return gzfail(OFL_ESPACE, "gunzip: output buffer too small");
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(nthreads, 1), mem.size()));
    std::vector<int> bad(nt, 0);
    auto work = [&](int t) {
        z_stream z;
        memset(&z, 0, sizeof(z));
        if (inflateInit2(&z, -15) != Z_OK) { bad[t] = 1; return; }
        const size_t m0 = mem.size() * t / nt, m1 = mem.size() * (t + 1) / nt;
        for (size_t i = m0; i < m1 && !bad[t]; ++i) {
            const M& m = mem[i];
            inflateReset(&z);
            z.next_in = const_cast<Bytef*>(src + m.in);
            z.avail_in = (uInt)m.in_len;
            z.next_out = dst + m.out;
            z.avail_out = m.isize;
            // every byte of the deflate data used, as the device inflate requires:
            // a byte between the data and the trailer is not a gzip member
            if (inflate(&z, Z_FINISH) != Z_STREAM_END || z.avail_in != 0 || z.total_out != m.isize ||
                crc32(0L, dst + m.out, m.isize) != m.crc)
                bad[t] = 1;
        }
        inflateEnd(&z);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
    for (int b : bad)
        if (b) return gzfail(OFL_EINVAL, "gunzip: corrupt member (inflate, size or CRC-32 mismatch)");
    return OFL_OK;
}

int ofl_gzip_member_index(const uint8_t* src, size_t n, int64_t* index, int64_t cap_members, int64_t* nmembers,
                          size_t* out_len, uint32_t* max_isize, int* all_tlz) {
    if (!src || !nmembers || !out_len) return gzfail(OFL_EINVAL, "member index: null argument");
    std::vector<gz::GzMember> mem;
    size_t total = 0;
    if (int rc = parse_stream(src, n, mem, total)) return rc;
    *nmembers = (int64_t)mem.size();
    *out_len = total;
    uint32_t mx = 0;
    bool tl = !mem.empty();
    for (const gz::GzMember& m : mem) { mx = std::max(mx, m.isize); tl = tl && m.tlz; }
    if (max_isize) *max_isize = mx;
    if (all_tlz) *all_tlz = tl ? 1 : 0;
    if (!index) return OFL_OK;
    if (cap_members < (int64_t)mem.size()) return gzfail(OFL_ESPACE, "member index: index array too small");
    for (size_t i = 0; i < mem.size(); ++i) {
        const gz::GzMember& m = mem[i];
        gz::idx_pack(index + gz::kIdxWords * i, m.in, m.in_len, m.tlz, m.out, m.isize, m.crc);
    }
    return OFL_OK;
}

size_t ofl_inflate_tlz_workspace_bytes(int64_t nmembers) { return gz::inflate_ws(nmembers).end; }

int ofl_inflate_tlz_async(const uint8_t* src, const int64_t* index, int64_t first, int64_t count, uint8_t* out,
                          size_t out_cap, void* ws, size_t ws_bytes, void* stream) {
    return inflate_tlz_enqueue(src, index, first, count, out, out_cap, ws, ws_bytes, stream, first == 0);
}

int ofl_inflate_tlz_launch(const uint8_t* src, const int64_t* index, int64_t first, int64_t count, uint8_t* out,
                           size_t out_cap, void* ws, size_t ws_bytes, void* stream) {
    return inflate_tlz_enqueue(src, index, first, count, out, out_cap, ws, ws_bytes, stream, false);
}

int ofl_inflate_tlz_launch_lut(const uint8_t* src, const int64_t* index, int64_t first, int64_t count, uint8_t* out,
                               size_t out_cap, void* ws, size_t ws_bytes, const float* lut_tab, const int64_t* lut_start,
                               const int64_t* lut_end, int32_t lut_n, void* stream) {
    if (lut_n < 1 || !lut_tab || !lut_start || !lut_end) return gzfail(OFL_EINVAL, "inflate lut: empty table");
    const LutDev lut{lut_tab, lut_start, lut_end, lut_n};
    return inflate_tlz_enqueue(src, index, first, count, out, out_cap, ws, ws_bytes, stream, false, &lut);
}

int ofl_inflate_tlz_check(int64_t nmembers, void* ws, size_t ws_bytes, void* stream) {
    if (nmembers == 0) return OFL_OK;
    if (!ws || ws_bytes < ofl_inflate_tlz_workspace_bytes(nmembers)) return gzfail(OFL_ESPACE, "inflate: workspace too small");
    int h = 0;
    if (int rc = read_status(ws, static_cast<hipStream_t>(stream), &h)) return rc;
    return inflate_status(h, true);
}

int ofl_inflate_tlz_wait(const uint8_t* src, const int64_t* index, int64_t nmembers, uint8_t* out, size_t out_cap,
                         void* ws, size_t ws_bytes, void* stream) {
    if (nmembers == 0) return OFL_OK;
    if (!ws || ws_bytes < ofl_inflate_tlz_workspace_bytes(nmembers)) return gzfail(OFL_ESPACE, "inflate: workspace too small");
    int h = 0;
    if (int rc = read_status(ws, static_cast<hipStream_t>(stream), &h)) return rc;
    const int rc = inflate_status(h, true);
    if (rc != OFL_EFORMAT) return rc;
    // not what the TLZ decoder expects: the generic inflate decides (any
    // valid deflate data decodes there; corrupt data fails there too)
    uint32_t mx = 0;
    std::vector<int64_t> hidx(gz::kIdxWords * (size_t)nmembers);
    GZHIP(hipMemcpy(hidx.data(), index, sizeof(int64_t) * hidx.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nmembers; ++i) mx = std::max(mx, GZ_IDX_ISIZE(hidx[gz::kIdxWords * i + gz::kIdxSize]));
    return ofl_inflate_members(src, index, nmembers, mx, out, out_cap, ws, ws_bytes, stream);
}

int ofl_inflate_tlz(const uint8_t* src, const int64_t* index, int64_t nmembers, uint8_t* out, size_t out_cap, void* ws,
                    size_t ws_bytes, void* stream) {
    if (nmembers < 0 || (nmembers && (!src || !index || !out))) return gzfail(OFL_EINVAL, "inflate: null argument");
    if (int rc = ofl_inflate_tlz_async(src, index, 0, nmembers, out, out_cap, ws, ws_bytes, stream)) return rc;
    return ofl_inflate_tlz_wait(src, index, nmembers, out, out_cap, ws, ws_bytes, stream);
}

int ofl_gzip_profile(int enable) {
    std::lock_guard<std::mutex> g(g_prof_m);
    for (ProfRec& r : g_prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof_pending.clear();
    g_prof_on = enable != 0;
    return OFL_OK;
}

int ofl_gzip_profile_collect(char* names, size_t names_cap, double* ms, int64_t* launches, int max_kernels, int* nkernels) {
    if (!names || !ms || !launches || !nkernels) return gzfail(OFL_EINVAL, "profile: null argument");
    std::lock_guard<std::mutex> g(g_prof_m);
    std::vector<std::string> nm;
    std::vector<double> t;
    std::vector<int64_t> k;
    for (ProfRec& r : g_prof_pending) {
        float e = 0.f;
        GZHIP(hipEventSynchronize(r.b));
        GZHIP(hipEventElapsedTime(&e, r.a, r.b));
        size_t i = 0;
        while (i < nm.size() && nm[i] != r.name) ++i;
        if (i == nm.size()) { nm.push_back(r.name); t.push_back(0.0); k.push_back(0); }
        t[i] += e;
        k[i] += 1;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof_pending.clear();
    std::string all;
    const int nk = (int)std::min<size_t>(nm.size(), (size_t)max_kernels);
    for (int i = 0; i < nk; ++i) {
        all += nm[i];
        all += '\n';
        ms[i] = t[i];
        launches[i] = k[i];
    }
    if (all.size() + 1 > names_cap) return gzfail(OFL_ESPACE, "profile: names buffer too small");
    std::memcpy(names, all.c_str(), all.size() + 1);
    *nkernels = nk;
    return OFL_OK;
}

int ofl_inflate_members(const uint8_t* src, const int64_t* index, int64_t nmembers, uint32_t max_isize, uint8_t* out,
                        size_t out_cap, void* ws, size_t ws_bytes, void* stream) {
    if (nmembers < 0 || (nmembers && (!src || !index || !out))) return gzfail(OFL_EINVAL, "inflate: null argument");
    const gz::InflateWs W = gz::inflate_ws(nmembers);
    if (!ws || ws_bytes < W.counts) return gzfail(OFL_ESPACE, "inflate: workspace too small (256 bytes)");
    static const bool window = [] { const char* v = getenv("OFL_GZ_INFLATE"); return v && v[0] == 'w'; }();
    if (window && max_isize > 65536u)
        return gzfail(OFL_EFORMAT, "inflate: members above 64 KiB of output need the ring decoder");
    if (nmembers == 0) return OFL_OK;
    GZHIP(gz_device_setup());
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* status = reinterpret_cast<int*>(static_cast<char*>(ws) + W.status);
    GZHIP(hipMemsetAsync(status, 0, sizeof(int), st));
    gz::InfArgs a{src, index, nmembers, out, (uint64_t)out_cap, status};
    // OFL_GZ_INFLATE=window: whole-member LDS windows (A/B); default: a
    // 1 KiB LDS ring per member, output stored as produced
    // 1 KiB ring: with the table-driven decode the kernel is scalar-unit
    // bound and more members per CU pay (1 / 2 KiB / 512 B: 12.4 / 13.1 /
    // 12.8 ms for the 1 GiB set; before, 1, 2 and 4 KiB measured the same)
    // the (length, distance) pair table: opt-in (OFL_GZ_PAIR=1).  Measured
    // slower on the 1 GiB rank set: 16.8 vs 12.4 ms per inflate launch
    // (profiles/r03_kc_pair_ab.txt): the 4 KiB table per member cuts the
    // members resident per CU from 26 to 15, and the decode is bound by the
    // scalar issue of many members, not by one member's steps
    static const bool pair = [] { const char* v = getenv("OFL_GZ_PAIR"); return v && v[0] == '1'; }();
    gzprof_begin(st);
    if (!window && pair)
        hipLaunchKernelGGL((gz::k_inflate_members<1024, true, true>), dim3((unsigned)nmembers), dim3(64),
                           sizeof(gz::InfSmem<1024, true>), st, a);
    else if (!window)
        hipLaunchKernelGGL((gz::k_inflate_members<1024, true, false>), dim3((unsigned)nmembers), dim3(64),
                           sizeof(gz::InfSmem<1024, false>), st, a);
    else if (max_isize <= 16384u)
        hipLaunchKernelGGL((gz::k_inflate_members<16384, false, false>), dim3((unsigned)nmembers), dim3(64),
                           sizeof(gz::InfSmem<16384, false>), st, a);
    else
        hipLaunchKernelGGL((gz::k_inflate_members<65536, false, false>), dim3((unsigned)nmembers), dim3(64),
                           sizeof(gz::InfSmem<65536, false>), st, a);
    gzprof_end(st, "k_inflate_members");
    GZHIP(hipGetLastError());
    int h = 0;
    if (int rc = read_status(ws, st, &h)) return rc;
    return inflate_status(h, false);
}

}  // extern "C"

