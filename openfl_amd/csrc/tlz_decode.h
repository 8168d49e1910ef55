// tlz_decode.h -- the TLZ decoder of the gzip codec (deflate_kernels.hip):
// k_tlz_ops and k_tlz_resolve (the format and the scheme: tlz_encode.h), and
// the kernels that pack the encoder's members into one stream.
#pragma once
#include "gz_inflate.h"
#include "tlz_encode.h"

namespace gz {
namespace tlz {

// ---- inflate --------------------------------------------------------------
constexpr int kDecLitBits = kLitMax, kDecDistBits = kDistMax;
using DecLit = InfCodeT<kDecLitBits, 288>;
using DecDist = InfCodeT<kDecDistBits, 32>;
struct DecSmem {
    DecLit lit;
    DecDist dist;
    uint8_t lens[320];
};
struct DecArgs {
    // device stream: readable, and already landed, 64 bytes past every
    // member's trailer (BitIn's look-ahead at the end bound; the pipelined
    // inflate launches a member only once the H2D piece holding its end plus
    // those 64 bytes has landed, lossy.gunzip_device / _INFLATE_LOOKAHEAD;
    // the last piece is followed by 128 bytes of padding)
    const uint8_t* src;
    const int64_t* idx;      // per member: an index record (gz_format.h)
    int64_t nmem;
    uint8_t* out;
    uint64_t out_cap;
    uint32_t* cnt;           // [nmem][kMemSeg] ops per segment
    int* status;
    // the fused LUT decode (k_tlz_resolve<true>): the values stored are
    // lut_tab[t][rank] for the element's tensor t (elements [lut_start[t],
    // lut_end[t]) of the stream's float32 output, sorted); elements between
    // tensors store the rank itself
    const float* lut_tab;
    const int64_t* lut_start;
    const int64_t* lut_end;
    int32_t lut_n;
    int32_t dbg;             // diagnostics (OFL_TLZ_DEC_STATS): timing printf of every 256th member
};

// bytes of the stream (any alignment) through a 128-bit block register pair
struct BitIn {
    const uint4* base;       // 16-byte aligned
    uint4 cur, nxt;
    int64_t blk;             // block index of cur
    int wi;                  // next word of cur
    uint64_t bb;
    int bc;
    DEVI uint32_t word(int k) const { return k == 0 ? cur.x : k == 1 ? cur.y : k == 2 ? cur.z : cur.w; }
    DEVI void start(const uint8_t* src, uint64_t bit) {  // src 16-byte aligned
        base = reinterpret_cast<const uint4*>(src);
        blk = (int64_t)(bit >> 7);
        cur = base[blk];
        nxt = base[blk + 1];
        wi = (int)((bit >> 5) & 3u);
        const int sk = (int)(bit & 31u);
        bb = (uint64_t)(word(wi) >> sk);
        bc = 32 - sk;
        adv();
        fill();
    }
    DEVI void adv() {
        if (++wi == 4) { cur = nxt; ++blk; nxt = base[blk + 1]; wi = 0; }
    }
    DEVI void fill() {  // >= 33 bits in bb
        while (bc <= 32) {
            bb |= (uint64_t)word(wi) << bc;
            bc += 32;
            adv();
        }
    }
    DEVI uint32_t peek() const { return (uint32_t)bb; }
    DEVI void drop(int n) { bb >>= n; bc -= n; }
    DEVI uint32_t get(int n) { const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1ull)); drop(n); return v; }
    DEVI uint64_t pos() const { return (uint64_t)(blk * 128 + wi * 32) - (uint64_t)bc; }
};

// K1: one wavefront per member; the block header on all lanes (wave-uniform),
// then lane s decodes segment s's symbols into op records written over that
// segment's own output bytes (kSeg values = 8 KiB >= 4 bytes per op).
__global__ __launch_bounds__(64) void k_tlz_ops(DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    DecSmem& S = *reinterpret_cast<DecSmem*>(smem_raw);
    const int lane = threadIdx.x;
    const int64_t m = blockIdx.x;
    if (m >= a.nmem) return;
    const int64_t* ix = a.idx + kIdxWords * m;
    const int64_t doff = ix[kIdxIn];
    const uint32_t in_len = GZ_IDX_IN_LEN(ix[kIdxLen]);
    const int64_t out_off = ix[kIdxOut];
    const uint32_t isize = GZ_IDX_ISIZE(ix[kIdxSize]);
    const uint8_t* data = a.src + doff;
    const uint32_t ntok = isize / 4u;
    const int nseg = (int)((ntok + kSeg - 1) >> kSegLog);
    int err = 0;
    if ((isize & 3u) || ntok == 0 || nseg > kMemSeg || (out_off & 3) || (uint64_t)out_off + isize > a.out_cap) err = kInfRange;
    // the 'OZ' subfield ends where the deflate data starts
    const uint8_t* oz = data - table_bytes(nseg) - kOzTable;
    if (!err) {
        if (oz[0] != 'O' || oz[1] != 'Z' || oz[kOzVersion] != kVersion || oz[kOzSegLog] != kSegLog ||
            rd16(oz + kOzNseg) != (uint32_t)nseg || rd32(oz + kOzValues) != ntok)
            err = kInfCorrupt;
    }
    if (err) {
        if (lane == 0) atomicOr(a.status, err);
        return;
    }
    auto seg_bit = [&](int s) -> uint32_t {
        const uint8_t* p = data - table_bytes(nseg) + table_bytes(s);
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    };
    const uint64_t dbit = 8ull * (uint64_t)doff;  // the data's first bit in the stream
    // the segment table is untrusted input: every entry must lie inside the
    // member's data and the entries must increase, or no lane may start a
    // decoder there (a bad entry would send BitIn far outside the stream)
    const uint64_t ebit = dbit + 8ull * (uint64_t)in_len;  // one past the data's last bit
    {
        const uint32_t sb = lane < nseg ? seg_bit(lane) : 0u;
        const uint32_t sp = lane > 0 && lane < nseg ? seg_bit(lane - 1) : 0u;
        const bool bad = lane < nseg && ((uint64_t)sb >= 8ull * (uint64_t)in_len || (lane > 0 && sb <= sp));
        if (__ballot(bad)) {
            if (lane == 0) atomicOr(a.status, kInfCorrupt);
            return;
        }
    }
    const uint64_t t_start = a.dbg ? wall_clock64() : 0;
    // ---- the block header, on every lane (wave-uniform) ----
    BitIn in;
    in.start(a.src, dbit);
    if (in.get(1) != 1u || in.get(2) != 2u) err = kInfCorrupt;  // BFINAL, dynamic
    int nlit = 0, ndist = 0;
    if (!err) {
        nlit = (int)in.get(5) + 257;
        ndist = (int)in.get(5) + 1;
        const int ncl = (int)in.get(4) + 4;
        if (nlit > 286 || ndist > 30) err = kInfCorrupt;
        for (int i = lane; i < 19; i += 64) S.lens[i] = 0;
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < ncl && !err; ++i) {
            in.fill();
            const uint32_t v = in.get(3);
            if (lane == 0) S.lens[c_clord[i]] = (uint8_t)v;
        }
        __builtin_amdgcn_wave_barrier();
        if (!err && !inf_build(S.lit, S.lens, 19, kAlphaPlain, kSetFull)) err = kInfCorrupt;
        const int total = nlit + ndist;
        int i = 0;
        while (!err && i < total) {
            if (in.pos() > ebit) { err = kInfCorrupt; break; }  // ran past the data (wave-uniform)
            in.fill();
            const uint32_t e = S.lit.fast[in.peek() & (uint32_t)(DecLit::kSize - 1)];
            const int l = (int)(e & 15u);
            if (!l || (e & 0x300u)) { err = kInfCorrupt; break; }
            in.drop(l);
            const int sy = (int)(e >> 16);
            if (sy < 16) {
                if (lane == 0) S.lens[i] = (uint8_t)sy;
                ++i;
                continue;
            }
            int rep, val = 0;
            if (sy == 16) {
                if (i == 0) { err = kInfCorrupt; break; }
                __builtin_amdgcn_wave_barrier();
                val = S.lens[i - 1];
                rep = 3 + (int)in.get(2);
            } else if (sy == 17) {
                rep = 3 + (int)in.get(3);
            } else {
                rep = 11 + (int)in.get(7);
            }
            if (i + rep > total) { err = kInfCorrupt; break; }
            __builtin_amdgcn_wave_barrier();
            for (int k = lane; k < rep; k += 64) S.lens[i + k] = (uint8_t)val;
            __builtin_amdgcn_wave_barrier();
            i += rep;
        }
        __builtin_amdgcn_wave_barrier();
        if (!err) {
            // every code must fit the first-level tables (the encoder limits them)
            bool longc = false;
            for (int k = lane; k < total; k += 64) longc |= S.lens[k] > (k < nlit ? kDecLitBits : kDecDistBits);
            if (__ballot(longc) || S.lens[256] == 0) err = kInfCorrupt;
        }
        if (!err) {
            const uint8_t dl = lane < ndist ? S.lens[nlit + lane] : 0;
            __builtin_amdgcn_wave_barrier();
            for (int k = nlit + lane; k < 288; k += 64) S.lens[k] = 0;
            __builtin_amdgcn_wave_barrier();
            if (lane < 32) S.lens[288 + lane] = lane < ndist ? dl : 0;
            __builtin_amdgcn_wave_barrier();
            if (!inf_build(S.lit, S.lens, nlit, kAlphaLit, kSetLone) || !inf_build(S.dist, S.lens + 288, ndist, kAlphaDist, kSetLone)) err = kInfCorrupt;
        }
        if (!err && in.pos() != dbit + seg_bit(0)) err = kInfCorrupt;  // the ops start where the table says
    }
    if (err) {
        if (lane == 0) atomicOr(a.status, err);
        return;
    }
    __builtin_amdgcn_wave_barrier();
    const uint64_t t_hdr = a.dbg ? wall_clock64() : 0;
    // ---- lane s: segment s ----
    const int s = lane;
    if (s < nseg) {
        const uint32_t T = min((uint32_t)kSeg, ntok - ((uint32_t)s << kSegLog));
        uint32_t* const opo = reinterpret_cast<uint32_t*>(a.out + out_off + ((int64_t)s << (kSegLog + 2)));
        in.start(a.src, dbit + seg_bit(s));
        uint32_t produced = 0, nops = 0;
        const uint32_t before = (uint32_t)s << kSegLog;  // values of the member before this segment
        // op records are collected four at a time and stored as one 16-byte
        // write: every lane writes its own segment's region, so a store
        // instruction is 64 scattered transactions, and one per record made
        // the stores the kernel's limit
        uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        const bool al16 = (reinterpret_cast<uintptr_t>(opo) & 15u) == 0;
        auto emit = [&](uint32_t rec) {
            const uint32_t k = nops & 3u;
            b0 = k == 0 ? rec : b0;
            b1 = k == 1 ? rec : b1;
            b2 = k == 2 ? rec : b2;
            b3 = k == 3 ? rec : b3;
            if (k == 3) {
                if (al16) {
                    reinterpret_cast<uint4*>(opo)[nops >> 2] = make_uint4(b0, b1, b2, b3);
                } else {  // a member whose output does not start 16-byte aligned
                    opo[nops - 3] = b0; opo[nops - 2] = b1; opo[nops - 1] = b2; opo[nops] = b3;
                }
            }
            ++nops;
        };
        // a corrupt segment must not decode on past its member: the lane
        // stops once its bit window's block passes the data's last block + 1
        // (reads stay within ~48 bytes past the data; the stream is padded
        // for that), checked on the block index instead of the bit position
        const int64_t blim = (int64_t)(ebit >> 7) + 1;
        while (produced < T) {
            if (in.blk > blim) { err = kInfCorrupt; break; }
            in.fill();
            uint32_t e = S.lit.fast[in.peek() & (uint32_t)(DecLit::kSize - 1)];
            int l = (int)(e & 15u);
            if (!l) { err = kInfCorrupt; break; }
            in.drop(l);
            uint32_t kind = (e >> 8) & 3u;
            if (kind == (uint32_t)kKindLit) {  // a value's 4 literal bytes
                uint32_t bytes = e >> 16;
                in.fill();
#pragma unroll
                for (int y = 1; y < 4; ++y) {
                    e = S.lit.fast[in.peek() & (uint32_t)(DecLit::kSize - 1)];
                    l = (int)(e & 15u);
                    if (!l || ((e >> 8) & 3u) != (uint32_t)kKindLit) { err = kInfCorrupt; break; }
                    in.drop(l);
                    bytes |= (e >> 16) << (8 * y);
                }
                if (err) break;
                const float f = __uint_as_float(bytes);
                const int id = (int)f;
                if (!(id >= 0 && id < 32 && __float_as_uint((float)id) == bytes)) { err = kInfCorrupt; break; }
                emit(0x80000000u | (uint32_t)id);
                produced += 1;
            } else if (kind == (uint32_t)kKindCopy) {
                const uint32_t len = (e >> 16) + in.get((int)((e >> 4) & 15u));
                in.fill();
                const uint32_t f = S.dist.fast[in.peek() & (uint32_t)(DecDist::kSize - 1)];
                const int l2 = (int)(f & 15u);
                in.drop(l2);  // (l2 == 0 or a wrong kind fails below, before anything is used)
                const uint32_t d = (f >> 16) + in.get((int)((f >> 4) & 15u));
                const uint32_t lt = len >> 2, dt = d >> 2;
                // every check at once: one branch out instead of one per test
                const bool bad = (l2 == 0) | (((f >> 8) & 3u) != (uint32_t)kKindCopy) | (((len | d) & 3u) != 0u) |
                                 (lt - (uint32_t)kMinL > (uint32_t)(kMaxL - kMinL)) | (produced + lt > T) |
                                 (dt > before + produced) | (dt > (uint32_t)kWin);
                if (bad) { err = kInfCorrupt; break; }
                emit(lt | (dt << 7));
                produced += lt;
            } else {
                err = kInfCorrupt;
                break;
            }
        }
        if (!err) {
            if (s + 1 < nseg) {
                if (in.pos() != dbit + seg_bit(s + 1)) err = kInfCorrupt;
            } else {  // end of block, then the data ends at the next byte boundary
                in.fill();
                const uint32_t e = S.lit.fast[in.peek() & (uint32_t)(DecLit::kSize - 1)];
                const int l = (int)(e & 15u);
                if (!l || ((e >> 8) & 3u) != (uint32_t)kKindEnd) err = kInfCorrupt;
                else {
                    in.drop(l);
                    if ((in.pos() - dbit + 7u) / 8u != in_len) err = kInfCorrupt;
                }
            }
        }
        {  // the last < 4 records
            const uint32_t k = nops & 3u, q = nops & ~3u;
            if (k > 0) opo[q] = b0;
            if (k > 1) opo[q + 1] = b1;
            if (k > 2) opo[q + 2] = b2;
        }
        a.cnt[m * kMemSeg + s] = nops;
        if (err) atomicOr(a.status, err);
        if (a.dbg && (m & 255) == 0) {
            uint32_t dt = (uint32_t)(wall_clock64() - t_hdr), no = nops;
            for (int o = 32; o > 0; o >>= 1) {
                dt = max(dt, (uint32_t)__shfl_xor((int)dt, o, 64));
                no = max(no, (uint32_t)__shfl_xor((int)no, o, 64));
            }
            if (lane == 0)
                printf("tlz_ops m=%lld hdr_ticks=%u lanes_max_ticks=%u lane0_ops=%u max_ops=%u\n", (long long)m,
                       (uint32_t)(t_hdr - t_start), dt, nops, no);
        }
    }
}

// K2: one block per member; per segment: op positions (block scan), each
// value's source (pointer jumping in LDS; sources before the segment are in
// the value ring), the values as float32, CRC-32 of the member, ISIZE.
constexpr int kRNT = 256, kRPer = kSeg / kRNT;     // resolve: threads per member block, values per thread
constexpr int kLutSlots = 4;                       // fused LUT: tensor tables per segment in LDS
// resolve's CRC advances: table i advances by 2^(5 + i) bytes for i < 7 (a
// thread's 32 bytes .. a wave's 2 KiB), table 7 by a segment's 8 KiB
static_assert(kSegLog == 11, "resolve's CRC tables assume 2048-value segments");
static_assert(kRPer * 32 == kRNT, "one thread per (value slot, id) entry of the resolve's CRC table");
DEVI int adv_k(int i) { return i < 7 ? 5 + i : 13; }
// the resolve's value ring: the window and one segment (LDS per block decides
// how many member blocks share a CU: 4 at < 40 KiB)
constexpr uint32_t kVRing = kWin + kSeg;
struct ResSmem {
    uint32_t adv[8][8][16];        // CRC advance by 2^adv_k(i) bytes, per input nibble (table form of c_adv)
    uint32_t cid[kRPer][32];       // raw CRC of a thread's 32 bytes with only value q = id (from 0)
    alignas(16) uint8_t v[kVRing];  // ids by member position mod kVRing
    uint32_t opr[kSeg];            // the segment's op records
    alignas(16) uint16_t e[kSeg];   // 0x8000 | id (resolved) or the distance to the source
    uint32_t cnt[kMemSeg];         // ops per segment (k_tlz_ops)
    uint32_t crct[1][256];
    uint32_t scan[kRNT / 64];
    uint32_t crc_w[kRNT / 64];
    uint32_t crc_raw;
    float lt[kLutSlots][32];       // fused LUT: the tables of kLutSlots tensors from the segment's first
    int64_t lsa[kLutSlots], lea[kLutSlots];  // their element ranges in the stream
    int32_t ls[kLutSlots], le[kLutSlots];    // the same relative to the segment start (clamped)
    int32_t lt0, ln;               // the first of those tensors, how many
};
// the tensor of element g (-1: none), by binary search over the sorted starts
DEVI int lut_find(const DecArgs& a, int64_t g) {
    int lo = 0, hi = a.lut_n - 1, t = -1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        if (a.lut_start[mid] <= g) { t = mid; lo = mid + 1; } else hi = mid - 1;
    }
    return t >= 0 && g < a.lut_end[t] ? t : -1;
}
template <bool LUT>
__global__ __launch_bounds__(kRNT) void k_tlz_resolve(DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    ResSmem& S = *reinterpret_cast<ResSmem*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t m = blockIdx.x;
    if (m >= a.nmem) return;
    if (*reinterpret_cast<volatile int*>(a.status)) return;  // K1 found corrupt data (block-uniform)
    const int64_t* ix = a.idx + kIdxWords * m;
    const int64_t out_off = ix[kIdxOut];
    const uint32_t isize = GZ_IDX_ISIZE(ix[kIdxSize]), want_crc = GZ_IDX_CRC(ix[kIdxSize]);
    const uint32_t ntok = isize / 4u;
    const int nseg = (int)((ntok + kSeg - 1) >> kSegLog);
    {
        uint32_t r = (uint32_t)tid;
        for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1;
        S.crct[0][tid] = r;
    }
    if (tid == 0) S.crc_raw = 0;
    // the advances as nibble tables: adv(x) = XOR_j T[j][nibble j of x], 8
    // independent LDS reads instead of a 32-step loop over the matrix columns
    for (int e = tid; e < 8 * 8 * 16; e += kRNT) {
        const int i = e >> 7, j = (e >> 4) & 7, v = e & 15;
        uint32_t r = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) r ^= ((v >> b) & 1) ? c_adv[adv_k(i)][4 * j + b] : 0u;
        S.adv[i][j][v] = r;
    }
    if (tid < kMemSeg) S.cnt[tid] = tid < nseg ? a.cnt[m * kMemSeg + tid] : 0u;
    __syncthreads();
    {  // the raw CRC is linear: a thread's 32 bytes hash to the XOR of one entry per value
        const int q = tid >> 5;
        const uint32_t bits = __float_as_uint((float)(tid & 31));
        uint32_t cr = 0;
#pragma unroll
        for (int k = 0; k < kRPer; ++k) cr = crc4(S.crct, cr, k == q ? bits : 0u);
        S.cid[q][tid & 31] = cr;
    }
    __syncthreads();
    auto advt = [&](uint32_t x, int i) -> uint32_t {
        uint32_t r = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) r ^= S.adv[i][j][(x >> (4 * j)) & 15u];
        return r;
    };
    int bad = 0;
    // a segment's op records (over its own output bytes) are loaded one
    // segment ahead, into registers, so that their latency overlaps the
    // previous segment's resolve (they were the loop's first dependent loads)
    constexpr int kOpPer = kSeg / kRNT;  // >= one op per value: nops <= kSeg
    uint32_t pre[kOpPer];
    auto fetch = [&](int sg) {
        const uint32_t n = sg < nseg ? S.cnt[sg] : 0u;
        const uint32_t* opi = reinterpret_cast<const uint32_t*>(a.out + out_off) + ((int64_t)sg << kSegLog);
#pragma unroll
        for (int i = 0; i < kOpPer; ++i) {
            const uint32_t k = (uint32_t)(tid + i * kRNT);
            pre[i] = k < n ? opi[k] : 0u;
        }
    };
    fetch(0);
    uint64_t t_a = a.dbg ? wall_clock64() : 0, d_pre = 0, d_jump = 0, d_val = 0;
    uint32_t jumps = 0;
    for (int s = 0; s < nseg; ++s) {
        const int c0 = s << kSegLog;
        const int T = (int)min((uint32_t)kSeg, ntok - (uint32_t)c0);
        const uint32_t nops = S.cnt[s];
        if (nops > (uint32_t)T) { bad = kInfCorrupt; break; }  // (block-uniform)
        float* const yo = reinterpret_cast<float*>(a.out + out_off) + c0;
#pragma unroll
        for (int i = 0; i < kOpPer; ++i) S.opr[tid + i * kRNT] = pre[i];
        fetch(s + 1);
        const int64_t g0 = out_off / 4 + c0;  // the segment's first element of the stream
        if (LUT) {
            // the slots hold the tensors from the one holding (or following)
            // the segment's first element: loaded for the member's first
            // segment, then moved on only where a tensor ended before this
            // segment (a global search per segment cost ~6 us of dependent
            // loads on every block's critical path)
            if (tid == 0) {
                int t = -1;
                if (s == 0 || (S.ln > 0 && S.lea[0] <= g0 && S.lt0 + 1 < a.lut_n)) {
                    int lo = s == 0 ? 0 : S.lt0, hi = a.lut_n - 1;
                    t = a.lut_n;
                    while (lo <= hi) {  // the first tensor ending after g0
                        const int mid = (lo + hi) >> 1;
                        if (a.lut_end[mid] > g0) { t = mid; hi = mid - 1; } else lo = mid + 1;
                    }
                    S.lt0 = t;
                    S.ln = min(kLutSlots, a.lut_n - t);
                }
                S.scan[0] = t >= 0 ? 1u : 0u;  // reload (the scan words are free until the block scan)
            }
            __syncthreads();
            const int t0 = S.lt0, ln = S.ln;
            if (S.scan[0]) {
                for (int k = tid; k < ln * 32; k += kRNT) S.lt[k >> 5][k & 31] = a.lut_tab[(int64_t)(t0 + (k >> 5)) * 32 + (k & 31)];
                if (tid < ln) { S.lsa[tid] = a.lut_start[t0 + tid]; S.lea[tid] = a.lut_end[t0 + tid]; }
            }
            __syncthreads();
            if (tid < ln) {
                S.ls[tid] = (int32_t)max<int64_t>(-1, min<int64_t>(kSeg + 1, S.lsa[tid] - g0));
                S.le[tid] = (int32_t)max<int64_t>(-1, min<int64_t>(kSeg + 1, S.lea[tid] - g0));
            }
        }
        __syncthreads();
        // positions: each thread a contiguous run of ops
        const uint32_t o_lo = nops * tid / kRNT, o_hi = nops * (tid + 1) / kRNT;
        uint32_t run = 0;
        for (uint32_t o = o_lo; o < o_hi; ++o) { const uint32_t r = S.opr[o]; run += (r >> 31) ? 1u : (r & 127u); }
        uint32_t tot;
        uint32_t p = block_scan<kRNT>(run, S.scan, &tot);
        if (tot != (uint32_t)T) { bad = kInfCorrupt; break; }  // block-uniform
        for (uint32_t o = o_lo; o < o_hi; ++o) {
            const uint32_t r = S.opr[o];
            if (r >> 31) {
                S.e[p++] = (uint16_t)(0x8000u | (r & 31u));
            } else {
                const uint32_t l = r & 127u, d = r >> 7;
                for (uint32_t k = 0; k < l; ++k) S.e[p + k] = (uint16_t)d;
                p += l;
            }
        }
        __syncthreads();
        uint64_t t_b = a.dbg ? wall_clock64() : 0;
        if (a.dbg) d_pre += t_b - t_a;
        // pointer jumping: an unresolved entry points at its source; a source
        // before the segment is a value of the ring
        const int rb0 = (int)((uint32_t)c0 % kVRing);
        // (a resolved entry stays resolved: each thread skips the ones it
        // saw resolved, so later rounds read only the 43 %, 7 %, ... left)
        uint32_t um = (1u << kRPer) - 1u;
#pragma unroll 1
        for (;;) {
            ++jumps;
            int pend = 0;
            uint32_t nm = 0;
#pragma unroll
            for (int i = 0; i < kRPer; ++i) {
                const int k = tid + i * kRNT;
                if (!((um >> i) & 1u) || k >= T) continue;
                const uint32_t e = S.e[k];
                if (e & 0x8000u) continue;
                const int src = k - (int)e;
                uint32_t ne;
                if (src < 0) {  // a value before the segment: ring slot (c0 + src) mod kVRing, src >= -kWin
                    const int r = rb0 + src;
                    ne = 0x8000u | S.v[r < 0 ? r + (int)kVRing : r];
                }
                else {
                    const uint32_t es = S.e[src];
                    ne = (es & 0x8000u) ? es : e + es;
                }
                S.e[k] = (uint16_t)ne;
                if (!(ne & 0x8000u)) { pend = 1; nm |= 1u << i; }
            }
            um = nm;
            if (!__syncthreads_or(pend)) break;
        }
        if (a.dbg) { const uint64_t t = wall_clock64(); d_jump += t - t_b; t_b = t; }
        // values: ring, output (float32), raw CRC-32
        {
            const int k0 = kRPer * tid;
            const int nv = max(0, min(kRPer, T - k0));
            uint32_t crc = 0;
            float f[kRPer];
            // the thread's 8 entries as one 16-byte read, its 8 ids into the
            // ring as one 8-byte write (c0 + k0 and kVRing are multiples of 8:
            // the 8 ring slots never wrap)
            static_assert(kRPer == 8 && kVRing % 8 == 0, "one b128 read, one b64 ring write per thread");
            const uint4 ev = *reinterpret_cast<const uint4*>(&S.e[k0]);
            const uint32_t ew[4] = {ev.x, ev.y, ev.z, ev.w};
            uint32_t idw[2] = {0u, 0u};
#pragma unroll
            for (int q = 0; q < kRPer; ++q) {
                const uint32_t id = q < nv ? ((ew[q >> 1] >> (16 * (q & 1))) & 31u) : 0u;
                f[q] = (float)id;
                idw[q >> 2] |= id << (8 * (q & 3));
                if (q < nv) crc ^= S.cid[q][id];
            }
            if (nv == kRPer) {
                *reinterpret_cast<uint2*>(&S.v[(uint32_t)(c0 + k0) % kVRing]) = make_uint2(idw[0], idw[1]);
            } else {
                for (int q = 0; q < nv; ++q) S.v[(uint32_t)(c0 + k0 + q) % kVRing] = (uint8_t)(idw[q >> 2] >> (8 * (q & 3)));
            }
            if (nv < kRPer) {  // a partial last piece: the values' own chain
                crc = 0;
#pragma unroll
                for (int q = 0; q < kRPer; ++q)
                    if (q < nv) crc = crc4(S.crct, crc, __float_as_uint(f[q]));
            }
            if (LUT) {  // the values through the element's tensor table (the CRC above is the ranks')
                const int ln = S.ln;
                int j = 0;  // the slot of this thread's first element (segment-relative k0)
                while (j < ln && k0 >= S.le[j]) ++j;
                if (j < ln && k0 >= S.ls[j] && k0 + kRPer <= S.le[j]) {  // all its values in one tensor
#pragma unroll
                    for (int q = 0; q < kRPer; ++q) f[q] = S.lt[j][(uint32_t)f[q]];
                } else {
#pragma unroll
                    for (int q = 0; q < kRPer; ++q) {
                        const int k = k0 + q;
                        const uint32_t id = (uint32_t)f[q];
                        int jj = 0;
                        while (jj < ln && k >= S.le[jj]) ++jj;
                        float v = f[q];
                        if (jj < ln) {
                            if (k >= S.ls[jj]) v = S.lt[jj][id];
                        } else if (ln == kLutSlots) {  // past the tables in LDS: a segment over many small tensors
                            const int t = lut_find(a, g0 + k);
                            if (t >= 0) v = a.lut_tab[(int64_t)t * 32 + id];
                        }
                        f[q] = v;
                    }
                }
            }
            if (nv == kRPer && (reinterpret_cast<uintptr_t>(yo + k0) & 15u) == 0) {
                float4* y4 = reinterpret_cast<float4*>(yo + k0);
#pragma unroll
                for (int u = 0; u < kRPer / 4; ++u) y4[u] = make_float4(f[4 * u], f[4 * u + 1], f[4 * u + 2], f[4 * u + 3]);
            } else {
                for (int q = 0; q < nv; ++q) yo[k0 + q] = f[q];
            }
            uint32_t wcrc;
            if (T == kSeg) {
                uint32_t x = crc;
#pragma unroll
                for (int l = 0; l < 6; ++l) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)x, 1 << l, 64);
                    const uint32_t sh = advt(x, l);  // 2^(5 + l) bytes
                    x = (lane & (1 << l)) ? x : (sh ^ o);
                }
                wcrc = x;
            } else {
                uint32_t x = nv ? crc_adv(crc, 4u * (uint32_t)(T - k0 - nv)) : 0u;
                for (int o = 32; o > 0; o >>= 1) x ^= (uint32_t)__shfl_xor((int)x, o, 64);
                wcrc = x;
            }
            if (lane == 0) S.crc_w[wv] = wcrc;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t raw = 0;
            if (T == kSeg) {
                for (int w = 0; w < kRNT / 64; ++w) raw = advt(raw, 6) ^ S.crc_w[w];  // 2^kSegLog bytes
                S.crc_raw = advt(S.crc_raw, 7) ^ raw;                                   // 2^(kSegLog + 2)
            } else {
                for (int w = 0; w < kRNT / 64; ++w) raw ^= S.crc_w[w];
                S.crc_raw = crc_adv(S.crc_raw, 4u * (uint32_t)T) ^ raw;
            }
        }
        __syncthreads();
        if (a.dbg) { const uint64_t t = wall_clock64(); d_val += t - t_b; t_a = t; }
    }
    if (a.dbg && (m & 255) == 0 && tid == 0)
        printf("tlz_resolve m=%lld load_scan_ticks=%llu jump_ticks=%llu values_ticks=%llu jump_rounds=%u segs=%d\n",
               (long long)m, (unsigned long long)d_pre, (unsigned long long)d_jump, (unsigned long long)d_val, jumps, nseg);
    if (tid == 0) {
        if (bad) atomicOr(a.status, bad);
        else if ((crc_adv(0xffffffffu, isize) ^ S.crc_raw ^ 0xffffffffu) != want_crc) atomicOr(a.status, kInfCrc);
    }
}
}  // namespace tlz

// members -> one contiguous stream (slots of any stride).  The destination is
// usually mapped pinned host memory, written across PCIe: every store is an
// aligned 16-byte one (the source realigned with alignbyte; slots are 4-byte
// aligned), only the < 16 bytes at either end of a member are byte stores.
// (Byte stores for the 3 in 4 members that start misaligned ran at 8.5 GB/s.)
// one member's bytes from its slot to dst (256 threads; 16-byte stores)
DEVI void pack_member(const uint8_t* src, uint8_t* dst, uint32_t n) {
    const uint32_t head = (uint32_t)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    if (n <= head + 16u) {
        for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
        return;
    }
    const uint32_t body = (n - head) >> 4;  // aligned 16-byte stores
    const uint32_t tail0 = head + 16u * body;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t i = tail0 + threadIdx.x; i < n; i += 256) dst[i] = src[i];
    const uint32_t sh = head & 3u;             // source offset of the body, mod 4
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (head & ~3u));
    uint4* d = reinterpret_cast<uint4*>(dst + head);
    for (uint32_t i = threadIdx.x; i < body; i += 256) {
        const uint32_t* q = s + 4u * i;
        uint4 v;
        if (sh == 0) {
            v = make_uint4(q[0], q[1], q[2], q[3]);
        } else {  // the 5th word is within the slot: the body ends >= 1 byte before n
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
            v.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
            v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
            v.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
            v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
        }
        d[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_gzip_pack(const uint8_t* slots, uint64_t stride, const uint32_t* sizes,
                                                   const uint64_t* off, uint8_t* packed) {
    if (off[blockIdx.x] == ~0ull) return;  // the batch does not fit the output (reported by the scan)
    pack_member(slots + (int64_t)blockIdx.x * stride, packed + off[blockIdx.x], sizes[blockIdx.x]);
}

// the batched path's pack, enqueued right behind the batch's scan with no
// host round trip: the batch's first offset and end come from the scan's
// output (off[0], off[nb]); a batch that fits the device staging goes there
// (stage + off - first, then one DMA), a larger one (nearly incompressible
// ranks) straight into the mapped pinned output at its offsets
__global__ __launch_bounds__(256) void k_gzip_pack_batch(const uint8_t* slots, uint64_t stride, const uint32_t* sizes,
                                                         const uint64_t* off, int nb, uint8_t* stage,
                                                         uint64_t stage_cap, uint8_t* mapped) {
    const uint64_t first = off[0], end = off[nb];
    if (first == ~0ull || off[blockIdx.x] == ~0ull) return;  // the batch does not fit the output (reported by the scan)
    uint8_t* dst = end - first <= stage_cap ? stage + (off[blockIdx.x] - first) : mapped + off[blockIdx.x];
    pack_member(slots + (int64_t)blockIdx.x * stride, dst, sizes[blockIdx.x]);
}

}  // namespace gz
