// lossy_kernels.hip -- gfx950 kernels for the k-means / sparsify / ternary
// pipelines of openfl/pipelines (reference: /root/reference):
//   kc_pipeline.py:36-114   KmeansTransformer (sklearn KMeans k=6, n_init=6)
//   skc_pipeline.py:33-187  SparsityTransformer + KmeansTransformer
//   stc_pipeline.py:30-143  SparsityTransformer + TernaryTransformer
//
// This file is the host driver; the kernels are in the headers it includes:
//   lossy_layout.h  host-only: constants, the chunk table, workspace layouts
//   lossy_device.h  what the kernels share (reductions, chunk_of, visit)
//   lossy_single.h  the one-tensor kernels (label, ternary, statistics, LUT)
//   lossy_kmeans.h  batched k-means, k_label_apply, k_lut_batch
//   lossy_topk.h    batched top-k, k_ternary_batch
//
// Every pass is a device kernel: the O(n) passes stream (coalesced 16-B loads,
// per-block LDS/register reduction, one atomic per block and quantity), and the
// decisions between them -- k-means++ seeding and Lloyd on the histogram, the
// centre updates, the radix-select digit walks, the tie scans -- are one
// workgroup or one wave per tensor.  A batched call therefore enqueues all its
// passes and synchronises `stream` once, to copy the per-tensor results back.
// The k-means and top-k entry points (batched or one tensor) and
// ofl_ternary_stats return host scalars and so end with that sync;
// ofl_label_apply, ofl_lut_decode(_batch), ofl_ternary_ranks(_batch) and
// ofl_kmeans1d_label only enqueue.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

// (in this order: the device code keeps the order of the kernels' definitions)
#include "lossy_single.h"
#include "lossy_kmeans.h"
#include "lossy_topk.h"
#include "ofl_codec.h"
#include "ofl_util.h"

namespace {

thread_local std::string g_lerr;
int lfail(int code, const std::string& m) { g_lerr = m; return code; }
#define LHIP(x)                                                                                       \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) return lfail(OFL_EHIP, std::string(#x " failed: ") + hipGetErrorString(e_)); \
    } while (0)

int cu_count() {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}
int grid_for(int64_t n) {
    const int64_t want = (n + lossy::kNT * 16 - 1) / (lossy::kNT * 16);
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cu_count() * 8));
}

// a region of a workspace
template <typename T>
T* at(void* ws, lossy::Span s) { return reinterpret_cast<T*>(static_cast<char*>(ws) + s.off); }

lossy::KmParams km_params(const std::vector<double>& c) {
    lossy::KmParams p{};
    p.k = (int)c.size();
    for (int j = 0; j + 1 < p.k; ++j) p.mids[j] = (float)((c[j] + c[j + 1]) / 2);
    for (int j = 0; j < p.k; ++j) p.rank[j] = (float)j;
    return p;
}

}  // namespace

extern "C" {

const char* ofl_lossy_last_error(void) { return g_lerr.c_str(); }

size_t ofl_lossy_workspace_bytes(int64_t n) { return lossy::single_workspace_bytes(n); }

// ---- the round end's tail (k_label_apply, lossy_kmeans.h) -------------------
int ofl_label_apply(const float* x_arena, const ofl_label_rec* recs, int ntensors, const float* base, float* out,
                    void* stream) {
    if (!x_arena || !recs || !out || ntensors < 1) return lfail(OFL_EINVAL, "label_apply: bad arguments");
    const int cus = cu_count();
    // two 1024-thread workgroups fill a CU; they stride over the chunks
    for (int t0 = 0; t0 < ntensors; t0 += lossy::kLaMaxT)
        hipLaunchKernelGGL(base ? lossy::k_label_apply<true> : lossy::k_label_apply<false>, dim3((unsigned)(2 * cus)),
                           dim3(lossy::kBkmAccNT), 0, static_cast<hipStream_t>(stream), x_arena, recs + t0,
                           std::min(ntensors - t0, lossy::kLaMaxT), base, out);
    LHIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"

// ---- batched 1-D k-means (lossy_kmeans.h) -----------------------------------
namespace {
template <int KM1>
void bkm_launch_acc(int64_t blocks, hipStream_t st, const lossy::BkmArgs& a) {
    hipLaunchKernelGGL(lossy::k_bkm_acc<KM1>, dim3((unsigned)blocks), dim3(lossy::kBkmAccNT), 0, st, a);
}
template <int KM1>
void bkm_launch_label(int64_t blocks, hipStream_t st, const lossy::BkmArgs& a) {
    hipLaunchKernelGGL(lossy::k_bkm_label<KM1>, dim3((unsigned)blocks), dim3(lossy::kBkmAccNT), 0, st, a);
}
// the batched k-means behind every entry point; seeds (host, [ntensors]): one
// seed per tensor (ofl_kmeans1d_batch_seeds), else NULL and `seed` for all
int bkm_run(int ntensors, const float* x_arena, const int64_t* offsets, const int64_t* numels, int k, int n_init,
            uint64_t seed, const uint64_t* seeds, int max_exact, int value_f64, float* ranks_out,
            ofl_label_rec* label_tab, ofl_label_rec* value_tab, double* centres, int64_t* counts, double* inertia,
            int32_t* nuniq, double* uniq, void* ws, size_t ws_bytes, void* stream) {
    lossy::ChunkTable tab;
    const lossy::ChunkErr bad = lossy::chunk_table(ntensors, offsets, numels, tab);
    if (ntensors < 1 || !x_arena || bad == lossy::kChunkNull) return lfail(OFL_EINVAL, "kmeans: empty batch");
    if (label_tab || value_tab) {
        if (k > 8) return lfail(OFL_EINVAL, "kmeans: label records need k <= 8");
        for (int t = 0; t < ntensors; ++t)
            if (offsets[t] < 0 || (t > 0 && offsets[t] < offsets[t - 1] + numels[t - 1]))
                return lfail(OFL_EINVAL, "kmeans: label records need ascending, non-overlapping tensors");
    }
    if (k < 1 || k > lossy::kMaxK) return lfail(OFL_EINVAL, "kmeans: need 1 <= k <= 32");
    if (n_init < 1 || n_init > lossy::kBkmMaxInit || max_exact < 0)
        return lfail(OFL_EINVAL, "kmeans: 1 <= n_init <= 16, max_exact >= 0");
    if (bad == lossy::kChunkNumel || std::any_of(numels, numels + ntensors, [k](int64_t n) { return n < k; }))
        return lfail(OFL_EINVAL, "kmeans: need n >= k for every tensor");
    const lossy::KmeansLayout L = lossy::kmeans_layout(ntensors, tab.blocks);
    if (!ws || ws_bytes < L.total) return lfail(OFL_ESPACE, "kmeans: workspace too small");
    if (bad == lossy::kChunkBlocks) return lfail(OFL_EINVAL, "kmeans: batch too large");
    LHIP(ofl_util::per_device_once([] {
        return hipFuncSetAttribute((const void*)lossy::k_bkm_seed, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lossy::kBkmSeedLds);
    }));
    hipStream_t st = static_cast<hipStream_t>(stream);
    lossy::BkmArgs a{};
    a.x = x_arena;
    a.out = ranks_out;
    a.td = at<lossy::BkmTensor>(ws, L.td);
    a.ntensors = ntensors;
    a.k = k;
    a.n_init = n_init;
    a.value_f64 = value_f64 ? 1 : 0;
    a.seed = seed;
    a.seeds = seeds ? at<uint64_t>(ws, L.seeds) : nullptr;
    a.st = at<lossy::BkmState>(ws, L.st);
    a.hc = at<uint32_t>(ws, L.hc);
    a.hs = at<unsigned long long>(ws, L.hs);
    a.part = at<double>(ws, L.part);
    LHIP(hipMemcpyAsync(at<char>(ws, L.td), tab.td.data(), sizeof(lossy::BkmTensor) * ntensors, hipMemcpyHostToDevice, st));
    if (seeds) LHIP(hipMemcpyAsync(at<char>(ws, L.seeds), seeds, sizeof(uint64_t) * ntensors, hipMemcpyHostToDevice, st));
    LHIP(hipMemsetAsync(at<char>(ws, L.zeroed), 0, L.zeroed.bytes, st));
    const dim3 g((unsigned)tab.blocks), b(lossy::kNT);
    hipLaunchKernelGGL(lossy::k_bkm_minmax, g, b, 0, st, a);
    hipLaunchKernelGGL(lossy::k_bkm_hist, g, b, 0, st, a);
    hipLaunchKernelGGL(lossy::k_bkm_seed, dim3(ntensors * n_init), dim3(lossy::kBkmSeedNT), lossy::kBkmSeedLds, st, a);
    hipLaunchKernelGGL(lossy::k_bkm_pick, dim3((ntensors + 63) / 64), dim3(64), 0, st, a);
    for (int pass = 0; pass <= max_exact; ++pass) {
        a.final_pass = pass == max_exact;
        if (k <= 8) bkm_launch_acc<7>(tab.blocks, st, a);
        else if (k <= 16) bkm_launch_acc<15>(tab.blocks, st, a);
        else bkm_launch_acc<31>(tab.blocks, st, a);
        hipLaunchKernelGGL(lossy::k_bkm_update, dim3(ntensors), dim3(64), 0, st, a);
    }
    if (ranks_out) {
        if (k <= 8) bkm_launch_label<7>(tab.blocks, st, a);
        else if (k <= 16) bkm_launch_label<15>(tab.blocks, st, a);
        else bkm_launch_label<31>(tab.blocks, st, a);
    }
    if (label_tab || value_tab)
        hipLaunchKernelGGL(lossy::k_bkm_tab, dim3((ntensors + 63) / 64), dim3(64), 0, st, a, label_tab, value_tab);
    LHIP(hipGetLastError());
    std::vector<lossy::BkmState> sh(ntensors);
    LHIP(hipMemcpyAsync(sh.data(), a.st, sizeof(lossy::BkmState) * ntensors, hipMemcpyDeviceToHost, st));
    LHIP(hipStreamSynchronize(st));
    for (int t = 0; t < ntensors; ++t) {
        const float lo = lossy::unkey(~sh[t].mm[0]), hi = lossy::unkey(sh[t].mm[1]);
        if (!std::isfinite(lo) || !std::isfinite(hi) || sh[t].has_nan)
            return lfail(OFL_EINVAL, "kmeans: non-finite input");
        for (int j = 0; j < k; ++j) {
            if (centres) centres[(int64_t)t * k + j] = sh[t].cen[j];
            if (counts) counts[(int64_t)t * k + j] = sh[t].cnt[j];
            if (uniq) uniq[(int64_t)t * k + j] = j < sh[t].nuniq ? sh[t].uniq[j] : 0.0;
        }
        if (inertia) inertia[t] = sh[t].inertia;
        if (nuniq) nuniq[t] = sh[t].nuniq;
    }
    return OFL_OK;
}
}  // namespace

extern "C" {

size_t ofl_kmeans1d_batch_workspace_bytes(int ntensors, const int64_t* numels) {
    return lossy::kmeans_workspace_bytes(ntensors, numels);
}

int ofl_kmeans1d_batch(int ntensors, const float* x_arena, const int64_t* offsets, const int64_t* numels, int k,
                       int n_init, uint64_t seed, int max_exact, int value_f64, float* ranks_out, double* centres,
                       int64_t* counts, double* inertia, int32_t* nuniq, double* uniq, void* ws, size_t ws_bytes,
                       void* stream) {
    return ofl_kmeans1d_batch_tab(ntensors, x_arena, offsets, numels, k, n_init, seed, max_exact, value_f64, ranks_out,
                                  nullptr, centres, counts, inertia, nuniq, uniq, ws, ws_bytes, stream);
}

int ofl_kmeans1d_batch_tab(int ntensors, const float* x_arena, const int64_t* offsets, const int64_t* numels, int k,
                           int n_init, uint64_t seed, int max_exact, int value_f64, float* ranks_out,
                           ofl_label_rec* label_tab, double* centres, int64_t* counts, double* inertia,
                           int32_t* nuniq, double* uniq, void* ws, size_t ws_bytes, void* stream) {
    return bkm_run(ntensors, x_arena, offsets, numels, k, n_init, seed, nullptr, max_exact, value_f64, ranks_out,
                   label_tab, nullptr, centres, counts, inertia, nuniq, uniq, ws, ws_bytes, stream);
}

int ofl_kmeans1d_batch_seeds(int ntensors, const float* x_arena, const int64_t* offsets, const int64_t* numels, int k,
                             int n_init, const uint64_t* seeds, int max_exact, int value_f64, float* ranks_out,
                             ofl_label_rec* label_tab, ofl_label_rec* value_tab, double* centres, int64_t* counts,
                             double* inertia, int32_t* nuniq, double* uniq, void* ws, size_t ws_bytes, void* stream) {
    if (!seeds) return lfail(OFL_EINVAL, "kmeans: one seed per tensor is required");
    return bkm_run(ntensors, x_arena, offsets, numels, k, n_init, 0, seeds, max_exact, value_f64, ranks_out, label_tab,
                   value_tab, centres, counts, inertia, nuniq, uniq, ws, ws_bytes, stream);
}

size_t ofl_lut_decode_batch_workspace_bytes(int ntensors, int max_nk) {
    return lossy::lut_workspace_bytes(ntensors, max_nk);
}

int ofl_lut_decode_batch(int ntensors, const float* in_arena, const int64_t* offsets, const int64_t* numels,
                         const int32_t* nk, const float* keys, const float* vals, int max_nk, float* out_arena,
                         void* ws, size_t ws_bytes, void* stream) {
    if (ntensors < 1 || max_nk < 0 || max_nk > 64) return lfail(OFL_EINVAL, "lut: 1+ tensors, at most 64 keys");
    lossy::ChunkTable tab;
    const lossy::ChunkErr bad = lossy::chunk_table(ntensors, offsets, numels, tab);
    if (bad == lossy::kChunkNull || !nk) return lfail(OFL_EINVAL, "lut: offsets, numels and nk are required");
    const lossy::LutLayout L = lossy::lut_layout(ntensors, max_nk);
    if (ws_bytes < L.total + lossy::kWsSlack || !ws) return lfail(OFL_ESPACE, "lut: workspace too small");
    for (int t = 0; t < ntensors; ++t)
        if (nk[t] < 0 || nk[t] > max_nk) return lfail(OFL_EINVAL, "lut: key count out of range");
    if (bad == lossy::kChunkNumel) return lfail(OFL_EINVAL, "lut: tensor length out of range");
    if (bad == lossy::kChunkBlocks) return lfail(OFL_EINVAL, "lut: batch too large");
    if (tab.blocks == 0) return OFL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    lossy::LutBatchArgs a{in_arena, out_arena, at<lossy::BkmTensor>(ws, L.td), at<int32_t>(ws, L.nk),
                          at<float>(ws, L.keys), at<float>(ws, L.vals), ntensors, std::max(max_nk, 1)};
    LHIP(hipMemcpyAsync(at<char>(ws, L.td), tab.td.data(), sizeof(lossy::BkmTensor) * ntensors, hipMemcpyHostToDevice, st));
    LHIP(hipMemcpyAsync(at<char>(ws, L.nk), nk, 4 * (size_t)ntensors, hipMemcpyHostToDevice, st));
    if (max_nk) {
        LHIP(hipMemcpyAsync(at<char>(ws, L.keys), keys, 4 * (size_t)ntensors * max_nk, hipMemcpyHostToDevice, st));
        LHIP(hipMemcpyAsync(at<char>(ws, L.vals), vals, 4 * (size_t)ntensors * max_nk, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(lossy::k_lut_batch, dim3((unsigned)tab.blocks), dim3(lossy::kNT), 0, st, a);
    LHIP(hipGetLastError());
    return OFL_OK;
}

// single tensor, no labels: sorted centres, counts and inertia (replaces
// sklearn KMeans.fit in kc_pipeline.py:49-56 / skc_pipeline.py:127-131)
int ofl_kmeans1d_fit(const float* x, int64_t n, int k, int n_init, uint64_t seed, int max_exact,
                     double* centres, int64_t* counts, double* inertia, void* ws, size_t ws_bytes,
                     void* stream) {
    const int64_t off = 0;
    return ofl_kmeans1d_batch(1, x, &off, &n, k, n_init, seed, max_exact, 1, nullptr, centres, counts, inertia,
                              nullptr, nullptr, ws, ws_bytes, stream);
}

// labels as float32 values: out[i] = rank_of_cluster[nearest sorted centre]
int ofl_kmeans1d_label(const float* x, int64_t n, const double* centres, int k, const float* rank_of_cluster,
                       float* out, void* stream) {
    if (k < 1 || k > lossy::kMaxK) return lfail(OFL_EINVAL, "kmeans: bad k");
    std::vector<double> c(centres, centres + k);
    lossy::KmParams p = km_params(c);
    for (int j = 0; j < k; ++j) p.rank[j] = rank_of_cluster[j];
    hipLaunchKernelGGL(lossy::k_km_label, dim3(grid_for(n)), dim3(lossy::kNT), 0, static_cast<hipStream_t>(stream),
                       x, n, p, out);
    LHIP(hipGetLastError());
    return OFL_OK;
}

// ---- batched top-k by magnitude, ternary ranks (lossy_topk.h) ---------------
size_t ofl_sparsify_topk_batch_workspace_bytes(int ntensors, const int64_t* numels) {
    return lossy::topk_workspace_bytes(ntensors, numels);
}

int ofl_sparsify_topk_batch(int ntensors, const float* x_arena, const int64_t* offsets, const int64_t* numels,
                            const int64_t* ks, float* sparse_arena, float* kept_min, int64_t* n_pos, int64_t* n_neg,
                            int64_t* n_zero, double* abs_sum, int32_t* shifted, void* ws, size_t ws_bytes,
                            void* stream) {
    lossy::ChunkTable tab;
    const lossy::ChunkErr bad = lossy::chunk_table(ntensors, offsets, numels, tab);
    if (ntensors < 1 || !x_arena || !sparse_arena || bad == lossy::kChunkNull || !ks)
        return lfail(OFL_EINVAL, "sparsify: empty batch");
    if (bad == lossy::kChunkNumel) return lfail(OFL_EINVAL, "sparsify: need 1 <= k <= n");
    for (int t = 0; t < ntensors; ++t)
        if (ks[t] < 1 || ks[t] > numels[t]) return lfail(OFL_EINVAL, "sparsify: need 1 <= k <= n");
    const lossy::TopkLayout L = lossy::topk_layout(ntensors, tab.blocks);
    if (!ws || ws_bytes < L.total) return lfail(OFL_ESPACE, "sparsify: workspace too small");
    if (bad == lossy::kChunkBlocks) return lfail(OFL_EINVAL, "sparsify: batch too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<lossy::BtkState> sh(ntensors);
    for (int t = 0; t < ntensors; ++t) sh[t].k = sh[t].need = ks[t];
    lossy::BtkArgs a{};
    a.x = x_arena;
    a.out = sparse_arena;
    a.td = at<lossy::BkmTensor>(ws, L.td);
    a.ntensors = ntensors;
    a.st = at<lossy::BtkState>(ws, L.st);
    a.hist = at<uint32_t>(ws, L.hist);
    a.blk = at<lossy::BtkBlock>(ws, L.blk);
    LHIP(hipMemcpyAsync(at<char>(ws, L.td), tab.td.data(), sizeof(lossy::BkmTensor) * ntensors, hipMemcpyHostToDevice, st));
    LHIP(hipMemcpyAsync(a.st, sh.data(), sizeof(lossy::BtkState) * ntensors, hipMemcpyHostToDevice, st));
    LHIP(hipMemsetAsync(at<char>(ws, L.zeroed), 0, L.zeroed.bytes, st));
    const dim3 g((unsigned)tab.blocks), b(lossy::kNT);
    for (int pass = 0; pass < 3; ++pass) {
        a.pass = pass;
        hipLaunchKernelGGL(lossy::k_btk_hist, g, b, 0, st, a);
        hipLaunchKernelGGL(lossy::k_btk_digit, dim3(ntensors), dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(lossy::k_btk_ties, g, b, 0, st, a);
    hipLaunchKernelGGL(lossy::k_btk_scan, dim3(ntensors), dim3(64), 0, st, a);
    hipLaunchKernelGGL(lossy::k_btk_select, g, b, 0, st, a);
    hipLaunchKernelGGL(lossy::k_btk_final, dim3(ntensors), dim3(64), 0, st, a);
    LHIP(hipGetLastError());
    LHIP(hipMemcpyAsync(sh.data(), a.st, sizeof(lossy::BtkState) * ntensors, hipMemcpyDeviceToHost, st));
    LHIP(hipStreamSynchronize(st));
    for (int t = 0; t < ntensors; ++t) {
        if (kept_min) kept_min[t] = sh[t].kmin;
        if (shifted) shifted[t] = sh[t].shift != 0.0f;
        if (n_pos) n_pos[t] = sh[t].n_pos;
        if (n_neg) n_neg[t] = sh[t].n_neg;
        if (n_zero) n_zero[t] = sh[t].n_zero;
        if (abs_sum) abs_sum[t] = sh[t].abs_sum;
    }
    return OFL_OK;
}

// top-k by magnitude of one tensor (skc/stc SparsityTransformer._topk_func,
// skc_pipeline.py:72-94): the batched path with T = 1.  Exact k-th largest
// |x|; ties at the threshold kept lowest index first; dense float32 sparse
// array (kept values + shift, zeros elsewhere; shift = 1e-7 iff min(kept) <
// 1e-7, :92-93) and the kept-set statistics of the ternary / k-means stages.
int ofl_sparsify_topk(const float* x, int64_t n, int64_t k, float* sparse_out, float* kept_min,
                      int64_t* n_pos, int64_t* n_neg, int64_t* n_zero, double* abs_sum, int* shifted,
                      void* ws, size_t ws_bytes, void* stream) {
    const int64_t off = 0;
    int32_t sh = 0;
    const int rc = ofl_sparsify_topk_batch(1, x, &off, &n, &k, sparse_out, kept_min, n_pos, n_neg, n_zero, abs_sum,
                                           &sh, ws, ws_bytes, stream);
    if (rc == OFL_OK && shifted) *shifted = sh;
    return rc;
}

size_t ofl_ternary_ranks_batch_workspace_bytes(int ntensors) { return lossy::ternary_workspace_bytes(ntensors); }

int ofl_ternary_ranks_batch(int ntensors, const float* sparse_arena, const int64_t* offsets, const int64_t* numels,
                            const float* ranks3, float* out_arena, void* ws, size_t ws_bytes, void* stream) {
    lossy::ChunkTable tab;
    const lossy::ChunkErr bad = lossy::chunk_table(ntensors, offsets, numels, tab);
    if (ntensors < 1 || bad == lossy::kChunkNull || !ranks3) return lfail(OFL_EINVAL, "ternary: empty batch");
    const lossy::TernaryLayout L = lossy::ternary_layout(ntensors);
    if (!ws || ws_bytes < L.total + lossy::kWsSlack) return lfail(OFL_ESPACE, "ternary: workspace too small");
    if (bad == lossy::kChunkNumel) return lfail(OFL_EINVAL, "ternary: tensor length out of range");
    if (bad == lossy::kChunkBlocks) return lfail(OFL_EINVAL, "ternary: batch too large");
    if (tab.blocks == 0) return OFL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LHIP(hipMemcpyAsync(at<char>(ws, L.td), tab.td.data(), sizeof(lossy::BkmTensor) * ntensors, hipMemcpyHostToDevice, st));
    LHIP(hipMemcpyAsync(at<char>(ws, L.ranks3), ranks3, 12 * (size_t)ntensors, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lossy::k_ternary_batch, dim3((unsigned)tab.blocks), dim3(lossy::kNT), 0, st, sparse_arena,
                       out_arena, at<lossy::BkmTensor>(ws, L.td), ntensors, at<float>(ws, L.ranks3));
    LHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_ternary_stats(const float* x, int64_t n, int64_t* n_pos, int64_t* n_neg, double* abs_sum, void* ws,
                      size_t ws_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = grid_for(n), nw = grid * (lossy::kNT / 64);
    lossy::Carve carve;
    const lossy::Span c = carve.take(sizeof(unsigned long long) * 2), a = carve.take(sizeof(double));
    const lossy::Span cp = carve.take(sizeof(unsigned long long) * 2 * (size_t)nw);
    const lossy::Span ap = carve.take(sizeof(double) * (size_t)nw);
    if (carve.at > ws_bytes) return lfail(OFL_ESPACE, "ternary: workspace too small");
    hipLaunchKernelGGL(lossy::k_tstats, dim3(grid), dim3(lossy::kNT), 0, st, x, n, at<unsigned long long>(ws, cp),
                       at<double>(ws, ap));
    hipLaunchKernelGGL(lossy::k_tstats_final, dim3(1), dim3(64), 0, st, at<unsigned long long>(ws, cp),
                       at<double>(ws, ap), nw, at<unsigned long long>(ws, c), at<double>(ws, a));
    unsigned long long ch[2];
    LHIP(hipMemcpyAsync(ch, at<char>(ws, c), 16, hipMemcpyDeviceToHost, st));
    LHIP(hipMemcpyAsync(abs_sum, at<char>(ws, a), 8, hipMemcpyDeviceToHost, st));
    LHIP(hipStreamSynchronize(st));
    *n_pos = (int64_t)ch[0];
    *n_neg = (int64_t)ch[1];
    return OFL_OK;
}

int ofl_ternary_ranks(const float* sparse, int64_t n, float rank_neg, float rank_zero, float rank_pos, float* out,
                      void* stream) {
    hipLaunchKernelGGL(lossy::k_ternary, dim3(grid_for(n)), dim3(lossy::kNT), 0, static_cast<hipStream_t>(stream),
                       sparse, n, rank_neg, rank_zero, rank_pos, out);
    LHIP(hipGetLastError());
    return OFL_OK;
}

// in-place sequential key -> value replacement of the reference backward,
// emulated per element (kc_pipeline.py:81-83, stc_pipeline.py:139-142)
int ofl_lut_decode(const float* in, int64_t n, const float* keys, const float* vals, int nk, float* out,
                   void* stream) {
    if (nk < 0 || nk > 64) return lfail(OFL_EINVAL, "lut: at most 64 keys");
    lossy::LutParams p{};
    p.nk = nk;
    for (int j = 0; j < nk; ++j) { p.key[j] = keys[j]; p.val[j] = vals[j]; }
    hipLaunchKernelGGL(lossy::k_lut, dim3(grid_for(n)), dim3(lossy::kNT), 0, static_cast<hipStream_t>(stream),
                       in, n, p, out);
    LHIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"
