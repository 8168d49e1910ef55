// lossy_single.h -- the one-tensor kernels of lossy_kernels.hip (grid-stride,
// rule in the kernel arguments).  The batched kernels do the same work for an
// arena of tensors; these stay as the independent second implementation the
// tests compare them with, and as STCPipeline's per-tensor path.
#pragma once
#include "lossy_device.h"

namespace lossy {

struct KmParams {
    float mids[kMaxK];       // sorted midpoints between consecutive sorted centres (k-1 used)
    float rank[kMaxK];       // label value to write per cluster (float32 rank)
    int k;
};
DEVI int cluster_of(float v, const KmParams& p) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < kMaxK - 1; ++j) c += (j < p.k - 1 && p.mids[j] < v) ? 1 : 0;
    return c;
}

// ---- labels -> float32 ranks -------------------------------------------------
__global__ __launch_bounds__(kNT) void k_km_label(const float* x, int64_t n, KmParams p, float* out) {
    for (int64_t i = gtid(); i < n; i += gstride()) out[i] = p.rank[cluster_of(x[i], p)];
}

// ternary ranks of the sparse array (stc_pipeline.py:105-130): value > 0 ->
// rank_pos, < 0 -> rank_neg, else rank_zero; written as float32 (GZIP input)
__global__ __launch_bounds__(kNT) void k_ternary(const float* sparse, int64_t n, float rneg, float rzero,
                                                 float rpos, float* out) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        const float v = sparse[i];
        out[i] = v > 0.0f ? rpos : (v < 0.0f ? rneg : rzero);
    }
}

// TernaryTransformer statistics (stc_pipeline.py:120-123): fp64 sum of |x| and
// counts of x > 0, x < 0 (the rest are zeros)
// per-wave partials (sign counts, sum |x| in fp64), then one wave sums them in
// a fixed order: the ternary mean (stc_pipeline.py:120-123) is the same on
// every run (fp64 atomics would make its last bits depend on arrival order)
__global__ __launch_bounds__(kNT) void k_tstats(const float* x, int64_t n, unsigned long long* cnt_p,
                                                 double* abs_p) {
    uint32_t cp = 0, cn = 0;
    double as = 0.0;
    for (int64_t i = gtid(); i < n; i += gstride()) {
        const float v = x[i];
        cp += v > 0.0f;
        cn += v < 0.0f;
        as += fabs((double)v);
    }
    cp = wave_sum(cp); cn = wave_sum(cn); as = wave_sum(as);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = (int64_t)blockIdx.x * (kNT / 64) + (threadIdx.x >> 6);
        cnt_p[2 * w] = cp;
        cnt_p[2 * w + 1] = cn;
        abs_p[w] = as;
    }
}
__global__ __launch_bounds__(64) void k_tstats_final(const unsigned long long* cnt_p, const double* abs_p, int nw,
                                                     unsigned long long* cnt, double* abs_sum) {
    unsigned long long cp = 0, cn = 0;
    double as = 0.0;
    for (int w = threadIdx.x; w < nw; w += 64) { cp += cnt_p[2 * w]; cn += cnt_p[2 * w + 1]; as += abs_p[w]; }
    cp = wave_sum(cp); cn = wave_sum(cn); as = wave_sum(as);
    if (threadIdx.x == 0) { cnt[0] = cp; cnt[1] = cn; abs_sum[0] = as; }
}

// reference backward (kc_pipeline.py:81-83): for key in order: data[data == key] = value,
// applied in place and in sequence -- emulated exactly per element
struct LutParams { float key[64]; float val[64]; int nk; };
__global__ __launch_bounds__(kNT) void k_lut(const float* in, int64_t n, LutParams p, float* out) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        float v = in[i];
        for (int j = 0; j < p.nk; ++j) v = (v == p.key[j]) ? p.val[j] : v;
        out[i] = v;
    }
}

}  // namespace lossy
