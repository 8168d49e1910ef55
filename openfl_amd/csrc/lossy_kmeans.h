// lossy_kmeans.h -- the batched 1-D k-means kernels of lossy_kernels.hip, the
// label records they leave, the round end's tail that applies value records
// (k_label_apply), and the batched backward of the ranks (k_lut_batch).
#pragma once
#include "lossy_device.h"
#include "ofl_codec.h"

namespace lossy {

// ===========================================================================
// Batched 1-D k-means (KmeansTransformer.forward, kc_pipeline.py:47-63 and
// skc_pipeline.py:127-131, for many tensors of one fp32 arena) entirely on the
// device and deterministic (integer atomics and fixed-order reductions only):
//   k_bkm_minmax  per-tensor min / max                              (1 pass)
//   k_bkm_hist    per-tensor 4096-bin histogram: counts + fixed-point
//                 sums of the position inside the bin               (1 pass)
//   k_bkm_seed    one workgroup per (tensor, restart): weighted k-means++ with
//                 sklearn's 2 + ln(k) local trials, then Lloyd on the bin
//                 means through prefix sums (O(1) cluster edges); n_init
//                 restarts, lowest inertia
//   k_bkm_acc     exact Lloyd statistics on the data: per block, count /
//                 sum / sum of squares above every float32 midpoint (1 pass)
//   k_bkm_update  one wave per tensor: fixed-order sum of the block
//                 partials, new centres; stops when the float32 midpoints
//                 do not move or at sklearn's tolerance (then one more
//                 assignment pass); then counts, inertia, np.unique ranks
//   k_bkm_label   float32 rank of each element's cluster         (1 pass)
// A block covers kBkmChunk consecutive elements of one tensor.
// ===========================================================================
struct BkmArgs {
    const float* x;
    float* out;
    const BkmTensor* td;
    int32_t ntensors;
    int32_t k;
    int32_t n_init;
    int32_t value_f64;       // centre values as float64 (else rounded to float32)
    int32_t final_pass;
    int32_t pad_;
    uint64_t seed;
    const uint64_t* seeds;   // [T] one seed per tensor, each run as a batch of one (else NULL: seed, tensor index mixed in)
    BkmState* st;
    uint32_t* hc;            // [T][4096] counts
    unsigned long long* hs;  // [T][4096] sums of (position inside the bin) * 2^32
    double* part;            // [blocks][3][kMaxK] cumulative partials
};

// this block's tensor and element range.  (The k-means kernels take chunk_of's
// answer through these references and read the tensor's offset from the table
// where they use it: with the Chunk itself they compile to other code.)
DEVI void bkm_range(const BkmArgs& a, int& t, int64_t& i0, int64_t& i1) {
    const Chunk c = chunk_of(a.td, a.ntensors, blockIdx.x);
    t = c.t; i0 = c.i0; i1 = c.i1;
}

__global__ __launch_bounds__(kNT) void k_bkm_minmax(BkmArgs a) {
    __shared__ float rlo[kNT / 64], rhi[kNT / 64];
    int t; int64_t i0, i1;
    bkm_range(a, t, i0, i1);
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;  // fminf / fmaxf drop a NaN: flagged apart, for the host to refuse
    visit(a.x + a.td[t].off, i0, i1, [&](float v, int64_t) { lo = fminf(lo, v); hi = fmaxf(hi, v); nan = nan || v != v; });
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (__any(nan) && (threadIdx.x & 63) == 0) atomicOr(&a.st[t].has_nan, 1);
    if ((threadIdx.x & 63) == 0) { rlo[threadIdx.x >> 6] = lo; rhi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kNT / 64; ++w) { lo = fminf(lo, rlo[w]); hi = fmaxf(hi, rhi[w]); }
        atomicMax(&a.st[t].mm[0], ~fkey(lo));
        atomicMax(&a.st[t].mm[1], fkey(hi));
    }
}
DEVI void bkm_bounds(const BkmState& S, float& lo, float& hi, float& inv_w) {
    lo = unkey(~S.mm[0]);
    hi = unkey(S.mm[1]);
    inv_w = hi > lo ? (float)((double)kBkmBins / ((double)hi - (double)lo) * (1.0 - 1e-7)) : 0.0f;
}

// one 64-bit LDS atomic per element: count in bits [47, 64) (a block has at
// most 2^16 elements), the position inside the bin as 2^30 fixed point in
// bits [0, 47) (at most 2^16 * 2^30 = 2^46 per block); flushed as a count
// and a 2^32 fixed-point sum
constexpr int kBkmCntShift = 47;
__global__ __launch_bounds__(kNT) void k_bkm_hist(BkmArgs a) {
    static_assert(kBkmChunk <= (1 << 16), "packed histogram counts");
    __shared__ unsigned long long h[kBkmBins];
    for (int b = threadIdx.x; b < kBkmBins; b += kNT) h[b] = 0;
    int t; int64_t i0, i1;
    bkm_range(a, t, i0, i1);
    float lo, hi, inv_w;
    bkm_bounds(a.st[t], lo, hi, inv_w);
    __syncthreads();
    visit(a.x + a.td[t].off, i0, i1, [&](float v, int64_t) {
        const float f = (v - lo) * inv_w;
        int b = (int)f;
        b = b < 0 ? 0 : (b >= kBkmBins ? kBkmBins - 1 : b);
        float fr = f - (float)b;
        fr = fr < 0.f ? 0.f : (fr < 1.f ? fr : 0.99999994f);
        lds_add64(h, b, (1ull << kBkmCntShift) | (unsigned long long)(fr * 1073741824.0f));
    });
    __syncthreads();
    uint32_t* hc = a.hc + (int64_t)t * kBkmBins;
    unsigned long long* hs = a.hs + (int64_t)t * kBkmBins;
    for (int b = threadIdx.x; b < kBkmBins; b += kNT) {
        const unsigned long long v = h[b];
        if (v) {
            atomicAdd(&hc[b], (uint32_t)(v >> kBkmCntShift));
            atomicAdd(&hs[b], (v & ((1ull << kBkmCntShift) - 1)) << 2);
        }
    }
}

DEVI uint64_t bkm_rng(uint64_t& s) {  // xorshift64*
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
}
DEVI double bkm_uniform(uint64_t& s) { return (double)(bkm_rng(s) >> 11) * (1.0 / 9007199254740992.0); }
// first i in [0, n) with P[i] > u for an inclusive prefix P (last index if none)
template <typename T>
DEVI int bkm_first_above(const T* P, int n, double u) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)P[mid] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// first i in [0, n] with pts[i] > m (pts ascending)
DEVI int bkm_upper(const float* pts, int n, double m) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)pts[mid] > m) hi = mid; else lo = mid + 1;
    }
    return lo;
}
DEVI void bkm_set_centres(BkmState& S, const double* c, int k) {
    for (int j = 0; j < kMaxK; ++j) S.cen[j] = j < k ? c[j] : c[k - 1];
    for (int j = 0; j < kMaxK; ++j) S.mids[j] = j + 1 < k ? (float)((c[j] + c[j + 1]) / 2) : INFINITY;
}

// one workgroup per tensor: k-means of the weighted histogram points
// inclusive wave scan of one double per lane; total = the whole wave's sum
DEVI double wscan(double v, double& total) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    total = __shfl(v, 63, 64);
    return v;
}
// block (256 threads) sum / inclusive scan of one double per thread; fixed order
DEVI double bkm_bsum(double v, double* tmp) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (tmp[0] + tmp[1]) + (tmp[2] + tmp[3]);
    __syncthreads();
    return s;
}
DEVI double bkm_bscan(double v, double* tmp, double& total) {
    double t;
    v = wscan(v, t);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) tmp[w] = t;
    __syncthreads();
    double off = 0.0;
    for (int j = 0; j < w; ++j) off += tmp[j];
    total = (tmp[0] + tmp[1]) + (tmp[2] + tmp[3]);
    __syncthreads();
    return off + v;
}

// exclusive running max over the block's threads in thread order (256 threads)
DEVI float bkm_bscan_max_excl(float v, double* tmp) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v = fmaxf(v, u);
    }
    float ex = __shfl_up(v, 1, 64);
    if (lane == 0) ex = -INFINITY;
    if (lane == 63) tmp[w] = v;
    __syncthreads();
    for (int j = 0; j < w; ++j) ex = fmaxf(ex, (float)tmp[j]);
    __syncthreads();
    return ex;
}

// One workgroup per (tensor, restart): k-means of the 4096 histogram points (bin means,
// weight = count; empty bins keep their centre with weight 0, so the points
// stay sorted and the cluster edge of a midpoint m is found in O(1) from
// (m - lo) * inv_w).  Weighted k-means++ with sklearn's local trials, then
// Lloyd through prefix sums (lane j of wave 0 owns cluster j) to sklearn's
// tolerance.  k_bkm_pick keeps the restart with the lowest histogram inertia.
constexpr int kBkmSeedNT = 256;
constexpr size_t kBkmSeedLds = 4 * sizeof(float) * kBkmBins + 2 * sizeof(double) * kBkmBins;  // 128 KiB
__global__ __launch_bounds__(kBkmSeedNT) void k_bkm_seed(BkmArgs a) {
    static_assert(kBkmSeedNT == 256, "bkm_bsum/bkm_bscan assume 4 waves");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* W = reinterpret_cast<double*>(smem);
    double* S1 = W + kBkmBins;
    float* pts = reinterpret_cast<float*>(S1 + kBkmBins);
    float* wts = pts + kBkmBins;
    float* d2 = wts + kBkmBins;
    float* C = d2 + kBkmBins;
    __shared__ double tmp[4];
    __shared__ double cc[kMaxK];
    const int t = blockIdx.x / a.n_init, run = blockIdx.x % a.n_init;
    BkmState& S = a.st[t];
    const int k = a.k;
    auto emit = [&](double in) {  // this restart's result (thread 0)
        for (int j = 0; j < k; ++j) S.cand[run][j] = cc[j];
        S.cand_in[run] = in;
    };
    float lo, hi, inv_w;
    bkm_bounds(S, lo, hi, inv_w);
    if (!(hi > lo)) {  // constant (or non-finite: reported by the host) tensor
        if (threadIdx.x == 0) {
            for (int j = 0; j < k; ++j) cc[j] = lo;
            emit(0.0);
        }
        return;
    }
    constexpr int PER = kBkmBins / kBkmSeedNT;  // 16 consecutive bins per thread
    const int i0 = threadIdx.x * PER;
    const uint32_t* hc = a.hc + (int64_t)t * kBkmBins;
    const unsigned long long* hs = a.hs + (int64_t)t * kBkmBins;
    const double width = 1.0 / (double)inv_w;
    int occ = 0;
    double w0 = 0.0, s0 = 0.0, q0 = 0.0;
    for (int q = 0; q < PER; ++q) {
        const int b = i0 + q;
        const uint32_t cn = hc[b];
        const double fr = cn ? (double)hs[b] / 4294967296.0 / (double)cn : 0.5;
        const float p = (float)((double)lo + ((double)b + fr) * width);
        pts[b] = p;
        wts[b] = (float)cn;
        occ += cn ? 1 : 0;
        w0 += cn;
        s0 += (double)cn * p;
        q0 += (double)cn * p * p;
    }
    double tw, ts;
    double ew = bkm_bscan(w0, tmp, tw) - w0;
    double es = bkm_bscan(s0, tmp, ts) - s0;
    for (int q = 0; q < PER; ++q) { ew += wts[i0 + q]; es += (double)wts[i0 + q] * pts[i0 + q]; W[i0 + q] = ew; S1[i0 + q] = es; }
    const int nocc = (int)bkm_bsum((double)occ, tmp);
    const double sq = bkm_bsum(q0, tmp);  // (also publishes pts / W / S1)
    {  // rounding may break the order of neighbouring bin means: running max (block scan)
        float mx = -INFINITY;
        for (int q = 0; q < PER; ++q) mx = fmaxf(mx, pts[i0 + q]);
        float r = bkm_bscan_max_excl(mx, tmp);
        for (int q = 0; q < PER; ++q) { r = fmaxf(r, pts[i0 + q]); pts[i0 + q] = r; }
    }
    __syncthreads();
    if (nocc <= k) {  // no more occupied bins than clusters: they are the centres
        if (threadIdx.x == 0) {
            int j = 0;
            for (int b = 0; b < kBkmBins && j < k; ++b) if (wts[b] > 0) cc[j++] = pts[b];
            for (; j < k; ++j) cc[j] = cc[j - 1];
            emit(0.0);
        }
        return;
    }
    const double wt = W[kBkmBins - 1];
    const double mu = S1[kBkmBins - 1] / wt;
    const double tol = 1e-4 * fmax(sq / wt - mu * mu, 0.0);  // sklearn's _tolerance
    // first bin whose point lies above m (points sorted, each inside its bin)
    auto edge = [&](double m) -> int {
        int b = (int)floor((m - (double)lo) * (double)inv_w);
        b = b < 0 ? 0 : (b > kBkmBins ? kBkmBins : b);
        while (b > 0 && (double)pts[b - 1] > m) --b;
        while (b < kBkmBins && (double)pts[b] <= m) ++b;
        return b;
    };
    // every thread draws the same numbers
    const uint64_t sd = a.seeds ? a.seeds[t] : a.seed;
    const int tmix = a.seeds ? 0 : t;  // per-tensor seeds: the stream of tensor 0 of a one-tensor call
    uint64_t rs = (sd ^ (0x9E3779B97F4A7C15ull * (uint64_t)(tmix + 1)) ^ (0xD1B54A32D192ED03ull * (uint64_t)(run + 1))) | 1ull;
    for (int q = 0; q < 4; ++q) bkm_rng(rs);
    const int trials = 2 + (int)log((double)k);  // sklearn's n_local_trials
    {
        // ---- weighted k-means++ ----
        {
            const int i = bkm_first_above(W, kBkmBins, bkm_uniform(rs) * wt);
            const float c0 = pts[i];
            if (threadIdx.x == 0) cc[0] = c0;
            for (int q = 0; q < PER; ++q) { const float d = pts[i0 + q] - c0; d2[i0 + q] = d * d; }
        }
        for (int j = 1; j < k; ++j) {
            double loc = 0.0;
            for (int q = 0; q < PER; ++q) loc += (double)wts[i0 + q] * d2[i0 + q];
            double pot;
            double e = bkm_bscan(loc, tmp, pot) - loc;
            for (int q = 0; q < PER; ++q) { e += (double)wts[i0 + q] * d2[i0 + q]; C[i0 + q] = (float)e; }
            __syncthreads();
            double bpot = INFINITY;
            int bi = 0;
            for (int tr = 0; tr < trials; ++tr) {
                int ci = pot > 0.0 ? bkm_first_above(C, kBkmBins, bkm_uniform(rs) * pot)
                                   : (int)(bkm_rng(rs) % (uint64_t)kBkmBins);
                while (ci > 0 && wts[ci] == 0) --ci;  // (float rounding of C) never an empty bin
                const float cv = pts[ci];
                double np = 0.0;
                for (int q = 0; q < PER; ++q) { const float d = pts[i0 + q] - cv; np += (double)wts[i0 + q] * fminf(d2[i0 + q], d * d); }
                np = bkm_bsum(np, tmp);
                if (np < bpot) { bpot = np; bi = ci; }
            }
            const float cv = pts[bi];
            if (threadIdx.x == 0) cc[j] = cv;
            for (int q = 0; q < PER; ++q) { const float d = pts[i0 + q] - cv; d2[i0 + q] = fminf(d2[i0 + q], d * d); }
        }
        __syncthreads();
        // ---- Lloyd on the bin means, wave 0, lane j = cluster j ----
        if (threadIdx.x == 0)
            for (int i = 1; i < k; ++i) { const double v = cc[i]; int j = i - 1; while (j >= 0 && cc[j] > v) { cc[j + 1] = cc[j]; --j; } cc[j + 1] = v; }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            double cj = lane < k ? cc[lane] : 0.0;
            for (int it = 0; it < 300; ++it) {
                const double cn = __shfl_down(cj, 1, 64);
                const int end = lane + 1 < k ? edge((cj + cn) / 2) : kBkmBins;
                int start = __shfl_up(end, 1, 64);
                if (lane == 0) start = 0;
                double nc = cj;
                if (lane < k && end > start) {
                    const double w = W[end - 1] - (start ? W[start - 1] : 0.0);
                    const double sm = S1[end - 1] - (start ? S1[start - 1] : 0.0);
                    if (w > 0) nc = sm / w;
                }
                const double shift = wave_sum(lane < k ? (nc - cj) * (nc - cj) : 0.0);
                cj = nc;
                // an empty cluster keeps its centre and may fall out of order
                const double nx = __shfl_down(cj, 1, 64);
                if (__any(lane + 1 < k && nx < cj)) {
                    if (lane < k) cc[lane] = cj;
                    if (lane == 0)
                        for (int i = 1; i < k; ++i) { const double v = cc[i]; int j = i - 1; while (j >= 0 && cc[j] > v) { cc[j + 1] = cc[j]; --j; } cc[j + 1] = v; }
                    if (lane < k) cj = cc[lane];
                }
                if (shift <= tol) break;
            }
            if (lane < k) cc[lane] = cj;
        }
        __syncthreads();
        // ---- inertia of this run on the histogram ----
        double in = 0.0;
        for (int q = 0; q < PER; ++q) {
            const double p = pts[i0 + q];
            double bd = INFINITY;
            for (int j = 0; j < k; ++j) { const double d = (p - cc[j]) * (p - cc[j]); bd = d < bd ? d : bd; }
            in += (double)wts[i0 + q] * bd;
        }
        in = bkm_bsum(in, tmp);
        if (threadIdx.x == 0) emit(in);
    }
}

// the restart with the lowest histogram inertia (first on ties) seeds the exact passes
__global__ __launch_bounds__(64) void k_bkm_pick(BkmArgs a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.ntensors) return;
    BkmState& S = a.st[t];
    int b = 0;
    for (int r = 1; r < a.n_init; ++r) if (S.cand_in[r] < S.cand_in[b]) b = r;
    bkm_set_centres(S, S.cand[b], a.k);
}

// exact Lloyd statistics: per block, cumulative count / sum / sum of squares
// above each of the KM1 midpoints (+ totals); float per thread, double across.
// The sums are of d = v - pivot of v's cluster (its current centre in
// float32), not of v: d is as small as the cluster is wide, so the float sums
// and k_bkm_update's variance, inertia and centres (pivot + mean of d) lose
// nothing to the tensor's mean or to the distance between clusters.
constexpr int kBkmAccNT = 1024;  // VALU-heavy per element: 16 waves per block
DEVI float bkm_pivot(const BkmState& S, int j) { return (float)S.cen[j]; }
template <int KM1>
__global__ __launch_bounds__(kBkmAccNT) void k_bkm_acc(BkmArgs a) {
    constexpr int NV = KM1 + 1;
    __shared__ double red[kBkmAccNT / 64][3][NV];
    int t; int64_t i0, i1;
    bkm_range(a, t, i0, i1);
    const BkmState& S = a.st[t];
    if (S.converged == 1) return;
    float m[KM1], p[NV];
#pragma unroll
    for (int j = 0; j < KM1; ++j) m[j] = S.mids[j];
#pragma unroll
    for (int j = 0; j < NV; ++j) p[j] = bkm_pivot(S, j);
    // (d, d^2) of an element go into the pair sq[j] by one packed fma with
    // g = 1.0f or 0.0f: the sums a select of d or 0 would give, bit for bit
    // (a thread adds at most kBkmChunk / kBkmAccNT = 64 ones into n: exact)
    typedef float f2 __attribute__((ext_vector_type(2)));
    float n[NV];
    f2 sq[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) { n[j] = 0.f; sq[j] = f2{0.f, 0.f}; }
    visit<kBkmAccNT>(a.x + a.td[t].off, i0, i1, [&](float v, int64_t) {
        float pv = p[0];
#pragma unroll
        for (int j = 0; j < KM1; ++j) pv = v > m[j] ? p[j + 1] : pv;
        const float d = v - pv;
        const f2 e = {d, d * d};
        n[0] += 1.f; sq[0] += e;
#pragma unroll
        for (int j = 0; j < KM1; ++j) {
            const float g = v > m[j] ? 1.f : 0.f;
            n[j + 1] += g;
            sq[j + 1] = __builtin_elementwise_fma(e, f2{g, g}, sq[j + 1]);
        }
    });
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const double dn = wave_sum((double)n[j]), ds = wave_sum((double)sq[j].x), dq = wave_sum((double)sq[j].y);
        if ((threadIdx.x & 63) == 0) { red[w][0][j] = dn; red[w][1][j] = ds; red[w][2][j] = dq; }
    }
    __syncthreads();
    if (threadIdx.x < 3 * NV) {
        const int r = threadIdx.x / NV, j = threadIdx.x % NV;
        double acc = 0.0;
        for (int ww = 0; ww < kBkmAccNT / 64; ++ww) acc += red[ww][r][j];
        a.part[((int64_t)blockIdx.x * 3 + r) * kMaxK + j] = acc;
    }
}

// one wave per tensor: new centres from the partials.  Lane l sums blocks
// l, l+64, ... in order, then a fixed shuffle tree: deterministic.
__global__ __launch_bounds__(64) void k_bkm_update(BkmArgs a) {
    const int t = blockIdx.x;
    BkmState& S = a.st[t];
    if (S.converged == 1) return;
    const BkmTensor T = a.td[t];
    const int k = a.k;
    __shared__ double g[3][kMaxK + 1];
    for (int j = 0; j < k; ++j)
        for (int r = 0; r < 3; ++r) {
            double acc = 0.0;
            for (int b = T.blk0 + (int)threadIdx.x; b < T.blk0 + T.nblk; b += 64)
                acc += a.part[((int64_t)b * 3 + r) * kMaxK + j];
            acc = wave_sum(acc);
            if (threadIdx.x == 0) g[r][j] = acc;
        }
    if (threadIdx.x != 0) return;
    double cg[kMaxK + 1], sg[kMaxK + 1], qg[kMaxK + 1];
    for (int j = 0; j < k; ++j) { cg[j] = g[0][j]; sg[j] = g[1][j]; qg[j] = g[2][j]; }
    cg[k] = 0.0; sg[k] = 0.0; qg[k] = 0.0;
    // cluster j = (mid[j-1], mid[j]]: cumulative differences; Sm and Q are
    // sums of v - pivot[j] (k_bkm_acc)
    double N[kMaxK], Sm[kMaxK], Q[kMaxK], nc[kMaxK];
    double mean = 0.0;
    for (int j = 0; j < k; ++j) {
        N[j] = cg[j] - cg[j + 1];
        Sm[j] = sg[j] - sg[j + 1];
        Q[j] = qg[j] - qg[j + 1];
        nc[j] = N[j] > 0 ? (double)bkm_pivot(S, j) + Sm[j] / N[j] : S.cen[j];
        mean += N[j] * (double)bkm_pivot(S, j) + Sm[j];
    }
    mean /= cg[0];
    // the data's variance about its mean, cluster by cluster
    double var = 0.0;
    for (int j = 0; j < k; ++j) {
        const double e = (double)bkm_pivot(S, j) - mean;
        var += Q[j] + 2 * e * Sm[j] + e * e * N[j];
    }
    var /= cg[0];
    // sort the new centres with their statistics
    for (int i = 1; i < k; ++i) {
        const double v = nc[i], vn = N[i], vs = Sm[i], vq = Q[i];
        int j = i - 1;
        while (j >= 0 && nc[j] > v) { nc[j + 1] = nc[j]; N[j + 1] = N[j]; Sm[j + 1] = Sm[j]; Q[j + 1] = Q[j]; --j; }
        nc[j + 1] = v; N[j + 1] = vn; Sm[j + 1] = vs; Q[j + 1] = vq;
    }
    bool same = true;
    for (int j = 0; j + 1 < k; ++j) same = same && (float)((nc[j] + nc[j + 1]) / 2) == S.mids[j];
    // sklearn's stopping rule: sum of squared centre shifts <= 1e-4 x the
    // data variance; then one more assignment pass with the final centres
    // (converged = 2) so that labels, counts and inertia belong to them
    const double tol = 1e-4 * fmax(var, 0.0);
    double shift = 0.0;
    for (int j = 0; j < k; ++j) shift += (nc[j] - S.cen[j]) * (nc[j] - S.cen[j]);
    const bool pending = S.converged == 2;
    if (!same && !pending && !a.final_pass) {
        bkm_set_centres(S, nc, k);
        if (shift <= tol) S.converged = 2;
        return;
    }
    // final: counts and inertia of the assignment this pass was made with
    double in = 0.0;
    if (same && !pending) {  // strict convergence: centres = means of the unchanged clusters
        for (int j = 0; j < k; ++j) if (N[j] > 0) in += Q[j] - Sm[j] * Sm[j] / N[j];
        bkm_set_centres(S, nc, k);
    } else {  // keep the centres the assignment was made with
        for (int j = 0; j < k; ++j) {  // (statistics above are sorted by new centre: redo by cluster)
            const double c = S.cen[j] - (double)bkm_pivot(S, j);
            N[j] = cg[j] - cg[j + 1]; Sm[j] = sg[j] - sg[j + 1]; Q[j] = qg[j] - qg[j + 1];
            in += Q[j] - 2 * c * Sm[j] + c * c * N[j];
        }
    }
    S.inertia = in > 0 ? in : 0.0;
    // np.unique over the used centres (value dtype) and each cluster's rank
    double vals[kMaxK], uq[kMaxK];
    int nu = 0;
    for (int j = 0; j < k; ++j) {
        vals[j] = a.value_f64 ? S.cen[j] : (double)(float)S.cen[j];
        S.cnt[j] = (long long)(N[j] + 0.5);
    }
    for (int j = 0; j < k; ++j) {
        if (S.cnt[j] <= 0) continue;
        bool dup = false;
        for (int i = 0; i < nu; ++i) dup = dup || uq[i] == vals[j];
        if (!dup) uq[nu++] = vals[j];
    }
    for (int i = 1; i < nu; ++i) { const double v = uq[i]; int j = i - 1; while (j >= 0 && uq[j] > v) { uq[j + 1] = uq[j]; --j; } uq[j + 1] = v; }
    for (int j = 0; j < k; ++j) {
        int r = 0;
        while (r < nu && uq[r] < vals[j]) ++r;
        S.rank[j] = (float)r;
    }
    for (int i = 0; i < kMaxK; ++i) S.uniq[i] = i < nu ? uq[i] : 0.0;
    S.nuniq = nu;
    S.converged = 1;
}

template <int KM1>
__global__ __launch_bounds__(kBkmAccNT) void k_bkm_label(BkmArgs a) {
    int t; int64_t i0, i1;
    bkm_range(a, t, i0, i1);
    const BkmState& S = a.st[t];
    float m[KM1], r[KM1 + 1];
#pragma unroll
    for (int j = 0; j < KM1; ++j) m[j] = S.mids[j];
#pragma unroll
    for (int j = 0; j <= KM1; ++j) r[j] = S.rank[j < a.k ? j : a.k - 1];
    const float* x = a.x + a.td[t].off;
    float* out = a.out + a.td[t].off;
    auto rank_of = [&](float v) {
        float o = r[0];
#pragma unroll
        for (int j = 0; j < KM1; ++j) o = v > m[j] ? r[j + 1] : o;
        return o;
    };
    // x and out share the arena offset, so they are 16-B aligned together:
    // peel to alignment, then 16-B accesses (not the all-or-nothing form of k_lut_batch's map)
    int64_t a4 = i0;
    while (a4 < i1 && (reinterpret_cast<uintptr_t>(x + a4) & 15u)) ++a4;
    for (int64_t i = i0 + threadIdx.x; i < a4; i += kBkmAccNT) out[i] = rank_of(x[i]);
    const int64_t n4 = (i1 - a4) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + a4);
    float4* o4 = reinterpret_cast<float4*>(out + a4);
    for (int64_t i = threadIdx.x; i < n4; i += kBkmAccNT) {
        const float4 v = x4[i];
        o4[i] = make_float4(rank_of(v.x), rank_of(v.y), rank_of(v.z), rank_of(v.w));
    }
    for (int64_t i = a4 + 4 * n4 + threadIdx.x; i < i1; i += kBkmAccNT) out[i] = rank_of(x[i]);
}

static_assert(sizeof(ofl_label_rec) == 80, "lossy.LabelTable.REC_BYTES");
// each tensor's labelling rule as an ofl_label_rec (k <= 8): what k_bkm_label
// applies, for the gzip encoder to apply as it loads the values
// vtab: the same rule with each rank replaced by the float32 value the
// reference's backward decodes it to -- `for key in map: data[data == key] =
// map[key]` (kc_pipeline.py:79-83) with the map {i: uniq[i]} in order, so a
// value equal to a later key is replaced again -- for ofl_label_apply
__global__ __launch_bounds__(64) void k_bkm_tab(BkmArgs a, ofl_label_rec* tab, ofl_label_rec* vtab) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= a.ntensors) return;
    const BkmState& S = a.st[t];
    ofl_label_rec r;
    r.start = a.td[t].off;
    r.end = a.td[t].off + a.td[t].n;
    for (int j = 0; j < 8; ++j) {
        r.mid[j] = j < 7 ? S.mids[j] : INFINITY;
        r.rank[j] = S.rank[j < a.k ? j : a.k - 1];
    }
    if (tab) tab[t] = r;
    if (!vtab) return;
    for (int j = 0; j < 8; ++j) {
        float v = r.rank[j];
        for (int i = 0; i < S.nuniq; ++i) v = v == (float)i ? (float)S.uniq[i] : v;
        r.rank[j] = v;
    }
    vtab[t] = r;
}

// The round end's tail (ofl_label_apply): out = base + value of x's cluster,
// the labelling rule of k_bkm_label (the > chain: a NaN takes cluster 0) on
// value records.  The records live on the device, so the host does not know
// the chunk count: a fixed grid, every workgroup builds the chunk -> tensor
// table of chunk_of (first chunk of every record) in LDS and strides over the
// 2^16-element chunks.  16-B loads and stores over the aligned middle, scalar
// head and tail; the record's 16 floats stay in registers.
constexpr int kLaMaxT = 4096;  // records per launch (the LDS table)
// a record's rule in registers (scalars passed by value: kept in a closure or
// an array they end up in LDS behind a computed index)
struct LaRule { float m0, m1, m2, m3, m4, m5, m6, r0, r1, r2, r3, r4, r5, r6, r7; };
DEVI float la_val(const LaRule q, float v) {
    float o = q.r0;
    o = v > q.m0 ? q.r1 : o;
    o = v > q.m1 ? q.r2 : o;
    o = v > q.m2 ? q.r3 : o;
    o = v > q.m3 ? q.r4 : o;
    o = v > q.m4 ? q.r5 : o;
    o = v > q.m5 ? q.r6 : o;
    o = v > q.m6 ? q.r7 : o;
    return o;
}
// without a base the value itself (0 + v would turn a -0.0 into +0.0)
template <bool BASE>
DEVI float4 la_add(const LaRule q, float4 b, float4 v) {
    const float4 d = make_float4(la_val(q, v.x), la_val(q, v.y), la_val(q, v.z), la_val(q, v.w));
    return BASE ? make_float4(b.x + d.x, b.y + d.y, b.z + d.z, b.w + d.w) : d;
}
template <bool BASE>
DEVI void la_one(const LaRule q, const float* xa, const float* base, float* out, int64_t i) {
    const float d = la_val(q, xa[i]);
    out[i] = BASE ? base[i] + d : d;
}
template <bool BASE>
__global__ __launch_bounds__(kBkmAccNT) void k_label_apply(const float* xa, const ofl_label_rec* __restrict__ recs, int nt,
                                                           const float* base, float* out) {
    __shared__ int32_t first[kLaMaxT + 1];  // first[t] = chunks before record t
    for (int t = threadIdx.x; t < nt; t += kBkmAccNT) {
        const int64_t n = recs[t].end - recs[t].start;
        first[t + 1] = n > 0 ? (int32_t)((n + kBkmChunk - 1) / kBkmChunk) : 0;
    }
    if (threadIdx.x == 0) first[0] = 0;
    __syncthreads();
    if (threadIdx.x < 64) {  // inclusive scan: lane l owns `per` consecutive entries
        const int per = (nt + 63) / 64, lo = 1 + (int)threadIdx.x * per;
        const int hi = lo + per < nt + 1 ? lo + per : nt + 1;
        int32_t s = 0;
        for (int i = lo; i < hi; ++i) s += first[i];
        int32_t inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t u = __shfl_up(inc, o, 64);
            if ((int)threadIdx.x >= o) inc += u;
        }
        int32_t run = inc - s;
        for (int i = lo; i < hi; ++i) { run += first[i]; first[i] = run; }
    }
    __syncthreads();
    const int total = first[nt];
    // x, base and out are indexed alike: 16-B accesses where they are aligned together
    const uintptr_t px = reinterpret_cast<uintptr_t>(xa), po = reinterpret_cast<uintptr_t>(out);
    const bool vec = (((px ^ po) | (BASE ? px ^ reinterpret_cast<uintptr_t>(base) : 0)) & 15u) == 0;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        // (not chunk_of: an LDS table of first chunks, empty records, a wave-uniform result)
        int lo = 0, hi = nt - 1;
        while (lo < hi) {  // last record whose first chunk is <= c (empty records share their successor's)
            const int mid = (lo + hi + 1) >> 1;
            if (first[mid] <= c) lo = mid; else hi = mid - 1;
        }
        const int t = __builtin_amdgcn_readfirstlane(lo);
        const ofl_label_rec* R = recs + t;
        const int64_t rend = R->end;
        const int64_t i0 = R->start + (int64_t)(c - first[t]) * kBkmChunk;
        const int64_t i1 = i0 + kBkmChunk < rend ? i0 + kBkmChunk : rend;
        const LaRule q = {R->mid[0], R->mid[1], R->mid[2], R->mid[3], R->mid[4], R->mid[5], R->mid[6], R->rank[0],
                          R->rank[1], R->rank[2], R->rank[3], R->rank[4], R->rank[5], R->rank[6], R->rank[7]};
        int64_t a4 = i0;
        if (vec) while (a4 < i1 && (reinterpret_cast<uintptr_t>(xa + a4) & 15u)) ++a4; else a4 = i1;
        const int64_t n4 = (i1 - a4) >> 2;
        for (int64_t i = i0 + threadIdx.x; i < a4; i += kBkmAccNT) la_one<BASE>(q, xa, base, out, i);
        for (int64_t i = a4 + 4 * n4 + threadIdx.x; i < i1; i += kBkmAccNT) la_one<BASE>(q, xa, base, out, i);
        const float4* x4 = reinterpret_cast<const float4*>(xa + a4);
        const float4* b4 = reinterpret_cast<const float4*>(BASE ? base + a4 : xa);
        float4* o4 = reinterpret_cast<float4*>(out + a4);
        // two 16-B loads per array in flight per lane (a lane reads its own
        // elements before it writes them: out may alias x or base)
        int64_t i = threadIdx.x;
        for (; i + kBkmAccNT < n4; i += 2 * kBkmAccNT) {
            const float4 v0 = x4[i], v1 = x4[i + kBkmAccNT];
            const float4 b0 = BASE ? b4[i] : z4, b1 = BASE ? b4[i + kBkmAccNT] : z4;
            o4[i] = la_add<BASE>(q, b0, v0);
            o4[i + kBkmAccNT] = la_add<BASE>(q, b1, v1);
        }
        if (i < n4) o4[i] = la_add<BASE>(q, BASE ? b4[i] : z4, x4[i]);
    }
}

// Batched reference backward (kc_pipeline.py:79-83 per tensor): tensor t's
// float32 ranks -> values by the sequential in-place key->value replacement,
// one launch for the whole arena (blocks as in the k-means passes).
struct LutBatchArgs {
    const float* in;
    float* out;
    const BkmTensor* td;
    const int32_t* nk;     // [T]
    const float* keys;     // [T][max_nk]
    const float* vals;     // [T][max_nk]
    int32_t ntensors;
    int32_t max_nk;
};
__global__ __launch_bounds__(kNT) void k_lut_batch(LutBatchArgs a) {
    __shared__ float ks[64], vs[64];
    // (chunk_of written out: through the function the search's add comes out with its operands swapped)
    int lo = 0, hi = a.ntensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.td[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    const BkmTensor T = a.td[t];
    const int nk = a.nk[t];
    if (threadIdx.x < nk) {
        ks[threadIdx.x] = a.keys[(int64_t)t * a.max_nk + threadIdx.x];
        vs[threadIdx.x] = a.vals[(int64_t)t * a.max_nk + threadIdx.x];
    }
    __syncthreads();
    const int64_t i0 = (int64_t)(blockIdx.x - T.blk0) * kBkmChunk;
    const int64_t i1 = i0 + kBkmChunk < T.n ? i0 + kBkmChunk : T.n;
    const float* x = a.in + T.off;
    float* y = a.out + T.off;
    auto lut = [&](float v) {
        for (int j = 0; j < nk; ++j) v = (v == ks[j]) ? vs[j] : v;
        return v;
    };
    // (the map written out: see k_ternary_batch)
    if (((reinterpret_cast<uintptr_t>(x + i0) | reinterpret_cast<uintptr_t>(y + i0)) & 15u) == 0) {
        const int64_t n4 = (i1 - i0) >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x + i0);
        float4* y4 = reinterpret_cast<float4*>(y + i0);
        for (int64_t i = threadIdx.x; i < n4; i += kNT) {
            const float4 v = x4[i];
            y4[i] = make_float4(lut(v.x), lut(v.y), lut(v.z), lut(v.w));
        }
        for (int64_t i = i0 + 4 * n4 + threadIdx.x; i < i1; i += kNT) y[i] = lut(x[i]);
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += kNT) y[i] = lut(x[i]);
    }
}

}  // namespace lossy
