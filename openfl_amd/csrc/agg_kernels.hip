// agg_kernels.hip -- the aggregator's end-of-round arithmetic around the codec
// (reference: /root/reference/openfl):
//   interface/aggregation_functions/weighted_average.py:12-14
//       np.average(tensors, weights=weights, axis=0)
//   pipelines/tensor_codec.py:150-211  generate_delta (new - base),
//                                      apply_delta (base + delta)
//   component/aggregator/aggregator.py:780-865  _prepare_trained: average ->
//       delta -> compress -> decompress -> apply, per tensor
//
// Bit-exact with NumPy: np.average promotes to float64, multiplies every
// collaborator's tensor by its weight (one rounding), sums the products over
// the collaborator axis in order (axis-0 reductions accumulate row by row,
// starting from the first row), divides by the float64 sum of the weights
// (computed on the host with NumPy), then generate_delta subtracts the float32
// base in float64.  FMA contraction is disabled in these kernels so that every
// product and sum is rounded exactly as NumPy rounds it.  The codec then sees
// the delta rounded to float32 (torch.Tensor(float64 array), Eden.compress
// :579); apply_delta is a float32 add of the decoded delta.
//
// All tensors of a model update live in one flat arena; the kernels are
// elementwise over it (16-B vector I/O where the arena is aligned).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>

#include "median_net.h"
#include "ofl_codec.h"

namespace agg {

constexpr int kNT = 256;
constexpr int kMaxC = 16;  // collaborators per launch (more: chained through agg)

// ---- what the kernels below share ---------------------------------------------

// s + term(c0) + ... + term(n - 1), left to right and rounded after every
// operation: the sequence NumPy performs over the collaborator axis
template <class F>
__device__ __forceinline__ double add_in_order(double s, int c0, int n, F term) {
#pragma clang fp contract(off)
    for (int c = c0; c < n; ++c) s = s + term(c);
    return s;
}

// NumPy's pairwise sum of p(c0) .. p(c0 + n - 1), the order in which it
// reduces a 1-D array (numpy/_core/src/umath/loops_utils.h.src: < 8 terms
// summed from +0.0; up to 128 with eight accumulators combined
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) then the tail; larger blocks split in
// halves rounded down to a multiple of 8).  np_pairwise_block is the part
// for n <= 128, which does not recurse.
template <class F>
__device__ __forceinline__ double np_pairwise_block(F p, int c0, int n) {
#pragma clang fp contract(off)
    if (n < 8) {
        double r = 0.0;
        for (int k = 0; k < n; ++k) r = r + p(c0 + k);
        return r;
    }
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = p(c0 + k);
    int k = 8;
    for (; k < n - (n % 8); k += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + p(c0 + k + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; k < n; ++k) res = res + p(c0 + k);
    return res;
}
template <class F>
__device__ double np_pairwise(F p, int c0, int n) {
#pragma clang fp contract(off)
    if (n <= 128) return np_pairwise_block(p, c0, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise(p, c0, n2) + np_pairwise(p, c0 + n2, n - n2);
}

// where an average goes: the aggregate and generate_delta's outputs
struct DeltaOut {
    const float* base;  // nullable: delta = average when absent
    double* agg;        // nullable unless chained: running float64 sums / average
    double* delta64;    // nullable
    float* delta32;     // nullable
    __device__ __forceinline__ double delta(int64_t i, double avg) const {
#pragma clang fp contract(off)
        return base ? avg - (double)base[i] : avg;
    }
    __device__ __forceinline__ void put(int64_t i, double avg) const {
        const double d = delta(i, avg);
        if (agg) agg[i] = avg;
        if (delta64) delta64[i] = d;
        if (delta32) delta32[i] = (float)d;
    }
};

// listed element ranges of an arena, packed back to back
struct Ranges {
    const int64_t* start;  // device [nr]
    const int64_t* dst;    // device [nr + 1] exclusive prefix of the counts
    int nr;
    __device__ __forceinline__ int64_t total() const { return dst[nr]; }
    // packed index j -> its range; i: the arena element
    __device__ __forceinline__ int find(int64_t j, int64_t& i) const {
        int lo = 0, hi = nr - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (dst[mid] <= j) lo = mid; else hi = mid - 1;
        }
        i = start[lo] + (j - dst[lo]);
        return lo;
    }
};

// s + v[0] + v[STRIDE] + ... (m values staged in LDS), left to right: the
// dependent add chain that one lane runs, loads issued eight ahead of the adds
template <typename T, int STRIDE>
__device__ __forceinline__ T lds_chain(T s, const T* v, int m) {
#pragma clang fp contract(off)
    int k = 0;
    for (; k + 8 <= m; k += 8) {
        T t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = v[(k + q) * STRIDE];
#pragma unroll
        for (int q = 0; q < 8; ++q) s = s + t[q];
    }
    for (; k < m; ++k) s = s + v[k * STRIDE];
    return s;
}

// an elementwise kernel's body: quad(i) on 4 consecutive elements per thread
// while the arenas are 16-B aligned (vec), elem(i) on the tail; grid-stride
template <class Q, class E>
__device__ __forceinline__ void quads_then_tail(int64_t n, int vec, Q quad, E elem) {
    const int64_t stride = (int64_t)gridDim.x * kNT;
    const int64_t t0 = (int64_t)blockIdx.x * kNT + threadIdx.x;
    int64_t tail = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t q = t0; q < n4; q += stride) quad(4 * q);
        tail = 4 * n4;
    }
    for (int64_t i = tail + t0; i < n; i += stride) elem(i);
}

// ---- WeightedAverage ------------------------------------------------------------

struct WavgArgs {
    const float* x[kMaxC];
    double w[kMaxC];
    int nc;            // collaborators in this launch
    int first, last;   // first launch starts from the first product; last divides
    double wsum;       // float64 sum of all weights (NumPy's)
    DeltaOut o;
    int64_t n;
};

// running sum over this launch's collaborators, continuing from s0 (first
// launch: from the first product)
__device__ __forceinline__ double wavg_sum(const WavgArgs& a, int64_t i, double s0) {
#pragma clang fp contract(off)
    auto term = [&](int c) { return (double)a.x[c][i] * a.w[c]; };
    return add_in_order(a.first ? term(0) : s0, a.first ? 1 : 0, a.nc, term);
}

__device__ __forceinline__ void wavg_elem(const WavgArgs& a, int64_t i) {
#pragma clang fp contract(off)
    const double s = wavg_sum(a, i, a.first ? 0.0 : a.o.agg[i]);
    if (!a.last) { a.o.agg[i] = s; return; }
    a.o.put(i, s / a.wsum);
}

// 4 consecutive elements per thread: 16-B loads of every collaborator's
// tensor (the kernel reads 4 C + 4 bytes and writes 4 per element)
__device__ __forceinline__ void wavg_quad(const WavgArgs& a, int64_t i) {
#pragma clang fp contract(off)
    double s[4];
    if (a.first) {
        const float4 v = *reinterpret_cast<const float4*>(a.x[0] + i);
        s[0] = (double)v.x * a.w[0]; s[1] = (double)v.y * a.w[0];
        s[2] = (double)v.z * a.w[0]; s[3] = (double)v.w * a.w[0];
    } else {
        for (int k = 0; k < 4; ++k) s[k] = a.o.agg[i + k];
    }
    for (int c = a.first ? 1 : 0; c < a.nc; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(a.x[c] + i);
        const double w = a.w[c];
        s[0] = s[0] + (double)v.x * w; s[1] = s[1] + (double)v.y * w;
        s[2] = s[2] + (double)v.z * w; s[3] = s[3] + (double)v.w * w;
    }
    if (!a.last) {
        for (int k = 0; k < 4; ++k) a.o.agg[i + k] = s[k];
        return;
    }
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.o.base) b = *reinterpret_cast<const float4*>(a.o.base + i);
    const float bb[4] = {b.x, b.y, b.z, b.w};
    double d[4];
    for (int k = 0; k < 4; ++k) {
        const double avg = s[k] / a.wsum;
        if (a.o.agg) a.o.agg[i + k] = avg;
        d[k] = a.o.base ? avg - (double)bb[k] : avg;
    }
    if (a.o.delta64)
        for (int k = 0; k < 4; ++k) a.o.delta64[i + k] = d[k];
    if (a.o.delta32) *reinterpret_cast<float4*>(a.o.delta32 + i) = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
}

__global__ __launch_bounds__(kNT) void k_wavg_delta(WavgArgs a, int vec) {
    quads_then_tail(a.n, vec, [&](int64_t i) { wavg_quad(a, i); }, [&](int64_t i) { wavg_elem(a, i); });
}

// The streaming form of the same average: one collaborator per launch into a
// float64 sums arena, then one pass that divides and takes the delta.  The
// sequence of roundings per element is k_wavg_delta's: the first product is
// stored as it is (a -0.0 product stays -0.0, as wavg_sum keeps it; adding it
// to +0.0 would not),
// every later one is added to the running sum, the last pass divides by wsum.
// k_wavg_accumulate reads 4 + 8 and writes 8 bytes per element (first: no
// read of the sums), k_wavg_finish reads 8 + 4 and writes 8 + 4 (+ 8 with
// delta64).
struct AccArgs {
    const float* x;
    double w;
    int first;     // store the product instead of adding it
    double* sums;
    int64_t n;
};

__device__ __forceinline__ void acc_elem(const AccArgs& a, int64_t i) {
#pragma clang fp contract(off)
    const double p = (double)a.x[i] * a.w;
    a.sums[i] = a.first ? p : a.sums[i] + p;
}

// 4 consecutive elements per thread: one 16-B load of x, the sums as two
// 16-B pairs each way
__device__ __forceinline__ void acc_quad(const AccArgs& a, int64_t i) {
#pragma clang fp contract(off)
    const float4 v = *reinterpret_cast<const float4*>(a.x + i);
    double2* s2 = reinterpret_cast<double2*>(a.sums + i);
    double2 lo, hi;
    lo.x = (double)v.x * a.w; lo.y = (double)v.y * a.w;
    hi.x = (double)v.z * a.w; hi.y = (double)v.w * a.w;
    if (!a.first) {
        const double2 p = s2[0], q = s2[1];
        lo.x = p.x + lo.x; lo.y = p.y + lo.y;
        hi.x = q.x + hi.x; hi.y = q.y + hi.y;
    }
    s2[0] = lo;
    s2[1] = hi;
}

__global__ __launch_bounds__(kNT) void k_wavg_accumulate(AccArgs a, int vec) {
    quads_then_tail(a.n, vec, [&](int64_t i) { acc_quad(a, i); }, [&](int64_t i) { acc_elem(a, i); });
}

struct FinishArgs {
    double wsum;
    DeltaOut o;    // o.agg: the sums, divided in place
    int64_t n;
};

__device__ __forceinline__ void finish_elem(const FinishArgs& a, int64_t i) {
#pragma clang fp contract(off)
    a.o.put(i, a.o.agg[i] / a.wsum);
}

__device__ __forceinline__ void finish_quad(const FinishArgs& a, int64_t i) {
#pragma clang fp contract(off)
    double2* s2 = reinterpret_cast<double2*>(a.o.agg + i);
    double2 lo = s2[0], hi = s2[1];
    lo.x = lo.x / a.wsum; lo.y = lo.y / a.wsum;
    hi.x = hi.x / a.wsum; hi.y = hi.y / a.wsum;
    s2[0] = lo;
    s2[1] = hi;
    if (!a.o.delta64 && !a.o.delta32) return;
    if (a.o.base) {  // DeltaOut::delta on the four
        const float4 b = *reinterpret_cast<const float4*>(a.o.base + i);
        lo.x = lo.x - (double)b.x; lo.y = lo.y - (double)b.y;
        hi.x = hi.x - (double)b.z; hi.y = hi.y - (double)b.w;
    }
    if (a.o.delta64) {
        double2* d2 = reinterpret_cast<double2*>(a.o.delta64 + i);
        d2[0] = lo;
        d2[1] = hi;
    }
    if (a.o.delta32)
        *reinterpret_cast<float4*>(a.o.delta32 + i) = make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
}

__global__ __launch_bounds__(kNT) void k_wavg_finish(FinishArgs a, int vec) {
    quads_then_tail(a.n, vec, [&](int64_t i) { finish_quad(a, i); }, [&](int64_t i) { finish_elem(a, i); });
}

// Single-element tensors: NumPy reduces a (C, 1) stack as a 1-D array, i.e.
// np_pairwise of all C products.
struct PointArgs {
    const float* const* x;  // device [nc]
    const double* w;        // device [nc]
    int nc;
    double wsum;
    DeltaOut o;
    const int64_t* idx;     // device [np]
    int np;
};
__device__ __forceinline__ auto point_term(const PointArgs& a, int64_t i) {
#pragma clang fp contract(off)
    return [&a, i](int c) { return (double)a.x[c][i] * a.w[c]; };
}
__global__ __launch_bounds__(64) void k_wavg_points(PointArgs a) {
#pragma clang fp contract(off)
    for (int j = blockIdx.x * 64 + threadIdx.x; j < a.np; j += gridDim.x * 64) {
        const int64_t i = a.idx[j];
        a.o.put(i, np_pairwise(point_term(a, i), 0, a.nc) / a.wsum);
    }
}

// the float64 delta on listed element ranges, packed into out: the values
// the Eden seed's serial sums read (one range per tensor; single-element
// tensors use the pairwise order)
struct RangeArgs {
    PointArgs p;
    Ranges rg;
    const int32_t* single;  // device [rg.nr]
};
__global__ __launch_bounds__(kNT) void k_wavg_ranges(RangeArgs r, double* out) {
#pragma clang fp contract(off)
    const int64_t total = r.rg.total();
    for (int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x; j < total; j += (int64_t)gridDim.x * kNT) {
        int64_t i;
        const int t = r.rg.find(j, i);
        const auto term = point_term(r.p, i);
        const double s = r.single[t] ? np_pairwise(term, 0, r.p.nc) : add_in_order(term(0), 1, r.p.nc, term);
        out[j] = r.p.o.delta(i, s / r.p.wsum);
    }
}

// serial sum of each packed range, left to right like Python's sum() over
// NumPy scalars: one 256-thread block per range stages 2048 values at a
// time in LDS, then one lane runs the dependent add chain from LDS
// (lds_chain).  For float32 values the chain is a float32 add per element
// (sum() over np.float32 scalars); the sum is stored widened
template <typename T>
__global__ __launch_bounds__(256) void k_range_sums(const T* packed, const int64_t* dst, double* sums) {
    __shared__ T v[2048];
    const int r = blockIdx.x;
    const int64_t j0 = dst[r], j1 = dst[r + 1];
    T s = 0;
    for (int64_t c0 = j0; c0 < j1; c0 += 2048) {
        const int m = (int)(j1 - c0 < 2048 ? j1 - c0 : 2048);
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += 256) v[k] = packed[c0 + k];
        __syncthreads();
        if (threadIdx.x == 0) s = lds_chain<T, 1>(s, v, m);
    }
    if (threadIdx.x == 0) sums[r] = (double)s;
}

// CPython's hash of a finite float (Objects/object.c _Py_HashDouble, modulus
// 2^61 - 1): the 28-bit chunks of the mantissa folded with a rotation, then the
// exponent as a rotation, the sign, and -1 -> -2.  inf -> +-314159; NaN (an
// object-id hash in CPython >= 3.10, not reproducible) -> 0.
__device__ int64_t py_hash_double(double v) {
    const uint64_t MOD = (1ull << 61) - 1ull;
    if (isinf(v)) return v > 0 ? 314159 : -314159;
    if (isnan(v)) return 0;
    int e;
    double m = frexp(v, &e);
    int sign = 1;
    if (m < 0) { sign = -1; m = -m; }
    uint64_t x = 0;
    while (m != 0.0) {
        x = ((x << 28) & MOD) | x >> (61 - 28);
        m *= 268435456.0;
        e -= 28;
        const uint64_t y = (uint64_t)m;
        m -= (double)y;
        x += y;
        if (x >= MOD) x -= MOD;
    }
    e = e >= 0 ? e % 61 : 61 - 1 - ((-1 - e) % 61);
    x = ((x << e) & MOD) | x >> (61 - e);
    x = x * (uint64_t)(int64_t)sign;
    if (x == ~0ull) x = ~0ull - 1ull;
    return (int64_t)x;
}
// the Eden seed of each tensor from its serial sum and its np.random draw
// (eden_pipeline.py:771-772): (hash(sum * 13 + 7) + draw) % 2^16.  T is the
// type the sum was formed in: NumPy >= 2 scalar promotion keeps
// np.float32(sum) * 13 + 7 in float32 (two roundings); hash() of a np.float32
// is the hash of its value as a Python float
template <typename T>
__global__ __launch_bounds__(64) void k_seeds(const double* sums, const int64_t* draws, int n, uint32_t* seeds) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    T t = (T)sums[i] * (T)13;
    t = t + (T)7;
    const int64_t h = py_hash_double((double)t) + draws[i];
    seeds[i] = (uint32_t)(((h % 65536) + 65536) % 65536);
}

// apply_delta: out = base + delta (float32)
__global__ __launch_bounds__(kNT) void k_apply(const float* base, const float* delta, int64_t n, float* out) {
    const int64_t stride = (int64_t)gridDim.x * kNT;
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(delta) |
                         reinterpret_cast<uintptr_t>(out)) & 15u) ? 0 : n >> 2;
    const float4* b4 = reinterpret_cast<const float4*>(base);
    const float4* d4 = reinterpret_cast<const float4*>(delta);
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n4; i += stride) {
        const float4 b = b4[i], d = d4[i];
        o4[i] = make_float4(b.x + d.x, b.y + d.y, b.z + d.z, b.w + d.w);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += stride) out[i] = base[i] + delta[i];
}

// RandomShiftTransformer.backward with wire metadata (random_shift_pipeline.py:
// 45-68): data (float32) - shift (float64) in float64, as NumPy promotes
__global__ __launch_bounds__(kNT) void k_unshift64(const float* data, const double* shift, int64_t n, double* out) {
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT)
        out[i] = (double)data[i] - shift[i];
}

// apply_delta on listed ranges (device tables): the tensors the codec does
// not touch when the decode itself adds the base (ofl_eden_decode_add)
__global__ __launch_bounds__(kNT) void k_apply_ranges(const float* base, const float* delta, float* out, Ranges rg) {
    const int64_t total = rg.total();
    for (int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x; j < total; j += (int64_t)gridDim.x * kNT) {
        int64_t i;
        rg.find(j, i);
        out[i] = base[i] + delta[i];
    }
}

// the float32 delta (as k_wavg_delta writes it) on listed ranges only: the
// elements the fused round-end encode does not compute itself
// (ofl_eden_encode_wavg: slices of <= 2^15 elements and the tensors the codec
// does not touch)
__global__ __launch_bounds__(kNT) void k_wavg_delta32_ranges(WavgArgs a, Ranges rg) {
#pragma clang fp contract(off)
    const int64_t total = rg.total();
    for (int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x; j < total; j += (int64_t)gridDim.x * kNT) {
        int64_t i;
        rg.find(j, i);
        a.o.delta32[i] = (float)a.o.delta(i, wavg_sum(a, i, 0.0) / a.wsum);
    }
}

__global__ __launch_bounds__(64) void k_py_hash(const double* v, int n, int64_t* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = py_hash_double(v[i]);
}

}  // namespace agg

namespace {
thread_local std::string g_aerr;
int afail(int code, const std::string& m) { g_aerr = m; return code; }
#define AHIP(x)                                                                                        \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess) return afail(OFL_EHIP, std::string(#x " failed: ") + hipGetErrorString(e_)); \
    } while (0)

int cu_count() {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}

int grid_for(int64_t n, int per_thread) {
    const int64_t want = (n + (int64_t)agg::kNT * per_thread - 1) / ((int64_t)agg::kNT * per_thread);
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cu_count() * 16));
}

// an entry point's collaborator table (weights: xs again where it takes
// none): at least one tensor, none of them null
int check_collabs(const std::string& who, int ncollab, const float* const* xs, const void* weights) {
    if (ncollab < 1 || !xs || !weights) return afail(OFL_EINVAL, who + ": need at least one collaborator");
    for (int c = 0; c < ncollab; ++c)
        if (!xs[c]) return afail(OFL_EINVAL, who + ": null collaborator tensor");
    return OFL_OK;
}

// the first nc collaborators' slots of a kernel's argument struct
template <class A, class W>
void fill_args(A& a, const float* const* xs, const W* weights, int nc) {
    for (int c = 0; c < nc; ++c) {
        a.x[c] = xs[c];
        a.w[c] = weights[c];
    }
}

// 1 where the vector path may run: the nc collaborator tensors and every
// other arena a kernel touches (null: absent) are 16-B aligned
template <class... P>
int aligned16(const float* const* xs, int nc, const P*... arenas) {
    uintptr_t al = (reinterpret_cast<uintptr_t>(arenas) | ... | uintptr_t{0});
    for (int c = 0; c < nc; ++c) al |= reinterpret_cast<uintptr_t>(xs[c]);
    return (al & 15u) ? 0 : 1;
}

// the seeds of nranges packed ranges: their serial sums, then hash and draw
template <typename T>
void launch_sums_seeds(const T* packed, const int64_t* dst, int nranges, const int64_t* draws, uint32_t* seeds,
                       double* sums, hipStream_t st) {
    hipLaunchKernelGGL(agg::k_range_sums<T>, dim3(nranges), dim3(256), 0, st, packed, dst, sums);
    hipLaunchKernelGGL(agg::k_seeds<T>, dim3((nranges + 63) / 64), dim3(64), 0, st, sums, draws, nranges, seeds);
}
}  // namespace

extern "C" {

const char* ofl_agg_last_error(void) { return g_aerr.c_str(); }

int ofl_wavg_delta(int ncollab, const float* const* xs, const double* weights, double wsum, const float* base,
                   int64_t n, double* agg_out, double* delta64_out, float* delta32_out, void* stream) {
    if (int rc = check_collabs("wavg", ncollab, xs, weights)) return rc;
    if (n < 0) return afail(OFL_EINVAL, "wavg: negative size");
    if (ncollab > agg::kMaxC && !agg_out)
        return afail(OFL_EINVAL, "wavg: more than 16 collaborators need agg_out (running sums)");
    if (n == 0) return OFL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int g = grid_for(n, 4);
    agg::WavgArgs a{};
    a.wsum = wsum;
    a.n = n;
    for (int c0 = 0; c0 < ncollab; c0 += agg::kMaxC) {
        a.nc = std::min(agg::kMaxC, ncollab - c0);
        fill_args(a, xs + c0, weights + c0, a.nc);
        a.first = c0 == 0;
        a.last = c0 + a.nc == ncollab;
        a.o = {base, agg_out, a.last ? delta64_out : nullptr, a.last ? delta32_out : nullptr};
        const int vec = aligned16(a.x, a.nc, a.o.base, a.o.delta32, a.o.agg, a.o.delta64);
        hipLaunchKernelGGL(agg::k_wavg_delta, dim3(g), dim3(agg::kNT), 0, st, a, vec);
        AHIP(hipGetLastError());
    }
    return OFL_OK;
}

int ofl_wavg_accumulate(const float* x, double w, int first, int64_t n, double* sums, void* stream) {
    if (n < 0 || (n && (!x || !sums))) return afail(OFL_EINVAL, "wavg_accumulate: bad arguments");
    if (n == 0) return OFL_OK;
    agg::AccArgs a{x, w, first ? 1 : 0, sums, n};
    const int vec = aligned16(&x, 1, sums);
    hipLaunchKernelGGL(agg::k_wavg_accumulate, dim3(grid_for(n, 4)), dim3(agg::kNT), 0,
                       static_cast<hipStream_t>(stream), a, vec);
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_wavg_finish(double* sums, double wsum, const float* base, int64_t n, double* delta64_out, float* delta32_out,
                    void* stream) {
    if (n < 0 || (n && !sums)) return afail(OFL_EINVAL, "wavg_finish: bad arguments");
    if (delta64_out && delta64_out == sums) return afail(OFL_EINVAL, "wavg_finish: delta64_out must not be the sums");
    if (n == 0) return OFL_OK;
    agg::FinishArgs a{};
    a.wsum = wsum;
    a.o = {base, sums, delta64_out, delta32_out};
    a.n = n;
    const int vec = aligned16(&base, 0, base, sums, delta64_out, delta32_out);
    hipLaunchKernelGGL(agg::k_wavg_finish, dim3(grid_for(n, 4)), dim3(agg::kNT), 0, static_cast<hipStream_t>(stream),
                       a, vec);
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_wavg_delta_seeds(int ncollab, const float* const* xs_dev, const double* weights_dev, double wsum,
                         const float* base, int nranges, const int64_t* starts_dev, const int64_t* dst_dev,
                         const int32_t* single_dev, int64_t total, const int64_t* draws_dev, uint32_t* seeds_dev,
                         double* sums_dev, double* packed_dev, void* stream) {
    if (ncollab < 1 || ncollab > 2048 || nranges < 1) return afail(OFL_EINVAL, "wavg seeds: bad sizes");
    if (!xs_dev || !weights_dev || !starts_dev || !dst_dev || !single_dev || !draws_dev || !seeds_dev || !sums_dev ||
        (total > 0 && !packed_dev))
        return afail(OFL_EINVAL, "wavg seeds: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    agg::RangeArgs r{};
    r.p.x = xs_dev;
    r.p.w = weights_dev;
    r.p.nc = ncollab;
    r.p.wsum = wsum;
    r.p.o.base = base;
    r.rg = {starts_dev, dst_dev, nranges};
    r.single = single_dev;
    if (total > 0) hipLaunchKernelGGL(agg::k_wavg_ranges, dim3(grid_for(total, 1)), dim3(agg::kNT), 0, st, r, packed_dev);
    launch_sums_seeds<double>(packed_dev, dst_dev, nranges, draws_dev, seeds_dev, sums_dev, st);
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_py_hash_doubles(const double* v_dev, int n, int64_t* out_dev, void* stream) {
    if (n <= 0) return OFL_OK;
    hipLaunchKernelGGL(agg::k_py_hash, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), v_dev, n,
                       out_dev);
    AHIP(hipGetLastError());
    return OFL_OK;
}

size_t ofl_wavg_points_workspace_bytes(int ncollab, int npoints) {
    return 16 * (size_t)std::max(ncollab, 1) + 8 * (size_t)std::max(npoints, 1) + 512;
}

int ofl_wavg_delta_points(int ncollab, const float* const* xs, const double* weights, double wsum, const float* base,
                          int npoints, const int64_t* idx, double* agg_out, double* delta64_out, float* delta32_out,
                          void* ws, size_t ws_bytes, void* stream) {
    if (ncollab < 1 || ncollab > 2048 || !xs || !weights)
        return afail(OFL_EINVAL, "wavg points: 1 <= collaborators <= 2048");
    if (npoints < 1) return OFL_OK;
    if (!idx || !ws || ws_bytes < ofl_wavg_points_workspace_bytes(ncollab, npoints))
        return afail(OFL_ESPACE, "wavg points: workspace too small");
    std::string host(16 * (size_t)ncollab + 8 * (size_t)npoints, '\0');
    memcpy(host.data(), xs, 8 * (size_t)ncollab);
    memcpy(host.data() + 8 * (size_t)ncollab, weights, 8 * (size_t)ncollab);
    memcpy(host.data() + 16 * (size_t)ncollab, idx, 8 * (size_t)npoints);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    AHIP(hipMemcpyAsync(w, host.data(), host.size(), hipMemcpyHostToDevice, st));
    agg::PointArgs a{};
    a.x = reinterpret_cast<const float* const*>(w);
    a.w = reinterpret_cast<const double*>(w + 8 * (size_t)ncollab);
    a.idx = reinterpret_cast<const int64_t*>(w + 16 * (size_t)ncollab);
    a.nc = ncollab;
    a.wsum = wsum;
    a.np = npoints;
    a.o = {base, agg_out, delta64_out, delta32_out};
    hipLaunchKernelGGL(agg::k_wavg_points, dim3((npoints + 63) / 64), dim3(64), 0, st, a);
    AHIP(hipGetLastError());
    AHIP(hipStreamSynchronize(st));  // the staging string must outlive the copy
    return OFL_OK;
}

int ofl_apply_delta(const float* base, const float* delta, int64_t n, float* out, void* stream) {
    if (n < 0 || (n && (!base || !delta || !out))) return afail(OFL_EINVAL, "apply_delta: bad arguments");
    if (n == 0) return OFL_OK;
    hipLaunchKernelGGL(agg::k_apply, dim3(grid_for(n, 16)), dim3(agg::kNT), 0, static_cast<hipStream_t>(stream), base,
                       delta, n, out);
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_sub_f32_f64(const float* data, const double* shift, int64_t n, double* out, void* stream) {
    if (n < 0 || (n && (!data || !shift || !out))) return afail(OFL_EINVAL, "sub_f32_f64: bad arguments");
    if (n == 0) return OFL_OK;
    hipLaunchKernelGGL(agg::k_unshift64, dim3(grid_for(n, 16)), dim3(agg::kNT), 0, static_cast<hipStream_t>(stream),
                       data, shift, n, out);
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_wavg_delta32_ranges(int ncollab, const float* const* xs, const double* weights, double wsum,
                            const float* base, int nranges, const int64_t* starts, const int64_t* dst, int64_t total,
                            float* delta32_out, void* stream) {
    if (nranges < 1 || total <= 0) return OFL_OK;
    if (ncollab > agg::kMaxC) return afail(OFL_EINVAL, "wavg_delta32_ranges: at most 16 collaborators");
    if (!starts || !dst || !delta32_out) return afail(OFL_EINVAL, "wavg_delta32_ranges: bad arguments");
    if (int rc = check_collabs("wavg", ncollab, xs, weights)) return rc;
    agg::WavgArgs a{};
    a.wsum = wsum;
    a.n = total;
    a.nc = ncollab;
    fill_args(a, xs, weights, ncollab);
    a.first = 1;
    a.last = 1;
    a.o = {base, nullptr, nullptr, delta32_out};
    hipLaunchKernelGGL(agg::k_wavg_delta32_ranges, dim3(grid_for(total, 1)), dim3(agg::kNT), 0,
                       static_cast<hipStream_t>(stream), a, agg::Ranges{starts, dst, nranges});
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_apply_delta_ranges(const float* base, const float* delta, float* out, int nranges, const int64_t* starts,
                           const int64_t* dst, int64_t total, void* stream) {
    if (nranges < 1 || total <= 0) return OFL_OK;
    if (!base || !delta || !out || !starts || !dst) return afail(OFL_EINVAL, "apply_delta_ranges: bad arguments");
    hipLaunchKernelGGL(agg::k_apply_ranges, dim3(grid_for(total, 1)), dim3(agg::kNT), 0,
                       static_cast<hipStream_t>(stream), base, delta, out, agg::Ranges{starts, dst, nranges});
    AHIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"

// ---- robust aggregators: Median and GeometricMedian ---------------------------
// (reference: interface/aggregation_functions/median.py:48-49,
//  geometric_median.py:27-56)

namespace agg {

constexpr int kMedMaxC = 128;  // the LDS path's column height
constexpr int kMedLdsNT = 64;  // its block: 128 x 64 floats = 32 KiB of LDS

// a table of N collaborators carries its runtime count only when it is longer
// than kMaxC: up to kMaxC the kernels are instantiated per count, and the
// argument structs keep the size they have without the field
struct NoCount {};
template <int N>
using TableCount = std::conditional_t<(N > kMaxC), int, NoCount>;

template <int N>
struct MedArgs {
    const float* x[N];
    const float* base;  // nullable: delta = median when absent
    float* med;         // nullable
    float* delta;       // nullable: median - base, a float32 subtract
    int64_t n;
    [[no_unique_address]] TableCount<N> nc;
};
static_assert(sizeof(MedArgs<kMaxC>) == 8 * kMaxC + 32);

template <int C>
__device__ __forceinline__ void med_elem(const MedArgs<kMaxC>& a, int64_t i) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = a.x[c][i];
    const float m = mednet::median_of<C>(v);
    if (a.med) a.med[i] = m;
    if (a.delta) a.delta[i] = a.base ? m - a.base[i] : m;
}

// 4 consecutive elements per thread, 16-B loads of every collaborator's arena
// (the kernel reads 4 C + 4 bytes and writes 4 to 8 per element)
template <int C>
__device__ __forceinline__ void med_quad(const MedArgs<kMaxC>& a, int64_t i) {
    float4 q[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = *reinterpret_cast<const float4*>(a.x[c] + i);
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = q[c].x;
    const float m0 = mednet::median_of<C>(v);
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = q[c].y;
    const float m1 = mednet::median_of<C>(v);
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = q[c].z;
    const float m2 = mednet::median_of<C>(v);
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = q[c].w;
    const float m3 = mednet::median_of<C>(v);
    if (a.med) *reinterpret_cast<float4*>(a.med + i) = make_float4(m0, m1, m2, m3);
    if (a.delta) {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.base) b = *reinterpret_cast<const float4*>(a.base + i);
        *reinterpret_cast<float4*>(a.delta + i) =
            a.base ? make_float4(m0 - b.x, m1 - b.y, m2 - b.z, m3 - b.w) : make_float4(m0, m1, m2, m3);
    }
}

template <int C>
__global__ __launch_bounds__(kNT) void k_median(MedArgs<kMaxC> a, int vec) {
    quads_then_tail(a.n, vec, [&](int64_t i) { med_quad<C>(a, i); }, [&](int64_t i) { med_elem<C>(a, i); });
}

// 17..128 collaborators: every thread insertion-sorts its column in LDS, laid
// out [c][thread] so the lanes of a wave hit distinct banks
__global__ __launch_bounds__(kMedLdsNT) void k_median_lds(MedArgs<kMedMaxC> a) {
    __shared__ float col[kMedMaxC][kMedLdsNT];
    const int tid = threadIdx.x;
    for (int64_t i = (int64_t)blockIdx.x * kMedLdsNT + tid; i < a.n; i += (int64_t)gridDim.x * kMedLdsNT) {
        bool nan = false;
        for (int c = 0; c < a.nc; ++c) {
            const float x = a.x[c][i];
            nan |= x != x;
            int j = c;
            while (j > 0 && col[j - 1][tid] > x) {
                col[j][tid] = col[j - 1][tid];
                --j;
            }
            col[j][tid] = x;
        }
        float m = col[a.nc / 2][tid];
        if (!(a.nc & 1)) m = (col[a.nc / 2 - 1][tid] + m) * 0.5f;
        if (nan) m = NAN;
        if (a.med) a.med[i] = m;
        if (a.delta) a.delta[i] = a.base ? m - a.base[i] : m;
    }
}

// Weiszfeld's algorithm per tensor of an arena.  State per tensor t (device,
// float64): the weight row W[t][16], its in-order sum wsum[t] (np.average's
// denominator), the distances d[t][16], the objective, a done flag and the
// rounds run.  The current median m = (sum_c x_c W[t][c]) / wsum[t] is formed
// on the fly wherever it is needed, never stored between passes.
struct GmArgs {
    const float* x[kMaxC];
    int nc;
    const ofl_gm_chunk* chunks;  // [nchunks] (arena start, length <= 4096, tensor)
    int nchunks;
    const int32_t* tchunk0;      // [nt + 1] first chunk of every tensor
    int nt;
    double* W;        // [nt][16]
    double* wsum;     // [nt]
    double* obj;      // [nt]
    int32_t* done;    // [nt]
    int32_t* iters;   // [nt]
    double* partial;  // [nchunks][16] squared distances of one chunk
    double eps, ftol;
    DeltaOut o;
};
struct GmW0 {
    double w[kMaxC];
};

__global__ __launch_bounds__(64) void k_gm_init(GmArgs a, GmW0 w0) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nt) return;
    double s = 0.0;
    for (int c = 0; c < a.nc; ++c) {
        a.W[t * kMaxC + c] = w0.w[c];
        s = c ? s + w0.w[c] : w0.w[c];
    }
    a.wsum[t] = s;
    a.obj[t] = 0.0;
    a.done[t] = 0;
    a.iters[t] = 0;
}

template <int C>
__device__ __forceinline__ double gm_point(const GmArgs& a, const double (&w)[C], double wsum, int64_t i,
                                           float (&x)[C]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = a.x[c][i];
    return add_in_order((double)x[0] * w[0], 1, C, [&](int c) { return (double)x[c] * w[c]; }) / wsum;
}

// squared distances of every collaborator to the current median, one block per
// chunk; a finished tensor's chunks are skipped
template <int C>
__global__ __launch_bounds__(kNT) void k_gm_dist(GmArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[kNT / 64][kMaxC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
        const ofl_gm_chunk k = a.chunks[ch];
        if (a.done[k.tensor]) continue;
        double w[C], acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            w[c] = a.W[k.tensor * kMaxC + c];
            acc[c] = 0.0;
        }
        const double wsum = a.wsum[k.tensor];
        for (int e = tid; e < k.len; e += kNT) {
            float x[C];
            const double m = gm_point<C>(a, w, wsum, k.start + e, x);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double r = m - (double)x[c];
                acc[c] = acc[c] + r * r;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double s = acc[c];
            for (int off = 32; off; off >>= 1) s = s + __shfl_down(s, off);
            if (lane == 0) red[wave][c] = s;
        }
        __syncthreads();
        if (tid < C) a.partial[(int64_t)ch * kMaxC + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        __syncthreads();
    }
}

// After distance pass `pass` (0: the first average): add every tensor's chunk
// partials in chunk order, d_c = sqrt, objective sum_c W_c d_c with the weights
// the median was formed with, the reference's break test (strict <, so an
// objective of 0 never breaks), and unless this was the last pass the next
// weights W / max(eps, d), renormalised.  One 256-thread block per tensor.
__global__ __launch_bounds__(kNT) void k_gm_update(GmArgs a, int pass, int last) {
#pragma clang fp contract(off)
    constexpr int kStage = 128;  // chunk rows staged at a time (16 KiB of LDS)
    __shared__ double d[kMaxC], nw[kMaxC], stage[kStage * kMaxC];
    const int t = blockIdx.x, lane = threadIdx.x;
    if (a.done[t]) return;
    // the partial rows go through LDS (coalesced loads by the whole block), then
    // lane c runs collaborator c's add chain from LDS (lds_chain), as
    // k_range_sums does
    const int c0 = a.tchunk0[t], c1 = a.tchunk0[t + 1];
    double s = 0.0;
    for (int b = c0; b < c1; b += kStage) {
        const int m = c1 - b < kStage ? c1 - b : kStage;
        __syncthreads();
        for (int k = lane; k < m * kMaxC; k += kNT) stage[k] = a.partial[(int64_t)b * kMaxC + k];
        __syncthreads();
        if (lane < a.nc) s = lds_chain<double, kMaxC>(s, stage + lane, m);
    }
    if (lane < a.nc) d[lane] = sqrt(s);
    __syncthreads();
    if (lane) return;
    double* W = a.W + t * kMaxC;
    double obj = 0.0;
    for (int c = 0; c < a.nc; ++c) obj = obj + W[c] * d[c];
    const double prev = a.obj[t];
    a.obj[t] = obj;
    if (pass > 0) {
        a.iters[t] = pass;
        if (fabs(prev - obj) < a.ftol * obj) {
            a.done[t] = 1;
            return;
        }
    }
    if (last) return;
    for (int c = 0; c < a.nc; ++c) nw[c] = W[c] / (d[c] > a.eps ? d[c] : a.eps);
    // weights.sum() of nc <= 16 values: NumPy's pairwise order
    const double tot = np_pairwise_block([&](int c) { return nw[c]; }, 0, a.nc);
    double ws = 0.0;
    for (int c = 0; c < a.nc; ++c) {
        const double w = nw[c] / tot;
        W[c] = w;
        ws = c ? ws + w : w;
    }
    a.wsum[t] = ws;
}

// the aggregate with every tensor's final weights, and the deltas as
// k_wavg_delta writes them
template <int C>
__global__ __launch_bounds__(kNT) void k_gm_final(GmArgs a) {
#pragma clang fp contract(off)
    for (int ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
        const ofl_gm_chunk k = a.chunks[ch];
        double w[C];
#pragma unroll
        for (int c = 0; c < C; ++c) w[c] = a.W[k.tensor * kMaxC + c];
        const double wsum = a.wsum[k.tensor];
        for (int e = threadIdx.x; e < k.len; e += kNT) {
            const int64_t i = k.start + e;
            float x[C];
            a.o.put(i, gm_point<C>(a, w, wsum, i, x));
        }
    }
}

// the delta of an aggregate arena on listed ranges, packed: float64 aggregate
// -> agg - (double)base; float32 aggregate -> a float32 subtract
template <typename T>
__global__ __launch_bounds__(kNT) void k_agg_ranges(const T* agg, const float* base, Ranges rg, T* out) {
#pragma clang fp contract(off)
    const int64_t total = rg.total();
    for (int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x; j < total; j += (int64_t)gridDim.x * kNT) {
        int64_t i;
        rg.find(j, i);
        out[j] = base ? agg[i] - (T)base[i] : agg[i];
    }
}

}  // namespace agg

namespace {
template <int C>
void launch_median(const agg::MedArgs<agg::kMaxC>& a, int vec, hipStream_t st) {
    hipLaunchKernelGGL(agg::k_median<C>, dim3(grid_for(a.n, 4)), dim3(agg::kNT), 0, st, a, vec);
}
template <int C>
void launch_gm_dist(const agg::GmArgs& a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(agg::k_gm_dist<C>, dim3(grid), dim3(agg::kNT), 0, st, a);
}
template <int C>
void launch_gm_final(const agg::GmArgs& a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(agg::k_gm_final<C>, dim3(grid), dim3(agg::kNT), 0, st, a);
}
#define OFL_FOR_C16(F, c, ...)                                                                      \
    switch (c) {                                                                                    \
        case 1: F<1>(__VA_ARGS__); break;   case 2: F<2>(__VA_ARGS__); break;                       \
        case 3: F<3>(__VA_ARGS__); break;   case 4: F<4>(__VA_ARGS__); break;                       \
        case 5: F<5>(__VA_ARGS__); break;   case 6: F<6>(__VA_ARGS__); break;                       \
        case 7: F<7>(__VA_ARGS__); break;   case 8: F<8>(__VA_ARGS__); break;                       \
        case 9: F<9>(__VA_ARGS__); break;   case 10: F<10>(__VA_ARGS__); break;                     \
        case 11: F<11>(__VA_ARGS__); break; case 12: F<12>(__VA_ARGS__); break;                     \
        case 13: F<13>(__VA_ARGS__); break; case 14: F<14>(__VA_ARGS__); break;                     \
        case 15: F<15>(__VA_ARGS__); break; default: F<16>(__VA_ARGS__); break;                     \
    }

size_t gm_align(size_t v) { return (v + 255) & ~(size_t)255; }

// ofl_agg_delta_seeds for an aggregate of type T
template <typename T>
void launch_agg_seeds(const void* agg, const float* base, agg::Ranges rg, int64_t total, const int64_t* draws,
                      uint32_t* seeds, double* sums, void* packed_dev, hipStream_t st) {
    T* packed = static_cast<T*>(packed_dev);
    if (total > 0)
        hipLaunchKernelGGL(agg::k_agg_ranges<T>, dim3(grid_for(total, 1)), dim3(agg::kNT), 0, st,
                           static_cast<const T*>(agg), base, rg, packed);
    launch_sums_seeds<T>(packed, rg.dst, rg.nr, draws, seeds, sums, st);
}
}  // namespace

extern "C" {

int ofl_median_delta(int ncollab, const float* const* xs, const float* base, int64_t n, float* median_out,
                     float* delta_out, void* stream) {
    if (int rc = check_collabs("median", ncollab, xs, xs)) return rc;
    if (ncollab > agg::kMedMaxC) return afail(OFL_EINVAL, "median: at most 128 collaborators");
    if (n < 0) return afail(OFL_EINVAL, "median: negative size");
    if (n == 0 || (!median_out && !delta_out)) return OFL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ncollab <= agg::kMaxC) {
        agg::MedArgs<agg::kMaxC> a{{}, base, median_out, delta_out, n, {}};
        std::copy(xs, xs + ncollab, a.x);
        OFL_FOR_C16(launch_median, ncollab, a, aligned16(xs, ncollab, base, median_out, delta_out), st)
    } else {
        agg::MedArgs<agg::kMedMaxC> a{{}, base, median_out, delta_out, n, ncollab};
        std::copy(xs, xs + ncollab, a.x);
        const int64_t want = (n + agg::kMedLdsNT - 1) / agg::kMedLdsNT;
        const int g = (int)std::min<int64_t>(want, (int64_t)grid_for(n, 1) * 4);
        hipLaunchKernelGGL(agg::k_median_lds, dim3(g), dim3(agg::kMedLdsNT), 0, st, a);
    }
    AHIP(hipGetLastError());
    return OFL_OK;
}

size_t ofl_gmedian_workspace_bytes(int ntensors, int nchunks) {
    const size_t T = (size_t)std::max(ntensors, 1), K = (size_t)std::max(nchunks, 1);
    return gm_align(8 * T * agg::kMaxC) + 2 * gm_align(8 * T) + 2 * gm_align(4 * T) + gm_align(8 * K * agg::kMaxC) + 256;
}

int ofl_gmedian_delta(int ncollab, const float* const* xs, const double* w0, int maxiter, double eps, double ftol,
                      const float* base, int ntensors, const ofl_gm_chunk* chunks_dev, int nchunks,
                      const int32_t* tensor_chunk0_dev, double* agg_out, double* delta64_out, float* delta32_out,
                      int32_t* iters_out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_collabs("geometric median", ncollab, xs, w0)) return rc;
    if (ncollab > agg::kMaxC) return afail(OFL_EINVAL, "geometric median: at most 16 collaborators");
    if (ntensors < 1 || nchunks < 0 || maxiter < 0) return afail(OFL_EINVAL, "geometric median: bad sizes");
    if (!tensor_chunk0_dev || (nchunks && !chunks_dev)) return afail(OFL_EINVAL, "geometric median: null chunk table");
    if (!ws || ws_bytes < ofl_gmedian_workspace_bytes(ntensors, nchunks))
        return afail(OFL_ESPACE, "geometric median: workspace too small");
    const size_t T = (size_t)ntensors, K = (size_t)std::max(nchunks, 1);
    char* w = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
    agg::GmArgs a{};
    agg::GmW0 init{};
    std::copy(xs, xs + ncollab, a.x);
    std::copy(w0, w0 + ncollab, init.w);
    a.nc = ncollab;
    a.chunks = chunks_dev;
    a.nchunks = nchunks;
    a.tchunk0 = tensor_chunk0_dev;
    a.nt = ntensors;
    a.W = reinterpret_cast<double*>(w);        w += gm_align(8 * T * agg::kMaxC);
    a.wsum = reinterpret_cast<double*>(w);     w += gm_align(8 * T);
    a.obj = reinterpret_cast<double*>(w);      w += gm_align(8 * T);
    a.done = reinterpret_cast<int32_t*>(w);    w += gm_align(4 * T);
    a.iters = reinterpret_cast<int32_t*>(w);   w += gm_align(4 * T);
    a.partial = reinterpret_cast<double*>(w);  w += gm_align(8 * K * agg::kMaxC);
    if (iters_out) a.iters = iters_out;
    a.eps = eps;
    a.ftol = ftol;
    a.o = {base, agg_out, delta64_out, delta32_out};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = std::max(1, std::min(nchunks, cu_count() * 8));
    hipLaunchKernelGGL(agg::k_gm_init, dim3((ntensors + 63) / 64), dim3(64), 0, st, a, init);
    for (int pass = 0; pass <= maxiter; ++pass) {
        if (nchunks) OFL_FOR_C16(launch_gm_dist, ncollab, a, grid, st)
        hipLaunchKernelGGL(agg::k_gm_update, dim3(ntensors), dim3(agg::kNT), 0, st, a, pass, pass == maxiter ? 1 : 0);
    }
    if (nchunks && (agg_out || delta64_out || delta32_out)) OFL_FOR_C16(launch_gm_final, ncollab, a, grid, st)
    AHIP(hipGetLastError());
    return OFL_OK;
}

int ofl_agg_delta_seeds(const void* agg_dev, int agg_is_f64, const float* base, int nranges, const int64_t* starts_dev,
                        const int64_t* dst_dev, int64_t total, const int64_t* draws_dev, uint32_t* seeds_dev,
                        double* sums_dev, void* packed_dev, void* stream) {
    if (nranges < 1 || total < 0) return afail(OFL_EINVAL, "agg seeds: bad sizes");
    if (!agg_dev || !starts_dev || !dst_dev || !draws_dev || !seeds_dev || !sums_dev || (total > 0 && !packed_dev))
        return afail(OFL_EINVAL, "agg seeds: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const agg::Ranges rg{starts_dev, dst_dev, nranges};
    if (agg_is_f64)
        launch_agg_seeds<double>(agg_dev, base, rg, total, draws_dev, seeds_dev, sums_dev, packed_dev, st);
    else
        launch_agg_seeds<float>(agg_dev, base, rg, total, draws_dev, seeds_dev, sums_dev, packed_dev, st);
    AHIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"

// ---- FedOpt server optimisers: Adam, Yogi and Adagrad --------------------------
// (reference: interface/aggregation_functions/core/adaptive_aggregation.py:38-113,
//  utilities/optimizers/numpy/{adam,yogi,adagrad}_optimizer.py)
//
// With float32 parameters and Python-float collaborator weights every operation
// of the reference is one float32 NumPy operation (a Python float is a weak
// scalar: it is rounded to float32 once and the array's dtype holds), and none
// of them is a reduction whose order could differ.  The kernel performs the
// same float32 operations in the same order, contraction off, with the
// constants already rounded by the host:
//   g = +0.0f;  for c in order:  g = g + w_c * (base - x_c)        (sum() from 0)
//   Adam     m = b1 * m + (1 - b1) * g
//            v = b2 * v + (1 - b2) * (g * g)
//            p = p - (lr * (m / (1 - b1^t))) / (sqrtf(v / (1 - b2^t)) + eps)
//   Yogi     as Adam, v = b2 * v + ((1 - b2) * sign(g * g - v)) * (g * g)
//   Adagrad  v = v + g * g;  p = p - (lr * g) / (sqrtf(v) + eps)
// `/` and sqrtf are the correctly rounded float32 operations and float32
// denormals are kept, as in NumPy.  Per element the kernel reads 4 C + 16 bytes
// (collaborators, base, p, m, v; Adagrad: 4 C + 12) and writes 12 to 20 (p, m, v,
// and the optional aggregate and delta; Adagrad: 8 to 16); the state of an element
// is read and written by one thread.

namespace agg {

constexpr int kAdaMaxC = 128;  // the long pointer table's length

struct AdaIO {
    const float* base;
    float* p;
    float* m;      // unused by Adagrad
    float* v;
    float* agg;    // nullable: p after the step
    float* delta;  // nullable: p after the step - base, a float32 subtract
    int64_t n;
};
// N = kMaxC: <= 16 collaborators, unrolled; N = kAdaMaxC: 17..128, a runtime
// loop over the table
template <int N>
struct AdaArgs {
    const float* x[N];
    float w[N];
    AdaIO io;
    ofl_adaptive_consts k;
    [[no_unique_address]] TableCount<N> nc;
};
static_assert(sizeof(AdaArgs<kMaxC>) == 288);

// np.sign: -1, 0, +1, and the NaN itself for a NaN
__device__ __forceinline__ float np_signf(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == 0.f ? 0.f : d)); }

__device__ __forceinline__ void ada_update(const ofl_adaptive_consts& k, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
    const float gg = g * g;
    if (k.kind == OFL_ADAPTIVE_ADAGRAD) {
        v = v + gg;
        const float num = k.lr * g;
        const float den = sqrtf(v) + k.eps;
        p = p - num / den;
        return;
    }
    {
        const float a = k.beta1 * m;
        const float b = k.one_minus_beta1 * g;
        m = a + b;
    }
    if (k.kind == OFL_ADAPTIVE_YOGI) {
        const float s = np_signf(gg - v);
        const float a = k.beta2 * v;
        const float c = k.one_minus_beta2 * s;
        const float b = c * gg;
        v = a + b;
    } else {
        const float a = k.beta2 * v;
        const float b = k.one_minus_beta2 * gg;
        v = a + b;
    }
    const float mh = m / k.bias1;
    const float vh = v / k.bias2;
    const float num = k.lr * mh;
    const float den = sqrtf(vh) + k.eps;
    p = p - num / den;
}

template <int C, class A>
__device__ __forceinline__ void ada_elem(const A& a, int64_t i) {
#pragma clang fp contract(off)
    const bool moment = a.k.kind != OFL_ADAPTIVE_ADAGRAD;
    const float b = a.io.base[i];
    float g = 0.0f;
    if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = b - a.x[c][i];
            g = g + a.w[c] * d;
        }
    } else {
        for (int c = 0; c < a.nc; ++c) {
            const float d = b - a.x[c][i];
            g = g + a.w[c] * d;
        }
    }
    float p = a.io.p[i], m = moment ? a.io.m[i] : 0.f, v = a.io.v[i];
    ada_update(a.k, g, p, m, v);
    a.io.p[i] = p;
    if (moment) a.io.m[i] = m;
    a.io.v[i] = v;
    if (a.io.agg) a.io.agg[i] = p;
    if (a.io.delta) a.io.delta[i] = p - b;
}

// 4 consecutive elements per thread, 16-B loads and stores of every arena
template <int C, class A>
__device__ __forceinline__ void ada_quad(const A& a, int64_t i) {
#pragma clang fp contract(off)
    const bool moment = a.k.kind != OFL_ADAPTIVE_ADAGRAD;
    const float4 b = *reinterpret_cast<const float4*>(a.io.base + i);
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f;
    auto term = [&](const float4 x, const float w) {
        const float d0 = b.x - x.x, d1 = b.y - x.y, d2 = b.z - x.z, d3 = b.w - x.w;
        const float t0 = w * d0, t1 = w * d1, t2 = w * d2, t3 = w * d3;
        g0 = g0 + t0; g1 = g1 + t1; g2 = g2 + t2; g3 = g3 + t3;
    };
    if constexpr (C > 0) {
        float4 q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = *reinterpret_cast<const float4*>(a.x[c] + i);
#pragma unroll
        for (int c = 0; c < C; ++c) term(q[c], a.w[c]);
    } else {
        for (int c = 0; c < a.nc; ++c) term(*reinterpret_cast<const float4*>(a.x[c] + i), a.w[c]);
    }
    float4 p = *reinterpret_cast<const float4*>(a.io.p + i);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (moment) m = *reinterpret_cast<const float4*>(a.io.m + i);
    float4 v = *reinterpret_cast<const float4*>(a.io.v + i);
    ada_update(a.k, g0, p.x, m.x, v.x);
    ada_update(a.k, g1, p.y, m.y, v.y);
    ada_update(a.k, g2, p.z, m.z, v.z);
    ada_update(a.k, g3, p.w, m.w, v.w);
    *reinterpret_cast<float4*>(a.io.p + i) = p;
    if (moment) *reinterpret_cast<float4*>(a.io.m + i) = m;
    *reinterpret_cast<float4*>(a.io.v + i) = v;
    if (a.io.agg) *reinterpret_cast<float4*>(a.io.agg + i) = p;
    if (a.io.delta) *reinterpret_cast<float4*>(a.io.delta + i) = make_float4(p.x - b.x, p.y - b.y, p.z - b.z, p.w - b.w);
}

// C > 0: that many collaborators unrolled from AdaArgs<kMaxC>; C == 0: a.nc of
// AdaArgs<kAdaMaxC>
template <int C, class A>
__global__ __launch_bounds__(kNT) void k_adaptive(A a, int vec) {
    quads_then_tail(a.io.n, vec, [&](int64_t i) { ada_quad<C>(a, i); }, [&](int64_t i) { ada_elem<C>(a, i); });
}

}  // namespace agg

namespace {
template <int C, class A>
void launch_adaptive(const A& a, int vec, hipStream_t st) {
    hipLaunchKernelGGL((agg::k_adaptive<C, A>), dim3(grid_for(a.io.n, 4)), dim3(agg::kNT), 0, st, a, vec);
}
}  // namespace

extern "C" {

int ofl_adaptive_step(int ncollab, const float* const* xs, const float* weights, const float* base, int64_t n,
                      float* p, float* m, float* v, const ofl_adaptive_consts* k, float* agg_out, float* delta_out,
                      void* stream) {
    if (int rc = check_collabs("adaptive step", ncollab, xs, weights)) return rc;
    if (ncollab > agg::kAdaMaxC) return afail(OFL_EINVAL, "adaptive step: at most 128 collaborators");
    if (n < 0) return afail(OFL_EINVAL, "adaptive step: negative size");
    if (!k || k->kind < OFL_ADAPTIVE_ADAM || k->kind > OFL_ADAPTIVE_ADAGRAD)
        return afail(OFL_EINVAL, "adaptive step: kind must be OFL_ADAPTIVE_ADAM, _YOGI or _ADAGRAD");
    if (n == 0) return OFL_OK;
    if (!base || !p || !v || (k->kind != OFL_ADAPTIVE_ADAGRAD && !m))
        return afail(OFL_EINVAL, "adaptive step: base and the state arenas are required");
    const agg::AdaIO io{base, p, k->kind != OFL_ADAPTIVE_ADAGRAD ? m : nullptr, v, agg_out, delta_out, n};
    const int vec = aligned16(xs, ncollab, base, p, io.m, v, agg_out, delta_out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ncollab <= agg::kMaxC) {
        agg::AdaArgs<agg::kMaxC> a{{}, {}, io, *k, {}};
        fill_args(a, xs, weights, ncollab);
        OFL_FOR_C16(launch_adaptive, ncollab, a, vec, st)
    } else {
        agg::AdaArgs<agg::kAdaMaxC> a{{}, {}, io, *k, ncollab};
        fill_args(a, xs, weights, ncollab);
        launch_adaptive<0>(a, vec, st);
    }
    AHIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"
