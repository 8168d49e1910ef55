// lossy_device.h -- what the lossy kernels (lossy_kernels.hip) share: wave and
// block reductions, the LDS histogram adds, and the two steps the batched
// kernels share -- which tensor and chunk a block owns (chunk_of) and the walk
// over a chunk's elements (visit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lossy_layout.h"

#define DEVI __device__ __forceinline__

namespace lossy {

DEVI int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
DEVI int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }

template <typename T>
DEVI T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
DEVI float wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
DEVI float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// order-preserving float <-> uint32 (for atomic min/max)
DEVI uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// LDS histogram increment with wave aggregation for concentrated data: the
// lanes that share the first active lane's bin add once (popcount / wave
// sum), the others add directly.  Sparse or low-entropy inputs (top-k zeros,
// exponent digits) otherwise serialise up to 64 same-address LDS atomics.
DEVI void lds_count(uint32_t* h, int b) {
    const int bl = __builtin_amdgcn_readfirstlane(b);
    const unsigned long long m = __ballot(b == bl);
    if (__popcll(m) >= 8) {
        if (b == bl) {
            if ((int)(threadIdx.x & 63) == __builtin_ffsll((long long)m) - 1) atomicAdd(&h[bl], (uint32_t)__popcll(m));
        } else {
            atomicAdd(&h[b], 1u);
        }
    } else {
        atomicAdd(&h[b], 1u);
    }
}
DEVI void lds_add64(unsigned long long* h, int b, unsigned long long v) {
    const int bl = __builtin_amdgcn_readfirstlane(b);
    const unsigned long long m = __ballot(b == bl);
    if (__popcll(m) >= 8) {
        unsigned long long s = b == bl ? v : 0ull;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (b == bl) {
            if ((int)(threadIdx.x & 63) == __builtin_ffsll((long long)m) - 1) atomicAdd(&h[bl], s);
        } else {
            atomicAdd(&h[b], v);
        }
    } else {
        atomicAdd(&h[b], v);
    }
}

// 256-thread exclusive scan of one uint32 per thread (block total in `total`)
DEVI uint32_t block_excl_scan(uint32_t v, uint32_t* tmp, uint32_t& total) {
    // 256 threads: wave-level inclusive scan, then wave offsets
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) tmp[w] = inc;
    __syncthreads();
    uint32_t off = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < kNT / 64; ++j) { if (j < w) off += tmp[j]; total += tmp[j]; }
    __syncthreads();
    return off + inc - v;
}

// 256-thread block reductions through a 4-entry LDS array
template <typename V, typename Op>
DEVI V btk_breduce(V v, V* tmp, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    V r = tmp[0];
#pragma unroll
    for (int w = 1; w < kNT / 64; ++w) r = op(r, tmp[w]);
    return r;
}

// Block b of a batched launch: its tensor t (the last record whose first block
// is <= b), that tensor's record, and the elements [i0, i1) of the tensor that
// the block covers.
struct Chunk {
    int t;
    BkmTensor T;
    int64_t i0, i1;
};
DEVI int chunk_tensor(const BkmTensor* td, int ntensors, int b) {
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (td[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
DEVI Chunk chunk_of(const BkmTensor* td, int ntensors, unsigned b) {
    Chunk c;
    c.t = chunk_tensor(td, ntensors, (int)b);
    c.T = td[c.t];
    c.i0 = (int64_t)(b - c.T.blk0) * kBkmChunk;
    c.i1 = c.i0 + kBkmChunk < c.T.n ? c.i0 + kBkmChunk : c.T.n;
    return c;
}

// f(v, i) for every element of p[i0, i1) (i = index inside the tensor): 16-B
// loads over the aligned middle
template <int NT = kNT, typename F>
DEVI void visit(const float* p, int64_t i0, int64_t i1, F f) {
    int64_t a4 = i0;
    while (a4 < i1 && (reinterpret_cast<uintptr_t>(p + a4) & 15u)) ++a4;
    for (int64_t j = i0 + threadIdx.x; j < a4; j += NT) f(p[j], j);
    const int64_t n4 = (i1 - a4) >> 2;
    const float4* q = reinterpret_cast<const float4*>(p + a4);
    for (int64_t j = threadIdx.x; j < n4; j += NT) {
        const float4 v = q[j];
        const int64_t i = a4 + 4 * j;
        f(v.x, i); f(v.y, i + 1); f(v.z, i + 2); f(v.w, i + 3);
    }
    for (int64_t j = a4 + 4 * n4 + threadIdx.x; j < i1; j += NT) f(p[j], j);
}

// The element-wise maps (k_lut_batch, k_ternary_batch, k_btk_select: 16-B
// accesses where input and output are aligned together, else scalar) have no
// helper here: as a function taking the element rule, the same lines compile
// to other code in all three (profiles/r13_lossy_refactor_ab.txt).

}  // namespace lossy
