// lossy_topk.h -- the batched top-k kernels of lossy_kernels.hip, and the
// batched ternary ranks of the sparse arena they write (k_ternary_batch).
#pragma once
#include "lossy_device.h"

namespace lossy {

// ===========================================================================
// Batched exact top-k by magnitude (SparsityTransformer._topk_func,
// skc_pipeline.py:72-94 / stc_pipeline.py:53-91, for many tensors of one
// fp32 arena), device-resident and deterministic.  |x| bit patterns order like
// the magnitudes, so the k-th largest is found by a 3-digit radix select over
// the 31 magnitude bits (11 + 11 + 9):
//   k_btk_hist   per-tensor digit histogram of the elements matching the
//                prefix found so far                                 (1 pass)
//   k_btk_digit  one wave per tensor: the digit holding the need-th largest,
//                prefix/need update, histogram cleared for the next pass
// then T = the k-th largest |x| bits and `need` = ties at T kept (lowest index
// first, the reference's argsort order for ties being unspecified):
//   k_btk_ties   per block: ties at T, min kept-for-sure value (|x| > T), min
//                tie value, in-block tie rank of the first negative tie (1 pass)
//   k_btk_scan   one wave per tensor: exclusive prefix of the tie counts and
//                the exact minimum of the kept set -> the +1e-7 shift (:92-93)
//   k_btk_select dense sparse output (kept + shift, else 0) and per-block
//                kept-set statistics (1 pass: read x, write sparse)
//   k_btk_final  one wave per tensor: fixed-order sums of the statistics
// Blocks cover kBkmChunk consecutive elements of one tensor, as in k-means.
// ===========================================================================
struct BtkArgs {
    const float* x;
    float* out;
    const BkmTensor* td;
    int32_t ntensors;
    int32_t pass;
    BtkState* st;
    uint32_t* hist;       // [T][kRadix]
    BtkBlock* blk;        // [blocks]
};

DEVI int btk_shift(int pass) { return pass == 0 ? 20 : (pass == 1 ? 9 : 0); }
DEVI int btk_width(int pass) { return pass == 2 ? 9 : 11; }

__global__ __launch_bounds__(kNT) void k_btk_hist(BtkArgs a) {
    __shared__ uint32_t h[kRadix];
    for (int b = threadIdx.x; b < kRadix; b += kNT) h[b] = 0;
    const Chunk c = chunk_of(a.td, a.ntensors, blockIdx.x);
    const int t = c.t;
    const uint32_t prefix = a.st[t].prefix, pmask = a.st[t].pmask;
    const int sh = btk_shift(a.pass);
    const uint32_t dm = (1u << btk_width(a.pass)) - 1u;
    __syncthreads();
    visit(a.x + c.T.off, c.i0, c.i1, [&](float v, int64_t) {
        const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
        if ((m & pmask) == prefix) lds_count(h, (int)((m >> sh) & dm));  // ballots see the candidates only
    });
    __syncthreads();
    uint32_t* g = a.hist + (int64_t)t * kRadix;
    for (int b = threadIdx.x; b <= (int)dm; b += kNT) if (h[b]) atomicAdd(&g[b], h[b]);
}

__global__ __launch_bounds__(64) void k_btk_digit(BtkArgs a) {
    const int t = blockIdx.x, lane = threadIdx.x;
    BtkState& S = a.st[t];
    uint32_t* h = a.hist + (int64_t)t * kRadix;
    const int width = btk_width(a.pass), sh = btk_shift(a.pass);
    const int per = (1 << width) / 64;
    const int64_t need = S.need;
    int64_t s = 0;
    for (int j = 0; j < per; ++j) s += h[lane * per + j];
    // suffix sums from the top bin: S_l = sum over lanes >= l
    int64_t suf = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += u;
    }
    const unsigned long long hit = __ballot(suf >= need);
    const int L = hit ? 63 - __clzll((long long)hit) : 0;   // the need-th largest lies in lane L's bins
    if (lane == L) {
        int64_t acc = suf - s;  // elements in bins above lane L's range
        int d = lane * per;
        for (int b = lane * per + per - 1; b > lane * per; --b) {
            if (acc + (int64_t)h[b] >= need) { d = b; break; }
            acc += h[b];
        }
        S.prefix |= (uint32_t)d << sh;
        S.pmask |= (uint32_t)((1 << width) - 1) << sh;
        S.need = need - acc;
    }
    for (int j = 0; j < per; ++j) h[lane * per + j] = 0;
}

__global__ __launch_bounds__(kNT) void k_btk_ties(BtkArgs a) {
    __shared__ uint32_t tu[kNT / 64];
    __shared__ float tf[kNT / 64];
    __shared__ int64_t ti[kNT / 64];
    const Chunk ch = chunk_of(a.td, a.ntensors, blockIdx.x);
    const int64_t i0 = ch.i0;
    const uint32_t Tb = a.st[ch.t].prefix;
    const float* p = a.x + ch.T.off;
    uint32_t c = 0;
    float smin = INFINITY, tmin = INFINITY;
    int64_t neg = INT64_MAX;
    visit(p, i0, ch.i1, [&](float v, int64_t i) {
        const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
        if (m > Tb) smin = fminf(smin, v);
        if (m == Tb) {
            ++c;
            tmin = fminf(tmin, v);
            if (v < 0.0f && i < neg) neg = i;
        }
    });
    c = btk_breduce(c, tu, [](uint32_t x, uint32_t y) { return x + y; });
    smin = btk_breduce(smin, tf, [](float x, float y) { return fminf(x, y); });
    tmin = btk_breduce(tmin, tf, [](float x, float y) { return fminf(x, y); });
    neg = btk_breduce(neg, ti, [](int64_t x, int64_t y) { return x < y ? x : y; });
    int32_t rank = -1;
    if (neg != INT64_MAX) {  // rare: a negative tie -> its rank among the block's ties
        uint32_t r = 0;
        for (int64_t i = i0 + threadIdx.x; i < neg; i += kNT) r += (__float_as_uint(p[i]) & 0x7fffffffu) == Tb;
        rank = (int32_t)btk_breduce(r, tu, [](uint32_t x, uint32_t y) { return x + y; });
    }
    if (threadIdx.x == 0) {
        BtkBlock& B = a.blk[blockIdx.x];
        B.ties = c;
        B.neg_rank = rank;
        B.smin = smin;
        B.tmin = tmin;
    }
}

__global__ __launch_bounds__(64) void k_btk_scan(BtkArgs a) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const BkmTensor T = a.td[t];
    BtkState& S = a.st[t];
    const int64_t need = S.need;
    uint64_t carry = 0;
    float smin = INFINITY, tmin = INFINITY;
    int negkept = 0;
    for (int b0 = 0; b0 < T.nblk; b0 += 64) {
        const int b = b0 + lane;
        BtkBlock* B = a.blk + T.blk0 + b;
        const uint64_t c = b < T.nblk ? B->ties : 0;
        uint64_t inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (b < T.nblk) {
            const uint64_t base = carry + inc - c;
            B->tie_base = base;
            smin = fminf(smin, B->smin);
            tmin = fminf(tmin, B->tmin);
            if (B->neg_rank >= 0 && (int64_t)base + B->neg_rank < need) negkept = 1;
        }
        carry += __shfl(inc, 63, 64);
    }
    smin = wave_min(smin);
    tmin = wave_min(tmin);
    negkept = __any(negkept);
    if (lane == 0) {
        float kmin = smin;
        const float Tf = __uint_as_float(S.prefix);
        if (need > 0) kmin = fminf(kmin, (int64_t)carry <= need ? tmin : (negkept ? -Tf : Tf));
        S.kmin = kmin;
        // reference: `if min(topk_mag) - 0 < 10e-8: topk_mag = topk_mag + 10e-8`
        S.shift = ((double)kmin < 10e-8) ? (float)10e-8 : 0.0f;
    }
}

__global__ __launch_bounds__(kNT) void k_btk_select(BtkArgs a) {
    __shared__ uint32_t tu[kNT / 64];
    __shared__ double td[kNT / 64];
    const Chunk c = chunk_of(a.td, a.ntensors, blockIdx.x);
    const int t = c.t;
    const int64_t i0 = c.i0, i1 = c.i1;
    const uint32_t Tb = a.st[t].prefix;
    const int64_t need = a.st[t].need;
    const float shift = a.st[t].shift;
    BtkBlock& B = a.blk[blockIdx.x];
    const int64_t base = (int64_t)B.tie_base, nt = B.ties;
    const float* p = a.x + c.T.off;
    float* o = a.out + c.T.off;
    uint32_t cpos = 0, cneg = 0, czero = 0;
    double as = 0.0;
    auto kept = [&](float v) {
        const float w = v + shift;  // float32 add (NEP 50: python float is weak)
        cpos += w > 0.0f;
        cneg += w < 0.0f;
        czero += w == 0.0f;
        as += fabs((double)w);
        return w;
    };
    if (nt == 0 || base >= need || base + nt <= need) {
        // the block's ties are all dropped or all kept: no ordering needed
        const bool keep_ties = nt > 0 && base + nt <= need;
        auto f = [&](float v) {
            const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
            return (m > Tb || (keep_ties && m == Tb)) ? kept(v) : 0.0f;
        };
        if (((reinterpret_cast<uintptr_t>(p + i0) | reinterpret_cast<uintptr_t>(o + i0)) & 15u) == 0) {
            const int64_t n4 = (i1 - i0) >> 2;
            const float4* x4 = reinterpret_cast<const float4*>(p + i0);
            float4* y4 = reinterpret_cast<float4*>(o + i0);
            for (int64_t j = threadIdx.x; j < n4; j += kNT) {
                const float4 v = x4[j];
                y4[j] = make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
            }
            for (int64_t j = i0 + 4 * n4 + threadIdx.x; j < i1; j += kNT) o[j] = f(p[j]);
        } else {
            for (int64_t j = i0 + threadIdx.x; j < i1; j += kNT) o[j] = f(p[j]);
        }
    } else {
        // the boundary block: in-order tie ranks, kNT elements at a time
        int64_t ties = base;
        for (int64_t c0 = i0; c0 < i1; c0 += kNT) {
            const int64_t i = c0 + threadIdx.x;
            const bool in = i < i1;
            const float v = in ? p[i] : 0.0f;
            const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
            const uint32_t tie = (in && m == Tb) ? 1u : 0u;
            uint32_t tot;
            const uint32_t r = block_excl_scan(tie, tu, tot);
            const bool keep = in && (m > Tb || (tie && ties + (int64_t)r < need));
            ties += tot;
            if (in) o[i] = keep ? kept(v) : 0.0f;
        }
    }
    cpos = btk_breduce(cpos, tu, [](uint32_t x, uint32_t y) { return x + y; });
    cneg = btk_breduce(cneg, tu, [](uint32_t x, uint32_t y) { return x + y; });
    czero = btk_breduce(czero, tu, [](uint32_t x, uint32_t y) { return x + y; });
    as = btk_breduce(as, td, [](double x, double y) { return x + y; });
    if (threadIdx.x == 0) { B.cpos = cpos; B.cneg = cneg; B.czero = czero; B.asum = as; }
}

__global__ __launch_bounds__(64) void k_btk_final(BtkArgs a) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const BkmTensor T = a.td[t];
    uint64_t p = 0, n = 0, z = 0;
    double s = 0.0;
    for (int b = lane; b < T.nblk; b += 64) {
        const BtkBlock& B = a.blk[T.blk0 + b];
        p += B.cpos; n += B.cneg; z += B.czero; s += B.asum;
    }
    p = wave_sum(p); n = wave_sum(n); z = wave_sum(z); s = wave_sum(s);
    if (lane == 0) {
        BtkState& S = a.st[t];
        S.n_pos = (int64_t)p; S.n_neg = (int64_t)n; S.n_zero = (int64_t)z; S.abs_sum = s;
    }
}

// ternary ranks of a sparse arena, per-tensor (rank_neg, rank_zero, rank_pos)
// (stc_pipeline.py:105-130 then _float_to_int)
__global__ __launch_bounds__(kNT) void k_ternary_batch(const float* in, float* out, const BkmTensor* td, int nt,
                                                       const float* ranks3) {
    const Chunk c = chunk_of(td, nt, blockIdx.x);
    const float rn = ranks3[3 * c.t], rz = ranks3[3 * c.t + 1], rp = ranks3[3 * c.t + 2];
    const int64_t i0 = c.i0, i1 = c.i1;
    const float* x = in + c.T.off;
    float* y = out + c.T.off;
    auto f = [&](float v) { return v > 0.0f ? rp : (v < 0.0f ? rn : rz); };
    // (written out, as in k_lut_batch and k_btk_select: moved into a shared
    // function, the same lines compile to other code in all three)
    if (((reinterpret_cast<uintptr_t>(x + i0) | reinterpret_cast<uintptr_t>(y + i0)) & 15u) == 0) {
        const int64_t n4 = (i1 - i0) >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x + i0);
        float4* y4 = reinterpret_cast<float4*>(y + i0);
        for (int64_t i = threadIdx.x; i < n4; i += kNT) {
            const float4 v = x4[i];
            y4[i] = make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
        }
        for (int64_t i = i0 + 4 * n4 + threadIdx.x; i < i1; i += kNT) y[i] = f(x[i]);
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += kNT) y[i] = f(x[i]);
    }
}

}  // namespace lossy
