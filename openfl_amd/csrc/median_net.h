// median_net.h -- the median of C <= 16 floats held in registers, by a
// compile-time compare-exchange network (np.median's value for one column).
//
// The network is Batcher's odd-even merge sort on the next power of two; the
// padding slots stand for +inf, which never moves, so every exchange that
// touches one is dropped.  The exchange list is built at compile time and
// expanded as a pack, so every array index is a constant and the column stays
// in registers (a runtime-indexed per-thread array would go to scratch).  The
// compiler removes the exchanges the middle element does not depend on.
//
// Values: odd C -> the middle order statistic; even C -> (lo + hi) / 2 in
// float32 (one add, one halving: 3e38, 3e38 -> inf, as NumPy's mean of the
// two middle values); any NaN in the column -> NaN.  Tied -0.0 / +0.0 may come
// out with either sign.
#pragma once
#include <cmath>
#include <utility>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OFL_HD __host__ __device__ __forceinline__
#else
#define OFL_HD inline
#endif

namespace mednet {

constexpr int kMaxC = 16;

struct Net {
    int n = 0;
    int lo[64] = {}, hi[64] = {};  // 63 exchanges sort 16 values
};

template <int C>
constexpr Net make_net() {
    Net net;
    int N = 1;
    while (N < C) N *= 2;
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < N; j += 2 * k)
                for (int i = 0; i < k && i + j + k < N; ++i) {
                    const int a = i + j, b = i + j + k;
                    if (a / (2 * p) == b / (2 * p) && b < C) {
                        net.lo[net.n] = a;
                        net.hi[net.n] = b;
                        ++net.n;
                    }
                }
    return net;
}

OFL_HD void exchange(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}

template <int C, int... I>
OFL_HD void sort_net(float (&v)[C], std::integer_sequence<int, I...>) {
    constexpr Net net = make_net<C>();
    (exchange(v[net.lo[I]], v[net.hi[I]]), ...);
}

// v is left partially sorted
template <int C>
OFL_HD float median_of(float (&v)[C]) {
    static_assert(C >= 1 && C <= kMaxC, "register median: 1 <= C <= 16");
    bool nan = false;
#pragma unroll
    for (int c = 0; c < C; ++c) nan |= v[c] != v[c];
    constexpr Net net = make_net<C>();
    sort_net<C>(v, std::make_integer_sequence<int, net.n>{});
    float m;
    if constexpr (C % 2)
        m = v[C / 2];
    else
        m = (v[C / 2 - 1] + v[C / 2]) * 0.5f;  // halving is exact: same value as / 2
    return nan ? NAN : m;
}

}  // namespace mednet
