// median_net_host.cpp -- the 0/1 proof of openfl_amd/csrc/median_net.h on the
// host.  A compare-exchange network returns the right order statistic for every
// NaN-free input if and only if it does so for every input of zeros and ones,
// so for C = 1..16 all 2^C columns of 0/1 go through mednet::median_of<C> and
// are compared with the median of the std::sort-ed column (odd C: the middle
// value; even C: the float32 mean of the two middle values).
//
// Prints one line per C, "C <C> exchanges <n> columns <2^C> mismatches <k>",
// and exits 1 if any column differs.  Built and run by
// tests/test_robust_aggregation_cpu.py; needs only a C++17 compiler.
#include <algorithm>
#include <cstdio>

#include "median_net.h"

template <int C>
int check() {
    int bad = 0;
    for (unsigned m = 0; m < (1u << C); ++m) {
        float v[C], s[C];
        for (int c = 0; c < C; ++c) v[c] = s[c] = (float)((m >> c) & 1u);
        std::sort(s, s + C);
        const float ref = C % 2 ? s[C / 2] : (s[C / 2 - 1] + s[C / 2]) / 2.0f;
        const float got = mednet::median_of<C>(v);
        if (got != ref) {
            if (!bad) std::printf("C %d first mismatch: column %u got %g expected %g\n", C, m, got, ref);
            ++bad;
        }
    }
    std::printf("C %d exchanges %d columns %u mismatches %d\n", C, mednet::make_net<C>().n, 1u << C, bad);
    return bad;
}

template <int... C>
int check_all(std::integer_sequence<int, C...>) {
    return (check<C + 1>() + ...);
}

int main() {
    return check_all(std::make_integer_sequence<int, mednet::kMaxC>{}) ? 1 : 0;
}
