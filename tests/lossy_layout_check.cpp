// lossy_layout_check.cpp -- the host-only header of the lossy kernels
// (openfl_amd/csrc/lossy_layout.h) built and run alone, included exactly as
// the library includes it.  Each line of stdin is a case
//     <name> <T> <max_nk> <offset 0> <numel 0> <offset 1> <numel 1> ...
// and the program prints its chunk table, the regions and cleared spans of
// every family's workspace layout, and the totals the library reports:
//     case <name>
//     C <error> <blocks>              chunk_table's verdict
//     t <off> <n> <blk0> <nblk>       one per tensor
//     L <family> <end> <workspace bytes>
//     r <family> <region> <off> <bytes>
//     z <family> <span> <off> <bytes> <first region> <last region>
//     S <single-tensor workspace bytes for numel 0>
// Heap copies of exactly T entries, so a sanitizer sees any read past them.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lossy_layout.h"

namespace {
void region(const char* fam, const char* name, lossy::Span s) {
    std::printf("r %s %s %zu %zu\n", fam, name, s.off, s.bytes);
}
}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name;
        int T = 0, max_nk = 0;
        if (!(in >> name >> T >> max_nk) || T < 0) return 2;
        std::vector<int64_t> off(T), num(T);
        for (int t = 0; t < T; ++t)
            if (!(in >> off[t] >> num[t])) return 2;
        std::printf("case %s\n", name.c_str());
        lossy::ChunkTable tab;
        const lossy::ChunkErr e = lossy::chunk_table(T, off.data(), num.data(), tab);
        std::printf("C %d %lld\n", (int)e, (long long)tab.blocks);
        for (const lossy::BkmTensor& r : tab.td)
            std::printf("t %lld %lld %d %d\n", (long long)r.off, (long long)r.n, r.blk0, r.nblk);
        const int64_t blocks = lossy::count_chunks(T, num.data());

        const lossy::KmeansLayout K = lossy::kmeans_layout(T, blocks);
        std::printf("L kmeans %zu %zu\n", K.total, lossy::kmeans_workspace_bytes(T, num.data()));
        region("kmeans", "td", K.td); region("kmeans", "st", K.st); region("kmeans", "hc", K.hc);
        region("kmeans", "hs", K.hs); region("kmeans", "part", K.part); region("kmeans", "seeds", K.seeds);
        std::printf("z kmeans zeroed %zu %zu st hs\n", K.zeroed.off, K.zeroed.bytes);

        const lossy::TopkLayout P = lossy::topk_layout(T, blocks);
        std::printf("L topk %zu %zu\n", P.total, lossy::topk_workspace_bytes(T, num.data()));
        region("topk", "td", P.td); region("topk", "st", P.st); region("topk", "hist", P.hist);
        region("topk", "blk", P.blk);
        std::printf("z topk zeroed %zu %zu hist hist\n", P.zeroed.off, P.zeroed.bytes);

        const lossy::LutLayout U = lossy::lut_layout(T, max_nk);
        std::printf("L lut %zu %zu\n", U.total, lossy::lut_workspace_bytes(T, max_nk));
        region("lut", "td", U.td); region("lut", "nk", U.nk); region("lut", "keys", U.keys);
        region("lut", "vals", U.vals);

        const lossy::TernaryLayout R = lossy::ternary_layout(T);
        std::printf("L ternary %zu %zu\n", R.total, lossy::ternary_workspace_bytes(T));
        region("ternary", "td", R.td); region("ternary", "ranks3", R.ranks3);

        std::printf("S %zu\n", lossy::single_workspace_bytes(T ? num[0] : 0));
    }
    return 0;
}
