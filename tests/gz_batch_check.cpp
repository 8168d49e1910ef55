// Stand-alone checker of the batched gzip encoder's host-only code (gz_members.h:
// tlz_batch_layout, tlz_batch_plan, gzip_batch_ws) for tests/test_gz_batch_cpu.py.
// stdin: a tensor list per line, "offset:numel ..." ("-": empty).  stdout per list:
//   L ok members batch slot ops_stride stage bound | P ok | M start count tensor (table order)
//   O c0 j j ... (a launch's order) | W misalign ranks_end tab order tend end (workspace regions)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gz_members.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<int64_t> off, num;
        std::istringstream in(line == "-" ? "" : line);
        for (std::string tok; in >> tok;) {
            off.push_back(std::stoll(tok.substr(0, tok.find(':'))));
            num.push_back(std::stoll(tok.substr(tok.find(':') + 1)));
        }
        gz::TlzLayout L;
        size_t bound = 0;
        const bool ok = gz::tlz_batch_layout((int64_t)num.size(), num.data(), L, bound);
        printf("L %d %lld %lld %zu %zu %zu %zu\n", ok, (long long)L.members, (long long)L.batch, L.slot, L.ops_stride, L.stage, bound);
        gz::TlzBatchPlan P;
        const bool pok = gz::tlz_batch_plan((int64_t)num.size(), off.data(), num.data(), P);
        printf("P %d\n", pok);
        if (!pok) continue;
        for (const gz::tlz::MemberRec& r : P.rec) printf("M %lld %d %d\n", (long long)r.start, r.count, r.tensor);
        for (size_t c0 = 0; c0 < P.order.size(); c0 += gz::tlz::kBatch) {
            printf("O %zu", c0);
            for (size_t j = c0; j < P.order.size() && j < c0 + gz::tlz::kBatch; ++j) printf(" %d", P.order[j]);
            printf("\n");
        }
        for (uintptr_t mis : {0, 4}) {
            const gz::GzBatchWs W = gz::gzip_batch_ws(P.L, (int64_t)num.size(), (uintptr_t)0x7f12345600ull * 256 + mis);
            printf("W %d %zu %zu %zu %zu %zu\n", (int)mis, W.R.end, W.tab, W.order, W.tend, W.end);
        }
    }
    return 0;
}
