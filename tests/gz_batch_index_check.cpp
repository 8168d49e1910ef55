// Stand-alone checker of gz::inflate_batch_index (openfl_amd/csrc/gz_members.h)
// for tests/test_gz_batch_index_cpu.py.  argv[1]: native threads.  stdin: one
// payload per line, "hex pos out_off expect" ("-": empty), each copied into a
// heap block of exactly its length, so that a sanitizer sees a read past it.
// stdout: "V verdict..." | "N nlarge nsmall" | "M w0 w1 w2 w3" per record |
// "S payload..." for the one-segment members.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gz_format.h"
#include "gz_members.h"

int main(int argc, char** argv) {
    const int nthreads = argc > 1 ? atoi(argv[1]) : 1;
    std::vector<std::unique_ptr<uint8_t[]>> bufs;
    std::vector<const uint8_t*> src;
    std::vector<size_t> len;
    std::vector<int64_t> pos, out_off, expect;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream f(line);
        std::string hex;
        long long p, o, e;
        if (!(f >> hex >> p >> o >> e)) continue;
        const size_t n = hex == "-" ? 0 : hex.size() / 2;
        bufs.emplace_back(new uint8_t[n]);
        for (size_t i = 0; i < n; ++i) bufs.back()[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
        src.push_back(bufs.back().get());
        len.push_back(n);
        pos.push_back(p);
        out_off.push_back(o);
        expect.push_back(e);
    }
    std::vector<int32_t> verdict(src.size(), -1);
    gz::InflateBatchIndex X;
    gz::inflate_batch_index((int)src.size(), src.data(), len.data(), pos.data(), out_off.data(), expect.data(), nthreads,
                            verdict.data(), X);
    printf("V");
    for (int32_t v : verdict) printf(" %d", v);
    printf("\nN %lld %lld\n", (long long)X.nlarge, (long long)X.nsmall);
    for (size_t i = 0; i < X.rec.size(); i += gz::kIdxWords)
        printf("M %lld %lld %lld %lld\n", (long long)X.rec[i], (long long)X.rec[i + 1], (long long)X.rec[i + 2],
               (long long)X.rec[i + 3]);
    printf("S");
    for (int32_t p : X.small_payload) printf(" %d", p);
    printf("\n");
    return X.rec.size() == (size_t)gz::kIdxWords * (size_t)(X.nlarge + X.nsmall) ? 0 : 1;
}
