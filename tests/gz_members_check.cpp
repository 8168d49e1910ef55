// Stand-alone checker of the gzip codec's host-only code
// (openfl_amd/csrc/gz_format.h, gz_members.h): the parser of a member-indexed
// stream's headers, which reads untrusted bytes, and the workspace layouts.
// tests/test_gz_members_cpu.py feeds it the streams of tests/gz_members_cases.py
// and compares what it prints with the library's ofl_gzip_member_index and
// with the values recorded from the commit before this code moved into the
// headers (tests/golden/gz_index_parent.json).
//
// stdin: one stream per line, "name hex" ("name -" for the empty stream).
// Every stream is copied into a heap block of exactly its length, so that a
// sanitizer sees a read past its end.
//
// stdout:
//   stream name mode          mode: serial (walk_members alone), library
//                             (parse_members as the library calls it), small
//                             (4 threads, 256-byte pieces)
//   R rc nmembers total all_tlz
//   M w0 w1 w2 w3             the member's index record
// then the layouts:
//   W n misalign              the ofl_gzip_ranks workspace at 256 k + misalign
//   r name offset size        a region
//   E end bound               workspace bytes, ofl_gzip_ranks_bound
//   I nmembers status counts end      the inflate workspace
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "gz_format.h"
#include "gz_members.h"

namespace {

void report(const char* name, const char* mode, int rc, const std::vector<gz::GzMember>& mem, size_t total) {
    printf("stream %s %s\n", name, mode);
    bool tl = !mem.empty();
    for (const gz::GzMember& m : mem) tl = tl && m.tlz;
    printf("R %d %zu %zu %d\n", rc, mem.size(), total, tl ? 1 : 0);
    for (const gz::GzMember& m : mem) {
        int64_t r[gz::kIdxWords];
        gz::idx_pack(r, m.in, m.in_len, m.tlz, m.out, m.isize, m.crc);
        printf("M %lld %lld %lld %lld\n", (long long)r[0], (long long)r[1], (long long)r[2], (long long)r[3]);
    }
}

void check_stream(const std::string& name, const std::string& hex) {
    const size_t n = hex == "-" ? 0 : hex.size() / 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
    for (size_t i = 0; i < n; ++i) buf[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
    const uint8_t* src = buf.get();
    std::vector<gz::GzMember> mem;
    size_t total = 0;
    {
        size_t reached = 0;
        const bool ok = gz::walk_members(src, n, 0, n, mem, reached);
        if (!ok) mem.clear();
        for (const gz::GzMember& m : mem) total += m.isize;
        report(name.c_str(), "serial", ok ? OFL_OK : OFL_EFORMAT, mem, total);
    }
    const char* msg = "";
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    int rc = gz::parse_members(src, n, std::min(hw, 16u), (size_t)4 << 20, mem, total, &msg);
    report(name.c_str(), "library", rc, mem, total);
    rc = gz::parse_members(src, n, 4, 256, mem, total, &msg);
    report(name.c_str(), "small", rc, mem, total);
}

void check_layouts() {
    const int64_t B = 512 * 131072ll;
    const int64_t ns[] = {1, 2, 3, 2047, 2048, 2049, 131071, 131072, 131073, B - 1, B, B + 1, (int64_t)1 << 31};
    const uintptr_t origin = (uintptr_t)0x7f12345600ull * 256;
    for (int64_t n : ns)
        for (uintptr_t mis : {0, 4, 8, 255}) {
            const gz::GzRanksWs W = gz::gzip_ranks_ws(n, origin + mis);
            const size_t b = (size_t)W.L.batch;
            printf("W %lld %d\n", (long long)n, (int)mis);
            for (int i = 0; i < 2; ++i) printf("r slots%d %zu %zu\n", i, W.slots[i], b * W.L.slot);
            printf("r ops %zu %zu\n", W.ops, 4 * b * W.L.ops_stride);
            for (int i = 0; i < 2; ++i) printf("r sizes%d %zu %zu\n", i, W.sizes[i], 4 * b);
            for (int i = 0; i < 2; ++i) printf("r off%d %zu %zu\n", i, W.off[i], 8 * (b + 1));
            printf("r running %zu %zu\n", W.running, sizeof(uint64_t));
            printf("r bad %zu %zu\n", W.bad, sizeof(int));
            for (int i = 0; i < 2; ++i) printf("r stage%d %zu %zu\n", i, W.stage[i], W.L.stage);
            printf("E %zu %zu\n", W.end, gz::gzip_ranks_bound(n));
        }
    for (int64_t nm : {0, 1, 2, 511, 512, 513, 16384}) {
        const gz::InflateWs W = gz::inflate_ws(nm);
        printf("I %lld %zu %zu %zu\n", (long long)nm, W.status, W.counts, W.end);
    }
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t sp = line.find(' ');
        if (sp == std::string::npos) continue;
        check_stream(line.substr(0, sp), line.substr(sp + 1));
    }
    check_layouts();
    return 0;
}
