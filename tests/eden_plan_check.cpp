// Stand-alone checker of the Eden planner (openfl_amd/csrc/eden_plan.h): reads
// batches from stdin, one per line, builds their plans exactly as the library
// does and prints a canonical dump of each -- the layout, every field of every
// launch, what every launch resolves to, and the int tables.
// tests/test_eden_plan_cpu.py compares the dumps with the ones recorded from
// the commit before the planner moved into the header
// (tests/golden/eden_plan_parent.json).
//
// A case:  name n_bits wave_mib streams row2 pair sset fuse ntensors numel...
//          has_dims [nslices... dims...]
// Tensors lie in the arena as openfl_amd.codec.EdenPlan lays them: each starts
// at the next multiple of 64 elements.
//
// The dump (one record per line, fields in this order):
//   K id name                      the kernel table's ids and reported names (once)
//   case name
//   P nwaves ws_floats part_floats planes_bytes single ws_bytes nslices nints
//   S ws_off perm part_off pl_off pl_stride logp len ylen          per slice
//   L dir idx kind param lo mid a8 list_off tstart_off count blocks nu stream
//     btab_off ptab_off npair expl nt sset_off sset_groups bytes_moved bytes_alg
//   R ncu v id grid tab_off npair expl paired      after its L, for ncu 256 and
//     64; v = 1 (row A only): encode, the fused weighted-average call; decode,
//     an unaligned planes pointer
//   I ints, 16 per line
// A section (S; the L and R of one direction; I) of more than its limit is
// written as "tag# entries fnv1a64" over the lines it would have had.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eden_plan.h"

namespace {

// ---- the dump: shared word for word with the recorder of the golden -------
constexpr size_t kFullMax = 4096;    // slices and ints written in full
constexpr size_t kLaunchMax = 64;    // launches of one direction written in full

struct Section {
    std::string text;
    size_t lines = 0;
    void add(const std::string& s) { text += s; text += '\n'; ++lines; }
};
void emit(const char* tag, const Section& s, size_t entries, size_t limit) {
    if (entries <= limit) { fputs(s.text.c_str(), stdout); return; }
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s.text) { h ^= c; h *= 1099511628211ull; }
    printf("%s# %zu %016llx\n", tag, entries, (unsigned long long)h);
}
template <typename... T> std::string row(const char* tag, T... v) {
    std::ostringstream o;
    o << tag;
    ((o << ' ' << (long long)v), ...);
    return o.str();
}
struct SRow { int64_t ws_off, perm, part_off, pl_off, pl_stride, logp, len, ylen; };
struct LRow {
    int64_t kind, param, lo, mid, a8, list_off, tstart_off, count, blocks, nu, stream, btab_off, ptab_off, npair, expl, nt,
        sset_off, sset_groups, bytes_moved, bytes_alg;
};
struct RRow { int64_t id, grid, tab_off, npair, expl, paired; };
struct PRow { int64_t nwaves, ws_floats, part_floats, planes_bytes, single, ws_bytes; };

// A: the plan under the dump -- plan(), slices(), ints(), launches(enc),
// resolve(enc, idx, ncu, v)
template <typename A> void dump_case(const std::string& name, const A& a) {
    const std::vector<SRow> sl = a.slices();
    const std::vector<int32_t>& ints = a.ints();
    const PRow p = a.plan();
    printf("case %s\n", name.c_str());
    puts(row("P", p.nwaves, p.ws_floats, p.part_floats, p.planes_bytes, p.single, p.ws_bytes, sl.size(), ints.size()).c_str());
    Section S;
    for (const SRow& s : sl) S.add(row("S", s.ws_off, s.perm, s.part_off, s.pl_off, s.pl_stride, s.logp, s.len, s.ylen));
    emit("S", S, sl.size(), kFullMax);
    for (int enc = 1; enc >= 0; --enc) {
        const std::vector<LRow> L = a.launches(enc != 0);
        Section T;
        for (size_t i = 0; i < L.size(); ++i) {
            const LRow& l = L[i];
            T.add(row(enc ? "L e" : "L d", i, l.kind, l.param, l.lo, l.mid, l.a8, l.list_off, l.tstart_off, l.count, l.blocks,
                      l.nu, l.stream, l.btab_off, l.ptab_off, l.npair, l.expl, l.nt, l.sset_off, l.sset_groups, l.bytes_moved,
                      l.bytes_alg));
            for (int v = 0; v < (l.kind == 2 /* K_ROWA */ ? 2 : 1); ++v)
                for (int ncu : {256, 64}) {
                    const RRow r = a.resolve(enc != 0, (int)i, ncu, v);
                    T.add(row("R", ncu, v, r.id, r.grid, r.tab_off, r.npair, r.expl, r.paired));
                }
        }
        emit(enc ? "Le" : "Ld", T, L.size(), kLaunchMax);
    }
    Section I;
    for (size_t i = 0; i < ints.size(); i += 16) {
        std::string s = "I";
        for (size_t k = i; k < std::min(ints.size(), i + 16); ++k) s += ' ' + std::to_string(ints[k]);
        I.add(s);
    }
    emit("I", I, ints.size(), kFullMax);
}
// ---- end of the dump -------------------------------------------------------

struct Adapter {
    eden::Plan pl;
    PRow plan() const {
        return {pl.nwaves, pl.ws_floats, pl.part_floats, pl.planes_bytes, pl.single, eden::workspace_bytes(pl)};
    }
    std::vector<SRow> slices() const {
        std::vector<SRow> v;
        for (const eden::SliceDesc& D : pl.slices)
            v.push_back({D.ws_off, D.perm, D.part_off, D.pl_off, D.pl_stride, D.logp, D.len, D.ylen});
        return v;
    }
    const std::vector<int32_t>& ints() const { return pl.ints; }
    std::vector<LRow> launches(bool enc) const {
        std::vector<LRow> v;
        for (const eden::Launch& l : enc ? pl.enc : pl.dec)
            v.push_back({l.kind, l.param, l.lo, l.mid, l.a8, l.list_off, l.tstart_off, l.count, l.blocks, l.nu, l.stream,
                         l.btab_off, l.ptab_off, l.npair, l.expl, l.nt, l.sset_off, l.sset_groups, l.bytes_moved,
                         l.bytes_alg});
        return v;
    }
    RRow resolve(bool enc, int idx, int ncu, int v) const {
        eden::Resolved r;
        const char* err = eden::resolve(pl, (enc ? pl.enc : pl.dec)[idx], enc, ncu, enc && v, !v, r);
        if (err) return {-1, 0, 0, 0, 0, 0};
        return {r.id, r.grid, r.tab_off, r.npair, r.expl, r.paired};
    }
};

}  // namespace

int main() {
    for (int k = 0; k < eden::KERNEL_COUNT; ++k) printf("K %d %s\n", k, eden::kKernelName[k]);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name;
        long long n_bits, wave_mib, streams, row2, pair, sset, fuse, nt, has_dims = 0;
        if (!(in >> name >> n_bits >> wave_mib >> streams >> row2 >> pair >> sset >> fuse >> nt)) continue;
        std::vector<int64_t> numel(nt), offs(nt), dims;
        std::vector<int32_t> ns(nt);
        int64_t acc = 0;
        for (long long t = 0; t < nt; ++t) {
            long long n;
            in >> n;
            numel[t] = n;
            offs[t] = acc;
            acc += (n + 63) / 64 * 64;
        }
        in >> has_dims;
        if (has_dims) {
            long long v;
            for (long long t = 0; t < nt; ++t) { in >> v; ns[t] = (int32_t)v; }
            while (in >> v) dims.push_back(v);
        }
        if (!in && !in.eof()) { fprintf(stderr, "bad case line: %s\n", name.c_str()); return 2; }
        Adapter a;
        if (const char* err = eden::layout(a.pl, (int)nt, numel.data(), offs.data(), has_dims ? ns.data() : nullptr,
                                           has_dims ? dims.data() : nullptr, (int)n_bits)) {
            fprintf(stderr, "%s: %s\n", name.c_str(), err);
            return 2;
        }
        a.pl.wave_bytes = (int64_t)wave_mib << 20;
        a.pl.nstreams = (int)streams;
        a.pl.row2 = (int)row2;
        a.pl.pair = (int)pair;
        a.pl.sset = (int)sset;
        a.pl.fuse = (int)fuse;
        eden::build_schedule(a.pl, eden::kScheduleNcu);
        dump_case(name, a);
    }
    return 0;
}
