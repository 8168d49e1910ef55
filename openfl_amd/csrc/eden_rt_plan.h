// eden_rt_plan.h -- the schedule of the Eden round trip y = decode(encode(x))
// (ofl_eden_roundtrip), built from a plan's encode and decode schedules
// (eden_plan.h).  Host-only C++17 like the planner: own launch list, kernel
// ids and names, slice table and workspace size; Plan, its launch lists and
// workspace_bytes() are left as they are.
//
// A wave's launches become, on the wave's stream,
//   row A | encode's column launches | k_rt_row | k_finalize (the wave's
//   slices) | decode's column launches | row C
// so a wave's decode passes follow its encode passes while its intermediates
// sit in the Infinity Cache, and the planes of the large slices are never
// made.  A split 5-pass slice keeps its sub-waves: (row A, col) per sub-wave,
// the middle pass, (col, k_rt_row) per sub-wave, k_finalize, then decode's
// col per sub-wave, middle pass, (col, row C) per sub-wave.  The tiny / small
// slices keep their encode and decode launches, back to back on their stream,
// through a plane scratch appended to the workspace: their plane rows are
// packed there slice by slice (SliceDesc::pl_off / pl_stride of the round
// trip's own slice table), so the scratch is their planes' size and not the
// arena's.
#pragma once

#include "eden_plan.h"

namespace eden {

enum RtKernelId { RT_ROW, RT_KERNEL_COUNT };
constexpr const char* kRtKernelName[RT_KERNEL_COUNT] = {"ofl::k_rt_row"};

// dir: which schedule the launch comes from and how resolve() reads it
enum RtDir { RT_DEC = 0, RT_ENC = 1, RT_FUSED = 2 };  // RT_FUSED: encode's row C slot, run by k_rt_row
struct RtLaunch {
    Launch l;
    int dir;
};

struct RoundTrip {
    std::vector<RtLaunch> list;
    std::vector<SliceDesc> slices;  // the plan's, the tiny / small slices' planes in the scratch
    int64_t scratch_bytes = 0;
};

// workspace: the plan's own regions, then the small slices' plane scratch
inline int64_t rt_scratch_off(const Plan& pl) { return workspace_bytes(pl); }
inline int64_t rt_workspace_bytes(const Plan& pl, const RoundTrip& rt) {
    return rt_scratch_off(pl) + ((rt.scratch_bytes + 255) & ~255ll);
}

// -> nullptr, or what about the plan's schedules it could not follow
inline const char* build_roundtrip(const Plan& pl, RoundTrip& rt) {
    rt = RoundTrip{};
    rt.slices = pl.slices;
    for (SliceDesc& D : rt.slices) {
        if (D.logp > kRowLog) continue;
        D.pl_off = rt.scratch_bytes;
        D.pl_stride = (1ll << D.logp) / 8;
        rt.scratch_bytes += (D.pl_stride * pl.nbits + 15) & ~15ll;
    }
    const std::vector<Launch>&E = pl.enc, &Dl = pl.dec;
    auto small = [](const Launch& l) { return l.kind == K_TINY || l.kind == K_SMALL || l.kind == K_SSET; };
    size_t e = 0, d = 0;
    // the tiny / small slices' launches: encode, then decode behind it on the same stream
    auto small_run = [&] {
        while (e < E.size() && small(E[e])) rt.list.push_back({E[e++], RT_ENC});
        while (d < Dl.size() && small(Dl[d])) rt.list.push_back({Dl[d++], RT_DEC});
    };
    small_run();
    while (e < E.size() && E[e].kind == K_ROWA) {
        // the wave: up to the row A that follows a row C (a split slice has several of each)
        size_t ee = e;
        bool seen_c = false;
        for (; ee < E.size(); ++ee) {
            const int k = E[ee].kind;
            if (k == K_ROWC) seen_c = true;
            else if ((k == K_ROWA && seen_c) || small(E[ee]) || k == K_FINAL) break;
        }
        const size_t n = ee - e;
        if (!seen_c || d + n > Dl.size()) return "round trip: encode and decode schedules differ";
        for (size_t i = 0; i < n; ++i)
            if (E[e + i].kind != Dl[d + i].kind || E[e + i].stream != Dl[d + i].stream)
                return "round trip: encode and decode schedules differ";
        const Launch first = E[e];
        for (size_t i = e; i < ee; ++i) {
            RtLaunch r{E[i], E[i].kind == K_ROWC ? RT_FUSED : RT_ENC};
            if (r.dir == RT_FUSED) {  // reads and writes the fp32 tile: no algorithmic bytes
                r.l.bytes_moved = 2 * (r.l.bytes_moved - r.l.bytes_alg);
                r.l.bytes_alg = 0;
            }
            rt.list.push_back(r);
        }
        // the wave's scales, before its decode's last pass; row A carries the wave's slice list
        Launch f{K_FINAL, 0, 0, 0, first.list_off, -1, first.count, (int64_t)first.count};
        f.stream = first.stream;
        for (int i = 0; i < first.count; ++i) f.bytes_moved += 4ll << (pl.slices[pl.ints[first.list_off + i]].logp - kRowLog);
        rt.list.push_back({f, RT_ENC});
        for (size_t i = d; i < d + n; ++i)
            if (Dl[i].kind != K_ROWA) rt.list.push_back({Dl[i], RT_DEC});
        e = ee;
        d += n;
    }
    small_run();
    for (; e < E.size(); ++e)
        if (E[e].kind != K_FINAL) return "round trip: unexpected launch after the waves";
    if (d != Dl.size()) return "round trip: unexpected launch after the waves";
    return nullptr;
}

// What a round-trip launch runs: k_rt_row (rt = true; two blocks per CU, over
// the launch's tile table or explicit list, like encode's row C), or the
// plan's own kernel for the launch (eden::resolve).
struct RtResolved {
    Resolved r;
    bool rt;
};
inline const char* rt_resolve(const Plan& pl, const RtLaunch& x, int ncu, bool wavg, RtResolved& out) {
    out.rt = x.dir == RT_FUSED;
    const char* err = resolve(pl, x.l, x.dir != RT_DEC, ncu, wavg, true, out.r);
    if (!err && out.rt && out.r.id != ENC_ROWC2) err = "round trip: the fused row launch did not resolve as encode's row C";
    return err;
}

}  // namespace eden
