// eden_plan.h -- the Eden planner: from a batch of tensors to the slice
// descriptors, the waves and streams, every launch and every table the kernels
// index (formats: eden_desc.h), and from a launch to the kernel that runs it
// (resolve).  Pure integer logic on std::vectors, plain C++17 with no HIP
// header: eden_kernels.hip includes it for the library, and
// tests/eden_plan_check.cpp includes it to check plans on the CPU.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "eden_desc.h"

namespace eden {

using ofl::kColGroup;
using ofl::kColLog;
using ofl::kRowLog;
using ofl::kSetNT;
using ofl::kTinyNT;
using ofl::SliceDesc;

enum Kind { K_TINY, K_SMALL, K_ROWA, K_ROWC, K_COL, K_FINAL, K_COLM, K_SSET, K_COLMSET, KIND_COUNT };

struct Launch {
    int kind;        // Kind
    int param;       // p (small) / M (column)
    int lo;          // column passes: first transformed bit
    int mid;         // column: fused middle pass
    int list_off;    // into ints
    int tstart_off;  // into ints (multi-tile kernels), -1 otherwise
    int count;       // list entries
    int64_t blocks;  // tiles / work items; the grid unless resolve() says otherwise
    int a8 = 0;      // decode row A: every plane row is 8-byte aligned (8-byte plane words)
    int nu = 0;      // column: tile 0 of each slice writes the slice norm
    int stream = 0;  // 0: the caller's stream, 1: the plan's side stream, 2: its small-slice stream
    int btab_off = -1;  // column: per-block {slice, tile << 3 | group} table in ints
    int ptab_off = -1;  // row: the paired table {slice, tile << 3 | pair} in ints (npair entries)
    int npair = 0;
    // a sub-wave launch of a split 5-pass slice (split_wave_launches): it
    // covers the `blocks` tiles listed in btab_off ({slice, tile << 3}); row
    // launches that apply D1 may take the paired list ptab_off (npair entries)
    // instead
    bool expl = false;
    bool nt = false;  // column: the intermediate streams through HBM (k_col6<..., true>)
    int sset_off = -1;  // K_COLMSET: the small-set group table in ints
    int sset_groups = 0;  // K_COLMSET: its groups (the launch's first blocks)
    int64_t bytes_moved = 0;  // fp32/plane bytes this launch reads + writes (intermediates included)
    int64_t bytes_alg = 0;    // its share of the SURVEY 8(d) algorithmic bytes (x/y fp32 + planes only)
};

// Every kernel a plan can launch: eden_kernels.hip keeps one table entry
// (function, threads, LDS bytes) per id, in this order.  The compiler emits
// the template instances in the order the table names them, so the order here
// is the kernels' order in the code object.
enum KernelId {
    ENC_TINY, DEC_TINY, ENC_SSET, DEC_SSET, ENC_ROWA, DEC_ROWC, COL_MULTI, ENC_COLM_SET, DEC_COLM_SET, ENC_ROWC2,
    DEC_ROWC2, FINALIZE,
    DEC_ROWA_A8, DEC_ROWA, ENC_ROWA2, ENC_ROWA2_WAVG, DEC_ROWA2_A8, DEC_ROWA2,
    COL_MID6, COL_OUT6, COL_OUT7,
    COL6_MID7, COL6_MID8, COL6_MID9, COL6_MID10, COL6_MID7_NT,
    ENC_SMALL11, DEC_SMALL11, ENC_SMALL12, DEC_SMALL12, ENC_SMALL13, DEC_SMALL13, ENC_SMALL14, DEC_SMALL14,
    ENC_SMALL15, DEC_SMALL15,
    COL_MID1, COL_MID2, COL_MID3, COL_MID4, COL_MID5, COL_OUT5,
    KERNEL_COUNT
};

// The names the plan reports (ofl_eden_plan_launch_info): the row kernels'
// template arguments (<A8>, <WAVG>) are not part of them.
constexpr const char* kKernelName[KERNEL_COUNT] = {
    "ofl::k_enc_tiny", "ofl::k_dec_tiny", "ofl::k_enc_sset", "ofl::k_dec_sset", "ofl::k_enc_rowA", "ofl::k_dec_rowC",
    "ofl::k_col_multi", "ofl::k_enc_colm_set", "ofl::k_dec_colm_set", "ofl::k_enc_rowC2", "ofl::k_dec_rowC2",
    "ofl::k_finalize",
    "ofl::k_dec_rowA", "ofl::k_dec_rowA", "ofl::k_enc_rowA2", "ofl::k_enc_rowA2", "ofl::k_dec_rowA2", "ofl::k_dec_rowA2",
    "ofl::k_col<6, true>", "ofl::k_col<6, false>", "ofl::k_col<7, false>",
    "ofl::k_col6<7, true, 15>", "ofl::k_col6<8, true, 15>", "ofl::k_col6<9, true, 15>", "ofl::k_col6<10, true, 15>",
    "ofl::k_col6<7, true, 15, true>",
    "ofl::k_enc_small<11>", "ofl::k_dec_small<11>", "ofl::k_enc_small<12>", "ofl::k_dec_small<12>",
    "ofl::k_enc_small<13>", "ofl::k_dec_small<13>", "ofl::k_enc_small<14>", "ofl::k_dec_small<14>",
    "ofl::k_enc_small<15>", "ofl::k_dec_small<15>",
    "ofl::k_col<1, true>", "ofl::k_col<2, true>", "ofl::k_col<3, true>", "ofl::k_col<4, true>", "ofl::k_col<5, true>",
    "ofl::k_col<5, false>",
};

// The host-only state of a plan: the batch's layout (layout), the schedule
// knobs, and the schedule built from both (build_schedule).
struct Plan {
    int nbits = 8;
    int ntensors = 0;
    std::vector<SliceDesc> slices;
    std::vector<int64_t> t_planes_off, t_planes_bytes;
    std::vector<int32_t> t_first, t_nslices;
    int64_t planes_bytes = 0;
    int64_t ws_floats = 0;      // intermediates
    int64_t part_floats = 0;    // partials
    int64_t arena = 0;          // fp32 arena length: max over tensors of elem_offset + numel
    // slice ids per kernel class (fixed by the batch) and the schedule built
    // from them (build_schedule)
    std::vector<int32_t> tiny, small[5], large;
    int64_t wave_bytes = 0;     // intermediate bytes per wave of large slices; 0: one wave
    int nstreams = 1;           // 2: waves alternate between the caller's and a side stream
    int nwaves = 0;
    int row2 = -1;              // row launches on the two-blocks-per-CU kernels: -1 auto, 0 never, 1 always
    int pair = -1;              // their tile pairs sharing D1 words: -1 auto, 0 never, 1 whenever possible
    int sset = -1;              // tiny / small slices in one small-set launch: -1 default (yes), 0 no, 1 yes
    int fuse = -1;              // small-set groups fused into the column launch: -1 default (yes), 0 no, 1 yes
    bool single = false;        // every launch on the caller's stream (no fork / join) -- K_COLMSET plans
    std::vector<Launch> enc, dec;
    std::vector<int32_t> ints;  // launch lists, tile prefixes and tables (host copy; formats: eden_desc.h)
};

// Default large-slice schedule (see build_schedule):
// waves the size of the 256 MiB Infinity Cache's working half on two streams,
// with the two-blocks-per-CU row kernels (1-2 tiles per CU per wave).  Since
// the additive-LCG signs these beat 2 GiB waves on the Llama-3-8B step (429-431
// vs 426-427 GiB/s) and the 1 GiB set (470-474 vs 458-461); 256 MiB waves lose
// (420-422 / 450-452), profiles/r06_sched_ab.txt.  Slices above the wave size
// (the 2^29 ones) are waves of their own and keep the persistent kernels.
constexpr int64_t kDefaultWaveMiB = 128;
constexpr int64_t kDefaultStreams = 2;

// The schedule is built before any device is known, for this many CUs: the
// count enters the split-slice decision (split_wave_launches, through
// use_row2).  resolve() is evaluated at run time with the device's real count.
// The two differ on purpose; the schedule of a batch does not depend on the
// device it later runs on.
constexpr int kScheduleNcu = 256;

inline int64_t low_po2(int64_t n) { int64_t p = 1; while (p * 2 <= n) p *= 2; return n ? p : 0; }
inline int64_t high_po2(int64_t n) { int64_t p = 1; while (p < n) p *= 2; return n ? p : 0; }
inline int ilog2(int64_t v) { int l = 0; while ((1ll << l) < v) ++l; return l; }

// Reference slicing rule (eden_pipeline.py:569-606) -> slices of n elements
inline int slice_plan(int64_t n, int64_t* P_out, int64_t* len_out, int max_slices) {
    if (n <= 0) return 0;
    int64_t rem = n;
    int ns = 0;
    while ((double)(high_po2(rem) - rem) / (double)n > 0.1) {
        const int64_t low = low_po2(rem);
        if (ns < max_slices) {
            if (P_out) P_out[ns] = std::max<int64_t>(low, 8);
            if (len_out) len_out[ns] = low;
        }
        ++ns;
        rem -= low;
    }
    if (ns < max_slices) {
        if (P_out) P_out[ns] = std::max<int64_t>(high_po2(rem), 8);
        if (len_out) len_out[ns] = rem;
    }
    return ns + 1;
}

// The batch's layout: slice descriptors, per-tensor plane ranges and the
// per-class slice lists.  slice_dims (nullable): nslices[t] padded sizes per
// tensor instead of the slicing rule.  -> nullptr, or what is wrong.
inline const char* layout(Plan& pl, int ntensors, const int64_t* numel, const int64_t* elem_offset,
                          const int32_t* nslices, const int64_t* slice_dims, int n_bits) {
    pl.nbits = n_bits;
    pl.ntensors = ntensors;
    for (int t = 0; t < ntensors; ++t) pl.arena = std::max(pl.arena, elem_offset[t] + numel[t]);
    int64_t dims_pos = 0;
    for (int t = 0; t < ntensors; ++t) {
        const int64_t n = numel[t];
        std::vector<int64_t> Ps, Ls;  // padded sizes, valid input lengths
        if (slice_dims) {
            int64_t rem = n;
            for (int k = 0; k < nslices[t]; ++k) {
                const int64_t P = slice_dims[dims_pos + k];
                Ps.push_back(P);
                Ls.push_back(std::max<int64_t>(0, std::min<int64_t>(P, rem)));
                rem -= Ls.back();
            }
            dims_pos += nslices[t];
        } else {
            int ns = slice_plan(n, nullptr, nullptr, 0);
            Ps.resize(ns);
            Ls.resize(ns);
            slice_plan(n, Ps.data(), Ls.data(), ns);
        }
        int64_t Ptot = 0;
        for (int64_t P : Ps) {
            if (P < 8 || (P & (P - 1)) || P > (1ll << 29)) return "slice size must be a power of two in [8, 2^29]";
            Ptot += P;
        }
        pl.t_first.push_back((int32_t)pl.slices.size());
        pl.t_nslices.push_back((int32_t)Ps.size());
        const int64_t poff = (pl.planes_bytes + 255) & ~255ll;
        pl.t_planes_off.push_back(poff);
        pl.t_planes_bytes.push_back(Ptot / 8 * n_bits);
        pl.planes_bytes = poff + Ptot / 8 * n_bits;
        // Encode reads slice k from input offset sum(len_k') (Eden.compress
        // advances by the valid length, :599-602); decode writes slice k's P
        // outputs at sum(P_k') and truncates to total_dim (:650-657).  The two
        // differ only for n < ~150 with a sub-8 non-final slice (reproduced).
        int64_t off = 0, xoff = 0;
        for (size_t k = 0; k < Ps.size(); ++k) {
            const int64_t P = Ps[k];
            SliceDesc D{};
            D.x_off = elem_offset[t] + xoff;
            D.len = Ls[k];
            D.y_off = elem_offset[t] + off;
            D.ylen = std::max<int64_t>(0, std::min<int64_t>(P, n - off));
            D.pl_off = poff + off / 8;
            D.pl_stride = Ptot / 8;
            D.logp = ilog2(P);
            D.tensor = t;
            D.scale_idx = (int32_t)pl.slices.size();
            const int si = (int)pl.slices.size();
            if (D.logp <= 10) pl.tiny.push_back(si);
            else if (D.logp <= kRowLog) pl.small[D.logp - 11].push_back(si);
            else {
                D.part_off = (int32_t)pl.part_floats;  // ws_off: build_schedule
                pl.part_floats += P >> kRowLog;
                pl.large.push_back(si);
            }
            pl.slices.push_back(D);
            off += P;
            xoff += D.len;
        }
    }
    return nullptr;
}

inline int64_t workspace_bytes(const Plan& pl) {
    // intermediates | partials | norms, each 256-B aligned
    auto al = [](int64_t b) { return (b + 255) & ~255ll; };
    // per-slice norms are indexed by slice id (all slices, not only large ones)
    const int64_t nnu = (int64_t)pl.slices.size();
    return al(pl.ws_floats * 4) + al(pl.part_floats * 4) + al(nnu * 4) + 256;
}

// Row launches of fewer than kRow2MaxTilesPerCu tiles per CU use the
// two-blocks-per-CU kernels (k_enc_rowA2 / k_dec_rowA2 / k_dec_rowC2; outputs
// bit-identical).  plan_mode (Plan::row2) 0: never, 1: always, -1: below the
// threshold.
constexpr int64_t kRow2MaxTilesPerCu = 5;
inline bool use_row2(int64_t tiles, int ncu, int plan_mode) {
    return plan_mode >= 0 ? plan_mode == 1 : tiles < kRow2MaxTilesPerCu * (int64_t)ncu;
}

// row launches up to this many tiles carry a per-tile table (8 B per tile)
constexpr int64_t kRowTabMax = 1 << 16;
// two-blocks-per-CU row launches of more tiles than block slots run tile
// pairs sharing their D1 words (apply_signs_pair; plan_mode, Plan::pair,
// 0: never, 1: whenever the launch has a paired table)
inline bool use_pair(const Launch& l, int ncu, int plan_mode) {
    if (l.ptab_off < 0) return false;
    return plan_mode >= 0 ? plan_mode == 1 : l.blocks > 2 * (int64_t)ncu;
}

// Single-level heights up to kColMultiMax share one k_col_multi launch per
// wave.  Height 6 (2^21 slices) runs col_body<6> there (1024 threads, the
// k_col arithmetic), not k_col6<6, true, 15>: the two differ in the order of
// the row butterflies after D2, so their bytes differ slightly, and a
// standalone height-6 launch uses k_col<6, true> too.
constexpr int kColMultiMax = 6;
// the kernel of a middle pass of height 1..10, of an outer pass of height 5..7
constexpr KernelId kColMid[10] = {COL_MID1, COL_MID2, COL_MID3, COL_MID4, COL_MID5, COL_MID6,
                                  COL6_MID7, COL6_MID8, COL6_MID9, COL6_MID10};
constexpr KernelId kColOut[3] = {COL_OUT5, COL_OUT6, COL_OUT7};

// ---------------------------------------------------------------------------
// From a launch to its kernel
// ---------------------------------------------------------------------------
struct Resolved {
    KernelId id;
    int64_t grid;   // workgroups
    int tab_off;    // the block table in ints to pass as KArgs::btab (-1: none)
    int npair;      // KArgs::npair: entries of that table (0: the launch's tile prefix)
    bool expl;      // over an explicit tile list (a sub-wave of a split 5-pass slice)
    bool paired;    // a row launch whose table lists tile pairs
};

// What a launch runs -- decided here alone, for run() and for the names and
// details the plan reports.  ncu: the device's CU count (persistent row
// launches: one block per CU); wavg: the call is the fused weighted-average
// encode (base.wx), whose pass A is k_enc_rowA2<true> and never takes tile
// pairs; planes8: the call's planes pointer is 8-byte aligned (decode row A).
// -> nullptr, or the error (a height or size no kernel exists for).
inline const char* resolve(const Plan& pl, const Launch& l, bool enc, int ncu, bool wavg, bool planes8, Resolved& r) {
    r = Resolved{FINALIZE, l.blocks, l.btab_off, 0, l.expl, false};
    switch (l.kind) {
    case K_TINY: r.id = enc ? ENC_TINY : DEC_TINY; return nullptr;
    case K_SSET: r.id = enc ? ENC_SSET : DEC_SSET; return nullptr;
    case K_SMALL:
        if (l.param < 11 || l.param > 15) return "small slice size out of range";
        r.id = (KernelId)(ENC_SMALL11 + 2 * (l.param - 11) + (enc ? 0 : 1));
        return nullptr;
    case K_ROWA:
    case K_ROWC: {
        const bool rowa = l.kind == K_ROWA;
        wavg = wavg && rowa && enc;
        const bool signs = rowa ? enc : !enc;  // the pass that applies D1
        bool two = false;  // the two-blocks-per-CU kernel (k_*_row?2), else the persistent one
        r.grid = std::min<int64_t>(l.blocks, ncu);
        if (l.expl) {
            two = true;
            r.paired = signs && !wavg && l.ptab_off >= 0;
            r.tab_off = r.paired ? l.ptab_off : l.btab_off;
            r.npair = r.paired ? l.npair : (int)l.blocks;
            r.grid = std::min<int64_t>(r.npair, 2 * ncu);
        } else if (rowa ? wavg || use_row2(l.blocks, ncu, pl.row2)
                        // encode pass C has the two-blocks-per-CU kernel only (k_enc_rowC2)
                        : enc || use_row2(l.blocks, ncu, pl.row2)) {
            two = true;
            r.grid = std::min<int64_t>(l.blocks, 2 * ncu);
            if (signs && !wavg && use_pair(l, ncu, pl.pair)) {
                r.paired = true;
                r.tab_off = l.ptab_off;
                r.npair = l.npair;
                r.grid = std::min<int64_t>(l.npair, 2 * ncu);
            }
        }
        const bool a8 = l.a8 && planes8;
        if (rowa)
            r.id = enc ? (two ? (wavg ? ENC_ROWA2_WAVG : ENC_ROWA2) : ENC_ROWA)
                       : two ? (a8 ? DEC_ROWA2_A8 : DEC_ROWA2) : (a8 ? DEC_ROWA_A8 : DEC_ROWA);
        else
            r.id = enc ? ENC_ROWC2 : two ? DEC_ROWC2 : DEC_ROWC;
        return nullptr;
    }
    case K_COL:
        // build_schedule makes middle passes of heights 1..10 (k_col to
        // kColMultiMax, k_col6 above: measured, the 1024-thread k_col is ~4 %
        // faster on the plain M = 7 pass) and outer passes, the level-1 halves
        // of the two-level slices 2^26..2^29, of heights 5..7 (k_col)
        if (l.nt && l.param == 7 && l.mid) r.id = COL6_MID7_NT;
        else if (l.mid && l.param >= 1 && l.param <= 10) r.id = kColMid[l.param - 1];
        else if (!l.mid && l.param >= 5 && l.param <= 7) r.id = kColOut[l.param - 5];
        else return "column pass height out of range";
        return nullptr;
    case K_FINAL: r.id = FINALIZE; return nullptr;
    case K_COLM: r.id = COL_MULTI; return nullptr;
    case K_COLMSET: r.id = enc ? ENC_COLM_SET : DEC_COLM_SET; return nullptr;
    }
    return "unknown launch kind";
}

// ---------------------------------------------------------------------------
// The schedule
// ---------------------------------------------------------------------------
namespace detail {

inline int add_list(std::vector<int32_t>& ints, const std::vector<int32_t>& l) {
    const int o = (int)ints.size();
    ints.insert(ints.end(), l.begin(), l.end());
    return o;
}
inline int add_prefix(Plan& pl, const std::vector<int32_t>& l, int log_tile, int64_t& total) {
    const int o = (int)pl.ints.size();
    int64_t acc = 0;
    for (int32_t si : l) { pl.ints.push_back((int32_t)acc); acc += 1ll << (pl.slices[si].logp - log_tile); }
    pl.ints.push_back((int32_t)acc);
    total = acc;
    return o;
}

// The tiny / small slices' launches (stream 0; build_schedule places them).
inline std::vector<Launch> small_launches(Plan& pl) {
    std::vector<int32_t>& ints = pl.ints;
    std::vector<Launch> common;
    if (pl.sset != 0) {
        // one small-set launch: groups of one size, largest first; table of
        // {P (0: tiny), slice-list offset (from the table), count} per block
        std::vector<std::array<int32_t, 3>> groups;
        std::vector<int32_t> ids;
        auto add_groups = [&](int P, const std::vector<int32_t>& sl, int per) {
            for (size_t i = 0; i < sl.size(); i += per) {
                const int c = (int)std::min<size_t>(per, sl.size() - i);
                groups.push_back({P, (int32_t)ids.size(), c});
                ids.insert(ids.end(), sl.begin() + i, sl.begin() + i + c);
            }
        };
        for (int k = 4; k >= 0; --k) add_groups(11 + k, pl.small[k], kSetNT >> (6 + k));
        for (int p = 10; p >= 0; --p) {  // tiny slices: groups of one p (same barrier count)
            std::vector<int32_t> sl;
            for (int32_t si : pl.tiny) if (pl.slices[si].logp == p) sl.push_back(si);
            add_groups(0, sl, kSetNT / kTinyNT);
        }
        if (!groups.empty()) {
            const int o = (int)ints.size();
            const int nt = 3 * (int)groups.size();
            for (auto& g : groups) { ints.push_back(g[0]); ints.push_back(g[1] + nt); ints.push_back(g[2]); }
            ints.insert(ints.end(), ids.begin(), ids.end());
            common.push_back({K_SSET, 0, 0, 0, o, -1, (int)groups.size(), (int64_t)groups.size()});
        }
    } else {
        if (!pl.tiny.empty())
            common.push_back({K_TINY, 0, 0, 0, add_list(ints, pl.tiny), -1, (int)pl.tiny.size(), (int64_t)pl.tiny.size()});
        for (int k = 0; k < 5; ++k)
            if (!pl.small[k].empty())
                common.push_back({K_SMALL, 11 + k, 0, 0, add_list(ints, pl.small[k]), -1, (int)pl.small[k].size(),
                                  (int64_t)pl.small[k].size()});
    }
    return common;
}

struct Waves {
    std::vector<std::vector<int32_t>> waves;  // slice ids
    int64_t cap = 0;   // elements per wave (INT64_MAX: one wave)
    int nbuf = 1;      // workspace buffers = wave streams (wave w: buffer and stream w % nbuf)
};

// Large slices run in waves of at most wave_bytes of intermediates (a bigger
// slice is a wave of its own).  Packs them, and sets nwaves, ws_floats and
// every large slice's ws_off.  small: the plan has small-slice launches;
// sset: as one small-set launch.
inline Waves pack_waves(Plan& pl, bool small, bool sset) {
    Waves W;
    int64_t cap = pl.wave_bytes > 0 ? pl.wave_bytes / 4 : INT64_MAX;
    int64_t tot = 0;
    for (int32_t si : pl.large) tot += 1ll << pl.slices[si].logp;
    // more than one wave by size: the large slices largest first (stable), so
    // in-order packing fills each wave with slices of one size -- power-of-two
    // sizes pack whole waves, one column launch per wave (batch order and
    // smallest first both lost, profiles/r06_sort_roll_ab.txt).
    // Llama-3-8B: 210 waves of 1024 tiles (but the two 2^29 ones), 637
    // launches per direction instead of 258 waves of 512-1024 tiles and 909
    // launches; 434.8-435.4 -> 445.7-448.8 GiB/s
    std::vector<int32_t> sorted_large;
    if (tot > cap) {
        sorted_large = pl.large;
        std::stable_sort(sorted_large.begin(), sorted_large.end(),
                         [&](int32_t x, int32_t y) { return pl.slices[x].logp > pl.slices[y].logp; });
    }
    const std::vector<int32_t>& large = sorted_large.empty() ? pl.large : sorted_large;
    // two streams: at least two waves, so both streams have work -- unless
    // every large slice fits one wave and no small-slice launches could use
    // the second stream (at 2 GiB waves the 1 GiB set ran one wave on one
    // stream, 2.24 vs 2.29 ms; ResNet-50 keeps its two waves beside the small slices: 360
    // vs 369 us with one wave)
    // With the small-set launch a plan that fits one wave keeps it whole: the
    // one small-set launch runs beside it on the side stream (ResNet-50 0.288
    // vs 0.309 ms with two waves, profiles/r03_resnet50_sset_onewave_ab.txt)
    const bool split = (small && !sset) || tot > cap;
    // the split only feeds the second stream (everything fits one wave):
    // exactly two waves, cut where the halves are closest (in-order packing
    // against a half-total cap can leave a third wave behind the first on the
    // same stream -- ResNet-50: 417 vs 353 tiles per stream)
    int64_t cut = -1;
    if (pl.nstreams == 2 && split && tot <= cap && large.size() > 1) {
        int64_t pre = 0, best = INT64_MAX;
        for (size_t k = 0; k + 1 < large.size(); ++k) {
            pre += 1ll << pl.slices[large[k]].logp;
            const int64_t d = std::llabs(2 * pre - tot);
            if (d < best) { best = d; cut = (int64_t)k + 1; }
        }
    } else if (pl.nstreams == 2 && split) {
        cap = std::min(cap, std::max<int64_t>(1, (tot + 1) / 2));
    }
    int64_t acc = 0, wmax = 0;
    for (size_t k = 0; k < large.size(); ++k) {
        const int32_t si = large[k];
        const int64_t P = 1ll << pl.slices[si].logp;
        if (W.waves.empty() || (cut >= 0 ? (int64_t)k == cut : acc + P > cap)) { W.waves.emplace_back(); acc = 0; }
        W.waves.back().push_back(si);
        acc += P;
        wmax = std::max(wmax, acc);
    }
    W.cap = cap;
    W.nbuf = W.waves.size() > 1 ? pl.nstreams : 1;
    pl.nwaves = (int)W.waves.size();
    pl.ws_floats = W.nbuf * wmax;
    for (size_t w = 0; w < W.waves.size(); ++w) {
        int64_t off = (int64_t)(w % W.nbuf) * wmax;
        for (int32_t si : W.waves[w]) { pl.slices[si].ws_off = off; off += 1ll << pl.slices[si].logp; }
    }
    return W;
}

// A 5-pass slice bigger than the wave size (its own wave): passes 1-2
// (row bits 0..14, column level 1 bits 15..15+m1-1) touch only a
// sub-block of 2^(15+m1) consecutive elements, and so do passes 4-5,
// so they run sub-wave by sub-wave (half a wave of nibble-even tiles
// and their pair partners 2^(p-18) tiles up), each sub-wave's two
// passes back to back while its intermediate sits in the MALL; the
// middle pass (column level 2 + D2) spans the slice and runs whole,
// writing the slice norm (it follows every row-A sub-wave).  Launches
// of one stream run in order, so no other synchronisation.
// wl: the wave; s: its stream; lo_l, rp: its slice list and row-tile prefix
// in ints.  -> false: not such a wave, nothing added.
inline bool split_wave_launches(Plan& pl, const std::vector<int32_t>& wl, int64_t cap, int s, int lo_l, int rp, int a8,
                                int ncu) {
    if (!(wl.size() == 1 && cap != INT64_MAX && pl.slices[wl[0]].logp - kRowLog >= 11)) return false;
    std::vector<int32_t>& ints = pl.ints;
    const int32_t si = wl[0];
    const int p = pl.slices[si].logp, r = p - kRowLog, m1 = r / 2, m2 = r - m1;
    const int64_t ntile = 1ll << r, sub = 1ll << m1, P = 1ll << (p - 18);
    const int64_t cap_t = cap >> kRowLog;
    const int64_t half = (cap_t / 2) / sub * sub;  // sub-wave size: the wave size
    if (!(half >= sub && cap_t < ntile && ntile <= kRowTabMax && use_row2(2 * std::min(half, P), ncu, pl.row2)))
        return false;
    const bool pair = pl.pair != 0;
    const int lo_c = add_list(ints, wl);
    int64_t tiles_all = 0;
    const int tp = add_prefix(pl, wl, kColLog, tiles_all);
    struct SubWave { int tab_all, tab_pair; int64_t n_all, n_pair; };
    std::vector<SubWave> sws;
    for (int64_t reg = 0; reg < ntile; reg += 2 * P)
        for (int64_t c = 0; c < P; c += half) {
            const int64_t e = std::min(P, c + half);
            SubWave sw;
            sw.tab_all = (int)ints.size();
            for (int64_t h = 0; h < 2; ++h)
                for (int64_t t = reg + c + h * P; t < reg + e + h * P; ++t) {
                    ints.push_back(si);
                    ints.push_back((int32_t)(t << 3));
                }
            sw.n_all = 2 * (e - c);
            sw.tab_pair = (int)ints.size();
            for (int64_t t = reg + c; t < reg + e; ++t) {
                ints.push_back(si);
                ints.push_back((int32_t)(t << 3) | 1);
            }
            sw.n_pair = e - c;
            sws.push_back(sw);
        }
    auto rowl = [&](Kind k, const SubWave& sw, bool paired) {
        Launch l{k, 0, 0, 0, lo_l, rp, 1, sw.n_all};
        l.expl = true;
        l.btab_off = sw.tab_all;
        if (paired) { l.ptab_off = sw.tab_pair; l.npair = (int)sw.n_pair; }
        l.stream = s;
        return l;
    };
    auto coll = [&](const SubWave& sw) {
        Launch l{K_COL, m1, kRowLog, 0, lo_c, tp, 1, sw.n_all};
        l.expl = true;
        l.btab_off = sw.tab_all;
        l.stream = s;
        return l;
    };
    for (int dir = 0; dir < 2; ++dir) {
        const bool enc = dir == 1;
        std::vector<Launch>& L = enc ? pl.enc : pl.dec;
        for (const SubWave& sw : sws) {
            Launch ra = rowl(K_ROWA, sw, enc && pair);
            if (!enc) ra.a8 = a8;
            L.push_back(ra);
            L.push_back(coll(sw));
        }
        Launch mid{K_COL, m2, kRowLog + m1, 1, lo_c, tp, 1, tiles_all};
        mid.stream = s;
        mid.nt = m2 == 7;  // it streams its intermediate with nt loads and stores
        mid.nu = enc ? 1 : 0;  // after every row-A sub-wave: the slice norm
        L.push_back(mid);
        for (const SubWave& sw : sws) {
            L.push_back(coll(sw));
            L.push_back(rowl(K_ROWC, sw, !enc && pair));
        }
    }
    return true;
}

// An ordinary wave: row pass A, its column passes and row pass C back to
// back, so its intermediates are re-read while they still sit in the 256 MiB
// Infinity Cache.  sset: the small-set launch whose groups ride in the wave's
// k_col_multi launch (fused plans), else nullptr.
inline void wave_launches(Plan& pl, const std::vector<int32_t>& wl, int s, int lo_l, int rp, int64_t rows, int a8,
                          const Launch* sset) {
    std::vector<int32_t>& ints = pl.ints;
    std::map<int, std::vector<int32_t>> byp;  // column launches grouped by p
    for (int32_t si : wl) byp[pl.slices[si].logp].push_back(si);
    std::vector<Launch> ce, cd;
    // heights 1..kColMultiMax -> one k_col_multi
    std::vector<std::pair<int, const std::vector<int32_t>*>> mg;
    for (auto& kv : byp)
        if (kv.first - kRowLog >= 1 && kv.first - kRowLog <= kColMultiMax) mg.push_back({kv.first - kRowLog, &kv.second});
    if (mg.size() < 2) mg.clear();
    if (!mg.empty()) {
        const int gt = (int)ints.size();
        ints.resize(ints.size() + kColGroup * mg.size());
        int64_t blk = 0, mv = 0;
        for (size_t g = 0; g < mg.size(); ++g) {
            int64_t tiles = 0;
            const int lo_c = add_list(ints, *mg[g].second);
            const int tp = add_prefix(pl, *mg[g].second, kColLog, tiles);
            int32_t* G = &ints[gt + kColGroup * g];
            G[0] = mg[g].first;
            G[1] = lo_c - gt;
            G[2] = tp - gt;
            G[3] = (int32_t)mg[g].second->size();
            G[4] = (int32_t)blk;
            blk += tiles;
            for (int32_t si : *mg[g].second) mv += 8ll << pl.slices[si].logp;
        }
        Launch l{K_COLM, 0, kRowLog, 1, gt, -1, (int)mg.size(), blk};
        l.stream = s;
        l.bytes_moved = mv;
        if (sset) {  // the small-set groups ride in this launch (its first blocks)
            l.kind = K_COLMSET;
            l.sset_off = sset->list_off;
            l.sset_groups = sset->count;
            l.blocks += sset->count;
        }
        cd.push_back(l);
        l.nu = 1;  // encode: every group is a slice's first (only) column launch
        ce.push_back(l);
    }
    for (auto& kv : byp) {
        const int r = kv.first - kRowLog;
        if (!mg.empty() && r >= 1 && r <= kColMultiMax) continue;  // in the k_col_multi launch
        int64_t tiles = 0;
        const int lo_c = add_list(ints, kv.second);
        const int tp = add_prefix(pl, kv.second, kColLog, tiles);
        const int cnt = (int)kv.second.size();
        std::vector<Launch> seq;
        if (r <= 10) {
            seq.push_back({K_COL, r, kRowLog, 1, lo_c, tp, cnt, tiles});
            if (r == 10)  // k_col6<10, true, 15>: interleaved ws (256-B segments in the middle pass)
                for (int32_t si : kv.second) pl.slices[si].perm = 1;
        } else {  // two column levels; the middle launch carries D2
            const int m1 = r / 2, m2 = r - m1;
            seq.push_back({K_COL, m1, kRowLog, 0, lo_c, tp, cnt, tiles});
            seq.push_back({K_COL, m2, kRowLog + m1, 1, lo_c, tp, cnt, tiles});
            seq.push_back({K_COL, m1, kRowLog, 0, lo_c, tp, cnt, tiles});
        }
        for (Launch& l : seq) l.stream = s;
        cd.insert(cd.end(), seq.begin(), seq.end());
        seq[0].nu = 1;  // encode: the first column launch writes the slice norms
        ce.insert(ce.end(), seq.begin(), seq.end());
    }
    Launch ra{K_ROWA, 0, 0, 0, lo_l, rp, (int)wl.size(), rows};
    Launch rc{K_ROWC, 0, 0, 0, lo_l, rp, (int)wl.size(), rows};
    ra.stream = rc.stream = s;
    pl.enc.push_back(ra);
    pl.enc.insert(pl.enc.end(), ce.begin(), ce.end());
    pl.enc.push_back(rc);
    ra.a8 = a8;
    pl.dec.push_back(ra);
    pl.dec.insert(pl.dec.end(), cd.begin(), cd.end());
    pl.dec.push_back(rc);
}

// scales: one k_finalize per wave stream, after that stream's last row C,
// over the slices of its own waves.  A single finalize on the caller's
// stream would need a mid-call join, and a cross-queue wait costs the
// caller's queue ~10 us even when it is already satisfied (ResNet-50 trace)
inline void finalize_launches(Plan& pl, const Waves& W) {
    for (int s = 0; s < W.nbuf; ++s) {
        std::vector<int32_t> fl;
        for (size_t w = s; w < W.waves.size(); w += W.nbuf) fl.insert(fl.end(), W.waves[w].begin(), W.waves[w].end());
        if (fl.empty()) continue;
        Launch f{K_FINAL, 0, 0, 0, add_list(pl.ints, fl), -1, (int)fl.size(), (int64_t)fl.size()};
        f.stream = s;
        pl.enc.push_back(f);
    }
}

// column launches and the two-blocks-per-CU row launches: a per-block
// (per-tile) {slice, tile << 3 | group} table, so a block finds its tile
// with one load (a launch of few tiles per CU is latency-bound, and the
// prefix search is a chain of dependent loads); encode and decode share
// the table of the same list.  The persistent row kernels search their
// LDS copy of the prefix and take no table.
inline void make_tables(Plan& pl) {
    std::vector<int32_t>& ints = pl.ints;
    std::map<std::pair<int, int>, int> made;
    auto table = [&](Launch& l) {
        const auto key = std::make_pair(l.list_off, l.tstart_off);
        auto it = made.find(key);
        if (it != made.end()) { l.btab_off = it->second; return; }
        std::vector<int32_t> t;
        t.reserve(2 * (size_t)l.blocks);
        auto add_group = [&](int list_off, int pre_off, int count, int g) {
            for (int i = 0; i < count; ++i)
                for (int32_t k = 0; k < ints[pre_off + i + 1] - ints[pre_off + i]; ++k) {
                    t.push_back(ints[list_off + i]);
                    t.push_back((k << 3) | g);
                }
        };
        if (l.kind == K_COL || l.kind == K_ROWA || l.kind == K_ROWC) {
            add_group(l.list_off, l.tstart_off, l.count, 0);
        } else {  // K_COLM / K_COLMSET: l.count groups {M, list, tstart (relative), count, first block}
            for (int g = 0; g < l.count; ++g) {
                const int32_t* G = &ints[l.list_off + kColGroup * g];
                add_group(l.list_off + G[1], l.list_off + G[2], G[3], g);
            }
        }
        if ((int64_t)t.size() != 2 * (l.blocks - l.sset_groups)) return;  // inconsistent: keep the search
        l.btab_off = (int)ints.size();
        made[key] = l.btab_off;
        ints.insert(ints.end(), t.begin(), t.end());
    };
    for (auto* L : {&pl.enc, &pl.dec})
        for (Launch& l : *L)
            if (!l.expl && (l.kind == K_COL || l.kind == K_COLM || l.kind == K_COLMSET ||
                            ((l.kind == K_ROWA || l.kind == K_ROWC) && l.blocks <= kRowTabMax)))
                table(l);
    // the sign-applying row launches (encode A, decode C): a paired table,
    // one entry per tile of nibble-even position (its partner follows in
    // the same block) and per tile of a slice below 2^18 (unpaired)
    std::map<std::pair<int, int>, std::pair<int, int>> pmade;
    auto ptable = [&](Launch& l) {
        const auto key = std::make_pair(l.list_off, l.tstart_off);
        auto it = pmade.find(key);
        if (it != pmade.end()) { l.ptab_off = it->second.first; l.npair = it->second.second; return; }
        std::vector<int32_t> t;
        bool any = false;
        for (int i = 0; i < l.count; ++i) {
            const int32_t si = ints[l.list_off + i];
            const int p = pl.slices[si].logp;
            const int32_t nt = ints[l.tstart_off + i + 1] - ints[l.tstart_off + i];
            for (int32_t k = 0; k < nt; ++k) {
                if (p >= 18 && ((k >> (p - 18)) & 1)) continue;  // a partner
                t.push_back(si);
                t.push_back((k << 3) | (p >= 18 ? 1 : 0));
                any = any || p >= 18;
            }
        }
        if (!any) return;
        l.ptab_off = (int)ints.size();
        l.npair = (int)(t.size() / 2);
        pmade[key] = {l.ptab_off, l.npair};
        ints.insert(ints.end(), t.begin(), t.end());
    };
    for (Launch& l : pl.enc)
        if (!l.expl && l.kind == K_ROWA && l.tstart_off >= 0 && l.blocks <= kRowTabMax) ptable(l);
    for (Launch& l : pl.dec)
        if (!l.expl && l.kind == K_ROWC && l.tstart_off >= 0 && l.blocks <= kRowTabMax) ptable(l);
}

// per-launch byte accounting (bench / DESIGN.md roofline)
inline void account_bytes(Plan& pl) {
    const std::vector<int32_t>& ints = pl.ints;
    const int64_t n_bits = pl.nbits;
    for (int dir = 0; dir < 2; ++dir) {
        const bool enc = dir == 1;
        for (Launch& l : enc ? pl.enc : pl.dec) {
            if (l.kind == K_COLM) continue;  // counted when built (its list is a group table)
            int64_t mv = 0, al = 0;
            if (l.kind == K_SSET || l.kind == K_COLMSET) {  // group table {P, offset, count}, then the slice ids
                const int to = l.kind == K_SSET ? l.list_off : l.sset_off;
                const int ng = l.kind == K_SSET ? l.count : l.sset_groups;
                for (int g = 0; g < ng; ++g)
                    for (int i = 0; i < ints[to + 3 * g + 2]; ++i) {
                        const SliceDesc& D = pl.slices[ints[to + ints[to + 3 * g + 1] + i]];
                        const int64_t pb = n_bits * (1ll << D.logp) / 8;
                        mv += enc ? 4 * D.len + pb : pb + 4 * D.ylen;
                    }
                if (l.kind == K_SSET) l.bytes_moved = mv;
                else l.bytes_moved += mv;  // + the column part, counted when built
                l.bytes_alg = mv;
                continue;
            }
            for (int i = 0; i < l.count; ++i) {
                const SliceDesc& D = pl.slices[ints[l.list_off + i]];
                const int64_t P = 1ll << D.logp, pb = n_bits * P / 8;
                switch (l.kind) {
                case K_TINY: case K_SMALL:
                    mv += enc ? 4 * D.len + pb : pb + 4 * D.ylen; al = mv; break;
                case K_ROWA:
                    mv += enc ? 4 * D.len + 4 * P : pb + 4 * P; al += enc ? 4 * D.len : pb; break;
                case K_ROWC:
                    mv += enc ? 4 * P + pb : 4 * P + 4 * D.ylen; al += enc ? pb : 4 * D.ylen; break;
                case K_COL: mv += 8 * P; break;
                default: mv += 4 * (P >> kRowLog); break;
                }
                if (l.expl) {  // a sub-wave: its share of the slice's tiles
                    mv = mv / (P >> kRowLog) * l.blocks;
                    al = al / (P >> kRowLog) * l.blocks;
                }
            }
            l.bytes_moved = mv;
            l.bytes_alg = al;
        }
    }
}

}  // namespace detail

// Builds enc, dec and ints (and nwaves, ws_floats, single, every slice's
// ws_off and perm) from the layout and the knobs.  Waves share nstreams
// workspace buffers (wave w: buffer and stream w % nstreams); the scales are
// finalised once, after every wave.  ncu: kScheduleNcu (see there).
inline void build_schedule(Plan& pl, int ncu) {
    using namespace detail;
    pl.ints.clear();
    pl.enc.clear();
    pl.dec.clear();
    std::vector<Launch> common = small_launches(pl);
    const bool sset = pl.sset != 0;
    for (auto& D : pl.slices) D.perm = 0;
    const Waves W = pack_waves(pl, !common.empty(), sset);
    const std::vector<std::vector<int32_t>>& waves = W.waves;
    // the tiny / small slices are independent of the waves: with two wave
    // streams they get a third (latency-bound, they fill CUs beside both
    // waves; splitting them over two streams measured slower on ResNet-50,
    // 259-269 vs 273-276 GiB/s, profiles/r03_resnet50_row2_small2_ab.txt)
    bool small_own = false;
    if (W.nbuf == 2) {
        for (Launch& l : common) l.stream = 2;
        small_own = true;
    } else if (pl.nstreams == 2 && !waves.empty()) {
        // one wave (too few tiles to split): the small slices run beside it
        // on the side stream
        for (Launch& l : common) l.stream = 1;
        small_own = true;
    }
    // on their own stream the small-slice launches are enqueued after the
    // waves' (the critical path reaches the GPU first; each host enqueue costs
    // microseconds); on a shared stream they go first as before
    const bool small_last = !common.empty() && small_own;
    // decode row A reads 8-byte plane words when every plane row is 8-byte aligned
    int a8 = 1;
    for (int32_t si : pl.large) a8 &= (pl.slices[si].pl_off % 8 == 0) && (pl.slices[si].pl_stride % 8 == 0);
    // one wave with a k_col_multi launch and one small-set launch: fused
    // (k_*_colm_set), everything on the caller's stream
    bool fuse = false;
    if (pl.fuse != 0 && waves.size() == 1 && common.size() == 1 && common[0].kind == K_SSET) {
        std::set<int> hs;
        for (int32_t si : waves[0]) {
            const int r = pl.slices[si].logp - kRowLog;
            if (r >= 1 && r <= kColMultiMax) hs.insert(r);
        }
        fuse = hs.size() >= 2;  // wave_launches' condition for the k_col_multi launch
    }
    pl.single = fuse;
    if (fuse) for (Launch& l : common) l.stream = 0;
    if (!small_last && !fuse) pl.enc = pl.dec = common;
    for (size_t w = 0; w < waves.size(); ++w) {
        const int s = (int)(w % W.nbuf);
        int64_t rows = 0;
        const int lo_l = add_list(pl.ints, waves[w]);
        const int rp = add_prefix(pl, waves[w], kRowLog, rows);
        if (!split_wave_launches(pl, waves[w], W.cap, s, lo_l, rp, a8, ncu))
            wave_launches(pl, waves[w], s, lo_l, rp, rows, a8, fuse ? &common[0] : nullptr);
    }
    if (small_last && !fuse) {
        pl.enc.insert(pl.enc.end(), common.begin(), common.end());
        pl.dec.insert(pl.dec.end(), common.begin(), common.end());
    }
    finalize_launches(pl, W);
    make_tables(pl);
    account_bytes(pl);
}

}  // namespace eden
