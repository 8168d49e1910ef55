// eden_bf16_plan.h -- the schedules of encode from and decode into bfloat16
// arenas (ofl_eden_encode_bf16, ofl_eden_decode_add_bf16), derived from a
// plan's own as eden_acc_plan.h derives decode-accumulate's.  Host-only C++17
// like the planner.
//
// The launches are Plan::enc / Plan::dec themselves -- the same waves,
// streams, tile tables and workspace -- so nothing is built or stored: an
// encode's first row launch that resolve() gives k_enc_rowA or k_enc_rowA2,
// and a decode's last row launch that it gives k_dec_rowC or k_dec_rowC2, run
// that kernel's bf16 variant (eden_bf16.h), every other launch its own
// kernel.  Plan, resolve() and workspace_bytes() are left as they are.
//
// Slices of at most 2^15 elements keep their kernels and read / write a
// float32 side arena that holds their elements alone, packed range by range
// (small_ranges: the element ranges and their places in the side arena, from
// the slice table; bf16_slices: the slice table with those slices moved
// there), so its size follows the small slices and not the arena.  One range
// launch before the encode widens their inputs into it, one after the decode
// narrows their outputs out of it.
#pragma once

#include <algorithm>
#include <utility>

#include "eden_acc_plan.h"

namespace eden {

enum Bf16KernelId { BF16_ENC_ROWA, BF16_ENC_ROWA2, BF16_DEC_ROWC, BF16_DEC_ROWC2, BF16_KERNEL_COUNT };
constexpr const char* kBf16KernelName[BF16_KERNEL_COUNT] = {"ofl::k_enc_rowA_bf16", "ofl::k_enc_rowA2_bf16",
                                                            "ofl::k_dec_rowC_bf16", "ofl::k_dec_rowC2_bf16"};

// What launch l of Plan::enc (enc) or Plan::dec runs with bf16 arenas: r as
// resolve() gives it (grid, tables, pairing), bf the bf16 kernel in its place
// or -1 for the plan's own r.id.
inline const char* bf16_resolve(const Plan& pl, const Launch& l, bool enc, int ncu, bool planes8, Resolved& r, int& bf) {
    bf = -1;
    if (const char* err = resolve(pl, l, enc, ncu, false, planes8, r)) return err;
    if (enc && l.kind == K_ROWA) {
        if (r.id != ENC_ROWA && r.id != ENC_ROWA2) return "encode_bf16: encode's first row pass has no bf16 variant";
        bf = r.id == ENC_ROWA ? BF16_ENC_ROWA : BF16_ENC_ROWA2;
    }
    if (!enc && l.kind == K_ROWC) {
        if (r.id != DEC_ROWC && r.id != DEC_ROWC2) return "decode_add_bf16: decode's last row pass has no bf16 variant";
        bf = r.id == DEC_ROWC ? BF16_DEC_ROWC : BF16_DEC_ROWC2;
    }
    return nullptr;
}

// decode-accumulate against a bf16 base (ofl_eden_decode_accumulate_bf16,
// eden_dec_acc_bf16.h): acc_resolve's launches with the accumulate kernels'
// bf16 variants, one entry per AccKernelId
constexpr const char* kAcc16KernelName[ACC_KERNEL_COUNT] = {"ofl::k_dec_acc_rowC_bf16", "ofl::k_dec_acc_rowC2_bf16"};
// the bytes such a row launch moves, from its decode launch's: per valid
// element base 2 + sums 8 + 8 in place of y 4 (acc_bytes_moved with a 2-byte base)
inline int64_t acc16_bytes_moved(const Launch& l) { return l.bytes_moved + 4 * l.bytes_alg - l.bytes_alg / 2; }

// The bytes of a bf16 row launch, from its float32 launch's: the launch's
// algorithmic bytes are the arena's (x read, or y written), 4 per valid
// element there and 2 here; the intermediate as before.  (A base adds 4 / 2
// per element to either path and is in neither figure.)
inline int64_t bf16_bytes_moved(const Launch& l) { return l.bytes_moved - l.bytes_alg / 2; }
inline int64_t bf16_bytes_alg(const Launch& l) { return l.bytes_alg / 2; }

// The element ranges [s, e) of the slices of at most 2^15 elements -- their
// inputs (out = false: x_off, len) or outputs (out = true: y_off, ylen) -- in
// arena order, neighbours merged, as the table the range kernels take
// (QRanges, eden_bf16.h): s[nr] | e[nr] | dst[nr + 1] | cb[nr].  A range is
// walked in slots of 4 elements at arena indices that are multiples of 4 (the
// 8-byte accesses); dst is the exclusive prefix of the ranges' slot counts.
// Arena element i of range r lives at cb[r] + (i - s[r]) in the side arena:
// the ranges' slots back to back, so cb[r] = s[r] mod 4 (a slot is 16 aligned
// bytes there too) and the side arena holds 4 * slots elements (side).
struct SmallRanges {
    std::vector<int64_t> tab;
    int nr = 0;
    int64_t slots = 0;
    int64_t side() const { return 4 * slots; }
    // where arena element i (inside one of the ranges) lives in the side arena
    int64_t at(int64_t i) const {
        const int64_t* s = tab.data();
        const int r = (int)(std::upper_bound(s, s + nr, i) - s) - 1;
        return tab[3 * (size_t)nr + 1 + r] + (i - s[r]);
    }
};
inline SmallRanges small_ranges(const Plan& pl, bool out) {
    std::vector<std::pair<int64_t, int64_t>> v;
    for (const SliceDesc& D : pl.slices) {
        const int64_t s = out ? D.y_off : D.x_off, n = out ? D.ylen : D.len;
        if (D.logp <= kRowLog && n > 0) v.push_back({s, s + n});
    }
    std::sort(v.begin(), v.end());
    size_t m = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (m && v[m - 1].second == v[i].first) v[m - 1].second = v[i].second;
        else v[m++] = v[i];
    }
    v.resize(m);
    SmallRanges R;
    R.nr = (int)m;
    R.tab.resize(4 * m + 1);
    for (size_t i = 0; i < m; ++i) {
        R.tab[i] = v[i].first;
        R.tab[m + i] = v[i].second;
        R.tab[2 * m + i] = R.slots;
        R.tab[3 * m + 1 + i] = 4 * R.slots + (v[i].first & 3);
        R.slots += ((v[i].second + 3) >> 2) - (v[i].first >> 2);
    }
    R.tab[3 * m] = R.slots;
    return R;
}

// float32 elements of the side arena a plan's bf16 calls need (0: no slice of
// at most 2^15 elements): encode and decode use the same one
inline int64_t bf16_side_numel(const Plan& pl) {
    return std::max(small_ranges(pl, false).side(), small_ranges(pl, true).side());
}

// The slice table of the bf16 calls: the plan's, with x_off / y_off of the
// slices of at most 2^15 elements pointing into the side arena (rx / ry:
// small_ranges of the inputs / outputs).  A slice without valid input or
// output reads or writes nothing and gets offset 0.
inline std::vector<SliceDesc> bf16_slices(const Plan& pl, const SmallRanges& rx, const SmallRanges& ry) {
    std::vector<SliceDesc> out = pl.slices;
    for (SliceDesc& D : out) {
        if (D.logp > kRowLog) continue;
        D.x_off = D.len > 0 ? rx.at(D.x_off) : 0;
        D.y_off = D.ylen > 0 ? ry.at(D.y_off) : 0;
    }
    return out;
}

// 8-byte accesses of a bf16 arena need its large slices 4-element aligned
// (the caller's arena pointer 8-byte aligned on top): true for the default
// layout and every tensor offset that is a multiple of 4
inline bool bf16_aligned(const Plan& pl) {
    for (const SliceDesc& D : pl.slices)
        if (D.logp > kRowLog && ((D.x_off | D.y_off) & 3)) return false;
    return true;
}

}  // namespace eden
