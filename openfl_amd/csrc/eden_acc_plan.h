// eden_acc_plan.h -- the schedule of decode into the streaming average's sums
// (ofl_eden_decode_accumulate), derived from a plan's decode schedule as
// eden_rt_plan.h derives the round trip's.  Host-only C++17 like the planner.
//
// The launches are Plan::dec itself -- the same waves, streams, tile tables
// and workspace -- so nothing is built or stored: a launch that resolve()
// gives k_dec_rowC or k_dec_rowC2 runs that kernel's accumulate variant
// (eden_dec_acc.h), every other launch its own kernel.  Plan, resolve() and
// workspace_bytes() are left as they are.
#pragma once

#include "eden_plan.h"

namespace eden {

enum AccKernelId { ACC_ROWC, ACC_ROWC2, ACC_KERNEL_COUNT };
constexpr const char* kAccKernelName[ACC_KERNEL_COUNT] = {"ofl::k_dec_acc_rowC", "ofl::k_dec_acc_rowC2"};

// What launch l of Plan::dec runs in a decode-accumulate: r as resolve()
// gives it (grid, tables, pairing), acc the accumulate kernel in its place or
// -1 for the plan's own r.id.  last_row_resolve is the derivation itself,
// shared by every route that puts its own kernels in the last row pass's
// place (var: ACC_ROWC / ACC_ROWC2's index or -1).
inline const char* last_row_resolve(const Plan& pl, const Launch& l, int ncu, bool planes8, Resolved& r, int& var,
                                    const char* no_variant) {
    var = -1;
    if (const char* err = resolve(pl, l, false, ncu, false, planes8, r)) return err;
    if (l.kind == K_ROWC) {
        if (r.id != DEC_ROWC && r.id != DEC_ROWC2) return no_variant;
        var = r.id == DEC_ROWC ? ACC_ROWC : ACC_ROWC2;
    }
    return nullptr;
}
inline const char* acc_resolve(const Plan& pl, const Launch& l, int ncu, bool planes8, Resolved& r, int& acc) {
    return last_row_resolve(pl, l, ncu, planes8, r, acc, "decode_accumulate: decode's last row pass has no accumulate variant");
}

// Decode into the FedOpt gradient (ofl_eden_decode_adaptive_accumulate,
// eden_dec_ada.h) is the same derivation with its own two kernels in the
// last row pass's place: one id per AccKernelId, in its order.
enum AdaKernelId { ADA_ROWC = ACC_ROWC, ADA_ROWC2 = ACC_ROWC2, ADA_KERNEL_COUNT = ACC_KERNEL_COUNT };
constexpr const char* kAdaKernelName[ADA_KERNEL_COUNT] = {"ofl::k_dec_ada_rowC", "ofl::k_dec_ada_rowC2"};
inline const char* ada_resolve(const Plan& pl, const Launch& l, int ncu, bool planes8, Resolved& r, int& ada) {
    return last_row_resolve(pl, l, ncu, planes8, r, ada,
                            "decode_adaptive_accumulate: decode's last row pass has no gradient variant");
}

// The bytes a gradient row launch moves, from its decode launch's: the
// intermediate as before, and per valid element base 4 + g 4 + 4 in place of
// y 4 (an upload after the first; the first reads no g).  No algorithmic
// bytes: y is not written.
inline int64_t ada_bytes_moved(const Launch& l) { return l.bytes_moved + 2 * l.bytes_alg; }

// The bytes an accumulate row launch moves, from its decode launch's: the
// intermediate as before, and per valid element base 4 + sums 8 + 8 in place
// of y 4 (a delta upload after the first; the first reads no sums, an upload
// without a base no base).  No algorithmic bytes: y is not written.
inline int64_t acc_bytes_moved(const Launch& l) { return l.bytes_moved + 4 * l.bytes_alg; }

// slices of at most 2^15 elements keep their decode kernels and need y_small
inline bool has_small_slice(const Plan& pl) {
    for (const SliceDesc& D : pl.slices)
        if (D.logp <= kRowLog) return true;
    return false;
}

}  // namespace eden
