// eden_desc.h -- what the Eden planner (eden_plan.h, host) and the Eden kernels
// (eden_kernels.hip, device) share: the slice descriptor, the five constants
// both sides compute with, and the formats of the tables a plan keeps in its
// int32 array `ints`.  Plain C++17: no HIP header, nothing of the kernels.
#pragma once

#include <cstdint>

namespace ofl {

// ---------------------------------------------------------------------------
// Descriptors (host-built once per plan, uploaded on first use)
// ---------------------------------------------------------------------------
struct SliceDesc {
    int64_t x_off;      // encode: element offset of the slice's input in the fp32 arena
    int64_t y_off;      // decode: element offset of the slice's output in the fp32 arena
    int64_t ylen;       // decode: elements of this slice that land in the output
    int64_t ws_off;     // element offset of the slice's intermediate in ws (large slices)
    int64_t pl_off;     // byte offset of the slice's first byte of plane 0
    int64_t pl_stride;  // bytes between planes of this tensor (= P_tot(t) / 8)
    int64_t len;        // encode: valid input elements (<= P), zero padded to P
    int32_t logp;
    int32_t tensor;
    int32_t scale_idx;
    int32_t part_off;   // offset of this slice's partials (large slices)
    int32_t perm;       // ws layout of a 2^25 slice: element bit 15 stored at bit 5 (ws_pos)
    int32_t pad_;
};

constexpr int kTinyNT = 256;   // threads of a tiny slice's group (k_*_tiny; a sub-block of a small-set workgroup)
constexpr int kSetNT = 1024;   // threads of a small-set workgroup (k_*_sset, k_*_colm_set)
constexpr int kRowLog = 15;    // a row tile is 2^kRowLog contiguous elements
constexpr int kColLog = 15;    // a column tile is 2^kColLog elements
constexpr int kColGroup = 5;   // ints per group record of a k_col_multi launch

// ---------------------------------------------------------------------------
// Tables in `ints` (offsets are Launch fields, eden_plan.h; KArgs pointers in
// the kernels).  All entries are int32.
//
//  slice list     list_off, count entries: slice ids (KArgs::list)
//  tile prefix    tstart_off, count + 1 entries: prefix sums of the listed
//                 slices' tiles (2^(logp - kRowLog) row tiles, or
//                 2^(logp - kColLog) column tiles); the last is the launch's
//                 tile total (KArgs::tstart)
//  block table    btab_off, 2 entries per block: {slice, tile << 3 | group}
//                 -- the tile within the slice, the group within a
//                 k_col_multi launch (0 elsewhere).  A sub-wave of a split
//                 five-pass slice lists its tiles here explicitly, group 0
//                 (KArgs::btab)
//  paired table   ptab_off, 2 entries per block, npair blocks:
//                 {slice, tile << 3 | pair}; pair = 1: the block also runs
//                 tile + 2^(logp - 18), whose D1 words are the same; slices
//                 below 2^18 are listed tile by tile with pair = 0
//                 (KArgs::btab with KArgs::npair)
//  small-set      list_off (K_SSET) or sset_off (K_COLMSET), 3 entries per
//  groups         workgroup: {P (0: tiny), offset of the group's slice ids
//                 from the table's start, count}; the slice ids follow the
//                 group records (KArgs::list / KArgs::sset)
//  column groups  list_off (K_COLM / K_COLMSET), kColGroup entries per group:
//                 {M, slice list, tile prefix (both relative to the table's
//                 start), count, first block}
// ---------------------------------------------------------------------------

}  // namespace ofl
