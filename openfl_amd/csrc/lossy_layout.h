// lossy_layout.h -- the host-only part of the lossy kernels (lossy_kernels.hip),
// free of HIP so that it can be built and checked alone
// (tests/lossy_layout_check.cpp): the constants and plain records the host and
// the kernels share, the chunk table every batched entry point uploads, and
// the workspace layout of each batched family.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lossy {

constexpr int kNT = 256;
constexpr int kRadixBits = 11;    // radix-select digit
constexpr int kRadix = 1 << kRadixBits;
constexpr int kMaxK = 32;         // clusters supported
constexpr int kBkmChunk = 1 << 16;  // elements of one tensor that one block of a batched kernel covers
constexpr int kBkmBins = 4096;
constexpr int kBkmMaxInit = 16;  // k-means++ restarts (n_init), one workgroup each

// ---- the chunk table ---------------------------------------------------------
// One record per tensor of an arena: elements [off, off + n), covered by the
// nblk blocks blk0 .. blk0 + nblk - 1 of kBkmChunk elements each.
struct BkmTensor { int64_t off; int64_t n; int32_t blk0; int32_t nblk; };
static_assert(sizeof(BkmTensor) == 24, "the chunk table's record");

inline int64_t chunks_of(int64_t n) { return (n + kBkmChunk - 1) / kBkmChunk; }
// the block count alone, for the *_workspace_bytes queries (numels unchecked)
inline int64_t count_chunks(int ntensors, const int64_t* numels) {
    int64_t blocks = 0;
    for (int t = 0; t < ntensors; ++t) blocks += chunks_of(numels[t]);
    return blocks;
}

enum ChunkErr {
    kChunkOk = 0,
    kChunkNull,    // NULL offsets / numels
    kChunkNumel,   // a tensor of fewer than 0 or more than kBkmChunk * INT32_MAX elements
    kChunkBlocks,  // more than INT32_MAX blocks (td and blocks are complete)
};
struct ChunkTable {
    std::vector<BkmTensor> td;
    int64_t blocks = 0;
};
// The table of every batched entry point.  Entry points report the error with
// their own message, at their own place among their checks; each of them
// returns OFL_EINVAL for it before any HIP call.  A zero-length tensor is a
// record without blocks (the k-means and top-k entry points refuse it).
inline ChunkErr chunk_table(int ntensors, const int64_t* offsets, const int64_t* numels, ChunkTable& tab) {
    tab.td.clear();
    tab.blocks = 0;
    if (!offsets || !numels) return kChunkNull;
    tab.td.reserve(ntensors > 0 ? ntensors : 0);
    for (int t = 0; t < ntensors; ++t) {
        if (numels[t] < 0 || numels[t] > (int64_t)kBkmChunk * INT32_MAX) return kChunkNumel;
        const int64_t nb = chunks_of(numels[t]);
        tab.td.push_back({offsets[t], numels[t], (int32_t)tab.blocks, (int32_t)nb});
        tab.blocks += nb;
    }
    return tab.blocks > INT32_MAX ? kChunkBlocks : kChunkOk;
}

// ---- records in the workspaces -----------------------------------------------
struct BkmState {
    uint32_t mm[2];          // ~key(min), key(max): both reduced by atomicMax from 0
    int32_t converged;       // 0 running, 2 final assignment pass pending, 1 done
    int32_t nuniq;
    int32_t has_nan;         // k_bkm_minmax met a NaN (min / max drop it)
    int32_t pad_;
    double cen[kMaxK];       // sorted centres
    float mids[kMaxK];       // float32 midpoints of consecutive centres (+inf beyond k-1)
    float rank[kMaxK];       // float32 rank of each cluster's value
    double uniq[kMaxK];      // sorted distinct values of the used centres (value dtype)
    long long cnt[kMaxK];
    double inertia;
    double cand[kBkmMaxInit][kMaxK];  // sorted centres of each restart
    double cand_in[kBkmMaxInit];      // and its inertia on the histogram
};
struct BtkState {
    int64_t k;            // kept count (ceil(n p))
    int64_t need;         // rank from the top within the current prefix; after pass 3: ties kept
    uint32_t prefix, pmask;
    float kmin;           // min kept value (before the shift)
    float shift;          // 1e-7 or 0
    int64_t n_pos, n_neg, n_zero;
    double abs_sum;       // fp64 sum of |kept + shift|
};
struct BtkBlock {
    uint32_t ties;        // |x| bits == T in this block
    int32_t neg_rank;     // in-block tie rank of the first negative tie, -1 if none
    float smin;           // min value with |x| > T
    float tmin;           // min value with |x| == T
    uint64_t tie_base;    // ties in the tensor's earlier blocks
    uint32_t cpos, cneg, czero, pad_;
    double asum;
};

// ---- workspace layouts ---------------------------------------------------------
// Regions are carved in order, each rounded up to 256 bytes.  A layout names
// its regions, the spans its driver clears, and its end; *_workspace_bytes
// reports the end plus kWsSlack.
struct Span {
    size_t off, bytes;
    size_t end() const { return off + bytes; }
};
struct Carve {
    size_t at = 0;
    Span take(size_t bytes) {
        const Span s{at, (bytes + 255) & ~(size_t)255};
        at += s.bytes;
        return s;
    }
};
inline Span cover(Span first, Span last) { return {first.off, last.end() - first.off}; }
constexpr size_t kWsSlack = 256;

struct KmeansLayout {
    Span td, st, hc, hs, part, seeds;
    Span zeroed;  // states + both histograms
    size_t total;
};
inline KmeansLayout kmeans_layout(int T, int64_t blocks) {
    Carve c;
    KmeansLayout L;
    L.td = c.take(sizeof(BkmTensor) * T);
    L.st = c.take(sizeof(BkmState) * T);
    L.hc = c.take(sizeof(uint32_t) * kBkmBins * T);            // [T][4096] counts
    L.hs = c.take(sizeof(unsigned long long) * kBkmBins * T);  // [T][4096] fixed-point sums
    L.part = c.take(sizeof(double) * 3 * kMaxK * (size_t)std::max<int64_t>(blocks, 1));
    L.seeds = c.take(sizeof(uint64_t) * T);
    L.zeroed = cover(L.st, L.hs);
    L.total = c.at;
    return L;
}

struct TopkLayout {
    Span td, st, hist, blk;
    Span zeroed;  // the digit histogram
    size_t total;
};
inline TopkLayout topk_layout(int T, int64_t blocks) {
    Carve c;
    TopkLayout L;
    L.td = c.take(sizeof(BkmTensor) * T);
    L.st = c.take(sizeof(BtkState) * T);
    L.hist = c.take(sizeof(uint32_t) * kRadix * T);
    L.blk = c.take(sizeof(BtkBlock) * (size_t)std::max<int64_t>(blocks, 1));
    L.zeroed = L.hist;
    L.total = c.at;
    return L;
}

struct LutLayout {
    Span td, nk, keys, vals;
    size_t total;
};
inline LutLayout lut_layout(int T, int max_nk) {
    const size_t nt = (size_t)std::max(T, 1), mk = (size_t)std::max(max_nk, 1);
    Carve c;
    LutLayout L;
    L.td = c.take(sizeof(BkmTensor) * nt);
    L.nk = c.take(sizeof(int32_t) * nt);
    L.keys = c.take(sizeof(float) * nt * mk);
    L.vals = c.take(sizeof(float) * nt * mk);
    L.total = c.at;
    return L;
}

struct TernaryLayout {
    Span td, ranks3;
    size_t total;
};
inline TernaryLayout ternary_layout(int T) {
    const size_t nt = (size_t)std::max(T, 1);
    Carve c;
    TernaryLayout L;
    L.td = c.take(sizeof(BkmTensor) * nt);
    L.ranks3 = c.take(3 * sizeof(float) * nt);
    L.total = c.at;
    return L;
}

// what the *_workspace_bytes entry points report
inline size_t kmeans_workspace_bytes(int T, const int64_t* numels) {
    if (T < 1 || !numels) return kWsSlack;
    return kmeans_layout(T, count_chunks(T, numels)).total + kWsSlack;
}
inline size_t topk_workspace_bytes(int T, const int64_t* numels) {
    if (T < 1 || !numels) return kWsSlack;
    return topk_layout(T, count_chunks(T, numels)).total + kWsSlack;
}
inline size_t lut_workspace_bytes(int T, int max_nk) { return lut_layout(T, max_nk).total + kWsSlack; }
inline size_t ternary_workspace_bytes(int T) { return ternary_layout(T).total + kWsSlack; }
// the one-tensor k-means, top-k and ternary statistics
inline size_t single_workspace_bytes(int64_t n) {
    return std::max<size_t>({(size_t)1 << 20, kmeans_workspace_bytes(1, &n), topk_workspace_bytes(1, &n)});
}

}  // namespace lossy
