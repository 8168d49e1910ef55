// tlz_encode.h -- the TLZ encoder of the gzip codec (deflate_kernels.hip).
#pragma once
#include "gz_device.h"
#include "ofl_codec.h"

namespace gz {

// ============================================================================
// TLZ: token-LZ gzip of rank arrays (GZIPTransformer.forward,
// kc_pipeline.py:128-141, skc_pipeline.py:201-215, stc_pipeline.py:185-199)
// and its lane-parallel inflate (GZIPTransformer.backward,
// kc_pipeline.py:152-156: gzip.decompress).
//
// Format: a multi-member gzip stream (RFC 1952).  A member covers up to
// kMemTok float32 ranks (512 KiB of input) as ONE dynamic-Huffman deflate
// block (RFC 1951) over the whole 32 KiB window, whose copies are whole
// tokens: 12..256 bytes (3..64 float32 values) at distances that are
// multiples of 4 bytes; a value without a copy is its 4 literal bytes.  The
// member's values are cut into segments of kSeg; no copy crosses a segment
// end, so a decoder can start at any segment: an RFC 1952 extra subfield
// 'OZ' in the member header holds the bit offset (from the first bit of the
// deflate data) of every segment's first symbol.  gzip.decompress, zlib and
// any gzip reader skip the subfield and read the member as plain deflate.
//   header (28 + 4 nseg bytes): 1f 8b 08 04 | mtime 0 | xfl 0 | os ff | XLEN |
//     'O' 'Z' | LEN | version 1 | log2(kSeg) | nseg (u16) | member bytes (u32)
//     | values (u32) | nseg x u32 segment bit offsets
//   deflate data (one block, BFINAL = 1, BTYPE = 2) | CRC-32 | ISIZE
// (the field offsets and the format's constants: gz_format.h)
//
// Encoder (k_tlz_encode, one 512-thread block per member, a segment at a
// time): 3-gram chains (per-wave ballot matching, then the waves' and the
// earlier segments' last occurrences), the longest-match frontier of every
// position over kCand (12) chain candidates (1 <= 3 (length, distance)
// pairs), an optimal parse by a segmented backward DP (each thread its 4
// positions, the other threads' costs from the previous sweep, 4 sweeps)
// under a cost model re-estimated from the member's symbol counts after every
// segment, the DP's path followed by Jacobi rounds (every thread walks its 4
// positions from its left neighbour's exit until no entry changes), then one
// Huffman code per member and the bits.  The parse is what gzip -9 lacks: 0.115 of the input
// on KC ranks against gzip -9's 0.117 (tools/tlz_proto.c simulates it).
// Decoder: k_tlz_ops (one wavefront per member, one lane per segment:
// Huffman decode from the segment's bit offset with the member's tables in
// LDS; each lane writes its segment's ops into that segment's own output
// bytes) and k_tlz_resolve (one block per member, a segment at a time: op
// positions by a block scan, every value's source by pointer jumping in LDS
// against the window of earlier values, then the values, CRC-32, ISIZE).
namespace tlz {
constexpr int kNT = 512;                           // encoder threads per member block
constexpr int kPer = kSeg / kNT;                   // positions per thread
constexpr int kWin = 8192;                         // window, values (32 KiB)
constexpr int kMaxL = 64, kMinL = 3;               // copy length, values
#ifndef OFL_TLZ_CAND
// 11 chain candidates (round 5, after the DP rework made the frontier the
// largest phase): KC gzip phase 12.5 -> 12.1 ms per GiB for ratio 0.1165 ->
// 0.1167 (10: 11.9 ms, 0.1170; gzip -9: 0.1171-0.1174;
// profiles/r05_tlz_cand_sweep_ab.txt).  Round 4: 12 instead of 16, encode
// 14.0 -> 12.8 ms (profiles/r04_tlz_cand_ab2.txt)
#define OFL_TLZ_CAND 11
#endif
#ifndef OFL_TLZ_SWEEPS
#define OFL_TLZ_SWEEPS 4
#endif
constexpr int kCand = OFL_TLZ_CAND;                // chain candidates per position (A/B: -DOFL_TLZ_CAND)
constexpr int kBuckets = 512;                      // 3-gram buckets: exact for values < 8, hashed (into the same) above
constexpr int kBucketBits = 9;
static_assert(kBuckets == 1 << kBucketBits, "bucket ids are kBucketBits wide");
constexpr int kSweeps = OFL_TLZ_SWEEPS;            // DP sweeps (segments of kPer = 4 positions; tools/tlz_proto.c)
constexpr int kRing = 16384;                       // value ring (ids), + 8 mirrored bytes
constexpr int kLitMax = 11, kDistMax = 10;         // code length limits = the inflate's table bits
constexpr uint16_t kPending = 0xffffu;

struct EncSmem {
    alignas(16) uint8_t tok[kRing + 32];      // + the first 32 bytes again (a candidate's 20-byte read)
    union {
        struct {
            uint16_t prev[kRing];                  // distance to the previous same-bucket position (0: none), by position mod kRing
            union {
                uint16_t lastw[kNT / 64][kBuckets];  // chains: per wave, this segment: position - range start + 1
                uint32_t cost[2][kSeg + 8];        // then the DP's costs to the segment end, 1/8 bit
                uint32_t hw[kNT / 64][(kLit + kDist + 1) / 2];  // then per-wave symbol counts of the segment, two u16 per word
            };
        } m;
        struct {
            HScratch h;
            uint32_t hdrw[kHdrW];
            uint8_t hb[hdr_bytes(kMemSeg)];
            // the bit emission's tables (code | extra bits) << 0 | n << 24:
            // a literal value's first two and last two bytes, a copy length
            uint32_t litlo[32], lithi[32], lenw[kMaxL + 1];
        } f;
    } u;
    uint32_t head[2][kBuckets];                    // last position + 1 per bucket (earlier segments); segment c reads [c & 1], writes [~c & 1]
    uint16_t dec[kSeg];                            // chosen op: length (0: literal) | frontier entry << 8
    uint16_t entry[kNT + 1];                       // parse: each thread's first position
    uint32_t hl[kLit], hd[kDist], hc[kCL];
    uint32_t totl, totd;
    uint16_t symc[kLit + kDist];
    uint16_t litc[32], lenc[kMaxL + 1], dcst[kDist];
    uint8_t ll[kLit], ld[kDist], lc[kCL];
    uint16_t kl[kLit], kd[kDist], kc[kCL];
    uint32_t crct[1][256];                         // CRC-32 byte table (the word tables went to the DP's 32-bit costs)
    uint32_t adv13[8][16];                         // CRC advance by a segment's 8 KiB, per input nibble
    uint32_t cid4[kPer][32];                       // raw CRC of a thread's 16 bytes with only value q = id (from 0)
    uint32_t segop[kMemSeg + 1], segbit[kMemSeg];
    uint32_t scan[kNT / 64];
    uint32_t crc_w[kNT / 64];
    uint32_t ops_n, crc_raw, hdr_bits, total_bits, nrle, nlit_ndist;
    int bad;
    // fused k-means labelling (EncArgs::lab): the records of tensors lab_t0 ..
    // lab_t0 + 3 (start = end = INT64_MAX past the last); positions below
    // lab_hi lie in one of them or in no tensor
    int32_t lab_t0;
    int64_t lab_s[4], lab_e[4], lab_hi;
    float lab_m[4][8], lab_r[4][8];
};
static_assert(sizeof(EncSmem) <= 80 * 1024, "two member blocks per CU");

struct EncArgs {
    const float* x;
    int64_t n;
    int64_t mem0;            // first member of this launch
    uint8_t* slots;          // [members][slot_bytes]
    uint32_t* ops;           // [members][ops_stride]
    uint32_t* sizes;         // [members]
    int* bad;
    uint32_t slot_bytes, ops_stride;
    int aligned;             // x is 16-byte aligned
    uint64_t* phases;        // diagnostics (OFL_GZ_PHASES): block 0's time per phase (10 ns ticks), else null
    const ofl_label_rec* lab;  // non-null: x holds values, labelled through these records as they load
    int32_t lab_n;
};
constexpr int kEncPhases = 16;

// k-means label of one value (k_bkm_label's rule, lossy_kmeans.h)
DEVI float lab_rank(float v, const float* m, const float* r) {
    float o = r[0];
#pragma unroll
    for (int j = 0; j < 7; ++j) o = v > m[j] ? r[j + 1] : o;
    return o;
}
// wave 0: the label window for a segment starting at s0 -- the first tensor
// ending after s0 (64-way search from the previous window, ends ascending)
// and the three after it
DEVI void lab_fill(const EncArgs& a, EncSmem& S, int64_t s0, int lane) {
    int lo = S.lab_t0, hi = a.lab_n;
    while (lo < hi) {
        const int stride = (hi - lo + 63) >> 6;
        const int i = lo + lane * stride;
        const int cnt = __popcll(__ballot(i < hi && a.lab[i].end <= s0));
        if (cnt == 0) break;
        const int nlo = lo + (cnt - 1) * stride + 1;
        hi = min(lo + cnt * stride, hi);
        lo = nlo;
    }
    if (lane < 4) {
        const int t = lo + lane;
        if (t < a.lab_n) {
            const ofl_label_rec r = a.lab[t];
            S.lab_s[lane] = r.start;
            S.lab_e[lane] = r.end;
#pragma unroll
            for (int j = 0; j < 8; ++j) { S.lab_m[lane][j] = r.mid[j]; S.lab_r[lane][j] = r.rank[j]; }
        } else {
            S.lab_s[lane] = S.lab_e[lane] = INT64_MAX;
        }
    }
    if (lane == 0) {
        S.lab_t0 = lo;
        S.lab_hi = lo + 4 < a.lab_n ? a.lab[lo + 4].start : INT64_MAX;
    }
}
// the label of the value v at arena position g (any position of the segment)
DEVI float lab_one(const EncArgs& a, const EncSmem& S, int64_t g, float v) {
    const int sl = (g >= S.lab_s[1]) + (g >= S.lab_s[2]) + (g >= S.lab_s[3]);
    if (g >= S.lab_s[sl] && g < S.lab_e[sl]) return lab_rank(v, S.lab_m[sl], S.lab_r[sl]);
    if (g < S.lab_hi) return 0.f;  // between tensors
    int lo = S.lab_t0 + 4, hi = a.lab_n - 1;  // past the window (> 4 tensors in this segment): last start <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.lab[mid].start <= g) lo = mid; else hi = mid - 1;
    }
    const ofl_label_rec& r = a.lab[lo];
    return g >= r.start && g < r.end ? lab_rank(v, r.mid, r.rank) : 0.f;
}

DEVI int pslot(int p) { return p & (kRing - 1); }
// the DP's costs live modulo 2^16: all candidates of one position lie within
// 64 values of each other, < 64 x 4 literals x 15 bits x 8 < 2^15 apart
DEVI bool lt16(uint32_t a, uint32_t b) { return (int16_t)(uint16_t)(a - b) < 0; }
DEVI uint32_t tk4r(const uint8_t* tok, int p) {
    const int r = p & (kRing - 1);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(tok);
    return __builtin_amdgcn_alignbyte(w[(r >> 2) + 1], w[r >> 2], (uint32_t)(r & 3));
}
// 3-gram bucket: exact for values < 8 (512 buckets), hashed into the same
// 512 above (a collision only adds chain entries the comparison rejects)
DEVI int bucket(const uint8_t* tok, int p) {
    const uint32_t v = tk4r(tok, p) & 0xffffffu;
    const uint32_t a = v & 0xffu, b = (v >> 8) & 0xffu, c = v >> 16;
    if ((a | b | c) < 8u) return (int)(a | (b << 3) | (c << 6));
    return (int)(((a | (b << 5) | (c << 10)) * 0x9E3779B1u) >> (32 - kBucketBits));
}
DEVI int match_len(const uint8_t* tok, int i, int j, int lim) {
    int L = 0;
    while (L < lim) {
        const uint32_t x = tk4r(tok, i + L) ^ tk4r(tok, j + L);
        if (x) { L += __builtin_ctz(x) >> 3; break; }
        L += 4;
    }
    return min(L, lim);
}
// raw CRC-32 of one little-endian word, a byte at a time (T: the byte table);
// used only at set-up and for a member's partial last piece
DEVI uint32_t crc4(const uint32_t (*T)[256], uint32_t c, uint32_t w) {
    c ^= w;
#pragma unroll
    for (int i = 0; i < 4; ++i) c = (c >> 8) ^ T[0][c & 0xffu];
    return c;
}
// 1/8 bit: -log2(count / total) >= 1 bit, an unseen symbol log2(total + 1) + 2
// bits, at most 15 bits
DEVI uint32_t sym_cost(uint32_t cnt, uint32_t tot) {
    const float v = cnt ? 8.f * (__log2f((float)tot) - __log2f((float)cnt))
                        : 8.f * (__log2f((float)tot + 1.f) + 2.f);
    return (uint32_t)fminf(120.f, fmaxf(8.f, rintf(v)));
}
// per-symbol costs -> the DP's tables: a literal value (its 4 bytes), a copy
// length (code + extra bits), a distance code (+ extra bits)
DEVI void tlz_model(EncSmem& S, int tid, bool prior) {
    for (int s = tid; s < kLit + kDist; s += kNT) {
        uint32_t c;
        if (prior) c = s < 256 ? 48u : s < kLit ? 32u : 40u;
        else c = s < kLit ? sym_cost(S.hl[s], S.totl) : sym_cost(S.hd[s - kLit], S.totd);
        S.symc[s] = (uint16_t)c;
    }
    __syncthreads();
    if (tid < 32) {
        const uint32_t b = __float_as_uint((float)tid);
        S.litc[tid] = (uint16_t)(S.symc[b & 0xffu] + S.symc[(b >> 8) & 0xffu] + S.symc[(b >> 16) & 0xffu] + S.symc[b >> 24]);
    } else if (tid < 32 + kMaxL + 1) {
        const int l = tid - 32;
        if (l >= kMinL) {
            const int lc = len_code(4u * (uint32_t)l);
            S.lenc[l] = (uint16_t)(S.symc[257 + lc] + 8u * c_lext[lc]);
        } else {
            S.lenc[l] = 0;
        }
    } else if (tid < 32 + kMaxL + 1 + kDist) {
        const int c = tid - 32 - kMaxL - 1;
        S.dcst[c] = (uint16_t)(S.symc[kLit + c] + 8u * c_dext[c]);
    }
    __syncthreads();
}
// block-wide exclusive scan of v over NT threads (returns the exclusive prefix; *total)
template <int NT>
DEVI uint32_t block_scan(uint32_t v, uint32_t* scan, uint32_t* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) scan[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < NT / 64; ++j) {
        base += j < w ? scan[j] : 0u;
        tot += scan[j];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_tlz_encode(EncArgs a) {  // 2 blocks per CU: 4 waves per SIMD
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EncSmem& S = *reinterpret_cast<EncSmem*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t ph_t = 0, ph_acc[kEncPhases] = {};
    const bool ph_on = a.phases && blockIdx.x == 0 && tid == 0;
    // (diagnostics: a barrier before every mark, so a phase's time is its
    // slowest wave's, not wave 0's; launch-uniform condition)
    auto PH = [&](int k) {
        if (a.phases) __syncthreads();
        if (ph_on) { const uint64_t t = wall_clock64(); if (k > 0) ph_acc[k] += t - ph_t; ph_t = t; }
    };
    PH(0);
    const int64_t g0 = (a.mem0 + blockIdx.x) * (int64_t)kMemTok;
    const int ntok = (int)min<int64_t>(kMemTok, a.n - g0);
    const int nseg = (ntok + kSeg - 1) >> kSegLog;
    uint32_t* const ops = a.ops + (int64_t)blockIdx.x * a.ops_stride;
    if (tid < 256) {
        uint32_t r = (uint32_t)tid;
        for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1;
        S.crct[0][tid] = r;
    } else if (tid < 256 + 128) {  // the per-segment CRC advance as nibble tables
        const int e = tid - 256, j = e >> 4, v = e & 15;
        uint32_t r = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) r ^= ((v >> b) & 1) ? c_adv[kSegLog + 2][4 * j + b] : 0u;
        S.adv13[j][v] = r;
    }
    for (int i = tid; i < kBuckets; i += kNT) {
        S.head[0][i] = S.head[1][i] = 0;
#pragma unroll
        for (int w = 0; w < kNT / 64; ++w) S.u.m.lastw[w][i] = 0;
    }
    for (int i = tid; i < kLit; i += kNT) S.hl[i] = 0;
    if (tid < kDist) S.hd[tid] = 0;
    if (tid < kCL) S.hc[tid] = 0;
    if (tid == 0) { S.totl = S.totd = 0; S.ops_n = 0; S.crc_raw = 0; S.bad = 0; S.lab_t0 = 0; S.lab_hi = INT64_MIN; }
    __syncthreads();
    // the raw CRC is linear: a thread's 16 bytes (4 values, ids < 32) hash to
    // the XOR of one table entry per value, 4 independent reads instead of
    // 16 dependent ones
    if (tid < kPer * 32) {
        const int q = tid >> 5;
        const uint32_t bits = __float_as_uint((float)(tid & 31));
        uint32_t cr = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) cr = crc4(S.crct, cr, k == q ? bits : 0u);
        S.cid4[q][tid & 31] = cr;
    }
    __syncthreads();
    tlz_model(S, tid, true);

    uint32_t crc_acc = 0, crc_last = 0;
    int nv_last = 0;
    for (int c = 0; c < nseg; ++c) {
        // thread-derived values recomputed every segment from an opaque tid
        // (hoisted out of the loop, they were spilled and reloaded instead)
        uint32_t tid_o = threadIdx.x;
        asm volatile("" : "+v"(tid_o));
        const int tid = (int)tid_o, lane = tid & 63, wv = tid >> 6;
        const int c0 = c << kSegLog;
        const int send = min(c0 + kSeg, ntok);
        const int lo = c0 + kPer * tid;                 // this thread's positions [lo, lo + kPer)
        if (a.lab) {  // a new label window when this segment reaches past the current one
            const int64_t lab_hi = S.lab_hi;
            if (g0 + send > lab_hi) {
                __syncthreads();
                if (wv == 0) lab_fill(a, S, g0 + c0, lane);
                __syncthreads();
            }
        }
        // ---- A: values -> ids in the ring, validity, raw CRC-32 ----
        uint32_t idw[kPer / 4] = {};                    // this thread's ids, packed 4 per word
        {
            const int nv = max(0, min(kPer, send - lo));
            float v[kPer];
            if (nv == kPer && a.aligned) {
                const float4* p = reinterpret_cast<const float4*>(a.x + g0 + lo);
#pragma unroll
                for (int u = 0; u < kPer / 4; ++u) {
                    const float4 v0 = p[u];
                    v[4 * u] = v0.x; v[4 * u + 1] = v0.y; v[4 * u + 2] = v0.z; v[4 * u + 3] = v0.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < kPer; ++q) v[q] = q < nv ? a.x[g0 + lo + q] : 0.f;
            }
            if (a.lab) {  // values -> ranks (the k-means labels the rank array would hold)
                const int64_t gp = g0 + lo;
                const int sl = (gp >= S.lab_s[1]) + (gp >= S.lab_s[2]) + (gp >= S.lab_s[3]);
                if (nv == kPer && gp >= S.lab_s[sl] && gp + kPer <= S.lab_e[sl]) {  // one tensor (the common case)
                    float m[7], r[8];
#pragma unroll
                    for (int j = 0; j < 7; ++j) m[j] = S.lab_m[sl][j];
#pragma unroll
                    for (int j = 0; j < 8; ++j) r[j] = S.lab_r[sl][j];
#pragma unroll
                    for (int q = 0; q < kPer; ++q) v[q] = lab_rank(v[q], m, r);
                } else {
#pragma unroll
                    for (int q = 0; q < kPer; ++q)
                        if (q < nv) v[q] = lab_one(a, S, gp + q, v[q]);
                }
            }
            uint32_t crc = 0;
            bool bad = false;
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                if (q < nv) {
                    const int t = (int)v[q];
                    const uint32_t bits = __float_as_uint(v[q]);
                    if (!(t >= 0 && t < 32 && bits == __float_as_uint((float)t))) bad = true;
                    const uint32_t id = (t >= 0 && t < 32) ? (uint32_t)t : 0u;
                    idw[q >> 2] |= id << (8 * (q & 3));
                    crc ^= S.cid4[q][id];  // (a bad value fails the member: its CRC is never used)
                }
            }
            if (nv < kPer) {  // a partial last piece: the values' own chain
                crc = 0;
#pragma unroll
                for (int q = 0; q < kPer; ++q)
                    if (q < nv) crc = crc4(S.crct, crc, __float_as_uint(v[q]));
            }
            if (bad) atomicOr(&S.bad, 1);
            for (int b = tid; b < kBuckets; b += kNT)  // the chains' wave tables (they share memory with the DP's costs)
#pragma unroll
                for (int w2 = 0; w2 < kNT / 64; ++w2) S.u.m.lastw[w2][b] = 0;
            const int r = lo & (kRing - 1);
#pragma unroll
            for (int u = 0; u < kPer / 4; ++u) {
                reinterpret_cast<uint32_t*>(S.tok)[(r >> 2) + u] = idw[u];
                if (r + 4 * u < 32) reinterpret_cast<uint32_t*>(S.tok)[((kRing + r) >> 2) + u] = idw[u];
            }
            // raw CRC-32 by Horner per thread: acc covers this thread's pieces
            // of the full segments so far (each advanced by the 8 KiB of every
            // later segment); the last segment's piece and the combination
            // over the threads follow the loop
            if (c + 1 < nseg) {
                uint32_t adv = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) adv ^= S.adv13[j][(crc_acc >> (4 * j)) & 15u];
                crc_acc = adv ^ crc;
            }
            else crc_last = crc, nv_last = nv;
        }
        __syncthreads();
        if (S.bad) {  // block-uniform
            if (tid == 0) { atomicOr(a.bad, 1); a.sizes[blockIdx.x] = 0; }
            return;
        }
        PH(1);
        // ---- B: 3-gram chains of [c0 - 2, send - 2) (the last two of a
        // segment wait for the next segment's values) ----
        const int s_ins = c == 0 ? 0 : c0 - 2;
        const int e_ins = send - 2;
        const int m_ins = max(0, e_ins - s_ins);
        const int part = (m_ins + kNT - 1) / kNT * 64;
        const int w_lo = s_ins + wv * part, w_hi = min(e_ins, w_lo + part);
        for (int p0 = w_lo; p0 < w_hi; p0 += 64) {
            const int p = p0 + lane;
            const bool act = p < w_hi;
            const int bk = act ? bucket(S.tok, p) : 0;
            uint64_t m = __ballot(act);
#pragma unroll
            for (int b = 0; b < kBucketBits; ++b) {  // buckets < 2^kBucketBits
                const bool on = ((bk >> b) & 1) != 0;
                const uint64_t bb = __ballot(act && on);
                m &= on ? bb : ~bb;
            }
            const uint64_t below = m & ((1ull << lane) - 1ull);
            uint32_t d;
            if (below) {
                d = (uint32_t)(lane - (63 - __builtin_clzll(below)));
            } else {
                const uint32_t lw = act ? S.u.m.lastw[wv][bk] : 0u;
                d = lw ? (uint32_t)(p - (s_ins + (int)lw - 1)) : kPending;
            }
            if (act) {
                S.u.m.prev[pslot(p)] = (uint16_t)d;
                if ((m >> lane) == 1ull) S.u.m.lastw[wv][bk] = (uint16_t)(p - s_ins + 1);
            }
        }
        PH(12);
        __syncthreads();
        // per bucket, in place: an exclusive prefix max of the waves' last
        // occurrences (the nearest one in an earlier wave's part: parts are
        // in wave order), and the next segment's heads; then every pending
        // position takes its link with one read
        const uint32_t* head = S.head[c & 1];
        for (int b = tid; b < kBuckets; b += kNT) {
            uint32_t run = 0;
#pragma unroll
            for (int w2 = 0; w2 < kNT / 64; ++w2) {
                const uint32_t t = S.u.m.lastw[w2][b];
                S.u.m.lastw[w2][b] = (uint16_t)run;
                run = max(run, t);
            }
            S.head[(c + 1) & 1][b] = run ? (uint32_t)s_ins + run : head[b];
        }
        __syncthreads();
        for (int p0 = w_lo; p0 < w_hi; p0 += 64) {
            const int p = p0 + lane;
            if (p < w_hi && S.u.m.prev[pslot(p)] == kPending) {
                const int bk = bucket(S.tok, p);
                const uint32_t lw = S.u.m.lastw[wv][bk];
                const uint32_t h = head[bk];
                uint32_t d = 0;
                if (lw) d = (uint32_t)(p - (s_ins + (int)lw - 1));
                else if (h && p - (int)(h - 1u) <= kWin) d = (uint32_t)(p - (int)(h - 1u));
                S.u.m.prev[pslot(p)] = (uint16_t)d;
            }
        }
        // the frontier reads the chain links of every position, pending ones
        // resolved just above by other waves (without this barrier a wave
        // could read a link before its writer: valid output, but not
        // deterministic -- tools/tlz_check.py "det")
        __syncthreads();
        PH(2);
        // ---- C: each position's frontier of (length, distance) pairs ----
        uint32_t fa[kPer], fb[kPer], fc[kPer];  // entries: length | distance << 7 (lengths increasing)
        int nf[kPer];
        {
            // chain candidates in increasing distance, branch-free: a
            // candidate's first 8 values are compared at once (3 aligned LDS
            // dwords, the 4 positions' loads issued together); a match of 8
            // or more values walks further behind one wave-uniform test (12
            // values at once cost 4 % more encode time for the same stream)
            const uint32_t* tw = reinterpret_cast<const uint32_t*>(S.tok);
            constexpr int kCW = 2;  // values compared at once: 4 kCW
            uint32_t ti[kPer][kCW];  // values i .. i + 4 kCW - 1 of each position
            {
                const int rb = (lo & (kRing - 1)) >> 2;  // lo is a multiple of 8
                uint32_t w[kCW + 3];
#pragma unroll
                for (int k = 0; k < kCW + 3; ++k) w[k] = tw[rb + k];
#pragma unroll
                for (int q = 0; q < kPer; ++q)
#pragma unroll
                    for (int k = 0; k < kCW; ++k) ti[q][k] = __builtin_amdgcn_alignbyte(w[(q >> 2) + k + 1], w[(q >> 2) + k], (uint32_t)(q & 3));
            }
            int j[kPer], bl[kPer], lim[kPer];
            bool act[kPer];
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const int i = lo + q;
                fa[q] = fb[q] = fc[q] = 0;
                bl[q] = kMinL - 1;  // an improvement is then also a copy of >= kMinL values
                lim[q] = min(kMaxL, send - i);
                const uint32_t pd = lim[q] >= kMinL ? S.u.m.prev[pslot(i)] : 0u;
                act[q] = pd != 0;
                j[q] = i - (int)pd;
            }
#pragma unroll 1
            for (int step = 0; step < kCand; ++step) {
                bool any = false;
#pragma unroll
                for (int h = 0; h < kPer; h += 4) {  // two halves: fewer loads in flight, fewer registers
                    uint32_t cw[4][kCW + 1], pd[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int q = h + u;
                        const int jj = act[q] ? j[q] : lo;
                        const int jb = (jj & (kRing - 1)) >> 2;
#pragma unroll
                        for (int k = 0; k <= kCW; ++k) cw[u][k] = tw[jb + k];
                        pd[u] = S.u.m.prev[pslot(jj)];
                    }
                    int Lq[4];
                    bool okq[4], longq[4];
                    bool anylong = false;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int q = h + u;
                        const int i = lo + q;
                        const uint32_t sh = (uint32_t)(j[q] & 3);
                        int L = 4 * kCW;
#pragma unroll
                        for (int k = kCW - 1; k >= 0; --k) {
                            const uint32_t x = __builtin_amdgcn_alignbyte(cw[u][k + 1], cw[u][k], sh) ^ ti[q][k];
                            L = x ? 4 * k + (__builtin_ctz(x) >> 3) : L;
                        }
                        okq[u] = act[q] && i - j[q] <= kWin;
                        longq[u] = okq[u] && L == 4 * kCW && lim[q] > 4 * kCW;
                        anylong |= longq[u];
                        Lq[u] = L;
                    }
                    // rare: a long match walks on.  One wave-uniform test for
                    // the four positions (per-position divergent branches cost
                    // ~50 scalar instructions per step even when no lane took them)
                    if (__builtin_expect(__ballot(anylong) != 0ull, 0)) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int q = h + u;
                            if (longq[u])
                                Lq[u] = 4 * kCW + match_len(S.tok, lo + q + 4 * kCW, j[q] + 4 * kCW, lim[q] - 4 * kCW);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int q = h + u;
                        const int i = lo + q;
                        const bool ok = okq[u];
                        const int L = min(Lq[u], lim[q]);
                        // branch-free (selects, no exec-mask juggling): the
                        // first two improvements go to fa and fb, and fc
                        // always takes the latest (the frontier's count is
                        // read off the three words after the walk)
                        const bool imp = ok && L > bl[q];
                        const uint32_t e = (uint32_t)L | ((uint32_t)(i - j[q]) << 7);
                        fb[q] = imp && fa[q] != 0u && fb[q] == 0u ? e : fb[q];
                        fa[q] = imp && fa[q] == 0u ? e : fa[q];
                        fc[q] = imp ? e : fc[q];
                        bl[q] = imp ? L : bl[q];
                        act[q] = ok && bl[q] < lim[q] && pd[u] != 0;
                        j[q] -= (int)pd[u];
                        any |= act[q];
                    }
                }
                if (!any) break;
            }
#pragma unroll
            for (int q = 0; q < kPer; ++q)  // 0..3 entries; fc repeats fa or fb below three
                nf[q] = fa[q] == 0u ? 0 : fb[q] == 0u ? 1 : fc[q] == fb[q] ? 2 : 3;
        }
        PH(3);
        // ---- D: segmented backward DP (kSweeps sweeps) ----
        // Costs are absolute (1/8 bit to the segment end, < 2^20: 2048 values
        // x 4 literals x 15 bits x 8), so a candidate is one 32-bit key
        // (cost << 3 | candidate index) and the best of a position is a plain
        // min: the index orders the candidates as the old strict-less scan
        // did (literal, lengths kMinL..kU, the three frontier entries), so
        // ties keep the earlier one and the parse is unchanged.  The sweep-
        // invariant part of every candidate is precomputed per position, 16
        // bits each (0xffff: no such candidate; a candidate's cost differs
        // from the literal's by < 3100, so it then never wins):
        //   cA[q] = literal | length 3 << 16, cB[q] = 4 | 5 << 16,
        //   cC[q] = 6 | entry a << 16, cD[q] = entry b | entry c << 16;
        //   a length l: its length + distance cost; an entry (its own length
        //   > kU): l | cost << 7, 0 = none
        uint32_t dc3[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const uint32_t da = nf[q] > 0 ? min(255u, (uint32_t)S.dcst[dist_code(4u * (fa[q] >> 7))]) : 0u;
            const uint32_t db = nf[q] > 1 ? min(255u, (uint32_t)S.dcst[dist_code(4u * (fb[q] >> 7))]) : 0u;
            const uint32_t dc = nf[q] > 2 ? min(255u, (uint32_t)S.dcst[dist_code(4u * (fc[q] >> 7))]) : 0u;
            dc3[q] = da | (db << 8) | (dc << 16);
        }
        __syncthreads();  // the wave tables are dead: the DP's costs take their memory
        for (int k = tid; k <= kSeg; k += kNT) {
            const int rem = max(0, send - c0 - k);
            S.u.m.cost[1][k] = 32u * (uint32_t)rem;  // sweep 0's estimate beyond a thread's positions: 4 bits per value
            if (k >= send - c0) S.u.m.cost[0][k] = 0;
        }
        __syncthreads();
        const int klo = kPer * tid;  // segment-relative
        {
            // own positions' costs in registers (indices are compile-time
            // after unrolling); lengths kMinL..kU branch-free, longer ones
            // only as the frontier entries' own lengths, whose costs beyond
            // this thread's positions come from the previous sweep
            constexpr int kU = 6;              // lengths unrolled: kMinL .. kU (longer: only the entries' own lengths; the same ratio, tools/tlz_proto.c)
            constexpr int kW = kU;             // costs beyond this thread's positions within reach
            static_assert(kU == 6 && kMinL == 3, "the packed candidate table holds lengths 3..6");
            constexpr uint32_t kNone = 0xffffu;
            uint32_t lenr[kU + 1];
#pragma unroll
            for (int l = kMinL; l <= kU; ++l) lenr[l] = S.lenc[l];
            uint32_t cA[kPer], cB[kPer], cC[kPer], cD[kPer];
            bool live[kPer];
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const uint32_t lit = min(511u, (uint32_t)S.litc[(idw[q >> 2] >> (8 * (q & 3))) & 0xffu]);
                const int La = (int)(fa[q] & 127u), Lb = (int)(fb[q] & 127u);
                const int Lm = nf[q] == 0 ? 0 : (int)((nf[q] == 1 ? fa[q] : nf[q] == 2 ? fb[q] : fc[q]) & 127u);
                live[q] = c0 + klo + q < send;
                uint32_t lc[kU + 1];
#pragma unroll
                for (int l = kMinL; l <= kU; ++l) {
                    const uint32_t e = l <= La ? 0u : l <= Lb ? 1u : 2u;
                    lc[l] = l <= Lm ? lenr[l] + ((dc3[q] >> (8 * e)) & 255u) : kNone;
                }
                uint32_t E[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int l = e == 0 ? La : e == 1 ? Lb : Lm;
                    const bool use = l > kU && l <= Lm && nf[q] > e;
                    const uint32_t dcost = (dc3[q] >> (8 * e)) & 255u;
                    E[e] = use ? (uint32_t)l | (min(511u, (uint32_t)S.lenc[l] + dcost) << 7) : 0u;
                }
                cA[q] = lit | (lc[3] << 16);
                cB[q] = lc[4] | (lc[5] << 16);
                cC[q] = lc[6] | (E[0] << 16);
                cD[q] = E[1] | (E[2] << 16);
            }
#pragma unroll 1
            for (int sw = 0; sw < kSweeps; ++sw) {
                uint32_t* cur = S.u.m.cost[sw & 1];
                const uint32_t* prv = S.u.m.cost[(sw + 1) & 1];
                uint32_t pw[kW + 1];
#pragma unroll
                for (int u = 0; u <= kW; ++u) pw[u] = prv[min(klo + kPer + u, kSeg)];
                // the frontier entries read costs of the previous sweep only:
                // their reads are issued here, before the chain, unconditionally
                // (el = 0 reads the position's own cost, then discarded:
                // behind a branch each cost ~5 scalar instructions of exec
                // juggling), and each position's best entry key is formed
                uint32_t me[kPer];
#pragma unroll
                for (int h = 0; h < kPer; h += 2) {  // two positions' six reads at a time (registers)
                    uint32_t pe[2][3];
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int e = 0; e < 3; ++e) {
                            const int q = h + u;
                            const uint32_t En = e == 0 ? (cC[q] >> 16) : e == 1 ? (cD[q] & 0xffffu) : (cD[q] >> 16);
                            pe[u][e] = prv[min(klo + q + (int)(En & 127u), kSeg)];
                        }
                    asm volatile("" : "+v"(pe[0][0]), "+v"(pe[0][1]), "+v"(pe[0][2]), "+v"(pe[1][0]), "+v"(pe[1][1]),
                                 "+v"(pe[1][2]));
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int q = h + u;
                        me[q] = 0xffffffffu;
#pragma unroll
                        for (int e = 0; e < 3; ++e) {
                            const uint32_t En = e == 0 ? (cC[q] >> 16) : e == 1 ? (cD[q] & 0xffffu) : (cD[q] >> 16);
                            const uint32_t cc = (((En >> 7) + pe[u][e]) << 3) | (uint32_t)(5 + e);
                            me[q] = min(me[q], (En & 127u) != 0u ? cc : 0xffffffffu);
                        }
                    }
                }
                uint32_t cr[kPer], key[kPer];
#pragma unroll
                for (int q = kPer - 1; q >= 0; --q) {
                    auto CV = [&](int kk) -> uint32_t { return kk < kPer ? cr[kk] : pw[kk - kPer]; };  // kk = q + l
                    uint32_t best = min((((cA[q] & 0xffffu) + CV(q + 1)) << 3), me[q]);
                    best = min(best, (((cA[q] >> 16) + CV(q + 3)) << 3) | 1u);
                    best = min(best, (((cB[q] & 0xffffu) + CV(q + 4)) << 3) | 2u);
                    best = min(best, (((cB[q] >> 16) + CV(q + 5)) << 3) | 3u);
                    best = min(best, (((cC[q] & 0xffffu) + CV(q + 6)) << 3) | 4u);
                    cr[q] = live[q] ? best >> 3 : 0u;
                    key[q] = best;
                }
                // (a position past the segment's values stores 0: its cost already)
#pragma unroll
                for (int q = 0; q < kPer; ++q) cur[klo + q] = cr[q];
                if (sw == kSweeps - 1) {  // the choices: length | frontier entry << 8 (0: literal)
#pragma unroll
                    for (int q = 0; q < kPer; ++q) {
                        if (!live[q]) continue;
                        const uint32_t k = key[q] & 7u;
                        uint32_t ch = 0;
                        if (k >= 5u) {
                            const uint32_t ent = k == 5u ? fa[q] : k == 6u ? fb[q] : fc[q];
                            ch = (ent & 127u) | ((k - 5u) << 8);
                        } else if (k >= 1u) {
                            const uint32_t l = k + 2u, La = fa[q] & 127u, Lb = fb[q] & 127u;
                            ch = l | ((l <= La ? 0u : l <= Lb ? 1u : 2u) << 8);
                        }
                        S.dec[klo + q] = (uint16_t)ch;
                    }
                }
                __syncthreads();
            }
        }
        PH(4);
        // ---- E: the DP's path from the segment start: Jacobi rounds ----
        auto nxt = [&](int p) -> int { const int l = S.dec[p - c0] & 0xff; return p + (l ? l : 1); };
        for (int i = tid; i < (kNT / 64) * ((kLit + kDist + 1) / 2); i += kNT) (&S.u.m.hw[0][0])[i] = 0;  // F's tables (the DP's costs are dead)
        {
            int p = tid == 0 ? c0 : max(c0, lo - kMaxL);
            while (p < lo && p < send) p = nxt(p);
            S.entry[tid] = (uint16_t)(p - c0);
        }
        __syncthreads();
#pragma unroll 1
        for (;;) {
            int p = c0 + S.entry[tid];
            while (p < lo + kPer && p < send) p = nxt(p);
            __syncthreads();
            int changed = 0;
            if (tid + 1 < kNT && (int)S.entry[tid + 1] != p - c0) { S.entry[tid + 1] = (uint16_t)(p - c0); changed = 1; }
            if (ph_on) ++ph_acc[11];
            if (!__syncthreads_or(changed)) break;
        }
        PH(5);
        // ---- F: this segment's ops, in order; symbol counts ----
        {
            uint32_t opm = 0;
            for (int p = c0 + S.entry[tid]; p < lo + kPer && p < send; p = nxt(p)) opm |= 1u << (p - lo);
            PH(13);
            uint32_t tot;
            const uint32_t off = block_scan<kNT>((uint32_t)__popc(opm), S.scan, &tot);
            PH(14);
            const uint32_t base = S.ops_n;
            uint32_t k = base + off;
            uint32_t nl = 0, nd = 0;
            // symbol counts into this wave's own table (same-wave atomics only)
            uint32_t* const hw = S.u.m.hw[wv];
            auto cnt = [&](int sym) { atomicAdd(&hw[sym >> 1], (sym & 1) ? 0x10000u : 1u); };
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                if (!((opm >> q) & 1u)) continue;
                const uint32_t dq = S.dec[klo + q];
                const uint32_t l = dq & 0xffu;
                uint32_t rec;
                if (l == 0) {
                    const uint32_t id = (idw[q >> 2] >> (8 * (q & 3))) & 0xffu;
                    rec = 0x80000000u | id;
                    const uint32_t b = __float_as_uint((float)id);
#pragma unroll
                    for (int y = 0; y < 4; ++y) cnt((int)((b >> (8 * y)) & 0xffu));
                    nl += 4;
                } else {
                    const uint32_t e = dq >> 8;
                    const uint32_t ent = e == 0 ? fa[q] : e == 1 ? fb[q] : fc[q];
                    const uint32_t d = ent >> 7;
                    rec = l | (d << 7);
                    cnt(257 + len_code(4u * l));
                    cnt(kLit + dist_code(4u * d));
                    nl += 1;
                    nd += 1;
                }
                ops[k++] = rec;
            }
            for (int o = 32; o > 0; o >>= 1) {
                nl += (uint32_t)__shfl_xor((int)nl, o, 64);
                nd += (uint32_t)__shfl_xor((int)nd, o, 64);
            }
            if (lane == 0) { atomicAdd(&S.totl, nl); atomicAdd(&S.totd, nd); }
            if (tid == 0) S.segop[c] = base;
            __syncthreads();
            if (tid == 0) S.ops_n = base + tot;
            for (int sym = tid; sym < kLit + kDist; sym += kNT) {  // merge the waves' counts
                uint32_t v = 0;
#pragma unroll
                for (int w = 0; w < kNT / 64; ++w) v += (S.u.m.hw[w][sym >> 1] >> (16 * (sym & 1))) & 0xffffu;
                if (sym < kLit) S.hl[sym] += v; else S.hd[sym - kLit] += v;
            }
        }
        PH(6);
        __syncthreads();  // the merged counts
        if (c + 1 < nseg) tlz_model(S, tid, false);
        PH(7);
    }

    {  // the member's raw CRC-32: every thread's pieces advanced to the member's end, XOR-ed
        const uint32_t bl = 4u * (uint32_t)(ntok - ((nseg - 1) << kSegLog));  // bytes of the last segment
        uint32_t r = nv_last ? crc_adv(crc_last, bl - 4u * kPer * (uint32_t)tid - 4u * (uint32_t)nv_last) : 0u;
        if (nseg > 1) r ^= crc_adv(crc_acc, (uint32_t)(kSeg * 4) + bl - 4u * kPer * (uint32_t)(tid + 1));
        for (int o = 32; o > 0; o >>= 1) r ^= (uint32_t)__shfl_xor((int)r, o, 64);
        if (lane == 0) S.crc_w[wv] = r;
        __syncthreads();
        if (tid == 0) {
            uint32_t x = 0;
            for (int w = 0; w < kNT / 64; ++w) x ^= S.crc_w[w];
            S.crc_raw = x;
        }
    }
    // ---- G: the member's Huffman code (lengths limited to the inflate's table bits) ----
    const int ln = lane;
    if (wv == 0) {
        HScratch& h = S.u.f.h;
        if (ln == 0) S.hl[256] = 1;  // end of block
        __builtin_amdgcn_wave_barrier();
        if (!huff_lengths_wave(S.hl, kLit, kLitMax, S.ll, h.w, true) && ln == 0) huff_lengths(S.hl, kLit, kLitMax, S.ll, h, true);
    } else if (wv == 1) {
        HScratch& h = S.u.f.h;
        const bool anyd = __ballot(ln < kDist && S.hd[ln] != 0u) != 0ull;
        if (!anyd && ln == 0) S.hd[0] = 1;  // one (unused) distance code
        __builtin_amdgcn_wave_barrier();
        huff_lengths_wave(S.hd, kDist, kDistMax, S.ld, reinterpret_cast<uint32_t*>(h.rle_ext), false);
    }
    __syncthreads();
    if (wv == 1) huff_codes_wave(S.ll, kLit, S.kl);
    if (wv == 2) huff_codes_wave(S.ld, kDist, S.kd);
    if (wv == 0) {  // run-length code of the code lengths (as RFC 1951 3.2.7)
        HScratch& h = S.u.f.h;
        int nlit = 257, ndist = 1;
        for (int cc = 0; cc < (kLit + 63) / 64; ++cc) {
            const int i = 64 * cc + ln;
            const uint64_t m = __ballot(i < kLit && S.ll[i] != 0);
            if (m) nlit = max(nlit, 64 * cc + 64 - __builtin_clzll(m));
        }
        {
            const uint64_t m = __ballot(ln < kDist && S.ld[ln] != 0);
            if (m) ndist = max(ndist, 64 - __builtin_clzll(m));
        }
        const int N = nlit + ndist;
        auto val = [&](int i) -> int { return i < nlit ? S.ll[i] : S.ld[i - nlit]; };
        uint64_t starts[(kLit + kDist + 63) / 64];
#pragma unroll
        for (int cc = 0; cc < (kLit + kDist + 63) / 64; ++cc) {
            const int i = 64 * cc + ln;
            starts[cc] = __ballot(i < N && (i == 0 || val(i) != val(i - 1)));
        }
        if (ln == 0) {
            int nr = 0, cc = 0, s0 = 0;
            uint64_t m = starts[0];
            m &= m - 1;
            for (;;) {
                while (!m && cc + 1 < (kLit + kDist + 63) / 64) m = starts[++cc];
                const int s1 = m ? 64 * cc + __builtin_ctzll(m) : N;
                if (m) m &= m - 1;
                const int cur = val(s0);
                int left = s1 - s0;
                if (cur == 0) {
                    while (left >= 11) { const int r = left < 138 ? left : 138; h.rle_sym[nr] = 18; h.rle_ext[nr++] = (uint16_t)(r - 11); left -= r; }
                    if (left >= 3) { h.rle_sym[nr] = 17; h.rle_ext[nr++] = (uint16_t)(left - 3); left = 0; }
                    while (left > 0) { h.rle_sym[nr] = 0; h.rle_ext[nr++] = 0; --left; }
                } else {
                    h.rle_sym[nr] = (uint16_t)cur; h.rle_ext[nr++] = 0; --left;
                    while (left >= 3) { const int r = left < 6 ? left : 6; h.rle_sym[nr] = 16; h.rle_ext[nr++] = (uint16_t)(r - 3); left -= r; }
                    while (left > 0) { h.rle_sym[nr] = (uint16_t)cur; h.rle_ext[nr++] = 0; --left; }
                }
                if (s1 >= N) break;
                s0 = s1;
            }
            for (int i = 0; i < nr; ++i) S.hc[h.rle_sym[i]]++;
            S.nrle = (uint32_t)nr;
            S.nlit_ndist = (uint32_t)(nlit | (ndist << 16));
        }
    }
    __syncthreads();
    if (wv == 0) {
        HScratch& h = S.u.f.h;
        huff_lengths_wave(S.hc, kCL, 7, S.lc, h.w, true);
        huff_codes_wave(S.lc, kCL, S.kc);
    }
    if (tid == 0) {  // the deflate block header's bits (words of the member's data start)
        HScratch& h = S.u.f.h;
        const int nr = (int)S.nrle, nlit = (int)(S.nlit_ndist & 0xffffu), ndist = (int)(S.nlit_ndist >> 16);
        int ncl = kCL;
        while (ncl > 4 && S.lc[c_clord[ncl - 1]] == 0) --ncl;
        uint64_t acc = 0;
        int nb = 0;
        uint32_t wi = 0, pos = 0;
        auto put = [&](uint32_t v, int n) {
            acc |= (uint64_t)v << nb;
            nb += n;
            pos += (uint32_t)n;
            if (nb >= 32) { S.u.f.hdrw[wi++] = (uint32_t)acc; acc >>= 32; nb -= 32; }
        };
        put(1u, 1);  // BFINAL
        put(2u, 2);  // BTYPE = dynamic
        put((uint32_t)(nlit - 257), 5);
        put((uint32_t)(ndist - 1), 5);
        put((uint32_t)(ncl - 4), 4);
        for (int i = 0; i < ncl; ++i) put(S.lc[c_clord[i]], 3);
        for (int i = 0; i < nr; ++i) {
            const int sy = h.rle_sym[i];
            put(S.kc[sy], S.lc[sy]);
            const int eb = sy == 16 ? 2 : (sy == 17 ? 3 : (sy == 18 ? 7 : 0));
            put(h.rle_ext[i], eb);
        }
        if (nb > 0) S.u.f.hdrw[wi] = (uint32_t)acc;
        S.hdr_bits = pos;
    }
    __syncthreads();

    PH(8);
    // ---- H: bits of the ops (a block scan of their costs), segment offsets ----
    // every op's code and extra bits come from small LDS tables (a literal
    // value: its four codes in two words; a length: code | extra bits) and
    // the distance's code index and extra bits by arithmetic
    if (tid < 32) {
        const uint32_t bb = __float_as_uint((float)tid);
        uint32_t v[2] = {0, 0}, n[2] = {0, 0};
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const uint32_t by = (bb >> (8 * y)) & 0xffu;
            v[y >> 1] |= (uint32_t)S.kl[by] << n[y >> 1];
            n[y >> 1] += S.ll[by];
        }
        S.u.f.litlo[tid] = v[0] | (n[0] << 24);
        S.u.f.lithi[tid] = v[1] | (n[1] << 24);
    } else if (tid >= 64 && tid < 64 + kMaxL + 1) {
        const int l = tid - 64;
        uint32_t w = 0;
        if (l >= kMinL) {
            int lc, ne;
            uint32_t ev;
            len_sym(4u * (uint32_t)l, lc, ne, ev);
            const uint32_t cl = S.ll[257 + lc];
            w = ((uint32_t)S.kl[257 + lc] | (ev << cl)) | ((cl + (uint32_t)ne) << 24);
        }
        S.u.f.lenw[l] = w;
    }
    __syncthreads();
    const uint32_t nops = S.ops_n, H = S.hdr_bits;
    const uint32_t o_lo = (uint32_t)((uint64_t)nops * tid / kNT), o_hi = (uint32_t)((uint64_t)nops * (tid + 1) / kNT);
    auto dist_w = [&](uint32_t dv) -> uint32_t {  // code | extra bits, n << 24 (n <= 10 + 13)
        int dc, ne;
        uint32_t ev;
        dist_sym(4u * dv, dc, ne, ev);
        const uint32_t cd = S.ld[dc];
        return ((uint32_t)S.kd[dc] | (ev << cd)) | ((cd + (uint32_t)ne) << 24);
    };
    auto op_bits = [&](uint32_t rec) -> uint32_t {
        if (rec >> 31) return (S.u.f.litlo[rec & 31u] >> 24) + (S.u.f.lithi[rec & 31u] >> 24);
        return (S.u.f.lenw[rec & 127u] >> 24) + (dist_w(rec >> 7) >> 24);
    };
    uint32_t mine = 0;
#pragma unroll 4
    for (uint32_t o = o_lo; o < o_hi; ++o) mine += op_bits(ops[o]);
    uint32_t tot;
    const uint32_t pos0 = H + block_scan<kNT>(mine, S.scan, &tot);
    if (tid == 0) S.total_bits = H + tot;
    const uint32_t D = (uint32_t)hdr_bytes(nseg);  // header bytes (a multiple of 4)
    uint32_t* const slot = reinterpret_cast<uint32_t*>(a.slots + (int64_t)blockIdx.x * a.slot_bytes);
    uint32_t* const dw = slot + D / 4;                    // the deflate data's words
    {
        const uint32_t nw = (H + tot + 15u + 7u + 64u + 31u) / 32u + 1u;
        for (uint32_t i = tid; i < nw; i += kNT) dw[i] = 0;
    }
    __syncthreads();
    if (tid == 0)
        for (uint32_t i = 0; i < (H + 31u) / 32u; ++i) atomicOr(&dw[i], S.u.f.hdrw[i]);
    {
        // the segments whose first op lies in this thread's range get their
        // bit offset here, as the emission passes that op
        int sidx = 0;
        while (sidx < nseg && S.segop[sidx] < o_lo) ++sidx;
        uint32_t next_seg = sidx < nseg ? S.segop[sidx] : 0xffffffffu;
        uint64_t acc = 0;
        int nb = (int)(pos0 & 31u);
        uint32_t wi = pos0 >> 5;
        bool first = true;
        auto put = [&](uint32_t w) {  // code | extra bits, n << 24 (n <= 24)
            acc |= (uint64_t)(w & 0xffffffu) << nb;
            nb += (int)(w >> 24);
            if (nb >= 32) {
                if (first) { atomicOr(&dw[wi], (uint32_t)acc); first = false; }
                else dw[wi] = (uint32_t)acc;
                ++wi;
                acc >>= 32;
                nb -= 32;
            }
        };
#pragma unroll 2
        for (uint32_t o = o_lo; o < o_hi; ++o) {
            if (o == next_seg) {
                S.segbit[sidx++] = 32u * wi + (uint32_t)nb;
                next_seg = sidx < nseg ? S.segop[sidx] : 0xffffffffu;
            }
            const uint32_t rec = ops[o];
            if (rec >> 31) {
                put(S.u.f.litlo[rec & 31u]);
                put(S.u.f.lithi[rec & 31u]);
            } else {
                put(S.u.f.lenw[rec & 127u]);
                put(dist_w(rec >> 7));
            }
        }
        if (nb > 0) atomicOr(&dw[wi], (uint32_t)acc);
    }
    __syncthreads();
    // ---- I: end of block, CRC-32, ISIZE, the member header ----
    if (tid == 0) {
        uint32_t p = S.total_bits;
        put_bits(dw, p, S.kl[256], S.ll[256]);
        p += S.ll[256];
        p = (p + 7u) & ~7u;
        const uint32_t crc32 = crc_adv(0xffffffffu, 4u * (uint32_t)ntok) ^ S.crc_raw ^ 0xffffffffu;
        put_bits(dw, p, crc32, 32);
        p += 32;
        put_bits(dw, p, 4u * (uint32_t)ntok, 32);
        p += 32;
        const uint32_t bytes = D + p / 8u;
        uint8_t* hb = S.u.f.hb;
        const uint32_t len = (uint32_t)(kOzFixed + table_bytes(nseg)), xlen = (uint32_t)kSubFixed + len;
        constexpr int kPre = kGzFixed + kSubFixed;  // the gzip header and the subfield's id and LEN
        const uint8_t fixed[kPre] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xff, (uint8_t)xlen, (uint8_t)(xlen >> 8),
                                     'O', 'Z', (uint8_t)len, (uint8_t)(len >> 8)};
        for (int i = 0; i < kPre; ++i) hb[i] = fixed[i];
        uint8_t* oz = hb + kGzFixed;
        oz[kOzVersion] = (uint8_t)kVersion;
        oz[kOzSegLog] = (uint8_t)kSegLog;
        oz[kOzNseg] = (uint8_t)nseg;
        oz[kOzNseg + 1] = (uint8_t)(nseg >> 8);
        for (int i = 0; i < 4; ++i) {
            oz[kOzBytes + i] = (uint8_t)(bytes >> (8 * i));
            oz[kOzValues + i] = (uint8_t)((uint32_t)ntok >> (8 * i));
        }
        for (int s = 0; s < nseg; ++s)
            for (int i = 0; i < 4; ++i) hb[kHdrFixed + 4 * s + i] = (uint8_t)(S.segbit[s] >> (8 * i));
        for (uint32_t i = 0; i < D / 4; ++i) slot[i] = reinterpret_cast<const uint32_t*>(hb)[i];
        a.sizes[blockIdx.x] = bytes;
    }
    PH(9);
    if (ph_on)
        for (int k = 0; k < kEncPhases; ++k) a.phases[k] = ph_acc[k];
}

}  // namespace tlz
}  // namespace gz
