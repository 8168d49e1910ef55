// gz_device.h -- device helpers of the gzip codec (deflate_kernels.hip): the
// RFC 1951 tables, bit, code and CRC-32 helpers, the Huffman code builder and
// the scan of the member sizes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gz_format.h"

#define DEVI __device__ __forceinline__

namespace gz {

constexpr int kLit = 286, kDist = 30, kCL = 19;

__constant__ uint16_t c_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129,
                                     193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__constant__ uint16_t c_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
                                     67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t c_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint32_t c_adv[32][32];       // raw CRC advance by 2^k zero bytes: GF(2) matrix columns

// Huffman scratch (the serial fallback of huff_lengths_wave, the RLE)
struct HScratch {
    uint32_t w[2 * kLit];
    int16_t parent[2 * kLit];
    int16_t sym[kLit];
    uint8_t dead[2 * kLit];
    uint16_t rle_sym[kLit + kDist];
    uint16_t rle_ext[kLit + kDist];
};
constexpr int kHdrW = 160;                 // deflate block header words (<= 4642 bits)

DEVI void put_bits(uint32_t* out, uint32_t pos, uint32_t val, int nb) {
    if (nb == 0) return;
    const uint32_t w = pos >> 5, sh = pos & 31u;
    atomicOr(&out[w], val << sh);
    if (sh + (uint32_t)nb > 32u) atomicOr(&out[w + 1], val >> (32u - sh));
}
DEVI uint32_t rev_bits(uint32_t c, int n) { return __brev(c) >> (32 - n); }
// distance code of a distance d in 1..32768 (RFC 1951 3.2.5): codes 0..3 are
// d - 1, then two codes per power of two
DEVI int dist_code(uint32_t d) {
    if (d <= 4u) return (int)d - 1;
    const uint32_t m = d - 1u;
    const int b = 31 - __builtin_clz(m);
    return 2 * b + (int)((m >> (b - 1)) & 1u);
}
// index into c_lbase (symbol 257 + index) of a length of l bytes, 3..258
DEVI int len_code(uint32_t l) {
    if (l == 258u) return 28;
    const uint32_t m = l - 3u;
    if (m < 8u) return (int)m;
    const int b = 31 - __builtin_clz(m);
    return 4 * (b - 1) + (int)((m >> (b - 2)) & 3u);
}
// a length's / distance's code with its extra bits computed (no table
// loads: the tables are in constant memory, and a per-lane index into them is
// a vector memory load per lookup): l, d in bytes, l in 11..258, d >= 1
DEVI void len_sym(uint32_t l, int& lc, int& ne, uint32_t& ev) {
    const uint32_t m = l - 3u;
    if (m < 8u) { lc = (int)m; ne = 0; ev = 0; return; }
    const int b = 31 - __builtin_clz(m);
    lc = 4 * (b - 1) + (int)((m >> (b - 2)) & 3u);
    ne = b - 2;
    ev = m & ((1u << ne) - 1u);
}
DEVI void dist_sym(uint32_t d, int& dc, int& ne, uint32_t& ev) {
    const uint32_t m = d - 1u;
    if (d <= 4u) { dc = (int)m; ne = 0; ev = 0; return; }
    const int b = 31 - __builtin_clz(m);
    dc = 2 * b + (int)((m >> (b - 1)) & 1u);
    ne = b - 1;
    ev = m & ((1u << ne) - 1u);
}
// advance by 2^k zero bytes (k uniform: the matrix columns are scalar loads)
DEVI uint32_t crc_adv_pow2(uint32_t v, int k) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) r ^= ((v >> i) & 1u) ? c_adv[k][i] : 0u;
    return r;
}
// raw (zero-initialised, reflected) CRC-32 steps, bitwise: a byte, a
// little-endian word
DEVI uint32_t crc_byte(uint32_t r, uint32_t b) {
    r ^= b;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
    return r;
}
DEVI uint32_t crc_word(uint32_t r, uint32_t w) {
    r ^= w;
#pragma unroll
    for (int k = 0; k < 32; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
    return r;
}
DEVI uint32_t crc_adv(uint32_t v, uint32_t len) {
    for (int k = 0; k < 32; ++k)
        if ((len >> k) & 1u) {
            uint32_t r = 0;
            for (int i = 0; i < 32; ++i) r ^= ((v >> i) & 1u) ? c_adv[k][i] : 0u;
            v = r;
        }
    return v;
}

// Huffman code lengths of freq[0..n) limited to maxlen (thread 0): two
// smallest live nodes merged until one is left; if too deep, halve the
// frequencies (keeping them >= 1) and rebuild
// complete: a lone symbol gets a partner (zlib accepts an incomplete code only
// for distances)
DEVI void huff_lengths(const uint32_t* freq, int n, int maxlen, uint8_t* len, HScratch& h, bool complete) {
    int m = 0;
    for (int s = 0; s < n; ++s) { len[s] = 0; if (freq[s]) { h.sym[m] = (int16_t)s; h.w[m] = freq[s]; ++m; } }
    if (m == 0) return;
    if (m == 1) {
        len[h.sym[0]] = 1;
        if (complete) len[h.sym[0] == 0 ? 1 : 0] = 1;
        return;
    }
    for (;;) {
        for (int i = 0; i < 2 * m; ++i) { h.dead[i] = 0; h.parent[i] = -1; }
        int nodes = m;
        for (int it = 0; it < m - 1; ++it) {
            int a = -1, b = -1;
            for (int i = 0; i < nodes; ++i) {
                if (h.dead[i]) continue;
                if (a < 0 || h.w[i] < h.w[a]) { b = a; a = i; }
                else if (b < 0 || h.w[i] < h.w[b]) b = i;
            }
            h.w[nodes] = h.w[a] + h.w[b];
            h.dead[a] = h.dead[b] = 1;
            h.parent[a] = h.parent[b] = (int16_t)nodes;
            ++nodes;
        }
        int deepest = 0;
        for (int i = 0; i < m; ++i) {
            int d = 0;
            for (int j = i; h.parent[j] >= 0; j = h.parent[j]) ++d;
            len[h.sym[i]] = (uint8_t)d;
            deepest = d > deepest ? d : deepest;
        }
        if (deepest <= maxlen) return;
        for (int i = 0; i < m; ++i) h.w[i] = (h.w[i] >> 1) | 1u;
    }
}
// canonical codes (RFC 1951 3.2.2), stored bit-reversed for LSB-first output
DEVI void huff_codes(const uint8_t* len, int n, uint16_t* code) {
    uint32_t cnt[16] = {0}, next[16];
    for (int s = 0; s < n; ++s) cnt[len[s]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + cnt[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)rev_bits(next[len[s]]++, len[s]) : 0;
}

// ---- the same on one wave (lanes 0..63 of the block) ----------------------
// The serial versions above are latency-bound on one lane (~60 % of a
// member's time).  The rank alphabets use a few dozen literal bytes and
// length / distance codes, so one symbol per lane fits: the used symbols are
// compacted in symbol order, bitonic-sorted by (weight, symbol) across the
// lanes (shfl_xor), and the two-queue merge (leaves in sorted order, internal
// nodes in creation order, both nondecreasing) runs on wave-uniform values
// through readlane / writelane; depths are assigned top-down.  Returns false
// (lengths zeroed) when more than 64 symbols occur: the caller then runs the
// serial huff_lengths on lane 0.  scratch: 64 LDS words.
DEVI uint32_t rdl(uint32_t v, int i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, i); }
DEVI uint32_t wrl(uint32_t v, int i, uint32_t old) { return (int)(threadIdx.x & 63u) == i ? v : old; }

DEVI bool huff_lengths_wave(const uint32_t* freq, int n, int maxlen, uint8_t* len, uint32_t* scratch, bool complete) {
    const int lane = (int)(threadIdx.x & 63u);
    int m = 0;
    for (int b = 0; b < n; b += 64) {
        const int s = b + lane;
        const uint32_t f = s < n ? freq[s] : 0u;
        const uint64_t mask = __ballot(f != 0u);
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        if (f != 0u && m + rank < 64) scratch[m + rank] = (f << 9) | (uint32_t)s;
        if (s < n) len[s] = 0;
        m += __popcll(mask);
    }
    if (m > 64) return false;
    if (m == 0) return true;
    if (m == 1) {
        const int s = (int)(scratch[0] & 511u);
        if (lane == 0) {
            len[s] = 1;
            if (complete) len[s == 0 ? 1 : 0] = 1;
        }
        return true;
    }
    uint32_t key0 = lane < m ? scratch[lane] : 0xffffffffu;
    for (;;) {
        uint32_t key = key0;
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)key, j, 64);
                const bool up = (lane & k) == 0, lower = (lane & j) == 0;
                key = (lower == up) ? min(key, o) : max(key, o);
            }
        const uint32_t w = key >> 9;  // lane i: the i-th smallest leaf weight
        uint32_t iw = 0, ca = 0, cb = 0;  // lane k: internal node k's weight and children
        int li = 0, ij = 0, ni = 0;
        for (int step = 0; step < m - 1; ++step) {
            uint32_t cw0, cw1;
            int c0, c1;
            {
                const uint32_t lw = li < m ? rdl(w, li) : 0xffffffffu, nw = ij < ni ? rdl(iw, ij) : 0xffffffffu;
                if (li < m && (ij >= ni || lw <= nw)) { c0 = li; cw0 = lw; ++li; } else { c0 = 64 + ij; cw0 = nw; ++ij; }
            }
            {
                const uint32_t lw = li < m ? rdl(w, li) : 0xffffffffu, nw = ij < ni ? rdl(iw, ij) : 0xffffffffu;
                if (li < m && (ij >= ni || lw <= nw)) { c1 = li; cw1 = lw; ++li; } else { c1 = 64 + ij; cw1 = nw; ++ij; }
            }
            iw = wrl(cw0 + cw1, ni, iw);
            ca = wrl((uint32_t)c0, ni, ca);
            cb = wrl((uint32_t)c1, ni, cb);
            ++ni;
        }
        uint32_t di = 0, dl = 0;  // depth of internal node k (lane k) / of the i-th leaf (lane i)
        int deepest = 0;
        for (int k = ni - 1; k >= 0; --k) {
            const uint32_t d = rdl(di, k) + 1u;
            const int a = (int)rdl(ca, k), b = (int)rdl(cb, k);
            if (a >= 64) di = wrl(d, a - 64, di); else { dl = wrl(d, a, dl); deepest = max(deepest, (int)d); }
            if (b >= 64) di = wrl(d, b - 64, di); else { dl = wrl(d, b, dl); deepest = max(deepest, (int)d); }
        }
        if (deepest <= maxlen) {
            if (lane < m) len[key & 511u] = (uint8_t)dl;
            return true;
        }
        // too deep: flatten the weights (>= 1) and rebuild, as huff_lengths
        key0 = lane < m ? (((((key0 >> 9) >> 1) | 1u)) << 9) | (key0 & 511u) : 0xffffffffu;
    }
}

// canonical codes on one wave: counts per length and ranks by ballots
DEVI void huff_codes_wave(const uint8_t* len, int n, uint16_t* code) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t cnt[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) cnt[b] = 0;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const int L = s < n ? len[s] : 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) cnt[b] += (uint32_t)__popcll(__ballot(L == b));
    }
    uint32_t run[16];
    uint32_t c = 0;
    run[0] = 0;
#pragma unroll
    for (int b = 1; b < 16; ++b) { c = (c + (b > 1 ? cnt[b - 1] : 0u)) << 1; run[b] = c; }
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const int L = s < n ? len[s] : 0;
        uint32_t mine = 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) {
            const uint64_t mk = __ballot(L == b);
            if (L == b) mine = run[b] + (uint32_t)__popcll(mk & below);
            run[b] += (uint32_t)__popcll(mk);
        }
        if (s < n) code[s] = L ? (uint16_t)rev_bits(mine, L) : 0;
    }
}

// exclusive scan of the member sizes (one block) -> offsets, total at [n]
// running (nullable): the stream bytes of earlier batches, added to every
// offset and advanced by this batch's total; cap: the output's size (a batch
// that would not fit sets *bad = 2 and advances nothing)
__global__ __launch_bounds__(1024) void k_gzip_scan(const uint32_t* sizes, int n, uint64_t* off, uint64_t* running,
                                                    uint64_t cap, int* bad) {
    __shared__ uint64_t part[1024 / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (n + 1023) / 1024;
    const int b0 = tid * per, b1 = std::min(n, b0 + per);
    uint64_t s = 0;
    for (int i = b0; i < b1; ++i) s += sizes[i];
    uint64_t inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) part[w] = inc;
    __syncthreads();
    const uint64_t run0 = running ? *running : 0;
    uint64_t tot = 0;
    for (int j = 0; j < 1024 / 64; ++j) tot += part[j];
    const bool fits = run0 + tot <= cap;
    uint64_t base = inc - s + run0;
    for (int j = 0; j < w; ++j) base += part[j];
    for (int i = b0; i < b1; ++i) { off[i] = fits ? base : ~0ull; base += sizes[i]; }
    if (tid == 1023) off[n] = base;
    __syncthreads();
    if (tid == 0 && running) {
        if (fits) *running = run0 + tot;
        else atomicOr(bad, 2);
    }
}

}  // namespace gz
