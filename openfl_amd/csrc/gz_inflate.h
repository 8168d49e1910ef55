// gz_inflate.h -- the generic member inflate of the gzip codec
// (deflate_kernels.hip).
#pragma once
#include "gz_device.h"

namespace gz {

// ============================================================================
// Device inflate of member-indexed streams (GZIPTransformer.backward,
// kc_pipeline.py:152-156: gzip.decompress).  One wavefront per member; the
// Huffman decode is inherently serial, so every lane runs it on the same
// (wave-uniform) values and the lanes split the work that is parallel: table
// construction, each copy's bytes (an overlapping copy d < L is the periodic
// extension out[p + i] = out[p - d + i % d]) and the store.  Default (RING):
// only the last WIN = 1 KiB of a member's output stays in LDS, every byte is
// also stored to global memory as it is produced, and the rare copy reaching
// further back than the ring reads those global bytes back (stored earlier by
// the same wavefront; a wavefront-scope acquire/release fence orders them);
// the window decoder (RING = false, OFL_GZ_INFLATE=window) keeps the whole
// output in a 16 / 64 KiB LDS window instead.  The compressed bytes stream
// through a small LDS ring.
// Any valid deflate data decodes (stored, fixed and dynamic blocks, RFC 1951).
// ISIZE and the CRC-32 (over the member's output, wave-parallel) are checked here.
constexpr int kRing = 512;                 // compressed-input ring per wave (bytes)
#ifndef OFL_INF_FASTBITS
#define OFL_INF_FASTBITS 9
#endif
#ifndef OFL_INF_WAVES
#define OFL_INF_WAVES 1
#endif
constexpr int kFastBits = OFL_INF_FASTBITS; // first-level decode table: codes of <= 9 bits

// A first-level table entry says what the symbol means, so the serial decode
// (scalar-unit bound: one SALU pipe per CU serves all its waves) needs no
// per-symbol branching on the symbol value:
//   bits 0..3   code length (0: the code is longer than kFastBits, or unused)
//   bits 4..7   extra bits that follow the code (length / distance codes)
//   bits 8..9   kind: 0 literal (or plain symbol), 1 length / distance, 2 end
//               of block, 3 not a valid symbol here
//   bits 16..31 value: literal byte / symbol, length base, distance base
enum { kKindLit = 0, kKindCopy = 1, kKindEnd = 2, kKindBad = 3 };
enum { kAlphaLit = 0, kAlphaDist = 1, kAlphaPlain = 2 };
template <int FB, int NS>
struct InfCodeT {                          // one canonical Huffman code
    static constexpr int kFB = FB, kSize = 1 << FB;
    uint32_t fast[kSize];                  // entries as above (code length in bits 0..3)
    uint16_t cnt[16];                      // codes per length
    uint16_t sorted[NS];                   // symbols ordered by (length, symbol)
};
// literal / length (and code-length) codes: 9-bit first level, 288 symbols;
// distance codes: 8-bit first level, 30 symbols -- 1.5 KiB less LDS per
// member (more members resident per CU for the scalar-bound decode; a
// distance code longer than 8 bits takes the canonical walk)
using InfCode = InfCodeT<kFastBits, 288>;
using InfDistCode = InfCodeT<8, 32>;
// (length, distance) pair table: the next kPairBits bits of the stream ->
// one whole copy when its length code, length extra bits, distance code and
// distance extra bits all fit in them: bits 0..4 bits consumed, 5..13
// length, 14..29 distance, bit 30 valid.  The device gzip's rank streams are
// mostly 4-byte copies (a token's previous occurrence) with short distance
// codes, so most copies decode with one table read instead of two decodes
// and two extra-bit reads on the scalar unit.
constexpr int kPairBits = 10;
constexpr int kPair = 1 << kPairBits;
template <int WIN, bool PAIR>
struct InfSmem {
    alignas(16) uint8_t win[WIN];          // the member's output
    alignas(4) uint8_t ring[kRing];
    InfCode lit;
    InfDistCode dist;
    uint8_t lens[320];                     // code lengths (literal/length | distance)
    uint32_t pair[PAIR ? kPair : 1];
};

struct InfArgs {
    const uint8_t* src;                    // device copy of the stream
    const int64_t* idx;                    // per member: an index record (gz_format.h)
    int64_t nmem;
    uint8_t* out;
    uint64_t out_cap;
    int* status;                           // OR of kInf* flags over the members
};

// base value and extra-bit count of a length code c (0..28) / a distance code
// c (0..29), RFC 1951 3.2.5, in closed form
DEVI uint32_t len_base(int c, int& ext) {
    if (c < 8) { ext = 0; return 3u + (uint32_t)c; }
    if (c == 28) { ext = 0; return 258u; }
    ext = (c >> 2) - 1;
    return ((4u + (uint32_t)(c & 3)) << ext) + 3u;
}
DEVI uint32_t dist_base(int c, int& ext) {
    if (c < 4) { ext = 0; return 1u + (uint32_t)c; }
    ext = (c >> 1) - 1;
    return ((2u + (uint32_t)(c & 1)) << ext) + 1u;
}
// the table entry of symbol s of an alphabet (code length not included)
DEVI uint32_t inf_entry(int s, int alpha) {
    int ext = 0;
    if (alpha == kAlphaPlain) return (uint32_t)s << 16;
    if (alpha == kAlphaDist) {
        if (s > 29) return (uint32_t)kKindBad << 8;
        const uint32_t b = dist_base(s, ext);
        return (b << 16) | ((uint32_t)kKindCopy << 8) | ((uint32_t)ext << 4);
    }
    if (s < 256) return (uint32_t)s << 16;
    if (s == 256) return (uint32_t)kKindEnd << 8;
    if (s > 285) return (uint32_t)kKindBad << 8;
    const uint32_t b = len_base(s - 257, ext);
    return (b << 16) | ((uint32_t)kKindCopy << 8) | ((uint32_t)ext << 4);
}

// canonical code from lengths (wave-parallel): counts and ranks by ballots,
// the fast table filled by the symbols' lanes.  false: over-subscribed, or
// (check != kSetAny) incomplete by zlib's rule (inflate_table): unused code
// space is an error unless no symbol has a code at all, or, for the literal
// and distance sets only (kSetLone), the longest code is 1 bit.  The
// code-length alphabet is never exempt (kSetFull).  The fixed codes leave
// distance codes 30 and 31 out of their 5-bit space by definition (kSetAny).
enum { kSetAny = 0, kSetLone = 1, kSetFull = 2 };
template <typename C>
DEVI bool inf_build(C& c, const uint8_t* lens, int n, int alpha, int check) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t below = (1ull << lane) - 1ull;
    for (int k = lane; k < C::kSize; k += 64) c.fast[k] = 0;
    uint32_t cnt[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) cnt[b] = 0;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const int L = s < n ? lens[s] : 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) cnt[b] += (uint32_t)__popcll(__ballot(L == b));
    }
    int left = 1;
#pragma unroll
    for (int b = 1; b < 16; ++b) { left = (left << 1) - (int)cnt[b]; if (left < 0) return false; }
    if (left > 0 && check != kSetAny) {  // wave-uniform: one test per table build
        uint32_t longer = 0;             // codes of 2 bits or more
#pragma unroll
        for (int b = 2; b < 16; ++b) longer += cnt[b];
        if (longer || (cnt[1] && check == kSetFull)) return false;
    }
    if (lane < 16) c.cnt[lane] = (uint16_t)(lane ? cnt[lane] : 0u);
    uint32_t off[16], next[16];
    uint32_t o = 0, code = 0;
#pragma unroll
    for (int b = 1; b < 16; ++b) {
        off[b] = o;
        o += cnt[b];
        code = (code + (b > 1 ? cnt[b - 1] : 0u)) << 1;
        next[b] = code;
    }
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const int L = s < n ? lens[s] : 0;
        uint32_t my_off = 0, my_code = 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) {
            const uint64_t mk = __ballot(L == b);
            if (L == b) {
                const uint32_t r = (uint32_t)__popcll(mk & below);
                my_off = off[b] + r;
                my_code = next[b] + r;
            }
            off[b] += (uint32_t)__popcll(mk);
            next[b] += (uint32_t)__popcll(mk);
        }
        if (L) {
            c.sorted[my_off] = (uint16_t)s;
            if (L <= C::kFB) {
                const uint32_t e = inf_entry(s, alpha) | (uint32_t)L;
                for (uint32_t k = rev_bits(my_code, L); k < (uint32_t)C::kSize; k += 1u << L) c.fast[k] = e;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// the pair table of a block's codes (wave-parallel, after both builds)
template <int WIN, bool PAIR>
DEVI void inf_build_pairs(InfSmem<WIN, PAIR>& S) {
    if constexpr (PAIR) {
        const int lane = (int)(threadIdx.x & 63u);
        for (int k = lane; k < kPair; k += 64) {
            uint32_t out = 0;
            const uint32_t e = S.lit.fast[k & (InfCode::kSize - 1)];
            const uint32_t l = e & 15u, x = (e >> 4) & 15u;
            if (l && ((e >> 8) & 3u) == (uint32_t)kKindCopy && l + x <= (uint32_t)kPairBits) {
                const uint32_t len = (e >> 16) + (((uint32_t)k >> l) & ((1u << x) - 1u));
                const uint32_t r = (uint32_t)k >> (l + x);
                const uint32_t f = S.dist.fast[r & (InfDistCode::kSize - 1)];
                const uint32_t l2 = f & 15u, x2 = (f >> 4) & 15u;
                const uint32_t nb = l + x + l2 + x2;
                if (l2 && ((f >> 8) & 3u) == (uint32_t)kKindCopy && nb <= (uint32_t)kPairBits) {
                    const uint32_t d = (f >> 16) + ((r >> l2) & ((1u << x2) - 1u));
                    out = nb | (len << 5) | (d << 14) | (1u << 30);
                }
            }
            S.pair[k] = out;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// wave-uniform value from LDS into a scalar register: the decode state then
// lives in SGPRs and its arithmetic runs on the scalar unit (one wave-wide
// VALU op per step of the serial decode would cost 4+ cycles each)
DEVI uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// codes longer than the first-level table: canonical walk, most significant
// bit first (rare: the slow path of inf_decode)
template <typename C>
DEVI uint32_t inf_decode_long(const C& c, uint64_t& bb, int& bc, int alpha) {
    int code = 0, first = 0, index = 0;
#pragma unroll 1
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bb & 1u);
        bb >>= 1;
        --bc;
        const int n = (int)uni(c.cnt[len]);
        if (code - first < n) return inf_entry((int)uni(c.sorted[index + code - first]), alpha);
        index += n;
        first = (first + n) << 1;
        code <<= 1;
    }
    return (uint32_t)kKindBad << 8;
}

// one symbol's table entry (needs >= 15 bits in bb), its code consumed;
// kKindBad if the bits are no code
template <typename C>
DEVI uint32_t inf_decode(const C& c, uint64_t& bb, int& bc, int alpha) {
    const uint32_t e = uni(c.fast[bb & (uint64_t)(C::kSize - 1)]);
    const int l = (int)(e & 15u);
    if (l) {
        bb >>= l;
        bc -= l;
        return e;
    }
    return inf_decode_long(c, bb, bc, alpha);
}

// RING = false: the member's whole output stays in the WIN-byte LDS window
// until it is complete, then one coalesced store.  RING = true: the LDS holds
// only the last WIN output bytes (a ring) and every byte also goes to global
// memory as it is produced; a copy reaching further back than the ring reads
// global memory (bytes this wavefront stored earlier: same-address order
// within a wavefront).  Less LDS per member -> more members per CU.
template <int WIN, bool RING, bool PAIR>
__global__ __launch_bounds__(64, OFL_INF_WAVES) void k_inflate_members(InfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    InfSmem<WIN, PAIR>& S = *reinterpret_cast<InfSmem<WIN, PAIR>*>(smem_raw);
    const int lane = threadIdx.x;
    const int64_t m = blockIdx.x;
    if (m >= a.nmem) return;
    const int64_t* ix = a.idx + kIdxWords * m;
    const uint8_t* src = a.src + ix[kIdxIn];
    const uint32_t in_len = GZ_IDX_IN_LEN(ix[kIdxLen]);
    const int64_t out_off = ix[kIdxOut];
    const uint32_t isize = GZ_IDX_ISIZE(ix[kIdxSize]), want_crc = GZ_IDX_CRC(ix[kIdxSize]);
    if ((!RING && isize > (uint32_t)WIN) || out_off < 0 || (uint64_t)out_off + isize > a.out_cap) {
        if (lane == 0) atomicOr(a.status, kInfRange);
        return;
    }
    uint8_t* const dst = a.out + out_off;
    constexpr uint32_t M = RING ? (uint32_t)WIN - 1u : 0xffffffffu;  // window index mask
    // bit reader: bb holds bc bits; pos = next ring byte; the ring holds [fill - kRing, fill)
    uint64_t bb = 0;
    int bc = 0;
    uint32_t pos = 0, fill = 0;
    auto refill = [&]() {  // the next kRing / 2 bytes (zeros past the end)
        for (int k = lane; k < kRing / 2; k += 64) {
            const uint32_t g = fill + (uint32_t)k;
            S.ring[g & (kRing - 1)] = g < in_len ? src[g] : 0;
        }
        fill += kRing / 2;
        __builtin_amdgcn_wave_barrier();
    };
    auto topup = [&]() {  // >= 33 bits in bb
        while (bc <= 32) {
            if (pos + 8u > fill) refill();
            const uint32_t* w = reinterpret_cast<const uint32_t*>(S.ring);
            const uint32_t q = (pos & (kRing - 1)) >> 2;
            const uint32_t v = uni(__builtin_amdgcn_alignbyte(w[(q + 1) & (kRing / 4 - 1)], w[q], pos & 3u));
            bb |= (uint64_t)v << bc;
            bc += 32;
            pos += 4;
        }
    };
    auto bits = [&](int n) -> uint32_t {  // n <= 32, bb holds >= n bits
        const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1ull));
        bb >>= n;
        bc -= n;
        return v;
    };
    int err = 0;
    uint32_t p = 0;  // output bytes so far
    bool last = false;
    while (!last && !err) {
        if (pos > in_len + 16u) { err = kInfCorrupt; break; }  // past the data (zeros)
        topup();
        last = bits(1) != 0;
        const int type = (int)bits(2);
        if (type == 0) {  // stored: byte-align, LEN, NLEN, raw bytes
            bits(bc & 7);
            topup();
            const uint32_t len = bits(16), nlen = bits(16);
            if ((len ^ 0xffffu) != nlen || p + len > isize) { err = kInfCorrupt; break; }
            pos -= (uint32_t)(bc >> 3);  // hand the buffered whole bytes back to the ring
            bb = 0;
            bc = 0;
            uint32_t left = len;
            while (left) {
                if (pos + 64u > fill) refill();
                const uint32_t ch = min(left, 64u);
                if ((uint32_t)lane < ch) {
                    const uint8_t v = S.ring[(pos + lane) & (kRing - 1)];
                    S.win[(p + lane) & M] = v;
                    if (RING) dst[p + lane] = v;
                }
                __builtin_amdgcn_wave_barrier();
                p += ch;
                pos += ch;
                left -= ch;
            }
            continue;
        }
        if (type == 3) { err = kInfCorrupt; break; }
        if (type == 1) {  // fixed codes (RFC 1951 3.2.6)
            for (int i = lane; i < 320; i += 64)
                S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
            __builtin_amdgcn_wave_barrier();
            inf_build(S.lit, S.lens, 288, kAlphaLit, kSetAny);
            inf_build(S.dist, S.lens + 288, 30, kAlphaDist, kSetAny);
            inf_build_pairs(S);
        } else {  // dynamic: code-length code, then the literal/length and distance lengths
            topup();
            const int nlit = (int)bits(5) + 257, ndist = (int)bits(5) + 1, ncl = (int)bits(4) + 4;
            if (nlit > 286 || ndist > 30) { err = kInfCorrupt; break; }
            for (int i = lane; i < 19; i += 64) S.lens[i] = 0;
            __builtin_amdgcn_wave_barrier();
            for (int i = 0; i < ncl; ++i) {
                topup();
                const uint32_t v = bits(3);
                if (lane == 0) S.lens[c_clord[i]] = (uint8_t)v;
            }
            __builtin_amdgcn_wave_barrier();
            if (!inf_build(S.lit, S.lens, 19, kAlphaPlain, kSetFull)) { err = kInfCorrupt; break; }
            const int total = nlit + ndist;
            int i = 0;
            while (i < total) {
                topup();
                const uint32_t ce = inf_decode(S.lit, bb, bc, kAlphaPlain);
                if (ce & 0x300u) { err = kInfCorrupt; break; }
                const int sy = (int)(ce >> 16);
                if (sy < 16) {
                    if (lane == 0) S.lens[i] = (uint8_t)sy;
                    ++i;
                    continue;
                }
                int rep, val = 0;
                if (sy == 16) {
                    if (i == 0) { err = kInfCorrupt; break; }
                    val = (int)uni(S.lens[i - 1]);
                    rep = 3 + (int)bits(2);
                } else if (sy == 17) {
                    rep = 3 + (int)bits(3);
                } else {
                    rep = 11 + (int)bits(7);
                }
                if (i + rep > total) { err = kInfCorrupt; break; }
                __builtin_amdgcn_wave_barrier();
                for (int k = lane; k < rep; k += 64) S.lens[i + k] = (uint8_t)val;
                __builtin_amdgcn_wave_barrier();
                i += rep;
            }
            if (err) break;
            __builtin_amdgcn_wave_barrier();
            if (uni(S.lens[256]) == 0) { err = kInfCorrupt; break; }
            // the distance lengths move out of the literal range before the builds
            const uint8_t dl = lane < ndist ? S.lens[nlit + lane] : 0;
            __builtin_amdgcn_wave_barrier();
            for (int k = nlit + lane; k < 288; k += 64) S.lens[k] = 0;
            __builtin_amdgcn_wave_barrier();
            if (lane < 32) S.lens[288 + lane] = lane < ndist ? dl : 0;
            __builtin_amdgcn_wave_barrier();
            if (!inf_build(S.lit, S.lens, nlit, kAlphaLit, kSetLone) || !inf_build(S.dist, S.lens + 288, ndist, kAlphaDist, kSetLone)) {
                err = kInfCorrupt;
                break;
            }
            inf_build_pairs(S);
        }
        // symbols of the block
        for (;;) {
            topup();
            if constexpr (PAIR) {
                const uint32_t pe = uni(S.pair[bb & (uint64_t)(kPair - 1)]);
                if (pe >> 30) {  // a whole copy from one lookup
                    const uint32_t nb = pe & 31u, len = (pe >> 5) & 511u, d = (pe >> 14) & 0xffffu;
                    bb >>= nb;
                    bc -= (int)nb;
                    if (d > p) { err = kInfCorrupt; break; }
                    if (p + len > isize) { err = kInfSize; break; }
                    __builtin_amdgcn_wave_barrier();
                    if ((!RING || d + len <= (uint32_t)WIN) && len <= 64u) {
                        if ((uint32_t)lane < len) {
                            const uint32_t k = (uint32_t)lane;
                            const uint8_t v = S.win[(p - d + (d >= len ? k : k % d)) & M];
                            S.win[(p + k) & M] = v;
                            if (RING) dst[p + k] = v;
                        }
                    } else if (!RING || d + len <= (uint32_t)WIN) {
                        for (uint32_t k = lane; k < len; k += 64) {
                            const uint8_t v = S.win[(p - d + (d >= len ? k : k % d)) & M];
                            S.win[(p + k) & M] = v;
                            if (RING) dst[p + k] = v;
                        }
                    } else {
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        for (uint32_t k = lane; k < len; k += 64) {
                            const uint8_t v = dst[p - d + k];
                            S.win[(p + k) & M] = v;
                            dst[p + k] = v;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    p += len;
                    continue;
                }
            }
            const uint32_t e = inf_decode(S.lit, bb, bc, kAlphaLit);
            const uint32_t kind = (e >> 8) & 3u;
            if (kind == kKindLit) {
                if (p >= isize) { err = kInfSize; break; }
                if (lane == 0) {
                    S.win[p & M] = (uint8_t)(e >> 16);
                    if (RING) dst[p] = (uint8_t)(e >> 16);
                }
                ++p;
            } else if (kind == kKindEnd) {
                break;
            } else {
                if (kind == kKindBad) { err = kInfCorrupt; break; }
                const uint32_t len = (e >> 16) + bits((int)((e >> 4) & 15u));
                topup();
                const uint32_t f = inf_decode(S.dist, bb, bc, kAlphaDist);
                if (((f >> 8) & 3u) != kKindCopy) { err = kInfCorrupt; break; }
                const uint32_t d = (f >> 16) + bits((int)((f >> 4) & 15u));
                if (d > p) { err = kInfCorrupt; break; }
                if (p + len > isize) { err = kInfSize; break; }
                __builtin_amdgcn_wave_barrier();
                if ((!RING || d + len <= (uint32_t)WIN) && len <= 64u) {  // one lane per byte, no loop
                    if ((uint32_t)lane < len) {
                        const uint32_t k = (uint32_t)lane;
                        const uint8_t v = S.win[(p - d + (d >= len ? k : k % d)) & M];
                        S.win[(p + k) & M] = v;
                        if (RING) dst[p + k] = v;
                    }
                } else if (!RING || d + len <= (uint32_t)WIN) {  // the source is in the window
                    if (d >= len) {
                        for (uint32_t k = lane; k < len; k += 64) {
                            const uint8_t v = S.win[(p - d + k) & M];
                            S.win[(p + k) & M] = v;
                            if (RING) dst[p + k] = v;
                        }
                    } else {
                        for (uint32_t k = lane; k < len; k += 64) {
                            const uint8_t v = S.win[(p - d + k % d) & M];
                            S.win[(p + k) & M] = v;
                            if (RING) dst[p + k] = v;
                        }
                    }
                } else {  // ring only: further back than the ring (d > WIN - len >= len)
                    // the source bytes are this wavefront's earlier global stores
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    for (uint32_t k = lane; k < len; k += 64) {
                        const uint8_t v = dst[p - d + k];
                        S.win[(p + k) & M] = v;
                        dst[p + k] = v;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                p += len;
            }
        }
    }
    // every byte of the deflate data used, none past it; the whole ISIZE produced
    if (!err && (pos - (uint32_t)(bc >> 3) != in_len)) err = kInfCorrupt;
    if (!err && p != isize) err = kInfSize;
    if (err) {
        if (lane == 0) atomicOr(a.status, err);
        return;
    }
    __builtin_amdgcn_wave_barrier();
    if (RING) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the CRC reads the stores back
    // CRC-32 of the output, checked here: lane l takes bytes [l sg, (l+1) sg)
    // of the output seen as the tail of 64 sg bytes (leading zeros leave a
    // zero-initialised CRC unchanged), bitwise (vector work beside the other
    // waves' scalar-bound decode), then a tree over the lanes whose level-l
    // shift (sg 2^l bytes) is the same for every lane.  The ring decoder
    // reads its own stores back (same-address order within a wavefront).
    {
        int lg = 0;
        while ((64ull << lg) < (uint64_t)isize) ++lg;
        const int64_t sg = 1ll << lg;
        const int64_t b0 = (int64_t)lane * sg - (int64_t)((64ull << lg) - isize);
        uint32_t r = 0;
        const bool vec = RING && sg >= 16 && ((reinterpret_cast<uintptr_t>(dst) | isize) & 15u) == 0;
        if (vec) {  // b0 is a multiple of 16 here
            for (int64_t i = b0 < 0 ? 0 : b0; i < b0 + sg; i += 64) {
                uint4 w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = i + 16 * k < b0 + sg ? reinterpret_cast<const uint4*>(dst + i)[k] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (i + 16 * k < b0 + sg) {
                        r = crc_word(r, w[k].x); r = crc_word(r, w[k].y);
                        r = crc_word(r, w[k].z); r = crc_word(r, w[k].w);
                    }
            }
        } else {
            for (int64_t i = b0 < 0 ? 0 : b0; i < b0 + sg; ++i) r = crc_byte(r, RING ? dst[i] : S.win[i]);
        }
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            const uint32_t x = (uint32_t)__shfl_xor((int)r, 1 << l, 64);
            const uint32_t sh = crc_adv_pow2(r, lg + l);
            r = (lane & (1 << l)) ? r : (sh ^ x);
        }
        if (lane == 0 && (crc_adv(0xffffffffu, isize) ^ r ^ 0xffffffffu) != want_crc) atomicOr(a.status, kInfCrc);
    }
    if (RING) return;  // already stored as produced
    __builtin_amdgcn_wave_barrier();
    if (((reinterpret_cast<uintptr_t>(dst) | isize) & 15u) == 0) {
        const uint4* w = reinterpret_cast<const uint4*>(S.win);
        for (uint32_t i = lane; i < isize / 16u; i += 64) reinterpret_cast<uint4*>(dst)[i] = w[i];
    } else {
        for (uint32_t i = lane; i < isize; i += 64) dst[i] = S.win[i];
    }
}

}  // namespace gz
