// gz_members.h -- the host-only part of the gzip codec (deflate_kernels.hip),
// free of HIP so that it can be built and checked alone
// (tests/gz_members_check.cpp): the parser of a member-indexed stream's
// headers -- untrusted bytes off the wire --, the CRC-32 advance matrices, and
// the layouts of the encoder's and the inflate's workspaces.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "gz_format.h"
#include "ofl_codec.h"

namespace gz {

// raw CRC-32 advance matrices for 2^k zero bytes
inline void crc_matrices(uint32_t (&m)[32][32]) {
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t r = i;
        for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1;
        tab[i] = r;
    }
    for (int i = 0; i < 32; ++i) { const uint32_t v = 1u << i; m[0][i] = tab[v & 0xffu] ^ (v >> 8); }
    auto apply = [](const uint32_t* M, uint32_t v) {
        uint32_t r = 0;
        for (int i = 0; i < 32; ++i) if ((v >> i) & 1u) r ^= M[i];
        return r;
    };
    for (int k = 1; k < 32; ++k)
        for (int i = 0; i < 32; ++i) m[k][i] = apply(m[k - 1], apply(m[k - 1], 1u << i));
}

// the members of a member-indexed stream (every header carries its size in
// an RFC 1952 extra subfield: 'BC' (BGZF: size - 1, 16 bits) or 'OZ' (TLZ:
// size, 32 bits, plus the segment table)): deflate data range, output
// offset, ISIZE, CRC-32 and whether it is a TLZ member
struct GzMember { size_t in, in_len, out; uint32_t isize, crc; bool tlz; };
// one member at pos: its size (0 if the bytes there are not a member header
// with a size field) and its record
inline size_t member_at(const uint8_t* src, size_t n, size_t pos, GzMember& m) {
    const uint8_t* h = src + pos;
    if (n - pos < (size_t)(kGzFixed + kSubFixed + kBcLen + kGzTrailer) || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 ||
        h[3] != 0x04)
        return 0;
    const size_t hdr = (size_t)kGzFixed + rd16(h + kGzXlen);  // the deflate data starts here
    if (hdr > n - pos) return 0;
    size_t bsize = 0;
    const uint8_t* oz = nullptr;  // the OZ subfield of a TLZ member
    for (size_t q = kGzFixed; q + kSubFixed <= hdr;) {
        const uint8_t* sub = h + q;
        const size_t sl = rd16(sub + kSubLen);
        if (q + kSubFixed + sl > hdr) return 0;
        if (sub[0] == 'B' && sub[1] == 'C' && sl == (size_t)kBcLen) bsize = (size_t)rd16(sub + kBcSize) + 1;
        if (sub[0] == 'O' && sub[1] == 'Z' && sl >= (size_t)tlz::kOzFixed) {
            const size_t nseg = rd16(sub + tlz::kOzNseg);
            bsize = rd32(sub + tlz::kOzBytes);
            // the segment table must end where the deflate data starts
            const bool is_tlz = sub[tlz::kOzVersion] == tlz::kVersion && sub[tlz::kOzSegLog] == tlz::kSegLog &&
                                sl == (size_t)tlz::kOzFixed + 4 * nseg && q + kSubFixed + sl == hdr && nseg >= 1 &&
                                nseg <= (size_t)tlz::kMemSeg;
            oz = is_tlz ? sub : nullptr;
        }
        q += kSubFixed + sl;
    }
    if (bsize < hdr + kGzTrailer || bsize > n - pos) return 0;
    const uint8_t* t = h + bsize - kGzTrailer;
    m.in = pos + hdr;
    m.in_len = bsize - hdr - kGzTrailer;
    m.crc = rd32(t);
    m.isize = rd32(t + 4);
    // a TLZ member's value count (the OZ field) must match its ISIZE
    m.tlz = false;
    if (oz) {
        const size_t ntok = rd32(oz + tlz::kOzValues), nseg = rd16(oz + tlz::kOzNseg);
        m.tlz = (m.isize & 3u) == 0 && ntok == m.isize / 4 && nseg == (ntok + tlz::kSeg - 1) / tlz::kSeg;
    }
    return bsize;
}

// walk the member chain over [pos, end); false if a header is not one.
// out offsets are relative to the walk's start
inline bool walk_members(const uint8_t* src, size_t n, size_t pos, size_t end, std::vector<GzMember>& mem,
                         size_t& reached) {
    size_t out = 0;
    while (pos < end) {
        GzMember m;
        const size_t bs = member_at(src, n, pos, m);
        if (!bs) return false;
        m.out = out;
        out += m.isize;
        mem.push_back(m);
        pos += bs;
    }
    reached = pos;
    return true;
}

// The chain is a dependent walk (each header gives the next one's offset), so
// one thread pays a cache miss per member.  Streams of two pieces of
// min_piece bytes or more are cut in up to max_threads pieces; each thread
// finds the first header at or after its piece's start (the member signature)
// and walks to the end of its piece; the pieces are then checked to link
// exactly (thread k's walk ends where thread k+1's starts), so a signature
// found inside compressed data, or a piece without a header, can only send
// the parse back to the serial walk, never give a wrong index.
// -> OFL_OK, or OFL_EFORMAT with *msg set
inline int parse_members(const uint8_t* src, size_t n, unsigned max_threads, size_t min_piece, std::vector<GzMember>& mem,
                         size_t& total, const char** msg) {
    mem.clear();
    total = 0;
    const int nt = (int)std::min<size_t>(max_threads, n / std::max<size_t>(min_piece, 1));
    bool par_ok = nt > 1;
    if (par_ok) {
        std::vector<std::vector<GzMember>> part(nt);
        std::vector<size_t> start(nt + 1, n), reached(nt, 0);
        std::vector<char> ok(nt, 0);
        auto work = [&](int t) {
            size_t p = n * t / nt;
            const size_t lim = n * (t + 1) / nt;
            if (t > 0) {  // the first member signature at or after p
                GzMember m;
                while (p < lim) {
                    const uint8_t* h = src + p;
                    if (h[0] == 0x1f && p + kGzFixed + kSubFixed <= n && h[1] == 0x8b && h[2] == 8 && h[3] == 4 &&
                        ((h[kGzFixed] == 'B' && h[kGzFixed + 1] == 'C') || (h[kGzFixed] == 'O' && h[kGzFixed + 1] == 'Z')) &&
                        member_at(src, n, p, m))
                        break;
                    ++p;
                }
            }
            start[t] = p;
            ok[t] = p < lim && walk_members(src, n, p, lim, part[t], reached[t]);
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
        // piece t's walk (from a true header, by induction from 0) ends on a
        // true header, which must be where piece t + 1 starts
        par_ok = start[0] == 0;
        for (int t = 0; t < nt && par_ok; ++t)
            par_ok = ok[t] && !part[t].empty() && reached[t] == (t + 1 < nt ? start[t + 1] : n);
        if (par_ok) {
            size_t cnt = 0;
            for (auto& p : part) cnt += p.size();
            mem.reserve(cnt);
            for (auto& p : part) mem.insert(mem.end(), p.begin(), p.end());
            for (GzMember& m : mem) { m.out = total; total += m.isize; }  // absolute output offsets
            return OFL_OK;
        }
        mem.clear();
        total = 0;
    }
    size_t reached0 = 0;
    if (!walk_members(src, n, 0, n, mem, reached0)) {
        mem.clear();
        *msg = "gunzip: not a member-indexed gzip stream";
        return OFL_EFORMAT;
    }
    for (const GzMember& m : mem) total += m.isize;
    return OFL_OK;
}

// ---- the encoder's sizes ----------------------------------------------------
struct TlzLayout {
    int64_t members, batch;
    size_t slot, ops_stride;
    size_t stage;  // a batch's device staging for the D2H: 1 byte per value
};
inline TlzLayout tlz_layout(int64_t n) {
    using namespace tlz;
    TlzLayout L;
    L.members = std::max<int64_t>(1, (n + kMemTok - 1) / kMemTok);
    L.batch = std::min<int64_t>(L.members, kBatch);
    const int64_t per = std::min<int64_t>(std::max<int64_t>(n, 1), kMemTok);
    L.slot = ((size_t)per * kSlotPerTok + kSlotPad + 255) & ~(size_t)255;
    L.ops_stride = ((size_t)per + 63) & ~(size_t)63;
    L.stage = ((size_t)L.batch * (size_t)per + 255) & ~(size_t)255;
    return L;
}

// the largest stream n values can give (ofl_gzip_ranks_bound)
inline size_t gzip_ranks_bound(int64_t n) {
    const TlzLayout L = tlz_layout(n);
    return (size_t)L.members * L.slot;
}

// The ofl_gzip_ranks workspace of n values at address base: every region's
// byte offset from base, each aligned (as an address) for its use.  end, the
// size to allocate, does not depend on base: it is the regions counted below
// plus kWsSmall, which holds the two words and whatever the align-ups skip
// (at most 255 + 4 + 255 bytes) for a base of any alignment.
constexpr size_t kWsSmall = 1024;
struct GzRanksWs {
    TlzLayout L;
    size_t slots[2];   // [batch][slot] member slots, double-buffered (the second: the pageable path's staging)
    size_t ops;        // [batch][ops_stride] uint32
    size_t sizes[2];   // [batch] uint32
    size_t off[2];     // [batch + 1] uint64
    size_t running;    // uint64
    size_t bad;        // int
    size_t stage[2];   // [stage] a batch's D2H staging
    size_t end;
};
inline GzRanksWs gzip_ranks_ws(int64_t n, uintptr_t base) {
    GzRanksWs W;
    W.L = tlz_layout(n);
    const size_t B = (size_t)W.L.batch;
    size_t at = 0, counted = 0;
    auto take = [&](size_t bytes, size_t align, bool count) {
        at += (align - (base + at) % align) % align;
        const size_t o = at;
        at += bytes;
        if (count) counted += bytes;
        return o;
    };
    for (size_t& s : W.slots) s = take(B * W.L.slot, 256, true);
    W.ops = take(4 * B * W.L.ops_stride, 4, true);
    for (size_t& s : W.sizes) s = take(4 * B, 4, true);
    for (size_t& s : W.off) s = take(8 * (B + 1), 8, true);
    W.running = take(8, 8, false);
    W.bad = take(4, 4, false);
    for (size_t& s : W.stage) s = take(W.L.stage, 256, true);
    W.end = counted + kWsSmall;
    return W;
}

// the inflate workspace: the status word, then the TLZ decoder's op counts
// ([nmembers][kMemSeg] uint32); the generic inflate needs the status alone
struct InflateWs { size_t status, counts, end; };
inline InflateWs inflate_ws(int64_t nmembers) {
    return {0, 256, 256 + 4 * (size_t)std::max<int64_t>(nmembers, 1) * tlz::kMemSeg};
}

}  // namespace gz
