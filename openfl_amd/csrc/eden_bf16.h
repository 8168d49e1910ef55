// eden_bf16.h -- encode from and decode into bfloat16 arenas
// (ofl_eden_encode_bf16, ofl_eden_decode_add_bf16).  The slices above 2^15
// elements read x and write y as bf16 in the row passes themselves:
//   k_enc_rowA_bf16, k_enc_rowA2_bf16   k_enc_rowA and k_enc_rowA2<false> with
//                                       another prologue (fetch_x / fix_x)
//   k_dec_rowC_bf16, k_dec_rowC2_bf16   k_dec_rowC and k_dec_rowC2 with another
//                                       epilogue (store_y / store_y_l)
// and everything between the prologue and the epilogue is those kernels' code
// on the same float32 values: widening bf16 is exact, so the planes and scales
// are those of the float32 path on the widened arena, and y is the float32
// path's y rounded once,
//     y16 = bf16_rne(base16 ? add_rn(widen(base16[i]), v) : v).
// Included by eden_kernels.hip after eden_dec_acc.h (the order of the kernels
// before it in the code object stays), inside namespace ofl.
//
// Data movement.  A thread holds 16 quads of 4 consecutive elements (element
// bits 0, 1 in register bits 0, 1 of the first and last layouts), so a quad of
// a bf16 arena is one 8-byte access of two registers: u << 16 and
// u & 0xffff0000 widen a register's two elements, bf16_rne and a v_perm-able
// shift / or narrow two results into one.  All arena accesses are nt (the
// rule of kIoLdAux / kIoStAux) through buffer views clamped to the tile's
// whole quads below the slice's length; the <= 3 elements of the quad that
// straddles it go one by one, block-uniform.  Nothing at or past the length
// is read (encode) or read or written (decode).
//   encode: 16 loads of 8 bytes per thread and tile.  The persistent kernel
//     keeps the next tile in flight packed -- 32 registers where k_enc_rowA
//     holds 64 -- and widens at the top of the loop.
//   decode: with a base, its 16 loads of 8 bytes (32 registers beside the 64
//     values) are all issued before the first store, so waiting for a quad's
//     base never waits for a store (loads and stores share one in-order
//     counter on gfx950); then 16 stores of 8 bytes.
//
// Slices of at most 2^15 elements keep their kernels on a float32 side arena
// that holds their elements alone (eden_bf16_plan.h): k_widen_ranges fills
// it from their input ranges before the encode, k_narrow_ranges rounds it
// (and adds the base) into their output ranges after the decode.
#pragma once

__device__ void raw_store_i32x2(i32x2 v, rsrc_t r, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.store.v2i32");

// bf16_rne, bf16_lo, bf16_hi, bf16_pack: ofl_util.h (shared with agg_kernels.hip)
DEVI float bf16_out(const uint16_t* b, int64_t i, float v) {  // element i of y before its rounding
    return b ? add_rn(bf16_lo(b[i]), v) : v;
}

// x tile in layout L, packed: one 8-byte load per register quad; live = false
// reads nothing
template <Lay L>
DEVI void fetch_x16(const KArgs& a, const SliceDesc& D, uint32_t tile, bool live, uint32_t base, i32x2 (&w)[16]) {
    static_assert(LT<L>::rb(0) == 0 && LT<L>::rb(1) == 1, "8-byte loads need element bits 0, 1 in registers 0, 1");
    const uint32_t e0 = tile << kRowLog;
    const uint32_t nv = live ? tile_valid(D.len - (int64_t)e0) : 0u;
    const rsrc_t r = mk_rsrc(a.x16 + D.x_off + e0, (nv & ~3u) * 2u);
#pragma unroll
    for (int g = 0; g < 16; ++g) w[g] = raw_load_i32x2(r, (int)(base * 2u), (int)(LT<L>::off(4 * g) * 2u), kIoLdAux);
}
DEVI void widen_x16(const i32x2 (&w)[16], float (&v)[64]) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        v[4 * g] = bf16_lo((uint32_t)w[g].x); v[4 * g + 1] = bf16_hi((uint32_t)w[g].x);
        v[4 * g + 2] = bf16_lo((uint32_t)w[g].y); v[4 * g + 3] = bf16_hi((uint32_t)w[g].y);
    }
}
// the valid head of the quad that straddles the slice's input length (as
// fix_x: block-uniform loads of the <= 3 values, taken by selects)
template <Lay L>
DEVI void fix_x16(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, float (&v)[64]) {
    const uint32_t e0 = tile << kRowLog;
    const uint32_t nv = tile_valid(D.len - (int64_t)e0);
    const uint32_t rem = nv & 3u;
    if (rem) {
        const uint32_t eb = nv & ~3u;
        const uint16_t* x = a.x16 + D.x_off + e0 + eb;
        const float x0 = bf16_lo(x[0]), x1 = rem > 1u ? bf16_lo(x[1]) : 0.0f, x2 = rem > 2u ? bf16_lo(x[2]) : 0.0f;
#pragma unroll
        for (int k = 0; k < 64; k += 4) {
            const bool hit = base + LT<L>::off(k) == eb;
            v[k] = hit ? x0 : v[k];
            v[k + 1] = hit ? x1 : v[k + 1];
            v[k + 2] = hit ? x2 : v[k + 2];
        }
    }
}

// The bf16 epilogue of a tile in layout L (in store_y_l's place): the whole
// quads below ylen through buffer views clamped to them -- the base's loads
// first, then the stores -- and the <= 3 elements of the quad that straddles
// ylen one by one.
template <Lay L>
DEVI void store_y16(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
    static_assert(LT<L>::rb(0) == 0 && LT<L>::rb(1) == 1, "8-byte stores need element bits 0, 1 in registers 0, 1");
    const uint32_t e0 = tile << kRowLog;
    const uint32_t nv = tile_valid(D.ylen - (int64_t)e0);
    const rsrc_t r = mk_rsrc(a.y16 + D.y_off + e0, (nv & ~3u) * 2u);
    if (a.base16) {
        const rsrc_t rb = mk_rsrc(a.base16 + D.y_off + e0, (nv & ~3u) * 2u);
        i32x2 b[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) b[g] = raw_load_i32x2(rb, (int)(base * 2u), (int)(LT<L>::off(4 * g) * 2u), kIoLdAux);
        asm volatile("" ::: "memory");  // the loads above stay above the stores below
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const uint32_t b0 = (uint32_t)b[g].x, b1 = (uint32_t)b[g].y;
            const i32x2 q = {(int)bf16_pack(add_rn(bf16_lo(b0), v[4 * g]), add_rn(bf16_hi(b0), v[4 * g + 1])),
                             (int)bf16_pack(add_rn(bf16_lo(b1), v[4 * g + 2]), add_rn(bf16_hi(b1), v[4 * g + 3]))};
            raw_store_i32x2(q, r, (int)(base * 2u), (int)(LT<L>::off(4 * g) * 2u), kIoStAux);
        }
    } else {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const i32x2 q = {(int)bf16_pack(v[4 * g], v[4 * g + 1]), (int)bf16_pack(v[4 * g + 2], v[4 * g + 3])};
            raw_store_i32x2(q, r, (int)(base * 2u), (int)(LT<L>::off(4 * g) * 2u), kIoStAux);
        }
    }
    if (nv & 3u) {
        const uint32_t eb = nv & ~3u;
        const int64_t i0 = D.y_off + e0 + eb;
#pragma unroll
        for (int k = 0; k < 64; k += 4)
            if (base + LT<L>::off(k) == eb) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if ((uint32_t)q < (nv & 3u))
                        a.y16[i0 + q] = (uint16_t)bf16_rne(__float_as_uint(bf16_out(a.base16, i0 + q, v[k + q])));
            }
    }
}

// encode pass A from a bf16 arena, persistent and prefetching (as k_enc_rowA)
__global__ __launch_bounds__(kRowNT) void k_enc_rowA_bf16(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s = reinterpret_cast<float*>(smem);
    float* red = reinterpret_cast<float*>(smem + kRowRed);
    const uint32_t tid = threadIdx.x;
    const TileWalk tw(a, reinterpret_cast<TileTab*>(smem + kRowTab), tid);
    int t = (int)blockIdx.x;
    if (t >= tw.total) return;
    const uint32_t base1 = LT<RS::L1>::base(tid), base3 = LT<RS::L3F>::base(tid);
    int si; uint32_t tile;
    tw.at(t, si, tile);
    i32x2 nx[16];
    fetch_x16<RS::L1>(a, udesc(a.d, si), tile, true, base1, nx);
    for (;;) {
        float v[64];
        widen_x16(nx, v);
        const SliceDesc D = udesc(a.d, si);
        const int tn = t + (int)gridDim.x;
        const bool more = tn < tw.total;
        int sn; uint32_t tln;
        tw.at(more ? tn : t, sn, tln);
        fetch_x16<RS::L1>(a, udesc(a.d, sn), tln, more, base1, nx);
        fix_x16<RS::L1>(a, D, tile, base1, v);
        const uint32_t b1 = seed_b(sld(a.seeds, D.tensor));
        float ss = sum_sq(v);
        apply_signs_direct<RS::L1>(v, tile << kRowLog, base1, D.logp, b1, 1.0f);
        stages<RS::L1, RS::F1a>(v);
        exchange<RS::L1, RS::L2>(v, s, tid);
        stages<RS::L2, RS::F1b>(v);
        exchange<RS::L2, RS::L3F>(v, s, tid);
        stages<RS::L3F, RS::F1c>(v);
        store_ws4<RS::L3F>(a, D, tile, base3, v);
        ss = block_sum<kRowNT>(ss, red);
        if (tid == 0) a.part[D.part_off + tile] = ss;
        if (!more) break;
        t = tn; si = sn; tile = tln;
    }
}

// encode pass A from a bf16 arena, two blocks per CU (as k_enc_rowA2<false>:
// the tile table, a paired table or a split 5-pass slice's explicit tile list)
__global__ __launch_bounds__(kRowNT, 4) void k_enc_rowA2_bf16(KArgs a) {
    using R = RowA2Set;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s = reinterpret_cast<float*>(smem);
    float* red = reinterpret_cast<float*>(smem + kRowC2Ex);
    uint32_t* stash = reinterpret_cast<uint32_t*>(smem + kRow2Stash);
    const int total = a.npair ? a.npair : (int)sld(a.tstart, a.count);
    for (int t = (int)blockIdx.x; t < total; t += (int)gridDim.x) {
      for (uint32_t h = 0;; ++h) {  // as in k_enc_rowA2
        int si; uint32_t tile0, pair;
        row_locate(a, t, si, tile0, &pair);
        const SliceDesc D = udesc(a.d, si);
        const uint32_t tid = opaque(threadIdx.x);  // as in k_enc_rowA2
        const uint32_t base1 = LT<R::A1>::base(tid), base3 = LT<R::A3>::base(tid);
        const uint32_t tile = h ? tile0 + (1u << (D.logp - 18)) : tile0;
        float v[64];
        {
            i32x2 w[16];
            fetch_x16<R::A1>(a, D, tile, true, base1, w);
            widen_x16(w, v);
        }
        fix_x16<R::A1>(a, D, tile, base1, v);
#pragma unroll
        for (int r = 0; r < 64; r += 8)
            asm volatile("" : "+v"(v[r]), "+v"(v[r + 1]), "+v"(v[r + 2]), "+v"(v[r + 3]), "+v"(v[r + 4]),
                         "+v"(v[r + 5]), "+v"(v[r + 6]), "+v"(v[r + 7]));
        const uint32_t b1 = seed_b(sld(a.seeds, D.tensor));
        float ss = sum_sq(v);
        asm volatile("" : "+v"(ss));  // as in k_enc_rowA2
        if (pair) apply_signs_pair<R::A1>(v, tile << kRowLog, base1, D.logp, b1, 1.0f, 1u + h, stash);
        else apply_signs_grouped<R::A1, true>(v, tile << kRowLog, base1, D.logp, b1, 1.0f);
        stages<R::A1, R::F1a>(v);
        exchange_half_lin<R::A1, R::A2, 14>(v, s, tid);
        stages<R::A2, R::F1b>(v);
        exchange_half_pad<R::A2, R::A3, 14>(v, s, tid);
        stages<R::A3, R::F1c>(v);
        store_ws_l<R::A3>(a, D, tile, base3, v);
        ss = block_sum<kRowNT>(ss, red);
        if (tid == 0) a.part[D.part_off + tile] = ss;
        if (h >= pair) break;
      }
    }
}

// decode pass C into a bf16 arena, persistent and prefetching (as k_dec_rowC)
__global__ __launch_bounds__(kRowNT) void k_dec_rowC_bf16(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s = reinterpret_cast<float*>(smem);
    const uint32_t tid = threadIdx.x;
    const TileWalk tw(a, reinterpret_cast<TileTab*>(smem + kRowTab), tid);
    int t = (int)blockIdx.x;
    if (t >= tw.total) return;
    const uint32_t base1 = LT<RS::L1>::base(tid), base3 = LT<RS::L3F>::base(tid);
    int si; uint32_t tile;
    tw.at(t, si, tile);
    float nx[64];
    fetch_ws4<RS::L3F>(a, udesc(a.d, si), tile, true, base3, nx);
    for (;;) {
        float v[64];
#pragma unroll
        for (int r = 0; r < 64; ++r) v[r] = nx[r];
        const SliceDesc D = udesc(a.d, si);
        const int tn = t + (int)gridDim.x;
        const bool more = tn < tw.total;
        int sn; uint32_t tln;
        tw.at(more ? tn : t, sn, tln);
        fetch_ws4<RS::L3F>(a, udesc(a.d, sn), tln, more, base3, nx);
        const uint32_t b1 = seed_b(sld(a.seeds, D.tensor));
        stages<RS::L3F, RS::F1c>(v);
        exchange<RS::L3F, RS::L2>(v, s, tid);
        stages<RS::L2, RS::F1b>(v);
        exchange<RS::L2, RS::L1>(v, s, tid);
        stages<RS::L1, RS::F1a>(v);
        const float mul = fold_scale(sldf(a.scales_in, D.scale_idx), (D.logp + 1) / 2, v);
        apply_signs_direct<RS::L1>(v, tile << kRowLog, base1, D.logp, b1, mul);
        store_y16<RS::L1>(a, D, tile, base1, v);
        if (!more) break;
        t = tn; si = sn; tile = tln;
    }
}

// decode pass C into a bf16 arena, two blocks per CU (as k_dec_rowC2)
__global__ __launch_bounds__(kRowNT, 4) void k_dec_rowC2_bf16(KArgs a) {
    using R = DecC2Set;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s = reinterpret_cast<float*>(smem);
    uint32_t* stash = reinterpret_cast<uint32_t*>(smem + kRow2Stash);
    const int total = a.npair ? a.npair : (int)sld(a.tstart, a.count);
    for (int t = (int)blockIdx.x; t < total; t += (int)gridDim.x) {
      for (uint32_t h = 0;; ++h) {  // as in k_enc_rowA2
        int si; uint32_t tile0, pair;
        row_locate(a, t, si, tile0, &pair);
        const SliceDesc D = udesc(a.d, si);
        const uint32_t tid = opaque(threadIdx.x);  // as in k_enc_rowA2
        const uint32_t base1 = LT<R::B1>::base(tid), base4 = LT<R::B4>::base(tid);
        const uint32_t tile = h ? tile0 + (1u << (D.logp - 18)) : tile0;
        float v[64];
        fetch_ws4<R::B1>(a, D, tile, true, base1, v, kDecC2LdAux);
        const uint32_t b1 = seed_b(sld(a.seeds, D.tensor));
        stages<R::B1, R::H1>(v);
        exchange_half_lin<R::B1, R::B2, 10>(v, s, tid);
        stages<R::B2, R::H2>(v);
        exchange_half_lin<R::B2, R::B3, 10>(v, s, tid);
        stages<R::B3, R::H3>(v);
        exchange_half_pad<R::B3, R::B4, 10>(v, s, tid);
        stages<R::B4, R::H4>(v);
        const float mul = fold_scale(sldf(a.scales_in, D.scale_idx), (D.logp + 1) / 2, v);
        if (pair) apply_signs_pair<R::B4>(v, tile << kRowLog, base4, D.logp, b1, mul, 1u + h, stash);
        else apply_signs_grouped<R::B4>(v, tile << kRowLog, base4, D.logp, b1, mul);
        store_y16<R::B4>(a, D, tile, base4, v);
        if (h >= pair) break;
      }
    }
}

// ---------------------------------------------------------------------------
// The small slices' side arena: listed element ranges [s, e) of an arena,
// walked in slots of 4 elements at arena indices that are multiples of 4
// (eden::small_ranges: s[nr] | e[nr] | dst[nr + 1] | cb[nr], dst the exclusive
// prefix of the ranges' slot counts).  The side arena holds the ranges' slots
// back to back: slot j is its elements 4j .. 4j + 3, so arena element i of
// range r is at cb[r] + (i - s[r]).  A slot that lies whole inside its range
// is one 8-byte access of the bf16 arena and one 16-byte access of the side
// arena while both are aligned for them (vec); a range's ragged first and
// last slot, and every slot otherwise, go element by element.
// ---------------------------------------------------------------------------
constexpr int kRangeNT = 256;
struct QRanges {
    const int64_t* tab;
    int nr;
    DEVI int64_t total() const { return tab[3 * (int64_t)nr]; }
    // slot j (side elements 4j ..) -> its range [s, e) and the slot's first arena element
    DEVI int64_t find(int64_t j, int64_t& s, int64_t& e) const {
        const int64_t* dst = tab + 2 * (int64_t)nr;
        int lo = 0, hi = nr - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (dst[mid] <= j) lo = mid; else hi = mid - 1;
        }
        s = tab[lo];
        e = tab[nr + lo];
        return ((s >> 2) + (j - dst[lo])) << 2;
    }
};
template <class Q, class E>
DEVI void range_slots(const QRanges& rg, int vec, Q quad, E elem) {
    const int64_t total = rg.total();
    for (int64_t j = (int64_t)blockIdx.x * kRangeNT + threadIdx.x; j < total; j += (int64_t)gridDim.x * kRangeNT) {
        int64_t s, e;
        const int64_t i = rg.find(j, s, e);
        if (vec && i >= s && i + 4 <= e) {
            quad(i, 4 * j);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q >= s && i + q < e) elem(i + q, 4 * j + q);
        }
    }
}

// x_small[c] = widen(x16[i]) on the ranges (c: element i's place in the side arena)
__global__ __launch_bounds__(kRangeNT) void k_widen_ranges(const uint16_t* x16, float* xs, QRanges rg, int vec) {
    range_slots(rg, vec,
        [&](int64_t i, int64_t c) {
            const uint2 w = *reinterpret_cast<const uint2*>(x16 + i);
            *reinterpret_cast<float4*>(xs + c) = make_float4(bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y));
        },
        [&](int64_t i, int64_t c) { xs[c] = bf16_lo(x16[i]); });
}

// y16[i] = bf16_rne(base16 ? add_rn(widen(base16[i]), y_small[c]) : y_small[c]) on the ranges
__global__ __launch_bounds__(kRangeNT) void k_narrow_ranges(const float* ys, const uint16_t* b16, uint16_t* y16, QRanges rg,
                                                           int vec) {
    range_slots(rg, vec,
        [&](int64_t i, int64_t c) {
            float4 f = *reinterpret_cast<const float4*>(ys + c);
            if (b16) {
                const uint2 b = *reinterpret_cast<const uint2*>(b16 + i);
                f = make_float4(add_rn(bf16_lo(b.x), f.x), add_rn(bf16_hi(b.x), f.y), add_rn(bf16_lo(b.y), f.z),
                                add_rn(bf16_hi(b.y), f.w));
            }
            *reinterpret_cast<uint2*>(y16 + i) = make_uint2(bf16_pack(f.x, f.y), bf16_pack(f.z, f.w));
        },
        [&](int64_t i, int64_t c) { y16[i] = (uint16_t)bf16_rne(__float_as_uint(bf16_out(b16, i, ys[c]))); });
}
