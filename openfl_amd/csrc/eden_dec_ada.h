// eden_dec_ada.h -- decode's last row pass folded into the FedOpt gradient
// (ofl_eden_decode_adaptive_accumulate): k_dec_ada_rowC and k_dec_ada_rowC2 are
// k_dec_rowC and k_dec_rowC2 with another epilogue.  Where those store the
// finished float32 tile to y so that k_adaptive_accumulate can read it back in
// the next launch, these fold it into the float32 gradient from the registers:
//     d = v[k]                                   decode's own bits
//     x = delta ? add_rn(base[i], d) : d         apply_delta (as store_y_l)
//     t = w * (base[i] - x)                      } ada_acc's operations
//     g[i] = (first ? +0.0f : g[i]) + t          } (agg_kernels.hip), contraction off
// The subtract, the product and the add are three float32 roundings; the add
// is kept on the first upload, so a -0.0 product becomes +0.0 as the chain
// from +0.0f makes it (unlike acc_quads, whose first product is stored).
// base - (base + d) is not simplified: the bits differ.  y is not written.
// Included by eden_kernels.hip after eden_dec_acc_bf16.h (the order of the
// kernels before it in the code object stays), inside namespace ofl.
//
// The base is the accumulator's gradient base (KArgs::wbase, always there);
// delta says that the same arena is also the upload's apply-delta base
// (KArgs::yadd, which the small slices' decode kernels read, is it or null).
// So there is one base stream, and first and delta are block-uniform branches
// around four copies of the quad walk inside each kernel.
//
// Data movement.  A thread holds 16 quads of 4 consecutive elements (element
// bits 0, 1 in register bits 0, 1 of both kernels' last layouts), so a quad is
// one 16-byte load of the base, one 16-byte load of g (not on the first
// upload) and one 16-byte store of g: 8 registers in flight per quad where
// acc_quads holds 12.  The quads are walked in order as acc_quads walks them:
// the loads of quad q + kAdaAhead are issued before the stores of quad q, so
// waiting for a quad's loads never waits for a store (loads and stores share
// one in-order counter on gfx950).  (kAdaAhead + 1) x 8 registers hold bytes
// in flight beside the 64 values.
//
// The base is read once per collaborator here and is streamed nt, the rule of
// the large slices' arena I/O.  g is read again by the next upload and stays
// cacheable (kAdaG*Aux below).
#pragma once

// quads of base and g in flight ahead of the fold: kAccAhead's depth.  A walk
// 4 ahead fits the 128-register budget of two blocks per CU as well (no
// scratch, the same occupancy) and measured 0.0770 against 0.0772-0.0776 ms
// per upload, inside the spread, so it was not kept
constexpr int kAdaAhead = kAccAhead;
constexpr int kAdaBaseLdAux = kIoLdAux;
// g is read again by the next upload a few hundred microseconds later and is
// kept cacheable both ways, as k_adaptive_accumulate keeps it: 0.0760-0.0761
// ms per upload against 0.0772-0.0776 with nt both ways, the weighted-average
// fold's policy for its sums (alternated processes)
constexpr int kAdaGLdAux = 0;
constexpr int kAdaGStAux = 0;

// ada_acc (agg_kernels.hip) on decode's d: one rounding per line
template <bool FIRST, bool DELTA>
DEVI float ada_fold(float w, float b, float d, float g) {
#pragma clang fp contract(off)
    const float x = DELTA ? add_rn(b, d) : d;
    const float s = b - x;
    const float t = w * s;
    return (FIRST ? 0.0f : g) + t;
}

// the tile's whole quads in order (rg / rb: the tile's g and base, clamped to
// them, so a quad at or past the bound reads zeros and stores nothing)
template <Lay L, bool FIRST, bool DELTA>
DEVI void ada_quads(const KArgs& a, rsrc_t rg, rsrc_t rb, uint32_t base, const float (&v)[64]) {
#pragma clang fp contract(off)
    const float w = a.ada_w;
    f32x4 b[16], gq[16];
    auto issue = [&](int q) {
        const uint32_t o = LT<L>::off(4 * q);
        b[q] = raw_load_f32x4(rb, (int)(base * 4u), (int)(o * 4u), kAdaBaseLdAux);
        if constexpr (!FIRST) gq[q] = raw_load_f32x4(rg, (int)(base * 4u), (int)(o * 4u), kAdaGLdAux);
    };
#pragma unroll
    for (int q = 0; q < kAdaAhead; ++q) issue(q);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (q + kAdaAhead < 16) issue(q + kAdaAhead);
        asm volatile("" ::: "memory");  // the loads above stay above the stores below
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t o = LT<L>::off(4 * q);
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = ada_fold<FIRST, DELTA>(w, b[q][e], v[4 * q + e], FIRST ? 0.0f : gq[q][e]);
        raw_store_f32x4(out, rg, (int)(base * 4u), (int)(o * 4u), kAdaGStAux);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The gradient epilogue of a tile in layout L (in store_y_l's / acc_y's
// place): the whole quads below ylen through buffer views clamped to them,
// then the <= 3 elements of the quad that straddles ylen, block-uniform.
// Nothing at or past ylen is read in the base, read or written in g.
template <Lay L, bool FIRST, bool DELTA>
DEVI void ada_y_fd(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
#pragma clang fp contract(off)
    static_assert(LT<L>::rb(0) == 0 && LT<L>::rb(1) == 1, "16-byte accesses need element bits 0, 1 in registers 0, 1");
    const uint32_t e0 = tile << kRowLog;
    const uint32_t nv = tile_valid(D.ylen - (int64_t)e0);
    const rsrc_t rg = mk_rsrc(a.g + D.y_off + e0, (nv & ~3u) * 4u);
    const rsrc_t rb = mk_rsrc(a.wbase + D.y_off + e0, (nv & ~3u) * 4u);
    ada_quads<L, FIRST, DELTA>(a, rg, rb, base, v);
    if (nv & 3u) {
        const uint32_t eb = nv & ~3u;
        float* gp = a.g + D.y_off + e0 + eb;
        const float* bp = a.wbase + D.y_off + e0 + eb;
#pragma unroll
        for (int k = 0; k < 64; k += 4)
            if (base + LT<L>::off(k) == eb) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if ((uint32_t)q < (nv & 3u)) gp[q] = ada_fold<FIRST, DELTA>(a.ada_w, bp[q], v[k + q], FIRST ? 0.0f : gp[q]);
            }
    }
}
template <Lay L>
DEVI void ada_y(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
    const bool delta = a.yadd != nullptr;
    if (a.acc_first) {
        if (delta) ada_y_fd<L, true, true>(a, D, tile, base, v);
        else ada_y_fd<L, true, false>(a, D, tile, base, v);
    } else {
        if (delta) ada_y_fd<L, false, true>(a, D, tile, base, v);
        else ada_y_fd<L, false, false>(a, D, tile, base, v);
    }
}

// decode pass C into the gradient, persistent and prefetching (as k_dec_rowC)
__global__ __launch_bounds__(kRowNT) OFL_NO_PK_F32 void k_dec_ada_rowC(KArgs a) {
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
        ada_y<RS::L1>(a, D, tile, base1, v);
        if (!more) break;
        t = tn; si = sn; tile = tln;
    }
}

// decode pass C into the gradient, two blocks per CU (as k_dec_rowC2: the tile
// table, a paired table or a split 5-pass slice's explicit tile list)
__global__ __launch_bounds__(kRowNT, 4) OFL_NO_PK_F32 void k_dec_ada_rowC2(KArgs a) {
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
        ada_y<R::B4>(a, D, tile, base4, v);
        if (h >= pair) break;
      }
    }
}
