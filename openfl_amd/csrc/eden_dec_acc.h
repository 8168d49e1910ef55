// eden_dec_acc.h -- decode's last row pass folded into the streaming average
// (ofl_eden_decode_accumulate): k_dec_acc_rowC and k_dec_acc_rowC2 are
// k_dec_rowC and k_dec_rowC2 with another epilogue.  Where those store the
// finished float32 tile to y so that k_wavg_accumulate can read it back in the
// next launch, these fold it into the float64 sums from the registers:
//     d = v[k]                              decode's own bits
//     x = base ? add_rn(base[i], d) : d     apply_delta (as store_y_l)
//     p = (double)x * w                     } acc_elem's operations
//     sums[i] = first ? p : sums[i] + p     } (agg_kernels.hip), contraction off
// y is not written.  Included by eden_kernels.hip after eden_rt_row.h (the
// order of the kernels before it in the code object stays), inside namespace
// ofl.
//
// Data movement.  A thread holds 16 quads of 4 consecutive elements (element
// bits 0, 1 in register bits 0, 1 of both kernels' last layouts), so a quad is
// one 16-byte load of the base and 32 bytes of sums: two 16-byte loads and two
// 16-byte stores.  The quads are walked in order with the loads of the next
// kAccAhead quads issued before the current quad is folded and stored -- the
// loads of quad g + kAccAhead precede the stores of quad g, so waiting for a
// quad's loads never waits for a store (loads and stores share one in-order
// counter on gfx950).  At most (kAccAhead + 1) x 12 registers hold bytes in
// flight beside the 64 values, which fits the 128-register budget of two
// blocks per CU; loading all 64 sums first would take 128 more.
//
// The sums and the base are streamed once per collaborator: nt both ways, the
// rule of the large slices' arena I/O (kIoLdAux / kIoStAux), so they do not
// push the wave's intermediates out of the Infinity Cache.
//
// first and base are block-uniform branches around four copies of the quad
// walk inside each kernel, so the two kernels are two instantiations.
#pragma once

constexpr int kAccLdAux = kIoLdAux;
constexpr int kAccStAux = kIoStAux;
constexpr int kAccAhead = 2;

typedef double f64x2 __attribute__((ext_vector_type(2)));

// the tile's whole quads in order (rs / rb: the tile's sums and base, clamped
// to them, so a quad at or past the bound reads zeros and stores nothing)
template <Lay L, bool FIRST, bool BASE>
DEVI void acc_quads(const KArgs& a, rsrc_t rs, rsrc_t rb, uint32_t base, const float (&v)[64]) {
#pragma clang fp contract(off)
    const double w = a.acc_w;
    f32x4 b[16], lo[16], hi[16];
    auto issue = [&](int g) {
        const uint32_t o = LT<L>::off(4 * g);
        if constexpr (BASE) b[g] = raw_load_f32x4(rb, (int)(base * 4u), (int)(o * 4u), kAccLdAux);
        if constexpr (!FIRST) {
            lo[g] = raw_load_f32x4(rs, (int)(base * 8u), (int)(o * 8u), kAccLdAux);
            hi[g] = raw_load_f32x4(rs, (int)(base * 8u + 16u), (int)(o * 8u), kAccLdAux);
        }
    };
#pragma unroll
    for (int g = 0; g < kAccAhead; ++g) issue(g);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        if (g + kAccAhead < 16) issue(g + kAccAhead);
        asm volatile("" ::: "memory");  // the loads above stay above the stores below
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t o = LT<L>::off(4 * g);
        double p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = BASE ? add_rn(b[g][q], v[4 * g + q]) : v[4 * g + q];
            p[q] = (double)x * w;
        }
        if constexpr (!FIRST) {
            const f64x2 s0 = __builtin_bit_cast(f64x2, lo[g]), s1 = __builtin_bit_cast(f64x2, hi[g]);
            p[0] = s0.x + p[0]; p[1] = s0.y + p[1];
            p[2] = s1.x + p[2]; p[3] = s1.y + p[3];
        }
        const f64x2 o0 = {p[0], p[1]}, o1 = {p[2], p[3]};
        raw_store_f32x4(__builtin_bit_cast(f32x4, o0), rs, (int)(base * 8u), (int)(o * 8u), kAccStAux);
        raw_store_f32x4(__builtin_bit_cast(f32x4, o1), rs, (int)(base * 8u + 16u), (int)(o * 8u), kAccStAux);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The accumulate epilogue of a tile in layout L (in store_y_l's place): the
// whole quads below ylen through buffer views clamped to them, then the <= 3
// elements of the quad that straddles ylen.  Nothing at or past ylen is read
// or written in sums.
template <Lay L, bool FIRST>
DEVI void acc_y_first(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
#pragma clang fp contract(off)
    static_assert(LT<L>::rb(0) == 0 && LT<L>::rb(1) == 1, "16-byte accesses need element bits 0, 1 in registers 0, 1");
    const uint32_t e0 = tile << kRowLog;
    const uint32_t nv = tile_valid(D.ylen - (int64_t)e0);
    const rsrc_t rs = mk_rsrc(a.sums + D.y_off + e0, (nv & ~3u) * 8u);
    if (a.yadd) {
        const rsrc_t rb = mk_rsrc(a.yadd + D.y_off + e0, (nv & ~3u) * 4u);
        acc_quads<L, FIRST, true>(a, rs, rb, base, v);
    } else {
        acc_quads<L, FIRST, false>(a, rs, rs, base, v);
    }
    if (nv & 3u) {
        const uint32_t eb = nv & ~3u;
        double* sp = a.sums + D.y_off + e0 + eb;
        const float* yb = a.yadd ? a.yadd + D.y_off + e0 + eb : nullptr;
#pragma unroll
        for (int k = 0; k < 64; k += 4)
            if (base + LT<L>::off(k) == eb) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if ((uint32_t)q < (nv & 3u)) {
                        const float x = yb ? add_rn(yb[q], v[k + q]) : v[k + q];
                        const double p = (double)x * a.acc_w;
                        sp[q] = FIRST ? p : sp[q] + p;
                    }
            }
    }
}
template <Lay L>
DEVI void acc_y(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
    if (a.acc_first) acc_y_first<L, true>(a, D, tile, base, v);
    else acc_y_first<L, false>(a, D, tile, base, v);
}

// decode pass C into the sums, persistent and prefetching (as k_dec_rowC)
__global__ __launch_bounds__(kRowNT) OFL_NO_PK_F32 void k_dec_acc_rowC(KArgs a) {
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
        acc_y<RS::L1>(a, D, tile, base1, v);
        if (!more) break;
        t = tn; si = sn; tile = tln;
    }
}

// decode pass C into the sums, two blocks per CU (as k_dec_rowC2: the tile
// table, a paired table or a split 5-pass slice's explicit tile list)
__global__ __launch_bounds__(kRowNT, 4) OFL_NO_PK_F32 void k_dec_acc_rowC2(KArgs a) {
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
        acc_y<R::B4>(a, D, tile, base4, v);
        if (h >= pair) break;
      }
    }
}
