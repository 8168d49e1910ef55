// eden_dec_acc_bf16.h -- decode's last row pass folded into the streaming
// average's sums against a bfloat16 base (ofl_eden_decode_accumulate_bf16):
// k_dec_acc_rowC_bf16 and k_dec_acc_rowC2_bf16 are k_dec_acc_rowC and
// k_dec_acc_rowC2 (eden_dec_acc.h) with another epilogue.  A bf16 base stands
// for its exact float32 widening and nothing is rounded to bf16 here:
//     d = v[k]                                      decode's own bits
//     x = base16 ? add_rn(widen(base16[i]), d) : d  apply_delta on the widened base
//     p = (double)x * w                             } acc_elem's operations
//     sums[i] = first ? p : sums[i] + p             } (agg_kernels.hip), contraction off
// so the sums are ofl_eden_decode_accumulate's on base16.float(), bit for bit.
// Included by eden_kernels.hip after eden_bf16.h (the order of the kernels
// before it in the code object stays), inside namespace ofl.
//
// Data movement.  A thread holds 16 quads of 4 consecutive elements; a quad is
// one 8-byte nt load of the base (two registers, as fetch_x16 / store_y16) and
// 32 bytes of sums, two 16-byte loads and two 16-byte stores: 2 + 16 + 16 = 34
// bytes per 4 elements where the float32 base takes 48 -- per element 22
// bytes instead of 24 with the intermediate's 4.  The quads are walked as
// acc_quads walks them: the loads of quad g + kAccAhead16 are issued before the
// stores of quad g (loads and stores share one in-order counter on gfx950), so
// at most (kAccAhead16 + 1) x 10 registers hold bytes in flight beside the 64
// values.  The base view is clamped to the tile's whole quads below ylen
// ((nv & ~3) * 2 bytes) like the sums view; the <= 3 elements of the quad that
// straddles ylen go one by one, block-uniform.  Nothing at or past ylen is read
// in the base, read or written in the sums.
//
// The slices of at most 2^15 elements keep their decode kernels, which write
// the packed float32 side arena of eden_bf16_plan.h (decoded, no base);
// k_acc_side_ranges then folds it into the sums on their output ranges, adding
// the widened base on the way.  The same kernel folds any packed float32
// buffer laid out by a table of that format (ofl_acc_side_ranges: the raw
// tensors of an upload).
#pragma once

// quads of base and sums in flight ahead of the fold: kAccAhead's depth (the
// two registers a quad's base gives back were not spent on a deeper walk:
// no depth beyond 2 has been measured)
constexpr int kAccAhead16 = kAccAhead;

// the tile's whole quads in order (rs / rb: the tile's sums and bf16 base,
// clamped to them, so a quad at or past the bound reads zeros and stores nothing)
template <Lay L, bool FIRST, bool BASE>
DEVI void acc_quads16(const KArgs& a, rsrc_t rs, rsrc_t rb, uint32_t base, const float (&v)[64]) {
#pragma clang fp contract(off)
    const double w = a.acc_w;
    i32x2 b[16];
    f32x4 lo[16], hi[16];
    auto issue = [&](int g) {
        const uint32_t o = LT<L>::off(4 * g);
        if constexpr (BASE) b[g] = raw_load_i32x2(rb, (int)(base * 2u), (int)(o * 2u), kAccLdAux);
        if constexpr (!FIRST) {
            lo[g] = raw_load_f32x4(rs, (int)(base * 8u), (int)(o * 8u), kAccLdAux);
            hi[g] = raw_load_f32x4(rs, (int)(base * 8u + 16u), (int)(o * 8u), kAccLdAux);
        }
    };
#pragma unroll
    for (int g = 0; g < kAccAhead16; ++g) issue(g);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        if (g + kAccAhead16 < 16) issue(g + kAccAhead16);
        asm volatile("" ::: "memory");  // the loads above stay above the stores below
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t o = LT<L>::off(4 * g);
        float x[4] = {v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
        if constexpr (BASE) {
            const uint32_t b0 = (uint32_t)b[g].x, b1 = (uint32_t)b[g].y;
            x[0] = add_rn(bf16_lo(b0), x[0]); x[1] = add_rn(bf16_hi(b0), x[1]);
            x[2] = add_rn(bf16_lo(b1), x[2]); x[3] = add_rn(bf16_hi(b1), x[3]);
        }
        double p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = (double)x[q] * w;
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

// The accumulate epilogue of a tile in layout L against a bf16 base (in
// acc_y's place): the whole quads below ylen through buffer views clamped to
// them, then the <= 3 elements of the quad that straddles ylen.
template <Lay L, bool FIRST>
DEVI void acc_y16_first(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
#pragma clang fp contract(off)
    static_assert(LT<L>::rb(0) == 0 && LT<L>::rb(1) == 1, "8- and 16-byte accesses need element bits 0, 1 in registers 0, 1");
    const uint32_t e0 = tile << kRowLog;
    const uint32_t nv = tile_valid(D.ylen - (int64_t)e0);
    const rsrc_t rs = mk_rsrc(a.sums + D.y_off + e0, (nv & ~3u) * 8u);
    if (a.base16) {
        const rsrc_t rb = mk_rsrc(a.base16 + D.y_off + e0, (nv & ~3u) * 2u);
        acc_quads16<L, FIRST, true>(a, rs, rb, base, v);
    } else {
        acc_quads16<L, FIRST, false>(a, rs, rs, base, v);
    }
    if (nv & 3u) {
        const uint32_t eb = nv & ~3u;
        const int64_t i0 = D.y_off + e0 + eb;
        double* sp = a.sums + i0;
#pragma unroll
        for (int k = 0; k < 64; k += 4)
            if (base + LT<L>::off(k) == eb) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if ((uint32_t)q < (nv & 3u)) {
                        const double p = (double)bf16_out(a.base16, i0 + q, v[k + q]) * a.acc_w;
                        sp[q] = FIRST ? p : sp[q] + p;
                    }
            }
    }
}
template <Lay L>
DEVI void acc_y16(const KArgs& a, const SliceDesc& D, uint32_t tile, uint32_t base, const float (&v)[64]) {
    if (a.acc_first) acc_y16_first<L, true>(a, D, tile, base, v);
    else acc_y16_first<L, false>(a, D, tile, base, v);
}

// decode pass C into the sums against a bf16 base, persistent and prefetching (as k_dec_acc_rowC)
__global__ __launch_bounds__(kRowNT) OFL_NO_PK_F32 void k_dec_acc_rowC_bf16(KArgs a) {
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
        acc_y16<RS::L1>(a, D, tile, base1, v);
        if (!more) break;
        t = tn; si = sn; tile = tln;
    }
}

// decode pass C into the sums against a bf16 base, two blocks per CU (as
// k_dec_acc_rowC2: the tile table, a paired table or a split 5-pass slice's
// explicit tile list)
__global__ __launch_bounds__(kRowNT, 4) OFL_NO_PK_F32 void k_dec_acc_rowC2_bf16(KArgs a) {
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
        acc_y16<R::B4>(a, D, tile, base4, v);
        if (h >= pair) break;
      }
    }
}

// sums[i] (=|+=) (double)(b16 ? add_rn(widen(b16[i]), side[c]) : side[c]) * w
// on the ranges of a QRanges table (c: element i's place in the packed
// float32 buffer `side`, eden_bf16.h).  A whole slot is one 16-byte side load,
// one 8-byte base load and the sums as two 16-byte pairs each way; a ragged
// slot goes element by element.
struct AccSideArgs {
    const float* side;
    const uint16_t* b16;  // nullable
    double* sums;
    double w;
    int first;            // store the product instead of adding it
};
__global__ __launch_bounds__(kRangeNT) OFL_NO_PK_F32 void k_acc_side_ranges(AccSideArgs a, QRanges rg, int vec) {
    range_slots(rg, vec,
        [&](int64_t i, int64_t c) {
#pragma clang fp contract(off)
            float4 f = *reinterpret_cast<const float4*>(a.side + c);
            if (a.b16) {
                const uint2 b = *reinterpret_cast<const uint2*>(a.b16 + i);
                f = make_float4(add_rn(bf16_lo(b.x), f.x), add_rn(bf16_hi(b.x), f.y), add_rn(bf16_lo(b.y), f.z),
                                add_rn(bf16_hi(b.y), f.w));
            }
            double2* s2 = reinterpret_cast<double2*>(a.sums + i);
            double2 lo, hi;
            lo.x = (double)f.x * a.w; lo.y = (double)f.y * a.w;
            hi.x = (double)f.z * a.w; hi.y = (double)f.w * a.w;
            if (!a.first) {
                const double2 p = s2[0], q = s2[1];
                lo.x = p.x + lo.x; lo.y = p.y + lo.y;
                hi.x = q.x + hi.x; hi.y = q.y + hi.y;
            }
            s2[0] = lo;
            s2[1] = hi;
        },
        [&](int64_t i, int64_t c) {
#pragma clang fp contract(off)
            const double p = (double)bf16_out(a.b16, i, a.side[c]) * a.w;
            a.sums[i] = a.first ? p : a.sums[i] + p;
        });
}
