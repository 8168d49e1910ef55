// eden_rt_row.h -- k_rt_row, the row pass of the Eden round trip
// y = decode(encode(x)) when nobody reads the bytes (ofl_eden_roundtrip):
// encode's last row pass and decode's first in one kernel, with no bit planes
// between them.  Included by eden_kernels.hip after its own kernels (their
// order in the code object stays), inside namespace ofl.
//
// Per 2^15-element tile, 512 threads x 64 registers, two blocks per CU:
//   ws -> L3 {5..10}            F2c   bits 5..10   } encode pass C
//      -> L4 {11..14, 9, 10}    F2d   bits 11..14  } (k_enc_rowC2's
//      -> L5 {0..4, 10}         F2e   bits 0..4    }  layouts and order)
//         quantise: z -> grid cell -> C[bin] over the value, <C[bin], y>
//         L5 again              G1    bits 0..4    } decode pass A
//      -> M2 {11..14, 5, 10}    G2    bits 11..14, 5   } (k_dec_rowA2's
//      -> M3 {6..9, 5, 10}      G3    bits 6..10   }  order) -> ws, in place
// The quantised tile is already in the layout decode's first five stages
// want (a thread holds two runs of 32 contiguous elements), so those run on
// the centroids where they are: four exchanges for what the two kernels do
// with four plus a plane pack, a plane unpack and a gather.  Every layout
// keeps element bit 10 at register index 5, so every exchange goes in two
// halves through the one 68 KiB buffer, and the butterflied bit order is the
// two kernels', so the tile holds the bits k_dec_rowA2 would have written from
// k_enc_rowC2's planes.
//
// The bin itself is never formed: a grid cell's entry (QEnt) holds the one
// boundary inside the cell and the centroids on either side, so one 16-byte
// LDS read and one compare give C[bin] -- the quantiser table is the centroid
// table.  No ballots, bit transposes, plane stores, plane loads or centroid
// gathers, and no plane-row alignment variants.
#pragma once

struct RtRowSet {
    static constexpr Lay L3 = RowC2Set::L3, L4 = RowC2Set::L4, L5 = RowC2Set::L5, M2{15, 11, 12, 13, 14, 5, 10},
                         M3{15, 6, 7, 8, 9, 5, 10};
    static constexpr uint32_t F2c = RowC2Set::F2c, F2d = RowC2Set::F2d, F2e = RowC2Set::F2e, G1 = DecA2Set::G1,
                              G2 = DecA2Set::G2, G3 = DecA2Set::G3;
    static constexpr int HB = 10;
};

// A run of 32 contiguous values -> their centroids, in place; returns
// <C[bins], y> as quant_pack32 does (the same products in the same order: 8
// table reads in flight per group, each group pinned before the next).
DEVI float quant_centroids32(float* v, float ysc, float zm64, const QTab* q) {
    float dot = 0.f;
    const float m64 = ysc * zm64;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float vg[8], z[8];
        uint32_t addr[8];
        pin_group<8>(&v[8 * g], vg);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            z[t] = vg[t] * m64;
            const float zc = __builtin_amdgcn_fmed3f(z[t], -(float)EDEN_GRID_OFF, (float)(EDEN_GRID_OFF - 1));
            addr[t] = (uint32_t)((int)floorf(zc) + EDEN_GRID_OFF);
        }
        QEnt e[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) e[t] = q->grid[addr[t]];
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);   // the 8 DS reads first
        __builtin_amdgcn_sched_group_barrier(0x002, 64, 0);  // then the VALU
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float c = e[t].b64 < z[t] ? e[t].chi : e[t].clo;
            dot = fmaf(c, vg[t], dot);
            v[8 * g + t] = c;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) asm volatile("" : "+v"(v[8 * g + t]));
        asm volatile("" : "+v"(dot)::"memory");  // group done before the next
    }
    return dot * ysc;
}

// Its butterflies are plain fp32 adds (no packed fp32 instructions): the sums
// round the same either way.  The feature is the device target's alone.
#if defined(__HIP_DEVICE_COMPILE__)
#define OFL_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define OFL_NO_PK_F32
#endif
__global__ __launch_bounds__(kRowNT, 4) OFL_NO_PK_F32 void k_rt_row(KArgs a) {
    using R = RtRowSet;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s = reinterpret_cast<float*>(smem);
    QTab* qt = reinterpret_cast<QTab*>(smem + kRowC2Ex);
    float* red = reinterpret_cast<float*>(smem + kRowC2Ex + sizeof(QTab));
    load_qtable<kRowNT>(qt, a.nbits);
    __syncthreads();
    const int total = a.npair ? a.npair : (int)sld(a.tstart, a.count);  // npair: an explicit tile list
    for (int t = (int)blockIdx.x; t < total; t += (int)gridDim.x) {
        const uint32_t tid = opaque(threadIdx.x);  // as in k_enc_rowA2
        const uint32_t base3 = LT<R::L3>::base(tid), baseo = LT<R::M3>::base(tid);
        int si; uint32_t tile;
        row_locate(a, t, si, tile);
        const SliceDesc D = udesc(a.d, si);
        float v[64];
        fetch_ws<kRowC2LdAux>(a, D, tile, true, base3, v);
        stages<R::L3, R::F2c>(v);
        exchange_half_pad<R::L3, R::L4, R::HB>(v, s, tid);
        stages<R::L4, R::F2d>(v);
        exchange_half_lin<R::L4, R::L5, R::HB>(v, s, tid);
        stages<R::L5, R::F2e>(v);
        __builtin_amdgcn_sched_barrier(0);
        const float nu = sldf(a.nu, si);
        const float ysc = pow2i(-((D.logp + 1) / 2));
        const float zm64 = 64.0f * (sqrtf((float)(1ll << D.logp)) / nu);
        float dot = 0.f;
        dot += quant_centroids32(&v[0], ysc, zm64, qt);
        dot += quant_centroids32(&v[32], ysc, zm64, qt);
        if (!(nu > 0.0f)) {  // a zero slice: encode writes zero planes, bin 0 everywhere
            dot = 0.f;
            const float c0 = g_centroids[a.nbits - 1][0];
#pragma unroll
            for (int r = 0; r < 64; ++r) v[r] = c0;
        }
        dot = block_sum<kRowNT>(dot, red);
        if (tid == 0) a.part[D.part_off + tile] = dot;
        stages<R::L5, R::G1>(v);
        exchange_half_pad<R::L5, R::M2, R::HB>(v, s, tid);
        stages<R::M2, R::G2>(v);
        exchange_half_pad<R::M2, R::M3, R::HB>(v, s, tid);
        stages<R::M3, R::G3>(v);
        store_ws_l<R::M3>(a, D, tile, baseo, v);
    }
}
