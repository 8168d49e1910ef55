// Lane-linear LDS exchange between two register layouts of a 2^15-element
// tile held by 512 threads x 64 registers, in two halves through a
// 2^14-float image (register bit 5 of both layouts is the same element bit,
// the half bit, and never enters the image).
//
// Write side: register r of wave w goes to  wave_base(w) + reg_off(r) + lane
// (dwords): one ds_write_addtid_b32 per register (address = M0 + imm16 +
// 4 * lane, no address VGPR; 128 B/clk/CU against ds_write_b32's 64).
// Read side: the image address of a tile element is a sum of one coefficient
// per set index bit (LinImg), so the address of (thread, register) of the
// destination layout splits into a per-thread base plus a compile-time
// immediate per register, and reads are ds_read_b32, or ds_read_b128 where
// the destination's registers 0, 1 are the elements on the source's lanes
// 0, 1 (lin_width).  The strides between the 256-byte rows are chosen per
// pair so that every read is conflict-free in its lane groups (lin_img),
// inside the 68 KiB of the padded element-indexed image.
//
// The address math is constexpr and free of device code, so the host checker
// (tests/test_lds_exchange_layouts.py) and the kernels share this one copy.
#pragma once
#include <cstdint>
#include <cstddef>

// A layout: tile of 2^nb elements; element bit r_i lives in register bit i
// (5 or 6 register bits: 32 or 64 elements per thread); the other element
// bits are the thread index, lowest first.
struct Lay { int nb, r0, r1, r2, r3, r4, r5 = -1; };

constexpr int lay_rb(const Lay& L, int i) {
    return i == 0 ? L.r0 : i == 1 ? L.r1 : i == 2 ? L.r2 : i == 3 ? L.r3 : i == 4 ? L.r4 : L.r5;
}
constexpr uint32_t lay_rmask(const Lay& L) {
    uint32_t m = 0;
    for (int i = 0; i < (L.r5 < 0 ? 5 : 6); ++i) m |= 1u << lay_rb(L, i);
    return m;
}
// tile element offset of register r / tile element base of thread tid
constexpr uint32_t lay_off(const Lay& L, int r) {
    uint32_t o = 0;
    for (int i = 0; i < (L.r5 < 0 ? 5 : 6); ++i) if ((r >> i) & 1) o |= 1u << lay_rb(L, i);
    return o;
}
constexpr uint32_t lay_base(const Lay& L, uint32_t tid) {
    uint32_t b = 0;
    int t = 0;
    for (int q = 0; q < L.nb; ++q)
        if (!((lay_rmask(L) >> q) & 1u)) { b |= ((tid >> t) & 1u) << q; ++t; }
    return b;
}

// Image of one half: dword coefficient of the source layout's register bit i
// (i < 5) and wave bit j; lane bit k always has 1 << k (ds_write_addtid_b32).
struct LinImg { uint32_t reg[5]; uint32_t wave[3]; };
// rows of 64 floats back to back
constexpr LinImg kLinPlain{{64, 128, 256, 512, 1024}, {2048, 4096, 8192}};

// budget: the padded half image of the element-indexed exchange (68 KiB)
constexpr uint32_t kLinBudget = (1u << 14) + (1u << 9) + (1u << 4);

constexpr uint32_t lin_reg_off(const LinImg& I, int r) {
    uint32_t o = 0;
    for (int i = 0; i < 5; ++i) if ((r >> i) & 1) o += I.reg[i];
    return o;
}
constexpr uint32_t lin_wave_base(const LinImg& I, uint32_t w) {
    uint32_t o = 0;
    for (int j = 0; j < 3; ++j) if ((w >> j) & 1u) o += I.wave[j];
    return o;
}
constexpr uint32_t lin_footprint(const LinImg& I) { return lin_wave_base(I, 7) + lin_reg_off(I, 31) + 64; }

// dword address in the image written from layout A of tile element e (the
// half bit of e is ignored); additive over disjoint bit sets of e
constexpr uint32_t lin_addr(const Lay& A, const LinImg& I, uint32_t e) {
    uint32_t a = 0;
    int t = 0;
    for (int q = 0; q < A.nb; ++q) {
        if (q == A.r5) continue;
        int reg = -1;
        for (int i = 0; i < 5; ++i) if (lay_rb(A, i) == q) reg = i;
        if ((e >> q) & 1u) a += reg >= 0 ? I.reg[reg] : t < 6 ? 1u << t : I.wave[t - 6];
        if (reg < 0) ++t;
    }
    return a;
}
// read side of destination layout B: thread base and register immediate
constexpr uint32_t lin_read_base(const Lay& A, const Lay& B, const LinImg& I, uint32_t tid) {
    return lin_addr(A, I, lay_base(B, tid));
}
constexpr uint32_t lin_read_off(const Lay& A, const Lay& B, const LinImg& I, int r) {
    return lin_addr(A, I, lay_off(B, r));
}

// dwords per read: 4 when B's registers 0, 1 hold the elements on A's lanes 0, 1
constexpr int lin_width(const Lay& A, const Lay& B) {
    int lane[2] = {-1, -1}, t = 0;
    for (int q = 0; q < A.nb && t < 2; ++q)
        if (!((lay_rmask(A) >> q) & 1u)) lane[t++] = q;
    return lay_rb(B, 0) == lane[0] && lay_rb(B, 1) == lane[1] ? 4 : 1;
}

// lane group of a ds_read_b128: {0-3,12-15,20-27}, {4-11,16-19,28-31} and the
// same two sets + 32 (lanes 2..4 of even / odd parity)
constexpr int lin_group128(int lane) { return 2 * (lane >> 5) + (((lane >> 2) ^ (lane >> 3) ^ (lane >> 4)) & 1); }

// every read instruction conflict-free within its lane groups: ds_read_b32,
// 2 x 32 lanes on 32 banks; ds_read_b128, 4 x 16 lanes on 16 sixteen-byte
// slots, addresses 16-byte aligned.  All registers of a thread add the same
// immediate, so the thread bases decide.
constexpr bool lin_reads_ok(const Lay& A, const Lay& B, const LinImg& I, int W) {
    if (W == 4)
        for (int r = 0; r < 64; r += 4) if (lin_read_off(A, B, I, r) & 3u) return false;
    for (uint32_t w = 0; w < 8; ++w) {
        uint64_t seen[4] = {0, 0, 0, 0};
        for (uint32_t l = 0; l < 64; ++l) {
            const uint32_t b = lin_read_base(A, B, I, 64 * w + l);
            if (W == 4 && (b & 3u)) return false;
            const int g = W == 4 ? lin_group128((int)l) : (int)(l >> 5);
            const uint32_t bank = W == 4 ? (b >> 2) & 15u : b & 31u;
            if ((seen[g] >> bank) & 1u) return false;
            seen[g] |= 1ull << bank;
        }
    }
    return true;
}
// where layout A keeps element bit q: lane bit 0..5, 8 + register bit, 16 + wave bit
constexpr int lin_src_pos(const Lay& A, int q) {
    int t = 0;
    for (int b = 0; b < A.nb; ++b) {
        if (b == A.r5) continue;
        int reg = -1;
        for (int i = 0; i < 5; ++i) if (lay_rb(A, i) == b) reg = i;
        if (b == q) return reg >= 0 ? 8 + reg : t < 6 ? t : 16 + (t - 6);
        if (reg < 0) ++t;
    }
    return -1;
}

// The image of a pair.  The destination's lanes 0..4 are five element bits;
// those on source lanes have their stride (1 << k dwords), those on source
// register or wave bits ("row bits") are given what is left:
//   ds_read_b32:  the five strides are 1, 2, 4, 8, 16 mod 32 (32 banks);
//   ds_read_b128: they are 4, 8, 16, 32 and 0 mod 64 (16 slots of 16 bytes),
//                 the 0 on one of lanes 2..4: a lane group is lanes 0, 1 free
//                 and lanes 2..4 of one parity, which {x, y, 0} keeps apart.
// Every other row bit is free.  Strides are then laid out smallest first,
// registers before waves, each the least value with its residue that clears
// the block below it, so no two elements share a dword.
constexpr LinImg lin_img(const Lay& A, const Lay& B, int W) {
    const uint32_t M = W == 4 ? 64 : 32;
    int pos[5] = {-1, -1, -1, -1, -1}, k = 0;
    for (int q = 0; q < B.nb && k < 5; ++q)
        if (!((lay_rmask(B) >> q) & 1u)) pos[k++] = lin_src_pos(A, q);
    uint32_t used = 0;
    for (k = 0; k < 5; ++k) if (pos[k] < 6) used |= 1u << pos[k];
    int zero = -1;
    if (W == 4) for (k = 2; k < 5; ++k) if (pos[k] >= 8) zero = k;
    int res[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // register bits 0..4, wave bits 0..2; -1: free
    uint32_t next = (uint32_t)W;
    for (k = 0; k < 5; ++k) {
        if (pos[k] < 8) continue;
        const int idx = pos[k] >= 16 ? 5 + pos[k] - 16 : pos[k] - 8;
        if (k == zero) { res[idx] = 0; continue; }
        while (next < M && (used & next)) next <<= 1;
        res[idx] = next < M ? (int)next : 0;  // none left: a conflicted image (lin_reads_ok says so)
        used |= next;
    }
    LinImg I{};
    uint32_t span = 64;
    for (int cls = 0; cls < 2; ++cls)
        for (int pass = 0; pass < 2; ++pass)
            for (int idx = cls ? 5 : 0; idx < (cls ? 8 : 5); ++idx) {
                if ((res[idx] > 0) != (pass == 1)) continue;
                const uint32_t m = res[idx] < 0 ? (uint32_t)W : M, r = res[idx] < 0 ? 0u : (uint32_t)res[idx];
                const uint32_t c = span + (r + m - span % m) % m;
                (idx < 5 ? I.reg[idx] : I.wave[idx - 5]) = c;
                span += c;
            }
    return I;
}

#if defined(__HIPCC__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// eight registers of one half from R0: M0 and its stores in one statement
// (nothing else in the kernels reads M0; one wait state after writing it)
template <LinImg I, int R0>
__device__ __forceinline__ void lin_store8(const float (&v)[64], uint32_t m0) {
#define LIN_O(k) "n"(4u * lin_reg_off(I, (R0 + k) & 31))
    asm volatile(
        "s_mov_b32 m0, %8\n\ts_nop 0\n\t"
        "ds_write_addtid_b32 %0 offset:%9\n\tds_write_addtid_b32 %1 offset:%10\n\t"
        "ds_write_addtid_b32 %2 offset:%11\n\tds_write_addtid_b32 %3 offset:%12\n\t"
        "ds_write_addtid_b32 %4 offset:%13\n\tds_write_addtid_b32 %5 offset:%14\n\t"
        "ds_write_addtid_b32 %6 offset:%15\n\tds_write_addtid_b32 %7 offset:%16"
        :
        : "v"(v[R0]), "v"(v[R0 + 1]), "v"(v[R0 + 2]), "v"(v[R0 + 3]), "v"(v[R0 + 4]), "v"(v[R0 + 5]),
          "v"(v[R0 + 6]), "v"(v[R0 + 7]), "s"(m0), LIN_O(0), LIN_O(1), LIN_O(2), LIN_O(3), LIN_O(4), LIN_O(5),
          LIN_O(6), LIN_O(7)
        : "memory", "m0");
#undef LIN_O
}

// A -> B through the image at s (LDS, 16-byte aligned, kLinBudget floats);
// the barriers are exchange_half_pad's.  W, CHECK: the microbenchmark's
// dword-read form of a pair that has no conflict-free one
template <Lay A, Lay B, int HB, int W = lin_width(A, B), bool CHECK = true>
__device__ __forceinline__ void exchange_half_lin(float (&v)[64], float* s, uint32_t tid) {
    static_assert(A.nb == 15 && B.nb == 15 && A.r5 == HB && B.r5 == HB, "half bit must be register bit 5 of both layouts");
    constexpr LinImg I = lin_img(A, B, W);
    static_assert(!CHECK || lin_reads_ok(A, B, I, W), "no conflict-free image for this pair");
    static_assert(lin_footprint(I) <= kLinBudget, "image over budget");
    // M0[15:0] and the 16-bit immediate; s sits at the start of the block's LDS
    static_assert(4u * lin_wave_base(I, 7) + 4096u < 65536u && 4u * lin_reg_off(I, 31) < 65536u, "store address out of range");
    const uint32_t s0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)s;
    const uint32_t m0 = __builtin_amdgcn_readfirstlane(s0 + 4u * lin_wave_base(I, tid >> 6));
    uint32_t bb = lin_read_base(A, B, I, tid) / W;
    asm volatile("" : "+v"(bb));  // not hoisted out of the tile loop
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 0) {
            lin_store8<I, 0>(v, m0); lin_store8<I, 8>(v, m0); lin_store8<I, 16>(v, m0); lin_store8<I, 24>(v, m0);
        } else {
            lin_store8<I, 32>(v, m0); lin_store8<I, 40>(v, m0); lin_store8<I, 48>(v, m0); lin_store8<I, 56>(v, m0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stores above are not the compiler's to count
        __syncthreads();
        if constexpr (W == 4) {
            typedef float f4v __attribute__((ext_vector_type(4)));
            const f4v* s4 = reinterpret_cast<const f4v*>(s);
#pragma unroll
            for (int r = 32 * h; r < 32 * h + 32; r += 4) {
                const f4v q = s4[bb + lin_read_off(A, B, I, r) / 4];
                v[r] = q.x; v[r + 1] = q.y; v[r + 2] = q.z; v[r + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int r = 32 * h; r < 32 * h + 32; ++r) v[r] = s[bb + lin_read_off(A, B, I, r)];
        }
        __syncthreads();
    }
}
#pragma clang diagnostic pop
#endif
