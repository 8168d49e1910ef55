// Host checker of openfl_amd/csrc/lds_exchange.h (tests/test_lds_exchange_layouts.py):
// for every layout pair that goes through exchange_half_lin, replay the
// stores and loads of all 512 threads on a model of the image and check
//   - every element of each half is stored once, inside the footprint, and
//     arrives in the thread and register the destination layout names;
//   - no store or load instruction has two lanes of one lane group on one
//     bank (ds_write_addtid_b32 / ds_read_b32: lanes 0-31 and 32-63, bank =
//     dword address mod 32; ds_read_b128: the four 16-lane groups below,
//     bank = dword address mod 64 for each of the four dwords);
//   - 16-byte loads are 16-byte aligned and return four consecutive registers;
//   - the footprint is within the budget and the store addresses fit M0's
//     16 bits and the 16-bit immediate.
// Control: the unpadded image on a pair that needs padding must show conflicts.
#include <cstdio>
#include <cstring>
#include <vector>
#include "lds_exchange.h"

struct Pair { const char* name; Lay a, b; int hb; };
// the two-block row kernels' layout sets of eden_kernels.hip: RowC2Set
// L3 -> L4 -> L5, DecA2Set C1 -> C2 -> C3, RowA2Set A1 -> A2 -> A3, DecC2Set
// B1 -> B2 -> B3 -> B4 (the kernels use some, tools/lds_exchange_bench.hip all)
static const Pair kPairs[] = {
    {"RowC2 L3->L4", {15, 5, 6, 7, 8, 9, 10}, {15, 11, 12, 13, 14, 9, 10}, 10},
    {"RowC2 L4->L5", {15, 11, 12, 13, 14, 9, 10}, {15, 0, 1, 2, 3, 4, 10}, 10},
    {"DecA2 C1->C2", {15, 0, 1, 2, 3, 4, 5}, {15, 11, 12, 13, 14, 9, 5}, 5},
    {"DecA2 C2->C3", {15, 11, 12, 13, 14, 9, 5}, {15, 6, 7, 8, 9, 10, 5}, 5},
    {"RowA2 A1->A2", {15, 0, 1, 11, 12, 13, 14}, {15, 2, 3, 4, 5, 6, 14}, 14},
    {"RowA2 A2->A3", {15, 2, 3, 4, 5, 6, 14}, {15, 10, 7, 8, 9, 6, 14}, 14},
    {"DecC2 B1->B2", {15, 0, 1, 7, 8, 9, 10}, {15, 2, 3, 4, 5, 6, 10}, 10},
    {"DecC2 B2->B3", {15, 2, 3, 4, 5, 6, 10}, {15, 0, 1, 11, 12, 13, 10}, 10},
    {"DecC2 B3->B4", {15, 0, 1, 11, 12, 13, 10}, {15, 0, 1, 14, 11, 12, 10}, 10},
};
// ds_read_b128 lane groups, one LDS cycle each
static const int kGroups128[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

struct Result { long wrong = 0, conflicts = 0, misaligned = 0, out_of_range = 0; };

static Result check(const Lay& A, const Lay& B, int hb, const LinImg& I, int W) {
    Result res;
    const uint32_t fp = lin_footprint(I);
    if (fp > kLinBudget) ++res.out_of_range;
    if (4u * lin_wave_base(I, 7) + 4096u >= 65536u || 4u * lin_reg_off(I, 31) >= 65536u) ++res.out_of_range;
    if (lay_rb(A, 5) != hb || lay_rb(B, 5) != hb) ++res.wrong;
    for (int h = 0; h < 2; ++h) {
        std::vector<long> img(kLinBudget, -1);
        // stores: one instruction per (wave, register), address M0 + imm + lane
        for (uint32_t w = 0; w < 8; ++w)
            for (int r = 0; r < 32; ++r) {
                int banks[2][32];
                std::memset(banks, 0, sizeof(banks));
                for (uint32_t l = 0; l < 64; ++l) {
                    const uint32_t tid = 64 * w + l;
                    const uint32_t a = lin_wave_base(I, w) + lin_reg_off(I, r) + l;
                    if (a >= fp || a >= kLinBudget) { ++res.out_of_range; continue; }
                    if (img[a] >= 0) ++res.wrong;  // stored twice
                    img[a] = (long)(lay_base(A, tid) | lay_off(A, r + 32 * h));
                    if (banks[l >> 5][a & 31]++) ++res.conflicts;
                }
            }
        for (uint32_t a = 0; a < kLinBudget; ++a)
            if (img[a] >= 0 && (int)((img[a] >> hb) & 1) != h) ++res.wrong;
        // loads: one instruction per (wave, W registers)
        std::vector<char> got(1u << 15, 0);
        for (uint32_t w = 0; w < 8; ++w)
            for (int r = 32 * h; r < 32 * h + 32; r += W) {
                int banks[4][64];
                std::memset(banks, 0, sizeof(banks));
                for (int g = 0; g < (W == 4 ? 4 : 2); ++g)
                    for (int k = 0; k < (W == 4 ? 16 : 32); ++k) {
                        const uint32_t l = W == 4 ? (uint32_t)kGroups128[g][k] : (uint32_t)(32 * g + k);
                        const uint32_t tid = 64 * w + l;
                        const uint32_t a = lin_read_base(A, B, I, tid) + lin_read_off(A, B, I, r);
                        if (W == 4 && (a & 3u)) ++res.misaligned;
                        for (int d = 0; d < W; ++d) {
                            if (a + d >= fp) { ++res.out_of_range; continue; }
                            const long want = (long)(lay_base(B, tid) | lay_off(B, r + d));
                            if (img[a + d] != want) ++res.wrong;
                            else got[want] = 1;
                            if (banks[g][(a + d) & (W == 4 ? 63 : 31)]++) ++res.conflicts;
                        }
                    }
            }
        for (uint32_t e = 0; e < (1u << 15); ++e)
            if ((int)((e >> hb) & 1u) == h && !got[e]) ++res.wrong;  // an element that never arrived
    }
    return res;
}

int main() {
    bool ok = true;
    for (const Pair& p : kPairs) {
        const int W = lin_width(p.a, p.b);
        const LinImg I = lin_img(p.a, p.b, W);
        const Result r = check(p.a, p.b, p.hb, I, W);
        std::printf("pair %s width %d image %u,%u,%u,%u,%u|%u,%u,%u footprint %u budget %u wrong %ld conflicts %ld "
                    "misaligned %ld range %ld constexpr_ok %d\n",
                    p.name, W, I.reg[0], I.reg[1], I.reg[2], I.reg[3], I.reg[4], I.wave[0], I.wave[1], I.wave[2],
                    lin_footprint(I), kLinBudget, r.wrong, r.conflicts, r.misaligned, r.out_of_range,
                    (int)lin_reads_ok(p.a, p.b, I, W));
        if (r.wrong || r.conflicts || r.misaligned || r.out_of_range || !lin_reads_ok(p.a, p.b, I, W)) ok = false;
    }
    // control: C1 -> C2 reads down the source's registers; rows back to back put 32 lanes on one bank
    const Result c = check(kPairs[2].a, kPairs[2].b, kPairs[2].hb, kLinPlain, 1);
    std::printf("control DecA2 C1->C2 image plain wrong %ld conflicts %ld constexpr_ok %d\n", c.wrong, c.conflicts,
                (int)lin_reads_ok(kPairs[2].a, kPairs[2].b, kLinPlain, 1));
    if (c.wrong || !c.conflicts || lin_reads_ok(kPairs[2].a, kPairs[2].b, kLinPlain, 1)) ok = false;
    return ok ? 0 : 1;
}
