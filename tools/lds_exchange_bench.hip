// lds_exchange_bench.hip -- the row passes' LDS exchange alone, three forms.
// 512-thread blocks, two per CU, 64 floats per thread; each block runs only
// the exchange in halves (store 32, barrier, load 32, barrier, twice) over
// many tiles, so the LDS pipe is the only thing busy:
//   (a) the padded element-indexed image, dword stores and loads
//       (exchange_half_pad of eden_kernels.hip);
//   (b) the lane-linear image, ds_write_addtid_b32 stores, ds_read_b32 loads;
//   (c) as (b) with ds_read_b128 loads, where the destination layout holds
//       contiguous runs (exchange_half_lin of lds_exchange.h).
// For the layout pairs of RowC2Set (L3->L4, L4->L5), DecA2Set (C1->C2,
// C2->C3), RowA2Set (A1->A2, A2->A3) and DecC2Set (B1->B2, B2->B3, B3->B4).
// Every form is first checked against the layouts: after one exchange of
// v[r] = element index, thread and register must hold the destination
// layout's element.
// Build: hipcc --offload-arch=gfx950 -std=c++20 -O3 -Iopenfl_amd/csrc -o lds_exchange_bench tools/lds_exchange_bench.hip
// Run:   ./lds_exchange_bench [tiles per block, default 2000]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lds_exchange.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr uint32_t cpad(uint32_t e) { return e + (e >> 5) + (e >> 10); }
template <int HB>
constexpr uint32_t cidx(uint32_t e) { return (e & ((1u << HB) - 1u)) | ((e >> (HB + 1)) << HB); }

// form (a): as eden_kernels.hip's exchange_half_pad
template <Lay A, Lay B, int HB>
__device__ __forceinline__ void exchange_half_pad(float (&v)[64], float* s, uint32_t tid) {
    uint32_t ba = cpad(cidx<HB>(lay_base(A, tid))), bb = cpad(cidx<HB>(lay_base(B, tid)));
    asm volatile("" : "+v"(ba), "+v"(bb));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int r = 32 * h; r < 32 * h + 32; ++r) s[ba + cpad(cidx<HB>(lay_off(A, r)))] = v[r];
        __syncthreads();
#pragma unroll
        for (int r = 32 * h; r < 32 * h + 32; ++r) v[r] = s[bb + cpad(cidx<HB>(lay_off(B, r)))];
        __syncthreads();
    }
}

// FORM 0: (a); 1: (b); 2: (c).  check: one exchange of the element indices,
// written out; else `tiles` exchanges, timed from outside.
template <Lay A, Lay B, int HB, int FORM>
__global__ __launch_bounds__(512, 4) void k_exch(float* out, int tiles, int check) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s = reinterpret_cast<float*>(smem);
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    float v[64];
#pragma unroll
    for (int r = 0; r < 64; ++r) v[r] = (float)(lay_base(A, tid) | lay_off(A, r));
    for (int t = 0; t < tiles; ++t) {
        if constexpr (FORM == 0) exchange_half_pad<A, B, HB>(v, s, tid);
        else if constexpr (FORM == 1) exchange_half_lin<A, B, HB, 1, false>(v, s, tid);
        else exchange_half_lin<A, B, HB>(v, s, tid);
    }
    if (check) {
#pragma unroll
        for (int r = 0; r < 64; ++r) out[((size_t)blockIdx.x * 512 + tid) * 64 + r] = v[r];
    } else {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < 64; ++r) acc += v[r];
        if (acc == -1.0f) out[0] = acc;  // never: the sums are of non-negative indices
    }
}

template <Lay A, Lay B, int HB, int FORM>
static double run_form(const char* pair, float* out, int tiles, int blocks, double mhz, bool& ok) {
    const size_t smem = sizeof(float) * kLinBudget;
    auto k = k_exch<A, B, HB, FORM>;
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    // one exchange, checked against layout B
    hipLaunchKernelGGL(k, dim3(2), dim3(512), smem, 0, out, 1, 1);
    CK(hipDeviceSynchronize());
    std::vector<float> h(2 * 512 * 64);
    CK(hipMemcpy(h.data(), out, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    int bad = 0;
    for (int b = 0; b < 2; ++b)
        for (uint32_t t = 0; t < 512; ++t)
            for (int r = 0; r < 64; ++r)
                if (h[((size_t)b * 512 + t) * 64 + r] != (float)(lay_base(B, t) | lay_off(B, r))) ++bad;
    if (bad) { ok = false; printf("%-8s form %c: %d of %zu registers WRONG\n", pair, 'a' + FORM, bad, h.size()); return 0; }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), smem, 0, out, tiles / 10 + 1, 0);  // warm-up
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(k, dim3(blocks), dim3(512), smem, 0, out, tiles, 0);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    // two blocks per CU share one LDS: per CU, 2 * tiles exchanges in `best`
    const double ns = best * 1e6 / (2.0 * tiles);
    printf("%-8s form %c: %8.1f ns = %7.0f cycles per exchange per tile (per CU; best of 5, %.3f ms)\n", pair,
           'a' + FORM, ns, ns * mhz * 1e-3, best);
    return ns;
}

// shader clock while the LDS pipe is busy: s_memtime against the 100 MHz wall clock
__global__ void k_clock(long long* o, int n) {
    __shared__ float s[64];
    const long long c0 = clock64(), w0 = wall_clock64();
    float a = (float)threadIdx.x;
    for (int i = 0; i < n; ++i) { s[threadIdx.x] = a; __syncthreads(); a += s[(threadIdx.x + 1) & 63]; __syncthreads(); }
    const long long c1 = clock64(), w1 = wall_clock64();
    if (threadIdx.x == 0) { o[0] = c1 - c0; o[1] = w1 - w0; o[2] = (long long)a; }
}

template <Lay A, Lay B, int HB>
static void run_pair(const char* pair, float* out, int tiles, int blocks, double mhz, bool& ok) {
    const double a = run_form<A, B, HB, 0>(pair, out, tiles, blocks, mhz, ok);
    const double b = run_form<A, B, HB, 1>(pair, out, tiles, blocks, mhz, ok);
    if (a > 0 && b > 0) printf("%-8s (b) / (a) = %.3f\n", pair, b / a);
    if (lin_width(A, B) == 4) {
        const double c = run_form<A, B, HB, 2>(pair, out, tiles, blocks, mhz, ok);
        if (a > 0 && c > 0) printf("%-8s (c) / (a) = %.3f\n", pair, c / a);
    } else {
        printf("%-8s form c: no contiguous runs in the destination, as (b)\n", pair);
    }
}

int main(int argc, char** argv) {
    const int tiles = argc > 1 ? atoi(argv[1]) : 2000;
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    const int blocks = 2 * p.multiProcessorCount;
    float* out;
    CK(hipMalloc(&out, sizeof(float) * 2 * 512 * 64));
    long long* clk;
    CK(hipMalloc(&clk, 3 * sizeof(long long)));
    hipLaunchKernelGGL(k_clock, dim3(1), dim3(64), 0, 0, clk, 200000);
    long long hc[3];
    CK(hipMemcpy(hc, clk, sizeof(hc), hipMemcpyDeviceToHost));
    int wall_khz = 100000;
    CK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0));
    const double mhz_meas = (double)hc[0] / (double)hc[1] * wall_khz * 1e-3;
    const double mhz = p.clockRate * 1e-3;
    printf("%s (%s), %d CUs, %d blocks of 512 threads, %d tiles per block\n", p.name, p.gcnArchName,
           p.multiProcessorCount, blocks, tiles);
    printf("cycles at the device's peak clock, %.0f MHz (s_memtime / wall clock of a one-wave loop: %.0f MHz)\n", mhz,
           mhz_meas);
    bool ok = true;
    constexpr Lay L3{15, 5, 6, 7, 8, 9, 10}, L4{15, 11, 12, 13, 14, 9, 10}, L5{15, 0, 1, 2, 3, 4, 10};
    constexpr Lay C1{15, 0, 1, 2, 3, 4, 5}, C2{15, 11, 12, 13, 14, 9, 5}, C3{15, 6, 7, 8, 9, 10, 5};
    run_pair<L3, L4, 10>("L3->L4", out, tiles, blocks, mhz, ok);
    run_pair<L4, L5, 10>("L4->L5", out, tiles, blocks, mhz, ok);
    run_pair<C1, C2, 5>("C1->C2", out, tiles, blocks, mhz, ok);
    run_pair<C2, C3, 5>("C2->C3", out, tiles, blocks, mhz, ok);
    // RowA2Set (k_enc_rowA2) and DecC2Set (k_dec_rowC2)
    constexpr Lay A1{15, 0, 1, 11, 12, 13, 14}, A2{15, 2, 3, 4, 5, 6, 14}, A3{15, 10, 7, 8, 9, 6, 14};
    constexpr Lay B1{15, 0, 1, 7, 8, 9, 10}, B2{15, 2, 3, 4, 5, 6, 10}, B3{15, 0, 1, 11, 12, 13, 10},
                  B4{15, 0, 1, 14, 11, 12, 10};
    run_pair<A1, A2, 14>("A1->A2", out, tiles, blocks, mhz, ok);
    run_pair<A2, A3, 14>("A2->A3", out, tiles, blocks, mhz, ok);
    run_pair<B1, B2, 10>("B1->B2", out, tiles, blocks, mhz, ok);
    run_pair<B2, B3, 10>("B2->B3", out, tiles, blocks, mhz, ok);
    run_pair<B3, B4, 10>("B3->B4", out, tiles, blocks, mhz, ok);
    CK(hipFree(out)); CK(hipFree(clk));
    return ok ? 0 : 1;
}
