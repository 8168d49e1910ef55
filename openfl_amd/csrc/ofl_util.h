// ofl_util.h -- small helpers shared by the kernel sources: host-side ones, and
// the device's bfloat16 widen / round.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <map>
#include <mutex>

namespace ofl_util {

// f() once per device (kernel attributes, __constant__ uploads are
// per-device state); the result is remembered per device.  Each call site
// (lambda type) has its own table.
template <typename F>
hipError_t per_device_once(F f) {
    static std::mutex mu;
    static std::map<int, hipError_t> done;
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    auto it = done.find(dev);
    if (it != done.end()) return it->second;
    const hipError_t r = f();
    done[dev] = r;
    return r;
}

// runs f() when the scope ends, on every return path
template <typename F>
struct ScopeExit {
    F f;
    explicit ScopeExit(F fn) : f(fn) {}
    ~ScopeExit() { f(); }
    ScopeExit(const ScopeExit&) = delete;
    ScopeExit& operator=(const ScopeExit&) = delete;
};

}  // namespace ofl_util

#if defined(__HIPCC__)  // device code: the .hip sources
namespace ofl {
// bfloat16 <-> float32 on the device, one copy for every kernel source.
// float32 bits -> bf16 bits, round to nearest even: the carry of the rounding
// runs into the exponent (0x7f7fffff -> +inf), +-0, +-inf and denormals follow
// by the same rule; a NaN keeps its sign and stays one (the quiet bit is set:
// its top 7 mantissa bits may all be 0)
__device__ __forceinline__ uint32_t bf16_rne(uint32_t u) {
    const uint32_t r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7fffffffu) > 0x7f800000u ? (u >> 16) | 0x40u : r;
}
// a 32-bit word holds two bf16 elements; widening is exact
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }  // the element at the lower address
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) {
    return bf16_rne(__float_as_uint(lo)) | (bf16_rne(__float_as_uint(hi)) << 16);
}
}  // namespace ofl
#endif

namespace ofl {
// f(0..n-1) on the caller and at least `workers` threads of a persistent
// native pool (csrc/serial_sum.cpp); false when every pool is busy with
// another caller (then nothing ran)
bool pool_run(int n, int workers, const std::function<void(int)>& f);
// exact serial float32 sum (csrc/serial_sum.cpp): s <- fl(s + x[i]) left to
// right, evaluated on up to nthreads threads (<= 0: the default); dst (or
// NULL) receives a copy of x, after which after_copy(ctx) (or NULL) runs on
// the calling thread while the sum goes on
float serial_sum_f32_mt_cb(const float* x, int64_t n, float* dst, int nthreads, void (*after_copy)(void*), void* ctx);
}  // namespace ofl
