// Shared helpers for libevreal_hip.so (gfx950 only; no CUDA/portable paths by design).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "evreal_hip.h"

namespace evr {
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int hip_fail(hipError_t e, const char* what, const char* file, int line);
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace evr

#define EVR_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) return evr::hip_fail(e_, #call, __FILE__, __LINE__);     \
    } while (0)
#define EVR_REQUIRE(cond, ...)                  \
    do {                                        \
        if (!(cond)) {                          \
            evr::set_error(__VA_ARGS__);        \
            return EVR_ERR_INVALID;             \
        }                                       \
    } while (0)
#define EVR_LAUNCH_CHECK() EVR_HIP(hipGetLastError())
// a call's workspace `ws` of `bytes` must exist and hold `need` bytes; `what` names the entry point (a string)
#define EVR_REQUIRE_WORKSPACE(what, ws, bytes, need)                                                        \
    do {                                                                                                    \
        if (!(ws) || (size_t)(bytes) < (size_t)(need)) {                                                    \
            evr::set_error("%s: workspace %zu B < required %zu B", what, (size_t)(bytes), (size_t)(need));  \
            return EVR_ERR_WORKSPACE;                                                                       \
        }                                                                                                   \
    } while (0)

namespace evr {
// a host vector into a device allocation of its own (weights, biases, tables: made once per handle)
template <typename T>   // float, unsigned, double
inline int upload(const std::vector<T>& h, T** d) {
    EVR_HIP(hipMalloc((void**)d, h.size() * sizeof(T) + 64));
    EVR_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return EVR_OK;
}
}  // namespace evr

// wave64 helpers
__device__ __forceinline__ int evr_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ double evr_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // valid in lane 0
}
__device__ __forceinline__ float evr_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
