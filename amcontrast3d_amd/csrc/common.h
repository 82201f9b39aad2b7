// Shared helpers for the gfx950 kernels (wave64 only; no dual paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/amc3d.h"

#define AMC_API extern "C" __attribute__((visibility("default")))

namespace amc {

constexpr int kWave = 64;

void set_error(const char *fmt, ...);

// launch epilogue: pick up a launch-configuration error without synchronising
inline int launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

inline int bad_arg(const char *what)
{
    set_error("%s", what);
    return (int)hipErrorInvalidValue;
}

inline int div_up(long a, long b) { return (int)((a + b - 1) / b); }

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }  // workspace sections start on 256-byte boundaries

// The reference's squared distance, evaluated as written (no contraction):
// (qx-x)*(qx-x) + (qy-y)*(qy-y) + (qz-z)*(qz-z)
__device__ __forceinline__ float dist2_ref(float qx, float qy, float qz, float x, float y, float z)
{
    const float dx = __fsub_rn(qx, x), dy = __fsub_rn(qy, y), dz = __fsub_rn(qz, z);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ double dist2_ref(double qx, double qy, double qz, double x, double y, double z)
{
    const double dx = __dsub_rn(qx, x), dy = __dsub_rn(qy, y), dz = __dsub_rn(qz, z);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Zero-fill as an ordinary kernel.  The library never uses hipMemsetAsync: under hipGraph replay a
// memset node was observed to race with the kernels captured after it on ROCm 7.2 (stale counters ->
// out-of-range scatter), whereas kernel nodes of one captured stream always run in order.
__global__ void fill_i32_kernel(int *__restrict__ p, int value, size_t count);
int fill_i32(int *p, int value, size_t count, hipStream_t stream);

// the dp columns W_dp (cout,3) of a neighbourhood layer's weight [W_dp | W_f] where they lie: row c at p + c * ld (ld = 3 for a
// contiguous copy, cin + 3 inside the layer's own weight matrix)
struct WDp {
    const float *p;
    long ld;
    __host__ __device__ explicit operator bool() const { return p != nullptr; }
    __device__ __forceinline__ float at(int c, int j) const { return p[c * ld + j]; }
};

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// number of set bits of `mask` below this lane
__device__ __forceinline__ int mbcnt(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

}  // namespace amc
