// Device helpers of the ragged-batch input code (room_input.hip, scannet_input.hip, voxel.hip): the room of an element, the
// rounding-explicit arithmetic for a coordinate type C = float or double, and the three-minima workgroup reduction.
#pragma once
#include "common.h"

namespace amc {

// the last room whose first element is <= i (tab: rooms + 1 ascending entries: points in offsets, voxels in vbase)
template <typename I>
__device__ __forceinline__ int room_seg(int rooms, const I *__restrict__ tab, I i)
{
    int lo = 0, hi = rooms - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float min_c(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double min_c(double a, double b) { return fmin(a, b); }

// the bit pattern of a value >= +0 as a radix key: non-negative floats and doubles order like their patterns
__device__ __forceinline__ unsigned order_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned long long order_bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// above every coordinate: where a minimum starts
template <typename C>
constexpr C kHuge = C(sizeof(C) == 4 ? 3.4e38 : 1.7e308);

// three minima of a workgroup of kThreads threads -> out[0..2] (written by threads 0..2; global or LDS: the caller
// synchronises before reading it).  s: kThreads / 64 rows of LDS.  min is exact, so the order of the fold does not matter
template <typename C, int kThreads>
__device__ __forceinline__ void block_min3(C mn[3], C (*s)[3], C *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = min_c(mn[j], __shfl_xor(mn[j], d, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s[wave][j] = mn[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        C v = s[0][threadIdx.x];
        for (int w = 1; w < kThreads / 64; ++w) v = min_c(v, s[w][threadIdx.x]);
        out[threadIdx.x] = v;
    }
}

}  // namespace amc
