// KNNGroup's coordinate arithmetic (models/layers/group.py:310-315): gather the neighbours' coordinates, subtract the
// query, and -- with normalize_dp -- divide every cloud by the largest neighbour offset length found in it.
//
//   dp[b, :, q, j] = support[b, idx[b, q, j], :] (- query[b, q, :])
//   dp[b]         /= max over (q, j) of sqrt((x*x + y*y) + z*z)
//
// The norm is written exactly so (fp32, no contraction, IEEE root and quotient).  The per-cloud maximum is an integer
// atomicMax on the bit pattern of the norms: they are non-negative, so the integer order is the float order, and a
// maximum does not depend on the order of its operands -- the same bits on every run, no float atomic.
#include "common.h"

namespace amc {

constexpr int KGD_THREADS = 256;

// lanes run along the flattened (query, neighbour) pair e: idx is read and each of the three dp planes written as 64
// consecutive words per wave; the support rows are the only scattered access (12 bytes each, L2-resident clouds).
__global__ __launch_bounds__(KGD_THREADS) void knn_group_dp_kernel(int n, int m, int k, const float *__restrict__ support,
                                                                   const float *__restrict__ query,
                                                                   const int *__restrict__ idx, int relative,
                                                                   float *__restrict__ dp, int *__restrict__ cloud_max)
{
    __shared__ int wave_max[KGD_THREADS / 64];
    const int bi = blockIdx.y;
    const size_t mk = (size_t)m * k;
    const unsigned e = blockIdx.x * KGD_THREADS + threadIdx.x;  // m * k < 2^31 (checked by the entry): 32-bit division
    int bits = 0;
    if (e < mk) {
        const int q = (int)(e / (unsigned)k);
        int i = idx[(size_t)bi * mk + e];
        i = min(max(i, 0), n - 1);  // a foreign index must not read outside the cloud
        const float *s = support + ((size_t)bi * n + i) * 3;
        float x = s[0], y = s[1], z = s[2];
        if (relative) {
            const float *c = query + ((size_t)bi * m + q) * 3;
            x = __fsub_rn(x, c[0]); y = __fsub_rn(y, c[1]); z = __fsub_rn(z, c[2]);
        }
        float *o = dp + (size_t)bi * 3 * mk + e;
        o[0] = x; o[mk] = y; o[2 * mk] = z;
        if (cloud_max) {
            const float r = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
            bits = __float_as_int(r);
        }
    }
    if (!cloud_max) return;  // uniform
    for (int s = 32; s > 0; s >>= 1) bits = max(bits, __shfl_xor(bits, s, 64));
    if (lane_id() == 0) wave_max[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < KGD_THREADS / 64; ++w) bits = max(bits, wave_max[w]);
        atomicMax(cloud_max + bi, bits);
    }
}

__global__ __launch_bounds__(KGD_THREADS) void knn_group_scale_kernel(size_t per_cloud, float *__restrict__ dp,
                                                                      const int *__restrict__ cloud_max)
{
    const size_t e = (size_t)blockIdx.x * KGD_THREADS + threadIdx.x;
    if (e >= per_cloud) return;
    const float s = __int_as_float(cloud_max[blockIdx.y]);
    float *o = dp + (size_t)blockIdx.y * per_cloud + e;
    *o = *o / s;  // IEEE quotient (hipcc rounds fp32 division and sqrtf correctly by default; __fsqrt_rn is the native approximation)
}

}  // namespace amc

using namespace amc;

AMC_API int amc3d_knn_group_dp(int b, int n, int m, int k, const float *support, const float *query, const int *idx,
                               int relative, int normalize, float *dp, float *cloud_max, void *stream_)
{
    if (b <= 0 || m <= 0 || k <= 0) return 0;
    const long lim = 0x7fffffffL;
    if (n <= 0 || b > 65535 || (long)b * n > lim || (long)b * m > lim || (long)b * m * k > lim || 3L * m * k > lim)
        return bad_arg("amc3d_knn_group_dp: sizes out of range");
    if (!support || !idx || !dp || (relative && !query) || (normalize && !cloud_max))
        return bad_arg("amc3d_knn_group_dp: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t mk = (size_t)m * k;
    int *cmax = normalize ? (int *)cloud_max : nullptr;
    if (cmax)
        if (int st = fill_i32(cmax, 0, (size_t)b, stream)) return st;
    hipLaunchKernelGGL(knn_group_dp_kernel, dim3(div_up((long)mk, KGD_THREADS), b), dim3(KGD_THREADS), 0, stream, n, m, k,
                       support, query, idx, relative, dp, cmax);
    if (cmax)
        hipLaunchKernelGGL(knn_group_scale_kernel, dim3(div_up(3L * (long)mk, KGD_THREADS), b), dim3(KGD_THREADS), 0, stream,
                           3 * mk, dp, (const int *)cmax);
    return launch_status("amc3d_knn_group_dp");
}
