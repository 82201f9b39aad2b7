// Separable neighbourhood aggregation (ASSA, models/layers/local_aggregation.py:127-131) without the x nsample tensors:
//   out[b, d*C + c, m] = red_k ( dp[b,d,m,k] * f[b,c,idx[b,m,k]] )     d in 0..2, red in {mean, sum, max}
// The reference expands the grouped features to (b,3,C,npoints,nsample), multiplies by dp and reduces; here a lane owns a
// channel, gathers the neighbour's contiguous C-float row from the POINT-major features f_pm (b,n,C) and keeps the three
// running reductions in registers.  Arithmetic (part of the contract, see include/amc3d.h): __fmul_rn per product,
// sequential __fadd_rn in ascending k from +0.0f, one __fdiv_rn by float(nsample) for the mean, first maximum (first NaN) for max.
//
// Work split: CL = 16 / 32 / 64 lanes along c (the smallest that covers C, else chunks of 64), 64 / CL queries per wave, so
// the narrow ASSANet widths (C = ceil(width / 3)) do not idle three quarters of a wave.  idx / dp of a query are the same
// address in every lane of its group: one broadcast transaction each.  The forward's output is channel-major (b,3C,npoints):
// a workgroup collects a tile of ASSA_TM queries in LDS and stores it with the lanes along npoints.
// Backward: the gradient arrives as rows g_pm (b,npoints,3C) (amc3d_transpose_cn by the caller) and leaves as rows df_pm
// (b,n,C); either float atomics of one C-float row segment per (query, neighbour) or a gather over the reverse lists.
#include "common.h"

namespace amc {

constexpr int ASSA_TM = 32;  // queries per workgroup of the forward (LDS tile 3 x CL x 33 floats: 25 KB at CL = 64)

enum { ASSA_MEAN = 0, ASSA_SUM = 1, ASSA_MAX = 2 };

__device__ __forceinline__ int assa_clamp(int v, int hi) { return min(max(v, 0), hi); }

// torch.max's rule: a later product replaces the kept one when it compares greater, or when it is the first NaN (a NaN
// is kept from then on, so a diverging run shows in the output as it does in the reference)
__device__ __forceinline__ bool assa_later_max(float p, float kept) { return p > kept || (p != p && kept == kept); }

template <int CL, int RED>
__global__ __launch_bounds__(256) void assa_forward_kernel(int C, int N, int M, int K, const float *__restrict__ f_pm,
                                                           const int *__restrict__ idx, const float *__restrict__ dp,
                                                           float *__restrict__ out, unsigned char *__restrict__ arg_pm)
{
    constexpr int QW = 64 / CL;  // queries a wave works on at once
    __shared__ float tile[3][CL][ASSA_TM + 1];
    const int b = blockIdx.z, c0 = blockIdx.y * CL, m0 = blockIdx.x * ASSA_TM;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ql = lane / CL, cl = lane % CL, c = c0 + cl;
    const bool has_c = c < C;
    const float *fb = f_pm + (size_t)b * N * C + (has_c ? c : 0);
    const size_t P = (size_t)M * K;
    for (int it = 0; it < ASSA_TM / (4 * QW); ++it) {
        const int q = (it * 4 + wave) * QW + ql, m = m0 + q;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        int a0 = 0, a1 = 0, a2 = 0;
        if (m < M) {
            const int *ip = idx + ((size_t)b * M + m) * K;
            const float *d0 = dp + (size_t)b * 3 * P + (size_t)m * K, *d1 = d0 + P, *d2 = d1 + P;
            for (int k0 = 0; k0 < K; k0 += 4) {  // four neighbours' loads in flight; the reductions keep ascending k
                int j[4];
                float v[4], x[4], y[4], z[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = min(k0 + u, K - 1);
                    j[u] = assa_clamp(ip[k], N - 1);
                    x[u] = d0[k]; y[u] = d1[k]; z[u] = d2[k];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = has_c ? fb[(size_t)j[u] * C] : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u;
                    if (k < K) {
                        const float p0 = __fmul_rn(x[u], v[u]), p1 = __fmul_rn(y[u], v[u]), p2 = __fmul_rn(z[u], v[u]);
                        if (RED == ASSA_MAX) {
                            if (k == 0 || assa_later_max(p0, r0)) { r0 = p0; a0 = k; }
                            if (k == 0 || assa_later_max(p1, r1)) { r1 = p1; a1 = k; }
                            if (k == 0 || assa_later_max(p2, r2)) { r2 = p2; a2 = k; }
                        } else {
                            r0 = __fadd_rn(r0, p0); r1 = __fadd_rn(r1, p1); r2 = __fadd_rn(r2, p2);
                        }
                    }
                }
            }
            if (RED == ASSA_MEAN) {
                const float kf = (float)K;
                r0 = __fdiv_rn(r0, kf); r1 = __fdiv_rn(r1, kf); r2 = __fdiv_rn(r2, kf);
            }
            if (RED == ASSA_MAX && arg_pm && has_c) {
                unsigned char *ap = arg_pm + ((size_t)b * M + m) * 3 * C + c;
                ap[0] = (unsigned char)a0; ap[C] = (unsigned char)a1; ap[2 * C] = (unsigned char)a2;
            }
        }
        tile[0][cl][q] = r0; tile[1][cl][q] = r1; tile[2][cl][q] = r2;
    }
    __syncthreads();
    // channel-major store: 32 consecutive queries of one output channel per half wave
    const int ml = threadIdx.x % ASSA_TM, row = threadIdx.x / ASSA_TM, m = m0 + ml;
    if (m >= M) return;
    for (int r = row; r < 3 * CL; r += 256 / ASSA_TM) {
        const int d = r / CL, c2 = c0 + r % CL;
        if (c2 < C) out[((size_t)b * 3 * C + (size_t)d * C + c2) * M + m] = tile[d][r % CL][ml];
    }
}

// the term of edge (m,k) for channel c (include/amc3d.h): mean / sum: s * ((dp0*g0 + dp1*g1) + dp2*g2); max: the same sum
// over the d whose stored arg-max is k, the others +0.0f
template <int RED>
__device__ __forceinline__ float assa_term(float x, float y, float z, float g0, float g1, float g2, int a0, int a1, int a2, int k,
                                           float s)
{
    if (RED == ASSA_MAX) {
        const float t0 = a0 == k ? __fmul_rn(x, g0) : 0.f, t1 = a1 == k ? __fmul_rn(y, g1) : 0.f,
                    t2 = a2 == k ? __fmul_rn(z, g2) : 0.f;
        return __fadd_rn(__fadd_rn(t0, t1), t2);
    }
    return __fmul_rn(s, __fadd_rn(__fadd_rn(__fmul_rn(x, g0), __fmul_rn(y, g1)), __fmul_rn(z, g2)));
}

// scatter with float atomics: a lane group adds one row segment of min(C, CL) floats per (query, neighbour)
template <int CL, int RED>
__global__ __launch_bounds__(256) void assa_backward_atomic_kernel(int C, int N, int M, int K, float s,
                                                                   const float *__restrict__ g_pm, const int *__restrict__ idx,
                                                                   const float *__restrict__ dp,
                                                                   const unsigned char *__restrict__ arg_pm,
                                                                   float *__restrict__ df_pm)
{
    constexpr int QW = 64 / CL;
    const int b = blockIdx.z, c = blockIdx.y * CL + (threadIdx.x & 63) % CL;
    const int m = blockIdx.x * (4 * QW) + (threadIdx.x >> 6) * QW + (threadIdx.x & 63) / CL;
    if (m >= M || c >= C) return;
    const size_t P = (size_t)M * K, row = ((size_t)b * M + m) * 3 * C + c;
    const float g0 = g_pm[row], g1 = g_pm[row + C], g2 = g_pm[row + 2 * C];
    int a0 = 0, a1 = 0, a2 = 0;
    if (RED == ASSA_MAX) { a0 = arg_pm[row]; a1 = arg_pm[row + C]; a2 = arg_pm[row + 2 * C]; }
    const int *ip = idx + ((size_t)b * M + m) * K;
    const float *d0 = dp + (size_t)b * 3 * P + (size_t)m * K, *d1 = d0 + P, *d2 = d1 + P;
    float *dfb = df_pm + (size_t)b * N * C + c;
    for (int k = 0; k < K; ++k) {
        if (RED == ASSA_MAX && a0 != k && a1 != k && a2 != k) continue;
        const int j = ip[k];
        if (j < 0 || j >= N) continue;
        atomicAdd(dfb + (size_t)j * C, assa_term<RED>(d0[k], d1[k], d2[k], g0, g1, g2, a0, a1, a2, k, s));
    }
}

// gather over the reverse lists: a lane group owns one support point and adds its incoming edges in list order
template <int CL, int RED>
__global__ __launch_bounds__(256) void assa_backward_csr_kernel(int C, int N, int M, int K, long G, float s,
                                                                const float *__restrict__ g_pm, const float *__restrict__ dp,
                                                                const unsigned char *__restrict__ arg_pm,
                                                                const int *__restrict__ rev_start,
                                                                const int *__restrict__ rev_edge, float *__restrict__ df_pm)
{
    constexpr int QW = 64 / CL;
    const int c = blockIdx.y * CL + (threadIdx.x & 63) % CL;
    const long g = (long)blockIdx.x * (4 * QW) + (threadIdx.x >> 6) * QW + (threadIdx.x & 63) / CL;
    if (g >= G || c >= C) return;
    const long b = g / N;
    const long P = (long)M * K, E = (long)(G / N) * P;
    const int e0 = (int)min((long)max(rev_start[g], 0), E), e1 = (int)min((long)max(rev_start[g + 1], e0), E);
    const float *d0 = dp + (size_t)b * 3 * P, *d1 = d0 + P, *d2 = d1 + P;
    const float *gb = g_pm + (size_t)b * M * 3 * C + c;
    const unsigned char *ab = RED == ASSA_MAX ? arg_pm + (size_t)b * M * 3 * C + c : nullptr;
    float acc = 0.f;
    for (int i = e0; i < e1; i += 4) {  // four edges' loads in flight; the sum keeps the list order
        int p[4];
        float x[4], y[4], z[4], g0[4], g1[4], g2[4];
        int a0[4], a1[4], a2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = (int)min((long)max(rev_edge[min(i + u, e1 - 1)], 0), P - 1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t row = (size_t)(p[u] / K) * 3 * C;
            x[u] = d0[p[u]]; y[u] = d1[p[u]]; z[u] = d2[p[u]];
            g0[u] = gb[row]; g1[u] = gb[row + C]; g2[u] = gb[row + 2 * C];
            if (RED == ASSA_MAX) { a0[u] = ab[row]; a1[u] = ab[row + C]; a2[u] = ab[row + 2 * C]; }
            else { a0[u] = a1[u] = a2[u] = 0; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u < e1)
                acc = __fadd_rn(acc, assa_term<RED>(x[u], y[u], z[u], g0[u], g1[u], g2[u], a0[u], a1[u], a2[u], p[u] % K, s));
    }
    df_pm[(size_t)g * C + c] = acc;
}

static int assa_check(const char *what, int b, int c, int n, int npoints, int nsample, int reduction)
{
    if (c <= 0 || n <= 0 || npoints <= 0 || nsample <= 0 || nsample > 255 || b > 65535 || reduction < ASSA_MEAN ||
        reduction > ASSA_MAX || (long)b * npoints * nsample >= (1L << 31) || (long)b * n >= (1L << 31) ||
        (long)b * npoints * 3 * c >= (1L << 40) || (long)b * n * c >= (1L << 40))
        return bad_arg(what);
    return 0;
}

#define ASSA_BY_RED(KERNEL, CL_, ...)                                                                              \
    do {                                                                                                           \
        if (reduction == ASSA_MEAN) hipLaunchKernelGGL((KERNEL<CL_, ASSA_MEAN>), grid, dim3(256), 0, stream, __VA_ARGS__); \
        else if (reduction == ASSA_SUM) hipLaunchKernelGGL((KERNEL<CL_, ASSA_SUM>), grid, dim3(256), 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<CL_, ASSA_MAX>), grid, dim3(256), 0, stream, __VA_ARGS__);                 \
    } while (0)

static int assa_lanes(int c) { return c <= 16 ? 16 : (c <= 32 ? 32 : 64); }

}  // namespace amc

using namespace amc;

AMC_API int amc3d_assa_aggregate_forward(int b, int c, int n, int npoints, int nsample, int reduction, const float *f_pm,
                                         const int *idx, const float *dp, float *out, unsigned char *arg_pm, void *stream_)
{
    if (b <= 0) return 0;
    if (assa_check("amc3d_assa_aggregate_forward: bad argument", b, c, n, npoints, nsample, reduction)) return (int)hipErrorInvalidValue;
    if (!f_pm || !idx || !dp || !out || (reduction == ASSA_MAX && !arg_pm)) return bad_arg("amc3d_assa_aggregate_forward: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const int cl = assa_lanes(c);
    const dim3 grid(div_up(npoints, ASSA_TM), div_up(c, cl), b);
    if (cl == 16) ASSA_BY_RED(assa_forward_kernel, 16, c, n, npoints, nsample, f_pm, idx, dp, out, arg_pm);
    else if (cl == 32) ASSA_BY_RED(assa_forward_kernel, 32, c, n, npoints, nsample, f_pm, idx, dp, out, arg_pm);
    else ASSA_BY_RED(assa_forward_kernel, 64, c, n, npoints, nsample, f_pm, idx, dp, out, arg_pm);
    return launch_status("amc3d_assa_aggregate_forward");
}

AMC_API int amc3d_assa_aggregate_backward(int b, int c, int n, int npoints, int nsample, int reduction, const float *g_pm,
                                          const int *idx, const float *dp, const unsigned char *arg_pm, float *df_pm, void *stream_)
{
    if (b <= 0) return 0;
    if (assa_check("amc3d_assa_aggregate_backward: bad argument", b, c, n, npoints, nsample, reduction)) return (int)hipErrorInvalidValue;
    if (!g_pm || !idx || !dp || !df_pm || (reduction == ASSA_MAX && !arg_pm)) return bad_arg("amc3d_assa_aggregate_backward: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const int st = fill_i32((int *)df_pm, 0, (size_t)b * n * c, stream);  // unreferenced support points: exact zeros
    if (st) return st;
    const float s = reduction == ASSA_MEAN ? 1.0f / (float)nsample : 1.0f;
    const int cl = assa_lanes(c);
    const dim3 grid(div_up(npoints, 4 * (64 / cl)), div_up(c, cl), b);
    if (cl == 16) ASSA_BY_RED(assa_backward_atomic_kernel, 16, c, n, npoints, nsample, s, g_pm, idx, dp, arg_pm, df_pm);
    else if (cl == 32) ASSA_BY_RED(assa_backward_atomic_kernel, 32, c, n, npoints, nsample, s, g_pm, idx, dp, arg_pm, df_pm);
    else ASSA_BY_RED(assa_backward_atomic_kernel, 64, c, n, npoints, nsample, s, g_pm, idx, dp, arg_pm, df_pm);
    return launch_status("amc3d_assa_aggregate_backward");
}

AMC_API int amc3d_assa_aggregate_backward_csr(int b, int c, int n, int npoints, int nsample, int reduction, const float *g_pm,
                                              const float *dp, const unsigned char *arg_pm, const int *rev_start,
                                              const int *rev_edge, float *df_pm, void *stream_)
{
    if (b <= 0) return 0;
    if (assa_check("amc3d_assa_aggregate_backward_csr: bad argument", b, c, n, npoints, nsample, reduction)) return (int)hipErrorInvalidValue;
    if (!g_pm || !dp || !rev_start || !rev_edge || !df_pm || (reduction == ASSA_MAX && !arg_pm))
        return bad_arg("amc3d_assa_aggregate_backward_csr: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const float s = reduction == ASSA_MEAN ? 1.0f / (float)nsample : 1.0f;
    const long G = (long)b * n;
    const int cl = assa_lanes(c);
    const dim3 grid(div_up(G, 4 * (64 / cl)), div_up(c, cl), 1);
    if (cl == 16) ASSA_BY_RED(assa_backward_csr_kernel, 16, c, n, npoints, nsample, G, s, g_pm, dp, arg_pm, rev_start, rev_edge, df_pm);
    else if (cl == 32) ASSA_BY_RED(assa_backward_csr_kernel, 32, c, n, npoints, nsample, G, s, g_pm, dp, arg_pm, rev_start, rev_edge, df_pm);
    else ASSA_BY_RED(assa_backward_csr_kernel, 64, c, n, npoints, nsample, G, s, g_pm, dp, arg_pm, rev_start, rev_edge, df_pm);
    return launch_status("amc3d_assa_aggregate_backward_csr");
}
