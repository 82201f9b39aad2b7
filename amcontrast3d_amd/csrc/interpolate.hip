// three_nn / three_interpolate (+grad) for gfx950.
// Reference: pointnet2_batch/src/interpolate_gpu.cu:16-59, 84-104, 127-149.
#include "common.h"
#include "grid_search.h"

namespace amc {

constexpr int NN_TILE = 512;  // known points per LDS tile
constexpr int NN_THREADS = 256;

// One thread per unknown point keeps its 3 best (strict '<' cascade, so the
// earlier index wins equal distances, exactly as the reference).  The reference
// holds the best distances in double; a double that only ever takes fp32 values
// (or the initial 1e40, which no fp32 exceeds and which casts to +inf on
// output) compares identically to fp32 with +inf as the initial value, so the
// fp64 pipe is not needed.  Known points are staged per workgroup in LDS as
// float4 and read as wave-wide broadcasts (one ds_read_b128 per candidate).
__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(int n, int m,
                                                              const float *__restrict__ unknown,
                                                              const float *__restrict__ known,
                                                              float *__restrict__ dist2, int *__restrict__ idx)
{
    __shared__ float4 tile[NN_TILE];
    const int bs = blockIdx.y;
    const int pt = blockIdx.x * NN_THREADS + threadIdx.x;
    const bool live = pt < n;
    const float *u = unknown + ((size_t)bs * n + (live ? pt : 0)) * 3;
    const float ux = u[0], uy = u[1], uz = u[2];
    const float *K = known + (size_t)bs * m * 3;

    const float inf = __builtin_inff();
    float best1 = inf, best2 = inf, best3 = inf;
    int besti1 = 0, besti2 = 0, besti3 = 0;

    for (int t0 = 0; t0 < m; t0 += NN_TILE) {
        const int tn = min(NN_TILE, m - t0);
        __syncthreads();
        for (int i = threadIdx.x; i < tn; i += NN_THREADS) {
            const float *p = K + (size_t)(t0 + i) * 3;
            tile[i] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        for (int k = 0; k < tn; ++k) {
            const float4 p = tile[k];
            const float d = dist2_ref(ux, uy, uz, p.x, p.y, p.z);
            if (d < best3) {  // rare after warm-up; the cascade below is the reference's
                const int kk = t0 + k;
                if (d < best1) {
                    best3 = best2; besti3 = besti2;
                    best2 = best1; besti2 = besti1;
                    best1 = d; besti1 = kk;
                } else if (d < best2) {
                    best3 = best2; besti3 = besti2;
                    best2 = d; besti2 = kk;
                } else {
                    best3 = d; besti3 = kk;
                }
            }
        }
    }
    if (live) {
        float *od = dist2 + ((size_t)bs * n + pt) * 3;
        int *oi = idx + ((size_t)bs * n + pt) * 3;
        od[0] = best1; od[1] = best2; od[2] = best3;
        oi[0] = besti1; oi[1] = besti2; oi[2] = besti3;
    }
}

// out[b,c,p] = w0*points[b,c,i0] + w1*points[b,c,i1] + w2*points[b,c,i2], evaluated
// left to right without contraction (interpolate_gpu.cu:103).  One thread per
// (b,p) keeps idx/weight in registers and walks the channels: coalesced stores.
// `base` (optional, (b,c,n)): out = base + interpolation -- the skip branch of a FeaturePropagation conv applied before
// the interpolation (W . [f1 ; up(f2)] = W1 . f1 + up(W2 . f2): the interpolation is linear and commutes with the 1x1 conv)
__global__ void three_interpolate_kernel(int c, int m, int n, int ch_per, const float *__restrict__ points,
                                         const int *__restrict__ idx, const float *__restrict__ weight,
                                         const float *__restrict__ base, float *__restrict__ out)
{
    const int bs = blockIdx.y;
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= n) return;
    const int *ii = idx + ((size_t)bs * n + pt) * 3;
    const float *ww = weight + ((size_t)bs * n + pt) * 3;
    const int i0 = ii[0], i1 = ii[1], i2 = ii[2];
    const float w0 = ww[0], w1 = ww[1], w2 = ww[2];
    const float *src = points + (size_t)bs * c * m;
    float *dst = out + (size_t)bs * c * n + pt;
    // blockIdx.z splits the channels so that coarse levels (few points, many channels) still fill the chip
    const int ch0 = blockIdx.z * ch_per, ch1 = min(c, ch0 + ch_per);
    for (int ch = ch0; ch < ch1; ++ch) {
        const float *row = src + (size_t)ch * m;
        const float v = __fadd_rn(__fadd_rn(__fmul_rn(w0, row[i0]), __fmul_rn(w1, row[i1])), __fmul_rn(w2, row[i2]));
        dst[(size_t)ch * n] = base ? __fadd_rn(base[(size_t)bs * c * n + pt + (size_t)ch * n], v) : v;
    }
}

// grad_points[b,c,idx_j] += grad_out[b,c,p] * w_j  (interpolate_gpu.cu:146-148)
__global__ void three_interpolate_grad_kernel(int c, int n, int m, const float *__restrict__ grad_out,
                                              const int *__restrict__ idx, const float *__restrict__ weight,
                                              float *__restrict__ grad_points)
{
    const int bs = blockIdx.y;
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= n) return;
    const int *ii = idx + ((size_t)bs * n + pt) * 3;
    const float *ww = weight + ((size_t)bs * n + pt) * 3;
    const int i0 = ii[0], i1 = ii[1], i2 = ii[2];
    const float w0 = ww[0], w1 = ww[1], w2 = ww[2];
    const float *src = grad_out + (size_t)bs * c * n + pt;
    float *dst = grad_points + (size_t)bs * c * m;
    for (int ch = 0; ch < c; ++ch) {
        const float g = src[(size_t)ch * n];
        float *row = dst + (size_t)ch * m;
        atomicAdd(row + i0, __fmul_rn(g, w0));
        atomicAdd(row + i1, __fmul_rn(g, w1));
        atomicAdd(row + i2, __fmul_rn(g, w2));
    }
}

// The same gradient as a gather over the reverse lists of idx (amc3d_group_csr with npoints = n, nsample = 3), no atomics:
//   grad_points[b,ch,t] = the sum over the positions p = u*3 + j of t's list, in list order (ascending p), of
//   __fmul_rn(grad_out[b,ch,u], weight[b,u,j]), by sequential __fadd_rn from +0.0f.
// A thread per (known point t, group of INTERP_CPT channels): the list is walked once for the group, the stores are contiguous
// over t.  Every element is written (an empty list: +0.0f).  grid (m tiles, channel groups, b)
constexpr int INTERP_CPT = 8;
__global__ __launch_bounds__(256) void three_interpolate_grad_csr_kernel(int c, int n, int m, const float *__restrict__ grad_out,
                                                                         const float *__restrict__ weight,
                                                                         const int *__restrict__ rev_start,
                                                                         const int *__restrict__ rev_edge,
                                                                         float *__restrict__ grad_points)
{
    const int bs = blockIdx.z;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int ch0 = blockIdx.y * INTERP_CPT;
    const int nch = min(INTERP_CPT, c - ch0);
    const int s = rev_start[(size_t)bs * m + t], e = rev_start[(size_t)bs * m + t + 1];
    const float *ww = weight + (size_t)bs * n * 3;
    const float *src = grad_out + ((size_t)bs * c + ch0) * n;
    float acc[INTERP_CPT];
#pragma unroll
    for (int k = 0; k < INTERP_CPT; ++k) acc[k] = 0.f;
    for (int i = s; i < e; i += 4) {  // four positions' loads in flight (a chain of dependent round trips otherwise); the adds
        int u[4];                     // keep the list order
        float w[4], g[4][INTERP_CPT];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = rev_edge[min(i + j, e - 1)];
            u[j] = p / 3;
            w[j] = ww[p];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < INTERP_CPT; ++k) g[j][k] = src[(size_t)(k < nch ? k : 0) * n + u[j]];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < e) {
#pragma unroll
                for (int k = 0; k < INTERP_CPT; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(g[j][k], w[j]));
            }
    }
    float *dst = grad_points + ((size_t)bs * c + ch0) * m + t;
#pragma unroll
    for (int k = 0; k < INTERP_CPT; ++k)
        if (k < nch) dst[(size_t)k * m] = acc[k];
}

// The same gradient summed in LDS: the destination of this scatter is small per (cloud, channel) -- grad_points[b][ch][0..m)
// is m floats -- so a workgroup that owns cloud b and `cg` consecutive channels keeps its whole output slab acc[cg][m] in
// LDS, streams over the cloud's n unknown points reading grad_out along its contiguous axis, adds the three products of a
// point with a hardware LDS float add (no return) and stores the slab once.  The slab of channels c0..c0+cg is one
// contiguous run of grad_points, so the store is a flat pass.  No global atomic, no scratch, no zero fill, no transpose;
// the summation order is unspecified, as in the reference.  grid (channel groups, b).
//
// The slab is held in DOUBLE and the adds are ds_add_f64: on gfx950 ds_add_f32 retires about one lane every three clocks
// whatever the addresses (0.79 adds/ns per CU measured, below the chip's global float-atomic rate), ds_add_f64 six to nine
// times as many (DESIGN.md "three_interpolate backward in LDS").  Every term is still the fp32 product __fmul_rn(g, w),
// exact as a double; the fp64 sum is rounded to fp32 once, on the way out.
//
// A wave takes IGL_PPL x 64 consecutive points at a time (a lane: IGL_PPL points 64 apart), holds their idx / weight in
// registers and walks its channels four at a time, all loads of a step issued before the adds.  Where n has fewer such
// chunks than the workgroup has waves (coarse levels), `csplit` sub-groups of the channels go to different waves.
constexpr int IGL_PPL = 2;
constexpr int IGL_CHUNK = 64 * IGL_PPL;
constexpr int IGL_MAX_CG = 16;
constexpr size_t IGL_LDS_BUDGET = 128 * 1024;  // bytes of slab a workgroup may take on the dispatched route
constexpr size_t IGL_LDS_LIMIT = 160 * 1024;   // what the hardware allows the explicit entry
constexpr int IGL_MIN_GROUPS = 256;            // one workgroup per CU before channels are grouped

template <bool ACCUMULATE>
__global__ __launch_bounds__(1024) void three_interpolate_grad_lds_kernel(int c, int n, int m, int cg, int csplit,
                                                                          const float *__restrict__ grad_out,
                                                                          const int *__restrict__ idx,
                                                                          const float *__restrict__ weight,
                                                                          float *__restrict__ grad_points)
{
    extern __shared__ double igl_acc[];  // [cnt][m]
    const int bs = blockIdx.y;
    const int c0 = blockIdx.x * cg;
    const int cnt = min(cg, c - c0);
    const int total = cnt * m;
    for (int i = threadIdx.x; i < total; i += blockDim.x) igl_acc[i] = 0.0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int chunks = (n + IGL_CHUNK - 1) / IGL_CHUNK;
    const int csub = (cnt + csplit - 1) / csplit;  // channels per sub-group
    const int *ii = idx + (size_t)bs * n * 3;
    const float *ww = weight + (size_t)bs * n * 3;
    const float *src = grad_out + ((size_t)bs * c + c0) * n;
    for (int u = wave; u < chunks * csplit; u += waves) {
        const int p0 = (u % chunks) * IGL_CHUNK + lane;
        const int k_lo = (u / chunks) * csub, k_hi = min(cnt, k_lo + csub);
        int pt[IGL_PPL], t[IGL_PPL][3];
        float w[IGL_PPL][3];
#pragma unroll
        for (int q = 0; q < IGL_PPL; ++q) {
            const int p = p0 + q * 64;
            const bool live = p < n;
            pt[q] = live ? p : 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                t[q][j] = ii[(size_t)pt[q] * 3 + j];
                w[q][j] = live ? ww[(size_t)pt[q] * 3 + j] : 0.f;
            }
            if (!live) pt[q] = -1;
        }
        for (int k = k_lo; k < k_hi; k += 4) {
            float g[4][IGL_PPL];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int q = 0; q < IGL_PPL; ++q)
                    g[kk][q] = (k + kk < k_hi && pt[q] >= 0) ? src[(size_t)(k + kk) * n + pt[q]] : 0.f;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (k + kk < k_hi) {
                    double *row = igl_acc + (k + kk) * m;
#pragma unroll
                    for (int q = 0; q < IGL_PPL; ++q)
                        if (pt[q] >= 0) {
#pragma unroll
                            for (int j = 0; j < 3; ++j)
                                (void)__hip_atomic_fetch_add(row + t[q][j], (double)__fmul_rn(g[kk][q], w[q][j]), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                }
            }
        }
    }
    __syncthreads();
    float *dst = grad_points + ((size_t)bs * c + c0) * m;
    for (int i = threadIdx.x; i < total; i += blockDim.x) dst[i] = (float)(ACCUMULATE ? (double)dst[i] + igl_acc[i] : igl_acc[i]);
}

// Workgroup size by n: enough waves to keep loads in flight at the fine levels, no idle waves at the coarse ones.
static int igl_threads(int n) { return n >= 8192 ? 1024 : n >= 1024 ? 512 : 256; }

// The dispatched route's channel group: the largest power of two whose slab fits the budget, halved while the grid would
// have fewer workgroups than CUs.  0: one channel's slab does not fit (or c < 8): not an LDS shape.
static int igl_cg(int b, int c, int m)
{
    if (c < 8 || m <= 0 || b > 65535) return 0;
    const size_t fit = IGL_LDS_BUDGET / ((size_t)m * sizeof(double));
    if (fit < 1) return 0;
    int cg = 1;
    while (cg * 2 <= IGL_MAX_CG && (size_t)cg * 2 <= fit && cg * 2 <= c) cg *= 2;
    while (cg > 1 && (long)b * div_up(c, cg) < IGL_MIN_GROUPS) cg /= 2;
    return cg;
}

static int igl_launch(int b, int c, int n, int m, int cg, int threads, bool accumulate, const float *grad_out, const int *idx,
                      const float *weight, float *grad_points, hipStream_t stream, const char *what)
{
    const size_t lds = (size_t)cg * m * sizeof(double);
    const int waves = threads / 64, chunks = n > 0 ? div_up(n, IGL_CHUNK) : 1;
    int csplit = chunks >= waves ? 1 : waves / chunks;
    if (csplit > cg) csplit = cg;
    const dim3 grid(div_up(c, cg), b);
    if (accumulate) {
        (void)hipFuncSetAttribute((const void *)three_interpolate_grad_lds_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IGL_LDS_LIMIT);
        hipLaunchKernelGGL(three_interpolate_grad_lds_kernel<true>, grid, dim3(threads), lds, stream, c, n, m, cg, csplit, grad_out, idx, weight, grad_points);
    } else {
        (void)hipFuncSetAttribute((const void *)three_interpolate_grad_lds_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IGL_LDS_LIMIT);
        hipLaunchKernelGGL(three_interpolate_grad_lds_kernel<false>, grid, dim3(threads), lds, stream, c, n, m, cg, csplit, grad_out, idx, weight, grad_points);
    }
    return launch_status(what);
}

}  // namespace amc

using namespace amc;

AMC_API int amc3d_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                           int *idx, void *workspace, size_t workspace_bytes, void *stream)
{
    if (b <= 0 || n <= 0) return 0;
    if (m < 0 || !unknown || !known || !dist2 || !idx) return bad_arg("amc3d_three_nn: bad argument");
    if (workspace && m >= 3 && grid_search_pays(b, m, n) && workspace_bytes >= grid_search_workspace_bytes(b, m, n))
        return three_nn_grid(b, n, m, unknown, known, dist2, idx, workspace, (hipStream_t)stream);
    hipLaunchKernelGGL(three_nn_kernel, dim3(div_up(n, NN_THREADS), b), dim3(NN_THREADS), 0, (hipStream_t)stream, n,
                       m, unknown, known, dist2, idx);
    return launch_status("amc3d_three_nn");
}

static int three_interpolate_launch(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                                    const float *base, float *out, void *stream);

AMC_API int amc3d_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                                    const float *weight, float *out, void *stream)
{
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (!points || !idx || !weight || !out) return bad_arg("amc3d_three_interpolate: null pointer");
    return three_interpolate_launch(b, c, m, n, points, idx, weight, nullptr, out, stream);
}

// out (b,c,n) = base (b,c,n) + three_interpolate(points (b,c,m)); out may alias base
AMC_API int amc3d_three_interpolate_add(int b, int c, int m, int n, const float *points, const int *idx,
                                        const float *weight, const float *base, float *out, void *stream)
{
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (!points || !idx || !weight || !base || !out) return bad_arg("amc3d_three_interpolate_add: null pointer");
    return three_interpolate_launch(b, c, m, n, points, idx, weight, base, out, stream);
}

static int three_interpolate_launch(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                                    const float *base, float *out, void *stream)
{
    long chunks = 262144 / ((long)b * n);
    if (chunks < 1) chunks = 1;
    if (chunks > c) chunks = c;
    const int ch_per = div_up(c, chunks);
    hipLaunchKernelGGL(three_interpolate_kernel, dim3(div_up(n, 256), b, div_up(c, ch_per)), dim3(256), 0,
                       (hipStream_t)stream, c, m, n, ch_per, points, idx, weight, base, out);
    return launch_status("amc3d_three_interpolate");
}

namespace amc {
int scatter_add_pm(int fan, int b, int c, int n, long entries, const float *grad_out, const int *idx,
                   const float *weight, float *grad_points, float *scratch, hipStream_t stream, const char *what);
}

AMC_API int amc3d_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                         const float *weight, float *grad_points, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (!grad_out || !idx || !weight || !grad_points) return bad_arg("amc3d_three_interpolate_grad: null pointer");
    if (const int cg = igl_cg(b, c, m))
        return igl_launch(b, c, n, m, cg, igl_threads(n), true, grad_out, idx, weight, grad_points, (hipStream_t)stream,
                          "amc3d_three_interpolate_grad");
    if (workspace && workspace_bytes >= (size_t)b * c * m * sizeof(float) && c >= 8)
        return scatter_add_pm(3, b, c, m, n, grad_out, idx, weight, grad_points, (float *)workspace,
                              (hipStream_t)stream, "amc3d_three_interpolate_grad");
    hipLaunchKernelGGL(three_interpolate_grad_kernel, dim3(div_up(n, 256), b), dim3(256), 0, (hipStream_t)stream, c, n,
                       m, grad_out, idx, weight, grad_points);
    return launch_status("amc3d_three_interpolate_grad");
}

// Which way amc3d_three_interpolate_grad takes for this shape: 0 one global atomic per term (c < 8), 1 point-major global
// atomics (needs the workspace; 0 without it), 2 summed in LDS.  cg / threads (optional): the LDS route's channel group
// and workgroup size, 0 on the other routes.
AMC_API int amc3d_three_interpolate_grad_route(int b, int c, int n, int m, int *cg, int *threads)
{
    const int g = (b > 0 && c > 0 && n > 0) ? igl_cg(b, c, m) : 0;
    if (cg) *cg = g;
    if (threads) *threads = g ? igl_threads(n) : 0;
    return g ? 2 : c >= 8 ? 1 : 0;
}

// The LDS route in overwrite form: every element of grad_points (b,c,m) is written (a known point that no unknown point
// names gets +0.0f), so the caller neither zero-fills nor passes a workspace.  Only for shapes whose route is 2.
AMC_API int amc3d_three_interpolate_grad_write(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                               const float *weight, float *grad_points, void *stream)
{
    if (b <= 0 || c <= 0 || m <= 0) return 0;
    const int cg = igl_cg(b, c, m);
    if (n < 0 || (n > 0 && (!grad_out || !idx || !weight)) || !grad_points || !cg)
        return bad_arg("amc3d_three_interpolate_grad_write: bad argument, or not a shape of the LDS route");
    return igl_launch(b, c, n, m, cg, igl_threads(n), false, grad_out, idx, weight, grad_points, (hipStream_t)stream,
                      "amc3d_three_interpolate_grad_write");
}

// The LDS kernel with the channel group and the workgroup size given (tools/interp_grad_bench.py sweeps them; the tests
// reach every kernel path at small shapes).  cg * m doubles must fit the 160 KiB of a CU; threads 256, 512 or 1024.
AMC_API int amc3d_three_interpolate_grad_lds(int b, int c, int n, int m, int cg, int threads, int accumulate,
                                             const float *grad_out, const int *idx, const float *weight, float *grad_points,
                                             void *stream)
{
    if (b <= 0 || c <= 0 || m <= 0) return 0;
    if (n < 0 || (n > 0 && (!grad_out || !idx || !weight)) || !grad_points || b > 65535 || cg < 1 ||
        (size_t)cg * m * sizeof(double) > IGL_LDS_LIMIT || (threads != 256 && threads != 512 && threads != 1024))
        return bad_arg("amc3d_three_interpolate_grad_lds: bad argument");
    return igl_launch(b, c, n, m, cg, threads, accumulate != 0, grad_out, idx, weight, grad_points, (hipStream_t)stream,
                      "amc3d_three_interpolate_grad_lds");
}

// amc3d_three_interpolate_grad without atomics: rev_start (b*m + 1) / rev_edge (b*n*3) = amc3d_group_csr(b, m, n, 3, idx).
// grad_points (b,c,m) is written whole (no zero fill needed); the summation order is fixed (see the kernel, include/amc3d.h).
AMC_API int amc3d_three_interpolate_grad_csr(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                             const float *weight, const int *rev_start, const int *rev_edge,
                                             float *grad_points, void *stream)
{
    (void)idx;  // the lists carry everything the indices say
    if (b <= 0 || c <= 0 || m <= 0) return 0;
    if (n < 0 || (n > 0 && (!grad_out || !weight)) || !rev_start || !rev_edge || !grad_points || b > 65535 ||
        div_up(c, INTERP_CPT) > 65535 || (long)n * 3 >= (1L << 31))
        return bad_arg("amc3d_three_interpolate_grad_csr: bad argument");
    hipLaunchKernelGGL(three_interpolate_grad_csr_kernel, dim3(div_up(m, 256), div_up(c, INTERP_CPT), b), dim3(256), 0,
                       (hipStream_t)stream, c, n, m, grad_out, weight, rev_start, rev_edge, grad_points);
    return launch_status("amc3d_three_interpolate_grad_csr");
}
