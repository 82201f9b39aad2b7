// ScanNet's training input on the device (gfx950): ScanNet.__getitem__ (dataset/scannetv2/scannet.py:140-176) plus the
// collate, for a batch of raw rooms.
//
// The reference, per room and in numpy: colours (feat + 1) * 127.5 in float32; the transform chain RandomRotateZ,
// RandomScale, ChromaticAutoContrast, RandomDropFeature, NumpyChromaticNormalize (transforms/point_transform_cpu.py:43-92,
// 192-209,304-332) on the WHOLE raw room; then crop_pc (dataset/data_util.py:146-174) and `heights`.  np.dot(pos_f32, R_f64)
// makes the positions float64, and they stay float64 through RandomScale and all of crop_pc, down to its final astype.
//   room stats      per room and colour channel: min / max of the input colours, then (second pass) the maximum of the
//                   colours after contrast and drop, NaN if any is NaN (hi == lo with contrast taken: 0 * inf) -- numpy's
//                   max() then returns NaN and `NaN > 1` is false: no /255.  kStatBlocks workgroups per room, fixed-order
//                   partials (min / max are exact, so any order gives the same result).
//   transform       one elementwise pass over all points of all rooms: positions in double as OpenBLAS's dgemm forms
//                   np.dot(p, R)[i, j] = fma(p2, R[2,j], fma(p1, R[1,j], p0 * R[0,j])), then * scale * mirror; colours in
//                   float32 in numpy's order.
//   crop tail       one workgroup per room: gathers voxel pick -> crop -> shuffle, subtracts the cropped cloud's float64
//                   min corner, casts to float32 and writes pos / x / y / heights into the room's slot of the (B,N,.) batch.
// The voxelise and crop between transform and tail are voxel.hip's *_f64 entry points.  Random draws are the caller's:
// the library has no generator.
//
// Per-room parameter record (ScanNetRoom, 16 doubles):
//   rot[9] row-major R (pos' = pos @ R), scale[3] (= scale * mirror per axis), contrast (0/1), w_keep = f32(1 - blend),
//   w_contrast = f32(blend) (NEP 50: numpy rounds the Python-double weights to float32 first), drop (0/1)
#include "room_common.h"

namespace amc {

struct ScanNetRoom { double rot[9], scale[3], contrast, w_keep, w_contrast, drop; };  // 16 doubles
struct ScanNetStats { float lo[3], hi[3], cmax, pad; };                                 // 8 floats

constexpr int kStatBlocks = 32;  // workgroups per room in the statistics passes (a cfg-4 batch is 2 rooms)
constexpr int kStatThreads = 256;

__device__ __forceinline__ float nan_f32() { return __int_as_float(0x7fc00000); }

// numpy's max(): NaN as soon as one operand is NaN
__device__ __forceinline__ float nanmax(float a, float b) { return (a != a || b != b) ? nan_f32() : fmaxf(a, b); }

// scannet.py:140: the .pth colours in [-1, 1] to 0..255, float32 arithmetic (weak Python scalars)
__device__ __forceinline__ float raw_colour(float f) { return __fmul_rn(__fadd_rn(f, 1.f), 127.5f); }

// ChromaticAutoContrast (:197-204) then RandomDropFeature (:311-314) on one channel
__device__ __forceinline__ float contrast_drop(float x, float lo, float hi, const ScanNetRoom &p)
{
    if (p.contrast != 0.0) {
        const float sc = __fdiv_rn(255.f, __fsub_rn(hi, lo));  // 255 / (hi - lo): inf when hi == lo
        x = __fadd_rn(__fmul_rn((float)p.w_keep, x), __fmul_rn((float)p.w_contrast, __fmul_rn(__fsub_rn(x, lo), sc)));
    }
    return p.drop != 0.0 ? 0.f : x;
}

// pass 1: per (room, workgroup) partial min / max of the input colours -> part[(b * kStatBlocks + blk) * 6 + {lo0..2, hi0..2}]
__global__ __launch_bounds__(kStatThreads) void scannet_minmax_kernel(const long long *__restrict__ off, const float *__restrict__ feat,
                                                                    float *__restrict__ part)
{
    __shared__ float s[kStatThreads / 64][6];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (long long i = off[b] + (long long)blk * kStatThreads + threadIdx.x; i < off[b + 1]; i += (long long)kStatBlocks * kStatThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = raw_colour(feat[i * 3 + c]);
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], d, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d, 64));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[wave][c] = lo[c]; s[wave][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = s[0][c];
        for (int w = 1; w < kStatThreads / 64; ++w) v = c < 3 ? fminf(v, s[w][c]) : fmaxf(v, s[w][c]);
        part[((size_t)b * kStatBlocks + blk) * 6 + c] = v;
    }
}

// pass 2: every workgroup folds its room's pass-1 partials (workgroup 0 stores lo / hi), then the partial maximum of the
// colours after contrast and drop (NaN-propagating) -> cpart[b * kStatBlocks + blk]
__global__ __launch_bounds__(kStatThreads) void scannet_cmax_kernel(const long long *__restrict__ off, const float *__restrict__ feat,
                                                                  const ScanNetRoom *__restrict__ par, const float *__restrict__ part,
                                                                  float *__restrict__ cpart, ScanNetStats *__restrict__ st)
{
    __shared__ float s_lh[6];
    __shared__ float s_m[kStatThreads / 64];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        const float *P = part + (size_t)b * kStatBlocks * 6;
        float v = P[c];
        for (int k = 1; k < kStatBlocks; ++k) v = c < 3 ? fminf(v, P[k * 6 + c]) : fmaxf(v, P[k * 6 + c]);
        s_lh[c] = v;
        if (blk == 0) { if (c < 3) st[b].lo[c] = v; else st[b].hi[c - 3] = v; }
    }
    __syncthreads();
    const ScanNetRoom p = par[b];
    const float lo[3] = {s_lh[0], s_lh[1], s_lh[2]}, hi[3] = {s_lh[3], s_lh[4], s_lh[5]};
    float m = -3.4e38f;
    for (long long i = off[b] + (long long)blk * kStatThreads + threadIdx.x; i < off[b + 1]; i += (long long)kStatBlocks * kStatThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m = nanmax(m, contrast_drop(raw_colour(feat[i * 3 + c]), lo[c], hi[c], p));
    }
    for (int d = 32; d >= 1; d >>= 1) m = nanmax(m, __shfl_xor(m, d, 64));
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float v = s_m[0];
        for (int w = 1; w < kStatThreads / 64; ++w) v = nanmax(v, s_m[w]);
        cpart[(size_t)b * kStatBlocks + blk] = v;
    }
}

__global__ void scannet_cmax_final_kernel(int b, const float *__restrict__ cpart, ScanNetStats *__restrict__ st)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b) return;
    float v = cpart[(size_t)r * kStatBlocks];
    for (int k = 1; k < kStatBlocks; ++k) v = nanmax(v, cpart[(size_t)r * kStatBlocks + k]);
    st[r].cmax = v;
    st[r].pad = 0.f;
}

__global__ __launch_bounds__(256) void scannet_transform_kernel(int b, long long total, const long long *__restrict__ off,
                                                                const float *__restrict__ coord, const float *__restrict__ feat,
                                                                const ScanNetRoom *__restrict__ par,
                                                                const ScanNetStats *__restrict__ st, const float *__restrict__ cmean,
                                                                const float *__restrict__ cstd, double *__restrict__ pos_out,
                                                                float *__restrict__ x_out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int r = room_seg<long long>(b, off, i);
    const ScanNetRoom &p = par[r];
    const double p0 = (double)coord[i * 3], p1 = (double)coord[i * 3 + 1], p2 = (double)coord[i * 3 + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // RandomRotateZ (np.dot as dgemm accumulates it), then RandomScale's `pos *= scale`
        const double v = __fma_rn(p2, p.rot[6 + j], __fma_rn(p1, p.rot[3 + j], __dmul_rn(p0, p.rot[j])));
        pos_out[i * 3 + j] = __dmul_rn(v, p.scale[j]);
    }
    const ScanNetStats s = st[r];
    const bool div255 = s.cmax > 1.f;  // false for a NaN maximum
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // NumpyChromaticNormalize (:327-332)
        float x = contrast_drop(raw_colour(feat[i * 3 + c]), s.lo[c], s.hi[c], p);
        if (div255) x = __fdiv_rn(x, 255.f);
        x_out[i * 3 + c] = __fdiv_rn(__fsub_rn(x, cmean[c]), cstd[c]);
    }
}

// slot k of the room's output: point sel[crop[perm[k]]] of the room (crop / perm NULL: identity)
__device__ __forceinline__ int tail_src(int k, const int *__restrict__ sel, const int *__restrict__ crop, const int *__restrict__ perm)
{
    const int c = perm ? perm[k] : k;
    return sel[crop ? crop[c] : c];
}

__global__ __launch_bounds__(1024) void scannet_crop_tail_kernel(int n, int g, const double *__restrict__ coord,
                                                               const float *__restrict__ x, const long long *__restrict__ y,
                                                               const int *__restrict__ sel, const int *__restrict__ crop,
                                                               const int *__restrict__ perm, float *__restrict__ pos_out,
                                                               float *__restrict__ x_out, float *__restrict__ heights,
                                                               long long *__restrict__ y_out)
{
    __shared__ double s_mn[16][3];
    __shared__ double s_corner[3];
    // crop_pc's last `coord -= coord.min(0)` (data_util.py:173): the min corner of the cropped cloud, in double (the
    // shuffle does not change the set, so the loop runs in crop order)
    double mn[3] = {kHuge<double>, kHuge<double>, kHuge<double>};
    for (int k = threadIdx.x; k < n; k += 1024) {
        const int s = tail_src(k, sel, crop, nullptr);
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fmin(mn[j], coord[(size_t)s * 3 + j]);
    }
    block_min3<double, 1024>(mn, s_mn, s_corner);
    __syncthreads();
    const double c0 = s_corner[0], c1 = s_corner[1], c2 = s_corner[2];
    for (int k = threadIdx.x; k < n; k += 1024) {
        const int s = tail_src(k, sel, crop, perm);
        const float q[3] = {(float)__dsub_rn(coord[(size_t)s * 3], c0), (float)__dsub_rn(coord[(size_t)s * 3 + 1], c1),
                            (float)__dsub_rn(coord[(size_t)s * 3 + 2], c2)};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pos_out[(size_t)k * 3 + j] = q[j];
            x_out[(size_t)k * 3 + j] = x[(size_t)s * 3 + j];
        }
        // scannet.py:174-175: pos[:, g] - pos[:, g].min() in float32.  That minimum is exactly 0 (the shifted cloud's
        // smallest coordinate is c - c = 0, and the cast keeps it), so heights is the float32 gravity coordinate itself.
        heights[k] = q[g];
        y_out[k] = y[s];
    }
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_scannet_stats_workspace_bytes(int b)
{
    if (b <= 0) return 0;
    return align256((size_t)b * kStatBlocks * 6 * sizeof(float)) + align256((size_t)b * kStatBlocks * sizeof(float));
}

AMC_API int amc3d_scannet_room_stats(int b, const long long *offsets, const float *feat, const double *params, float *stats,
                                     void *workspace, size_t workspace_bytes, void *stream_)
{
    if (b <= 0) return 0;
    if (!offsets || !feat || !params || !stats || !workspace || workspace_bytes < amc3d_scannet_stats_workspace_bytes(b))
        return bad_arg("amc3d_scannet_room_stats: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    float *part = (float *)workspace;
    float *cpart = (float *)((char *)workspace + align256((size_t)b * kStatBlocks * 6 * sizeof(float)));
    ScanNetStats *st = (ScanNetStats *)stats;
    hipLaunchKernelGGL(scannet_minmax_kernel, dim3(kStatBlocks, b), dim3(kStatThreads), 0, stream, offsets, feat, part);
    hipLaunchKernelGGL(scannet_cmax_kernel, dim3(kStatBlocks, b), dim3(kStatThreads), 0, stream, offsets, feat,
                       (const ScanNetRoom *)params, (const float *)part, cpart, st);
    hipLaunchKernelGGL(scannet_cmax_final_kernel, dim3(div_up(b, 64)), dim3(64), 0, stream, b, (const float *)cpart, st);
    return launch_status("amc3d_scannet_room_stats");
}

AMC_API int amc3d_scannet_transform_rooms(int b, long long total, const long long *offsets, const float *coord, const float *feat,
                                          const double *params, const float *stats, const float *color_mean,
                                          const float *color_std, double *pos_out, float *x_out, void *stream_)
{
    if (b <= 0 || total <= 0) return 0;
    if (!offsets || !coord || !feat || !params || !stats || !color_mean || !color_std || !pos_out || !x_out)
        return bad_arg("amc3d_scannet_transform_rooms: bad argument");
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return bad_arg("amc3d_scannet_transform_rooms: too many points");
    hipLaunchKernelGGL(scannet_transform_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, b, total, offsets, coord,
                       feat, (const ScanNetRoom *)params, (const ScanNetStats *)stats, color_mean, color_std, pos_out, x_out);
    return launch_status("amc3d_scannet_transform_rooms");
}

AMC_API int amc3d_scannet_crop_tail(int n, int gravity_dim, const double *coord, const float *x, const long long *y, const int *sel,
                                    const int *crop, const int *perm, float *pos_out, float *x_out, float *heights,
                                    long long *y_out, void *stream_)
{
    if (n <= 0) return 0;
    if (gravity_dim < 0 || gravity_dim > 2 || !coord || !x || !y || !sel || !pos_out || !x_out || !heights || !y_out)
        return bad_arg("amc3d_scannet_crop_tail: bad argument");
    hipLaunchKernelGGL(scannet_crop_tail_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream_, n, gravity_dim, coord, x, y, sel, crop,
                       perm, pos_out, x_out, heights, y_out);
    return launch_status("amc3d_scannet_crop_tail");
}
