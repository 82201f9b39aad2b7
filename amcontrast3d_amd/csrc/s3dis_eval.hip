// S3DIS validation and whole-room testing on the device (gfx950): a batch of sub-clouds with the S3DIS config's evaluation
// transforms (val: [PointsToTensor, PointCloudXYZAlign, ChromaticNormalize], used by test() as well), and the
// nearest-neighbour test mode.  The voxel tables, the multi-voxel split and the vote are those of voxel.hip / room_eval.hip.
//
// The reference (examples/segmentation/main.py:68-113 `load_data`, :559-588 the sub-cloud loop, :605 the expansion;
// dataset/s3dis/s3dis.py:94-144 the val item) does all of it in numpy / torch on the host, one sub-cloud at a time.
//   part batch      three launches.  Pass 1: per (row, chunk) partial minimum corner of the gathered coordinates (in their own
//                   precision) and partial maximum of the colours after the colour map.  Pass 2: per (row, chunk) partial column
//                   sums of q (the coordinates the alignment sees) in fp64: every thread adds its strided elements in ascending
//                   order, a butterfly over the wave, the waves and then the chunks in ascending order -- no atomics, the same
//                   bits on every run.  Pass 3: every workgroup folds its row's partials, the centre is fl32(sum / n), and
//                   pos / x / heights / y are written.  fl32(q - m) is monotone in q, so the gravity column's minimum after
//                   the centring is fl32(min q - m): pass 1's minimum serves, no pass over pos.  A given centre skips pass 2.
//   representatives one thread per voxel: parts[j] = idx_sort[start[v] + rnd[v] % count[v]], v = perm[j]; where[v] = j.
//   expand          one thread per room point: the logits of its voxel's representative and their argmax.
// NaN propagates as in numpy / torch: through a row's minimum, mean and maximum, and into no other row.
// Every value held against the reference goes through the _rn intrinsics; nothing may contract.  No memset, no float atomics.
#include "common.h"

namespace amc {

constexpr int kS3Chunks = 32;    // workgroups per row in the two statistics passes
constexpr int kS3Threads = 256;
constexpr int kS3Slots = 8;      // doubles per (row, chunk): min x y z, colour max, sum x y z, number of points summed

__device__ __forceinline__ double s3_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// numpy's / torch's min() / max(): NaN as soon as one operand is NaN
__device__ __forceinline__ double s3_nanmin(double a, double b) { return (a != a || b != b) ? s3_nan() : fmin(a, b); }
__device__ __forceinline__ double s3_nanmax(double a, double b) { return (a != a || b != b) ? s3_nan() : fmax(a, b); }

__device__ __forceinline__ float s3_sub32(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float s3_sub32(double a, double b) { return __double2float_rn(__dsub_rn(a, b)); }

// mode 0 (test, main.py:73): np.clip(f / 255., 0, 1).astype(np.float32), the division in the file's dtype -- np.clip keeps a
// NaN; mode 1 (val, s3dis.py:99): the raw colour, already float32
__device__ __forceinline__ float s3_colour(float f, int mode)
{
    if (mode == 1) return f;
    const float h = __fdiv_rn(f, 255.f);
    return h < 0.f ? 0.f : (h > 1.f ? 1.f : h);
}
__device__ __forceinline__ float s3_colour(double f, int mode)
{
    if (mode == 1) return __double2float_rn(f);
    const double h = __ddiv_rn(f, 255.0);
    return __double2float_rn(h < 0.0 ? 0.0 : (h > 1.0 ? 1.0 : h));
}

// the four values of a workgroup -> its slots; MINMAX (pass 1): 0-2 minimum, 3 maximum; else (pass 2) sums
template <int NV, bool MINMAX>
__device__ __forceinline__ void s3_block_fold(double (&v)[NV], double *__restrict__ out)
{
    __shared__ double s[kS3Threads / 64][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const double o = __shfl_xor(v[c], d, 64);
            v[c] = MINMAX ? (c < 3 ? s3_nanmin(v[c], o) : s3_nanmax(v[c], o)) : __dadd_rn(v[c], o);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NV; ++c) s[wave][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int c = threadIdx.x;
        double a = s[0][c];
        for (int w = 1; w < kS3Threads / 64; ++w)
            a = MINMAX ? (c < 3 ? s3_nanmin(a, s[w][c]) : s3_nanmax(a, s[w][c])) : __dadd_rn(a, s[w][c]);
        out[c] = a;
    }
}

// pass 1: part[(r * kS3Chunks + blk) * kS3Slots + {0..2 min corner, 3 colour max}]
template <typename T>
__global__ __launch_bounds__(kS3Threads) void s3dis_stats_kernel(int n, int npts, int mode, const int *__restrict__ idx,
                                                                 const T *__restrict__ coord, const T *__restrict__ colour,
                                                                 double *__restrict__ part)
{
    const int r = blockIdx.y, blk = blockIdx.x;
    const int *row = idx + (size_t)r * n;
    double v[4] = {1.7e308, 1.7e308, 1.7e308, -1.7e308};
    for (int k = blk * kS3Threads + threadIdx.x; k < n; k += kS3Chunks * kS3Threads) {
        const int q = row[k];
        if (q < 0 || q >= npts) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = s3_nanmin(v[c], (double)coord[(size_t)q * 3 + c]);
            v[3] = s3_nanmax(v[3], (double)s3_colour(colour[(size_t)q * 3 + c], mode));
        }
    }
    s3_block_fold<4, true>(v, part + ((size_t)r * kS3Chunks + blk) * kS3Slots);
}

// the row's minimum corner and colour maximum from pass 1's partials (min / max do not depend on the order)
__device__ __forceinline__ void s3_row_minmax(const double *__restrict__ P, double *s_st)
{
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        double v = P[c];
        for (int b = 1; b < kS3Chunks; ++b) v = c < 3 ? s3_nanmin(v, P[b * kS3Slots + c]) : s3_nanmax(v, P[b * kS3Slots + c]);
        s_st[c] = v;
    }
}

// pass 2: part[... + {4..6}] = the chunk's column sums of q, fp64; 7 = the number of points in them (exact in fp64)
template <typename T>
__global__ __launch_bounds__(kS3Threads) void s3dis_sums_kernel(int n, int npts, int mode, const int *__restrict__ idx,
                                                                const T *__restrict__ coord, double *__restrict__ part)
{
    __shared__ double s_st[4];
    const int r = blockIdx.y, blk = blockIdx.x;
    s3_row_minmax(part + (size_t)r * kS3Chunks * kS3Slots, s_st);
    __syncthreads();
    const int *row = idx + (size_t)r * n;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = blk * kS3Threads + threadIdx.x; k < n; k += kS3Chunks * kS3Threads) {
        const int q = row[k];
        if (q < 0 || q >= npts) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T x = coord[(size_t)q * 3 + c];
            const float qc = mode == 1 ? (float)x : s3_sub32(x, (T)s_st[c]);
            v[c] = __dadd_rn(v[c], (double)qc);
        }
        v[3] += 1.0;
    }
    s3_block_fold<4, false>(v, part + ((size_t)r * kS3Chunks + blk) * kS3Slots + 4);
}

struct S3Segs { int n, kind[3]; };  // kind: 0 pos (3 channels), 1 x (3), 2 heights (1)

// pass 3: centre (R,3), pos (R,n,3), x (R,Cx,n) channel-major, heights (R,n), y (R,n)
template <typename T>
__global__ __launch_bounds__(kS3Threads) void s3dis_write_kernel(int n, int npts, int mode, int g, int cx, S3Segs segs,
                                                                 const int *__restrict__ idx, const T *__restrict__ coord,
                                                                 const T *__restrict__ colour, const long long *__restrict__ label,
                                                                 const float *__restrict__ cmean, const float *__restrict__ cstd,
                                                                 const float *__restrict__ centre_in, const double *__restrict__ part,
                                                                 float *__restrict__ pos_out, float *__restrict__ x_out,
                                                                 float *__restrict__ heights, long long *__restrict__ y_out,
                                                                 float *__restrict__ centre_out)
{
    __shared__ double s_st[4];
    __shared__ float s_m[3];
    const int r = blockIdx.y;
    const double *P = part + (size_t)r * kS3Chunks * kS3Slots;
    s3_row_minmax(P, s_st);
    if (threadIdx.x >= 64 && threadIdx.x < 67) {
        const int c = threadIdx.x - 64;
        float m;
        if (centre_in) {
            m = centre_in[(size_t)r * 3 + c];
        } else {
            double a = P[4 + c], cnt = P[7];
            for (int b = 1; b < kS3Chunks; ++b) {  // ascending chunk order
                a = __dadd_rn(a, P[b * kS3Slots + 4 + c]);
                cnt += P[b * kS3Slots + 7];
            }
            m = __double2float_rn(__ddiv_rn(a, cnt));  // cnt = n unless the row holds indices outside the room
        }
        s_m[c] = m;
        if (blockIdx.x == 0) centre_out[(size_t)r * 3 + c] = m;
    }
    __syncthreads();
    const int k = blockIdx.x * kS3Threads + threadIdx.x;
    if (k >= n) return;
    const size_t rk = (size_t)r * n + k;
    const int q = idx[rk];
    if (q < 0 || q >= npts) return;
    const bool div255 = (float)s_st[3] > 1.f;  // ChromaticNormalize: false for a NaN maximum
    // the smallest q of the gravity column: test mode shifts by the row's own minimum (0, or NaN from a NaN coordinate)
    const T cg = (T)s_st[g];
    const float qmin = mode == 1 ? (float)cg : s3_sub32(cg, cg);
    const float zmin = __fsub_rn(qmin, s_m[g]);  // = min_k fl32(q_k[g] - m[g])
    float p[3], x[3], h = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T xc = coord[(size_t)q * 3 + c];
        const float qc = mode == 1 ? (float)xc : s3_sub32(xc, (T)s_st[c]);
        if (c == g) h = qc;
        p[c] = __fsub_rn(qc, s_m[c]);
        if (c == g) p[c] = __fsub_rn(p[c], zmin);
        float v = s3_colour(colour[(size_t)q * 3 + c], mode);
        if (div255) v = __fdiv_rn(v, 255.f);
        x[c] = __fdiv_rn(__fsub_rn(v, cmean[c]), cstd[c]);
        pos_out[rk * 3 + c] = p[c];
    }
    heights[rk] = h;
    if (y_out) y_out[rk] = label[q];
    float *xo = x_out + (size_t)r * cx * n + k;
    int ch = 0;
    for (int sgi = 0; sgi < segs.n; ++sgi) {
        const int kind = segs.kind[sgi];
        if (kind == 2) {
            xo[(size_t)ch * n] = h;
            ch += 1;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) xo[(size_t)(ch + c) * n] = kind == 0 ? p[c] : x[c];
            ch += 3;
        }
    }
}

__global__ __launch_bounds__(256) void room_representatives_kernel(int nvox, int npts, const int *__restrict__ start,
                                                                   const int *__restrict__ count, const int *__restrict__ idx_sort,
                                                                   const int *__restrict__ rnd, const int *__restrict__ perm,
                                                                   int *__restrict__ parts, int *__restrict__ where)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nvox) return;
    const int v = perm[j];
    if (v < 0 || v >= nvox) { parts[j] = -1; return; }  // not a voxel id: marked, nothing read (the Python wrapper refuses such a perm up front)
    const int c = count[v], d = rnd[v];
    const int s = start[v] + ((c > 0 && d >= 0) ? d % c : 0);
    parts[j] = (c > 0 && d >= 0 && s >= 0 && s < npts) ? idx_sort[s] : -1;
    where[v] = j;
}

__global__ __launch_bounds__(256) void expand_parts_kernel(int npts, int nc, int nvox, const float *__restrict__ logits,
                                                           const int *__restrict__ where, const int *__restrict__ idx_sort,
                                                           const int *__restrict__ voxel_idx, float *__restrict__ voted,
                                                           long long *__restrict__ pred)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= npts) return;
    const int v = voxel_idx[s], dst = idx_sort[s];
    if (v < 0 || v >= nvox || dst < 0 || dst >= npts) return;
    const int j = where[v];
    if (j < 0 || j >= nvox) return;
    float best = 0.f;
    int best_ch = 0;
    for (int ch = 0; ch < nc; ++ch) {
        const float m = logits[(size_t)ch * nvox + j];
        voted[(size_t)dst * nc + ch] = m;
        // torch.argmax: the first maximum, and a NaN counts as the maximum
        if (ch == 0 || (best == best && (m > best || m != m))) { best = m; best_ch = ch; }
    }
    pred[dst] = best_ch;
}

template <typename T>
static void s3dis_launch(int rows, int n, int npts, int mode, int g, int cx, S3Segs segs, const int *idx, const void *coord,
                         const void *colour, const long long *label, const float *cmean, const float *cstd, const float *centre_in,
                         float *pos_out, float *x_out, float *heights, long long *y_out, float *centre_out, double *part,
                         hipStream_t stream)
{
    const T *co = (const T *)coord, *cl = (const T *)colour;
    hipLaunchKernelGGL(s3dis_stats_kernel<T>, dim3(kS3Chunks, rows), dim3(kS3Threads), 0, stream, n, npts, mode, idx, co, cl, part);
    if (!centre_in)
        hipLaunchKernelGGL(s3dis_sums_kernel<T>, dim3(kS3Chunks, rows), dim3(kS3Threads), 0, stream, n, npts, mode, idx, co, part);
    hipLaunchKernelGGL(s3dis_write_kernel<T>, dim3(div_up(n, kS3Threads), rows), dim3(kS3Threads), 0, stream, n, npts, mode, g, cx,
                       segs, idx, co, cl, label, cmean, cstd, centre_in, (const double *)part, pos_out, x_out, heights, y_out,
                       centre_out);
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_s3dis_part_batch_workspace_bytes(int rows)
{
    return rows <= 0 ? 0 : (size_t)rows * kS3Chunks * kS3Slots * sizeof(double);
}

AMC_API int amc3d_s3dis_part_batch(int rows, int n, int npts, int mode, int coord_f64, int gravity_dim, int nseg,
                                   const int *seg_kinds, const int *idx, const void *coord, const void *colour,
                                   const long long *label, const float *color_mean, const float *color_std, const float *centre_in,
                                   float *pos_out, float *x_out, float *heights, long long *y_out, float *centre_out,
                                   void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rows <= 0 || n <= 0) return 0;
    if (npts <= 0 || mode < 0 || mode > 1 || coord_f64 < 0 || coord_f64 > 1 || gravity_dim < 0 || gravity_dim > 2 || nseg < 1 ||
        nseg > 3 || !seg_kinds || !idx || !coord || !colour || !color_mean || !color_std || !pos_out || !x_out || !heights ||
        !centre_out || (y_out && !label) || !workspace || ((uintptr_t)workspace & 7) ||
        workspace_bytes < amc3d_s3dis_part_batch_workspace_bytes(rows) || rows > 65535)
        return bad_arg("amc3d_s3dis_part_batch: bad argument");
    if (mode == 1 && coord_f64) return bad_arg("amc3d_s3dis_part_batch: the val item is float32 (s3dis.py:99)");
    S3Segs segs = {nseg, {0, 0, 0}};
    int cx = 0;
    for (int i = 0; i < nseg; ++i) {
        if (seg_kinds[i] < 0 || seg_kinds[i] > 2) return bad_arg("amc3d_s3dis_part_batch: segment kinds are 0 pos, 1 x, 2 heights");
        segs.kind[i] = seg_kinds[i];
        cx += seg_kinds[i] == 2 ? 1 : 3;
    }
    if (coord_f64)
        s3dis_launch<double>(rows, n, npts, mode, gravity_dim, cx, segs, idx, coord, colour, label, color_mean, color_std, centre_in,
                             pos_out, x_out, heights, y_out, centre_out, (double *)workspace, (hipStream_t)stream_);
    else
        s3dis_launch<float>(rows, n, npts, mode, gravity_dim, cx, segs, idx, coord, colour, label, color_mean, color_std, centre_in,
                            pos_out, x_out, heights, y_out, centre_out, (double *)workspace, (hipStream_t)stream_);
    return launch_status("amc3d_s3dis_part_batch");
}

AMC_API int amc3d_room_representatives(int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *rnd,
                                       const int *perm, int *parts, int *where, void *stream_)
{
    if (nvox <= 0) return 0;
    if (npts <= 0 || !start || !count || !idx_sort || !rnd || !perm || !parts || !where)
        return bad_arg("amc3d_room_representatives: bad argument");
    hipLaunchKernelGGL(room_representatives_kernel, dim3(div_up(nvox, 256)), dim3(256), 0, (hipStream_t)stream_, nvox, npts, start,
                       count, idx_sort, rnd, perm, parts, where);
    return launch_status("amc3d_room_representatives");
}

AMC_API int amc3d_expand_parts(int npts, int num_classes, int nvox, const float *logits, const int *where, const int *idx_sort,
                               const int *voxel_idx, float *voted, long long *pred, void *stream_)
{
    if (npts <= 0) return 0;
    if (num_classes <= 0 || nvox <= 0 || !logits || !where || !idx_sort || !voxel_idx || !voted || !pred)
        return bad_arg("amc3d_expand_parts: bad argument");
    hipLaunchKernelGGL(expand_parts_kernel, dim3(div_up(npts, 256)), dim3(256), 0, (hipStream_t)stream_, npts, num_classes, nvox,
                       logits, where, idx_sort, voxel_idx, voted, pred);
    return launch_status("amc3d_expand_parts");
}
