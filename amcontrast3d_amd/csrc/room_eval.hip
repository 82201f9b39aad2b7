// ScanNet validation and whole-room testing on the device (gfx950): the split of a room into sub-clouds, their gather into
// a model batch with the per-sub-cloud transforms, and the vote over overlapping logits.
//
// The reference (examples/segmentation/main_AA.py:71-116 `load_data`, :574-611 the sub-cloud loop, :662-671 the vote;
// dataset/scannetv2/scannet.py:140-176 the val item) does all three in numpy on the host, one sub-cloud at a time.
//   room parts      part i holds the (i mod count)-th point of every voxel, in the order of row i of `perm` (the stand-in for
//                   np.random.shuffle); `where` is the inverse permutation, so that the vote can find a voxel's slot.
//   part batch      two launches.  Pass 1: per (row, chunk) partial minimum corner of the gathered coordinates and partial
//                   maximum of the gathered colours after the colour map (wave reduce, then LDS across waves).  Pass 2: every
//                   workgroup folds its row's partials again (min / max do not depend on the order, so this is exact) and
//                   writes pos / x / heights / y.  NaN propagates through both, as numpy's min() / max() do.
//   vote            one thread per room point.  In a voxel partition the parts that hold a point are known in closed form
//                   (rank r of count c: parts r, r + c, r + 2c, ...), so the vote is a gather summed in ascending part order:
//                   no atomics, the same bits on every run.
// Every value held against numpy goes through the _rn intrinsics; nothing may contract.  No memset, no float atomics.
#include "common.h"

namespace amc {

constexpr int kPartChunks = 32;    // workgroups per row in the statistics pass
constexpr int kPartThreads = 256;

__device__ __forceinline__ float room_nan() { return __int_as_float(0x7fc00000); }
// numpy's max() / min(): NaN as soon as one operand is NaN
__device__ __forceinline__ float room_nanmax(float a, float b) { return (a != a || b != b) ? room_nan() : fmaxf(a, b); }
__device__ __forceinline__ float room_nanmin(float a, float b) { return (a != a || b != b) ? room_nan() : fminf(a, b); }

// mode 0 (test, main_AA.py:84): np.clip((f + 1) / 2., 0, 1) -- np.clip keeps a NaN;
// mode 1 (val, scannet.py:149): (f + 1) * 127.5.  float32 arithmetic (weak Python scalars).
__device__ __forceinline__ float part_colour(float f, int mode)
{
    const float a = __fadd_rn(f, 1.f);
    if (mode == 1) return __fmul_rn(a, 127.5f);
    const float h = __fdiv_rn(a, 2.f);
    return h < 0.f ? 0.f : (h > 1.f ? 1.f : h);
}

__global__ __launch_bounds__(256) void room_parts_kernel(int p, int nvox, int npts, const int *__restrict__ start,
                                                         const int *__restrict__ count, const int *__restrict__ idx_sort,
                                                         const int *__restrict__ perm, int *__restrict__ parts,
                                                         int *__restrict__ where)
{
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nvox) return;
    const size_t row = (size_t)i * nvox;
    const int v = perm[row + j];
    if (v < 0 || v >= nvox) { parts[row + j] = -1; return; }  // not a permutation: the wrapper checks parts >= 0
    const int c = count[v];
    const int s = start[v] + (c > 0 ? i % c : 0);
    parts[row + j] = (c > 0 && s >= 0 && s < npts) ? idx_sort[s] : -1;
    where[row + v] = j;
}

// pass 1: part[(r * kPartChunks + blk) * 4 + {min x, min y, min z, colour max}]
__global__ __launch_bounds__(kPartThreads) void part_stats_kernel(int n, int npts, int mode, const int *__restrict__ idx,
                                                                  const float *__restrict__ coord, const float *__restrict__ feat,
                                                                  float *__restrict__ part)
{
    __shared__ float s[kPartThreads / 64][4];
    const int r = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int *row = idx + (size_t)r * n;
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx = -3.4e38f;
    for (int k = blk * kPartThreads + threadIdx.x; k < n; k += kPartChunks * kPartThreads) {
        const int q = row[k];
        if (q < 0 || q >= npts) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn[c] = room_nanmin(mn[c], coord[(size_t)q * 3 + c]);
            mx = room_nanmax(mx, part_colour(feat[(size_t)q * 3 + c], mode));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) mn[c] = room_nanmin(mn[c], __shfl_xor(mn[c], d, 64));
        mx = room_nanmax(mx, __shfl_xor(mx, d, 64));
    }
    if (lane == 0) { s[wave][0] = mn[0]; s[wave][1] = mn[1]; s[wave][2] = mn[2]; s[wave][3] = mx; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        float v = s[0][c];
        for (int w = 1; w < kPartThreads / 64; ++w) v = c < 3 ? room_nanmin(v, s[w][c]) : room_nanmax(v, s[w][c]);
        part[((size_t)r * kPartChunks + blk) * 4 + c] = v;
    }
}

struct PartSegs { int n, kind[3]; };  // kind: 0 pos (3 channels), 1 x (3), 2 heights (1)

// pass 2: pos (R,n,3), x (R,Cx,n) channel-major, heights (R,n), y (R,n)
__global__ __launch_bounds__(kPartThreads) void part_write_kernel(int n, int npts, int mode, int g, int cx, PartSegs segs,
                                                                  const int *__restrict__ idx, const float *__restrict__ coord,
                                                                  const float *__restrict__ feat, const long long *__restrict__ label,
                                                                  const float *__restrict__ cmean, const float *__restrict__ cstd,
                                                                  const float *__restrict__ part, float *__restrict__ pos_out,
                                                                  float *__restrict__ x_out, float *__restrict__ heights,
                                                                  long long *__restrict__ y_out)
{
    __shared__ float s_st[4];
    const int r = blockIdx.y;
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        const float *P = part + (size_t)r * kPartChunks * 4;
        float v = P[c];
        for (int b = 1; b < kPartChunks; ++b) v = c < 3 ? room_nanmin(v, P[b * 4 + c]) : room_nanmax(v, P[b * 4 + c]);
        s_st[c] = v;
    }
    __syncthreads();
    const int k = blockIdx.x * kPartThreads + threadIdx.x;
    if (k >= n) return;
    const size_t rk = (size_t)r * n + k;
    const int q = idx[rk];
    if (q < 0 || q >= npts) return;
    const bool div255 = s_st[3] > 1.f;  // NumpyChromaticNormalize: false for a NaN maximum
    float p[3], x[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p[c] = __fsub_rn(coord[(size_t)q * 3 + c], s_st[c]);
        float v = part_colour(feat[(size_t)q * 3 + c], mode);
        if (div255) v = __fdiv_rn(v, 255.f);
        x[c] = __fdiv_rn(__fsub_rn(v, cmean[c]), cstd[c]);
        pos_out[rk * 3 + c] = p[c];
    }
    const float h = p[g];
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

__global__ __launch_bounds__(256) void vote_parts_kernel(int npts, int p, int nc, int nvox, const float *__restrict__ logits,
                                                         const int *__restrict__ where, const int *__restrict__ start,
                                                         const int *__restrict__ count, const int *__restrict__ idx_sort,
                                                         const int *__restrict__ voxel_idx, float *__restrict__ voted,
                                                         long long *__restrict__ pred)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= npts) return;
    const int v = voxel_idx[s];
    if (v < 0 || v >= nvox) return;
    const int c = count[v], r = s - start[v], dst = idx_sort[s];
    if (c <= 0 || r < 0 || r >= c || r >= p || dst < 0 || dst >= npts) return;
    const float votes = (float)((p - 1 - r) / c + 1);
    float best = 0.f;
    int best_ch = 0;
    for (int ch = 0; ch < nc; ++ch) {
        float acc = 0.f;
        bool first = true;
        for (int i = r; i < p; i += c) {  // ascending part order
            const int j = where[(size_t)i * nvox + v];
            const float x = (j >= 0 && j < nvox) ? logits[((size_t)i * nc + ch) * nvox + j] : room_nan();
            acc = first ? x : __fadd_rn(acc, x);
            first = false;
        }
        const float m = __fdiv_rn(acc, votes);
        voted[(size_t)dst * nc + ch] = m;
        // torch.argmax: the first maximum, and a NaN counts as the maximum
        if (ch == 0 || (best == best && (m > best || m != m))) { best = m; best_ch = ch; }
    }
    pred[dst] = best_ch;
}

}  // namespace amc

using namespace amc;

AMC_API int amc3d_room_parts(int p, int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *perm,
                             int *parts, int *where, void *stream_)
{
    if (p <= 0 || nvox <= 0) return 0;
    if (npts <= 0 || !start || !count || !idx_sort || !perm || !parts || !where || p > 65535)
        return bad_arg("amc3d_room_parts: bad argument");
    hipLaunchKernelGGL(room_parts_kernel, dim3(div_up(nvox, 256), p), dim3(256), 0, (hipStream_t)stream_, p, nvox, npts, start, count,
                       idx_sort, perm, parts, where);
    return launch_status("amc3d_room_parts");
}

AMC_API size_t amc3d_part_batch_workspace_bytes(int rows)
{
    return rows <= 0 ? 0 : (size_t)rows * kPartChunks * 4 * sizeof(float);
}

AMC_API int amc3d_part_batch(int rows, int n, int npts, int mode, int gravity_dim, int nseg, const int *seg_kinds, const int *idx,
                             const float *coord, const float *feat, const long long *label, const float *color_mean,
                             const float *color_std, float *pos_out, float *x_out, float *heights, long long *y_out,
                             void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rows <= 0 || n <= 0) return 0;
    if (npts <= 0 || mode < 0 || mode > 1 || gravity_dim < 0 || gravity_dim > 2 || nseg < 1 || nseg > 3 || !seg_kinds || !idx ||
        !coord || !feat || !color_mean || !color_std || !pos_out || !x_out || !heights || (y_out && !label) || !workspace ||
        workspace_bytes < amc3d_part_batch_workspace_bytes(rows) || rows > 65535)
        return bad_arg("amc3d_part_batch: bad argument");
    PartSegs segs = {nseg, {0, 0, 0}};
    int cx = 0;
    for (int i = 0; i < nseg; ++i) {
        if (seg_kinds[i] < 0 || seg_kinds[i] > 2) return bad_arg("amc3d_part_batch: segment kinds are 0 pos, 1 x, 2 heights");
        segs.kind[i] = seg_kinds[i];
        cx += seg_kinds[i] == 2 ? 1 : 3;
    }
    hipStream_t stream = (hipStream_t)stream_;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(part_stats_kernel, dim3(kPartChunks, rows), dim3(kPartThreads), 0, stream, n, npts, mode, idx, coord, feat, part);
    hipLaunchKernelGGL(part_write_kernel, dim3(div_up(n, kPartThreads), rows), dim3(kPartThreads), 0, stream, n, npts, mode, gravity_dim,
                       cx, segs, idx, coord, feat, label, color_mean, color_std, (const float *)part, pos_out, x_out, heights, y_out);
    return launch_status("amc3d_part_batch");
}

AMC_API int amc3d_vote_parts(int npts, int p, int num_classes, int nvox, const float *logits, const int *where, const int *start,
                             const int *count, const int *idx_sort, const int *voxel_idx, float *voted, long long *pred,
                             void *stream_)
{
    if (npts <= 0) return 0;
    if (p <= 0 || num_classes <= 0 || nvox <= 0 || !logits || !where || !start || !count || !idx_sort || !voxel_idx || !voted || !pred)
        return bad_arg("amc3d_vote_parts: bad argument");
    hipLaunchKernelGGL(vote_parts_kernel, dim3(div_up(npts, 256)), dim3(256), 0, (hipStream_t)stream_, npts, p, num_classes, nvox,
                       logits, where, start, count, idx_sort, voxel_idx, voted, pred);
    return launch_status("amc3d_vote_parts");
}
