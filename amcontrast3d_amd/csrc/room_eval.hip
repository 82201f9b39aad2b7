// Validation and whole-room testing on the device (gfx950), ScanNet and S3DIS: the split of a room into sub-clouds, their
// gather into a model batch with the per-sub-cloud evaluation transforms, and the vote over overlapping logits.
//
// The reference does all of it in numpy / torch on the host, one sub-cloud at a time.  ScanNet: examples/segmentation/
// main_AA.py:71-116 `load_data`, :574-611 the sub-cloud loop, :662-671 the vote; dataset/scannetv2/scannet.py:140-176 the val
// item.  S3DIS: examples/segmentation/main.py:68-113 `load_data`, :559-588 the sub-cloud loop with `val: [PointsToTensor,
// PointCloudXYZAlign, ChromaticNormalize]`, :605 the expansion; dataset/s3dis/s3dis.py:94-144 the val item.
//   voxel pick      one thread per (row, voxel): parts[i,j] = idx_sort[start[v] + d % count[v]], v = perm[i,j]; where[i,v] = j,
//                   the inverse permutation, so that the vote can find a voxel's slot.  room_parts (multi_voxel): count.max()
//                   rows, d = the row number; room_representatives (nearest_neighbor): one row, d = rnd[v].
//   part batch      rows of point indices -> a model batch, by a form (PartForm): the colour map, whether the row's minimum
//                   corner is subtracted, whether PointCloudXYZAlign follows.  Pass 1: per (row, chunk) partial minimum corner of
//                   the gathered coordinates and partial maximum of the colours after the colour map, held in fp64 (widening is
//                   exact).  Pass 2, only for the alignment's centre: per (row, chunk) partial column sums of q (the coordinates
//                   the alignment sees) in fp64: every thread adds its strided elements in ascending order, a butterfly over the
//                   wave, the waves and then the chunks in ascending order -- no atomics, the same bits on every run.  Pass 3:
//                   every workgroup folds its row's partials (min / max do not depend on the order, so this is exact), the
//                   centre is fl32(sum / n), and pos / x / heights / y are written.  fl32(q - m) is monotone in q, so the
//                   gravity column's minimum after the centring is fl32(min q - m): pass 1's minimum serves, no pass over pos.
//                   ScanNet (no alignment): passes 1 and 3.  S3DIS: all three, or 1 and 3 with a given centre.
//   vote            one thread per room point.  In a voxel partition the parts that hold a point are known in closed form
//                   (rank r of count c: parts r, r + c, r + 2c, ...), so the vote is a gather summed in ascending part order:
//                   no atomics, the same bits on every run.
//   expand          one thread per room point: the logits of its voxel's representative and their argmax.
// NaN propagates as in numpy / torch: through a row's minimum, mean and maximum, and into no other row.
// Every value held against the reference goes through the _rn intrinsics; nothing may contract.  No memset, no float atomics.
#include "common.h"

namespace amc {

constexpr int kPartChunks = 32;    // workgroups per row in the two statistics passes
constexpr int kPartThreads = 256;
constexpr int kPartSlots = 8;      // doubles per (row, chunk): min x y z, colour max, sum x y z, number of points summed

enum PartColour {
    kColourScanNetTest,  // main_AA.py:84: np.clip((f + 1) / 2., 0, 1), float32 arithmetic (weak Python scalars)
    kColourScanNetVal,   // scannet.py:149: (f + 1) * 127.5
    kColourS3disTest,    // main.py:73: np.clip(f / 255., 0, 1).astype(np.float32), the division in the file's dtype
    kColourS3disVal      // s3dis.py:99: the raw colour, already float32
};

// what differs between the datasets' evaluation items
struct PartForm {
    int colour_map;  // a PartColour
    bool shift_min;  // q = coordinate - the row's minimum corner (in the coordinate's type, then one cast to float), else q = it
    bool align;      // PointCloudXYZAlign: pos = q - the row's centre, then the gravity column minus its minimum; else pos = q
};

struct PartSegs { int n, kind[3]; };  // kind: 0 pos (3 channels), 1 x (3), 2 heights (1)

__device__ __forceinline__ float room_nan() { return __int_as_float(0x7fc00000); }
// numpy's / torch's min() / max(): NaN as soon as one operand is NaN
__device__ __forceinline__ double part_nanmin(double a, double b) { return (a != a || b != b) ? (double)room_nan() : fmin(a, b); }
__device__ __forceinline__ double part_nanmax(double a, double b) { return (a != a || b != b) ? (double)room_nan() : fmax(a, b); }

__device__ __forceinline__ float part_f32(float a) { return a; }
__device__ __forceinline__ float part_f32(double a) { return __double2float_rn(a); }
__device__ __forceinline__ float part_sub32(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float part_sub32(double a, double b) { return __double2float_rn(__dsub_rn(a, b)); }
__device__ __forceinline__ float part_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double part_div(double a, double b) { return __ddiv_rn(a, b); }

// np.clip keeps a NaN
template <typename T>
__device__ __forceinline__ T part_clip01(T h) { return h < (T)0 ? (T)0 : (h > (T)1 ? (T)1 : h); }

template <typename T>
__device__ __forceinline__ float part_colour(T f, int map)
{
    switch (map) {
    case kColourScanNetTest: return part_clip01(__fdiv_rn(__fadd_rn(part_f32(f), 1.f), 2.f));
    case kColourScanNetVal: return __fmul_rn(__fadd_rn(part_f32(f), 1.f), 127.5f);
    case kColourS3disTest: return part_f32(part_clip01(part_div(f, (T)255)));
    default: return part_f32(f);
    }
}

template <typename T>
__device__ __forceinline__ float part_q(T x, double row_min, bool shift_min)
{
    return shift_min ? part_sub32(x, (T)row_min) : part_f32(x);
}

__global__ __launch_bounds__(256) void room_pick_kernel(int nvox, int npts, const int *__restrict__ start,
                                                        const int *__restrict__ count, const int *__restrict__ idx_sort,
                                                        const int *__restrict__ rnd, const int *__restrict__ perm,
                                                        int *__restrict__ parts, int *__restrict__ where)
{
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nvox) return;
    const size_t row = (size_t)i * nvox;
    const int v = perm[row + j];
    if (v < 0 || v >= nvox) { parts[row + j] = -1; return; }  // not a voxel id: marked, nothing read (the wrappers refuse such a perm up front)
    const int c = count[v], d = rnd ? rnd[v] : i;
    const bool ok = c > 0 && d >= 0;
    const int s = start[v] + (ok ? d % c : 0);
    parts[row + j] = (ok && s >= 0 && s < npts) ? idx_sort[s] : -1;
    where[row + v] = j;
}

// the four values of a workgroup -> its slots; MINMAX (pass 1): 0-2 minimum, 3 maximum; else (pass 2) sums
template <bool MINMAX>
__device__ __forceinline__ void part_block_fold(double (&v)[4], double *__restrict__ out)
{
    __shared__ double s[kPartThreads / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double o = __shfl_xor(v[c], d, 64);
            v[c] = MINMAX ? (c < 3 ? part_nanmin(v[c], o) : part_nanmax(v[c], o)) : __dadd_rn(v[c], o);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s[wave][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        double a = s[0][c];
        for (int w = 1; w < kPartThreads / 64; ++w)
            a = MINMAX ? (c < 3 ? part_nanmin(a, s[w][c]) : part_nanmax(a, s[w][c])) : __dadd_rn(a, s[w][c]);
        out[c] = a;
    }
}

// pass 1: part[(r * kPartChunks + blk) * kPartSlots + {0..2 min corner, 3 colour max}]
template <typename T>
__global__ __launch_bounds__(kPartThreads) void part_stats_kernel(int n, int npts, int colour_map, const int *__restrict__ idx,
                                                                  const T *__restrict__ coord, const T *__restrict__ colour,
                                                                  double *__restrict__ part)
{
    const int r = blockIdx.y, blk = blockIdx.x;
    const int *row = idx + (size_t)r * n;
    double v[4] = {1.7e308, 1.7e308, 1.7e308, -1.7e308};
    for (int k = blk * kPartThreads + threadIdx.x; k < n; k += kPartChunks * kPartThreads) {
        const int q = row[k];
        if (q < 0 || q >= npts) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = part_nanmin(v[c], (double)coord[(size_t)q * 3 + c]);
            v[3] = part_nanmax(v[3], (double)part_colour(colour[(size_t)q * 3 + c], colour_map));
        }
    }
    part_block_fold<true>(v, part + ((size_t)r * kPartChunks + blk) * kPartSlots);
}

// the row's minimum corner and colour maximum from pass 1's partials (min / max do not depend on the order)
__device__ __forceinline__ void part_row_minmax(const double *__restrict__ P, double *s_st)
{
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        double v = P[c];
        for (int b = 1; b < kPartChunks; ++b) v = c < 3 ? part_nanmin(v, P[b * kPartSlots + c]) : part_nanmax(v, P[b * kPartSlots + c]);
        s_st[c] = v;
    }
}

// pass 2: part[... + {4..6}] = the chunk's column sums of q, fp64; 7 = the number of points in them (exact in fp64)
template <typename T>
__global__ __launch_bounds__(kPartThreads) void part_sums_kernel(int n, int npts, bool shift_min, const int *__restrict__ idx,
                                                                 const T *__restrict__ coord, double *__restrict__ part)
{
    __shared__ double s_st[4];
    const int r = blockIdx.y, blk = blockIdx.x;
    part_row_minmax(part + (size_t)r * kPartChunks * kPartSlots, s_st);
    __syncthreads();
    const int *row = idx + (size_t)r * n;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = blk * kPartThreads + threadIdx.x; k < n; k += kPartChunks * kPartThreads) {
        const int q = row[k];
        if (q < 0 || q >= npts) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __dadd_rn(v[c], (double)part_q(coord[(size_t)q * 3 + c], s_st[c], shift_min));
        v[3] += 1.0;
    }
    part_block_fold<false>(v, part + ((size_t)r * kPartChunks + blk) * kPartSlots + 4);
}

// pass 3: centre (R,3) when aligning, pos (R,n,3), x (R,Cx,n) channel-major, heights (R,n), y (R,n)
template <typename T>
__global__ __launch_bounds__(kPartThreads) void part_write_kernel(int n, int npts, PartForm form, int g, int cx, PartSegs segs,
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
    const double *P = part + (size_t)r * kPartChunks * kPartSlots;
    part_row_minmax(P, s_st);
    if (form.align && threadIdx.x >= 64 && threadIdx.x < 67) {
        const int c = threadIdx.x - 64;
        float m;
        if (centre_in) {
            m = centre_in[(size_t)r * 3 + c];
        } else {
            double a = P[4 + c], cnt = P[7];
            for (int b = 1; b < kPartChunks; ++b) {  // ascending chunk order
                a = __dadd_rn(a, P[b * kPartSlots + 4 + c]);
                cnt += P[b * kPartSlots + 7];
            }
            m = __double2float_rn(__ddiv_rn(a, cnt));  // cnt = n unless the row holds indices outside the room
        }
        s_m[c] = m;
        if (blockIdx.x == 0) centre_out[(size_t)r * 3 + c] = m;
    }
    __syncthreads();
    const int k = blockIdx.x * kPartThreads + threadIdx.x;
    if (k >= n) return;
    const size_t rk = (size_t)r * n + k;
    const int q = idx[rk];
    if (q < 0 || q >= npts) return;
    const bool div255 = (float)s_st[3] > 1.f;  // [Numpy]ChromaticNormalize: false for a NaN maximum
    // the smallest q of the gravity column (with shift_min 0, or NaN from a NaN coordinate), then centred
    const float zmin = form.align ? __fsub_rn(part_q((T)s_st[g], s_st[g], form.shift_min), s_m[g]) : 0.f;  // = min_k fl32(q_k[g] - m[g])
    float p[3], x[3], h = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float qc = part_q(coord[(size_t)q * 3 + c], s_st[c], form.shift_min);
        if (c == g) h = qc;
        p[c] = qc;
        if (form.align) {
            p[c] = __fsub_rn(qc, s_m[c]);
            if (c == g) p[c] = __fsub_rn(p[c], zmin);
        }
        float v = part_colour(colour[(size_t)q * 3 + c], form.colour_map);
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

// the arguments the two entry points share
struct PartArgs {
    int rows, n, npts, gravity_dim, nseg;
    const int *seg_kinds, *idx;
    const void *coord, *colour;
    const long long *label;
    const float *cmean, *cstd, *centre_in;
    float *pos_out, *x_out, *heights;
    long long *y_out;
    float *centre_out;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t stream;
};

static size_t part_workspace_bytes(int rows) { return rows <= 0 ? 0 : (size_t)rows * kPartChunks * kPartSlots * sizeof(double); }

template <typename T>
static void part_launch(PartForm form, int cx, PartSegs segs, const PartArgs &a)
{
    const T *co = (const T *)a.coord, *cl = (const T *)a.colour;
    double *part = (double *)a.workspace;
    const dim3 chunks(kPartChunks, a.rows), block(kPartThreads);
    hipLaunchKernelGGL(part_stats_kernel<T>, chunks, block, 0, a.stream, a.n, a.npts, form.colour_map, a.idx, co, cl, part);
    if (form.align && !a.centre_in)
        hipLaunchKernelGGL(part_sums_kernel<T>, chunks, block, 0, a.stream, a.n, a.npts, form.shift_min, a.idx, co, part);
    hipLaunchKernelGGL(part_write_kernel<T>, dim3(div_up(a.n, kPartThreads), a.rows), block, 0, a.stream, a.n, a.npts, form,
                       a.gravity_dim, cx, segs, a.idx, co, cl, a.label, a.cmean, a.cstd, a.centre_in, (const double *)part,
                       a.pos_out, a.x_out, a.heights, a.y_out, a.centre_out);
}

static int part_refuse(const char *who, const char *why)
{
    set_error("%s: %s", who, why);
    return (int)hipErrorInvalidValue;
}

static int part_check(PartForm form, const PartArgs &a, const char *who)
{
    if (a.npts <= 0 || a.gravity_dim < 0 || a.gravity_dim > 2 || a.nseg < 1 || a.nseg > 3 || !a.seg_kinds || !a.idx || !a.coord ||
        !a.colour || !a.cmean || !a.cstd || !a.pos_out || !a.x_out || !a.heights || (form.align && !a.centre_out) ||
        (a.y_out && !a.label) || !a.workspace || ((uintptr_t)a.workspace & 7) ||
        a.workspace_bytes < part_workspace_bytes(a.rows) || a.rows > 65535)
        return part_refuse(who, "bad argument");
    return 0;
}

static int part_batch(PartForm form, bool f64, const PartArgs &a, const char *who)
{
    PartSegs segs = {a.nseg, {0, 0, 0}};
    int cx = 0;
    for (int i = 0; i < a.nseg; ++i) {
        if (a.seg_kinds[i] < 0 || a.seg_kinds[i] > 2) return part_refuse(who, "segment kinds are 0 pos, 1 x, 2 heights");
        segs.kind[i] = a.seg_kinds[i];
        cx += a.seg_kinds[i] == 2 ? 1 : 3;
    }
    if (f64)
        part_launch<double>(form, cx, segs, a);
    else
        part_launch<float>(form, cx, segs, a);
    return launch_status(who);
}

static int room_pick(int p, int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *rnd,
                     const int *perm, int *parts, int *where, void *stream_, const char *who)
{
    hipLaunchKernelGGL(room_pick_kernel, dim3(div_up(nvox, 256), p), dim3(256), 0, (hipStream_t)stream_, nvox, npts, start, count,
                       idx_sort, rnd, perm, parts, where);
    return launch_status(who);
}

}  // namespace amc

using namespace amc;

AMC_API int amc3d_room_parts(int p, int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *perm,
                             int *parts, int *where, void *stream_)
{
    if (p <= 0 || nvox <= 0) return 0;
    if (npts <= 0 || !start || !count || !idx_sort || !perm || !parts || !where || p > 65535)
        return bad_arg("amc3d_room_parts: bad argument");
    return room_pick(p, nvox, npts, start, count, idx_sort, nullptr, perm, parts, where, stream_, "amc3d_room_parts");
}

AMC_API int amc3d_room_representatives(int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *rnd,
                                       const int *perm, int *parts, int *where, void *stream_)
{
    if (nvox <= 0) return 0;
    if (npts <= 0 || !start || !count || !idx_sort || !rnd || !perm || !parts || !where)
        return bad_arg("amc3d_room_representatives: bad argument");
    return room_pick(1, nvox, npts, start, count, idx_sort, rnd, perm, parts, where, stream_, "amc3d_room_representatives");
}

AMC_API size_t amc3d_part_batch_workspace_bytes(int rows) { return part_workspace_bytes(rows); }

AMC_API size_t amc3d_s3dis_part_batch_workspace_bytes(int rows) { return part_workspace_bytes(rows); }

AMC_API int amc3d_part_batch(int rows, int n, int npts, int mode, int gravity_dim, int nseg, const int *seg_kinds, const int *idx,
                             const float *coord, const float *feat, const long long *label, const float *color_mean,
                             const float *color_std, float *pos_out, float *x_out, float *heights, long long *y_out,
                             void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rows <= 0 || n <= 0) return 0;
    if (mode < 0 || mode > 1) return bad_arg("amc3d_part_batch: bad argument");
    const PartForm form = {mode == 1 ? kColourScanNetVal : kColourScanNetTest, true, false};
    const PartArgs a = {rows, n, npts, gravity_dim, nseg, seg_kinds, idx, coord, feat, label, color_mean, color_std, nullptr,
                        pos_out, x_out, heights, y_out, nullptr, workspace, workspace_bytes, (hipStream_t)stream_};
    if (int e = part_check(form, a, "amc3d_part_batch")) return e;
    return part_batch(form, false, a, "amc3d_part_batch");
}

AMC_API int amc3d_s3dis_part_batch(int rows, int n, int npts, int mode, int coord_f64, int gravity_dim, int nseg,
                                   const int *seg_kinds, const int *idx, const void *coord, const void *colour,
                                   const long long *label, const float *color_mean, const float *color_std, const float *centre_in,
                                   float *pos_out, float *x_out, float *heights, long long *y_out, float *centre_out,
                                   void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rows <= 0 || n <= 0) return 0;
    if (mode < 0 || mode > 1 || coord_f64 < 0 || coord_f64 > 1) return bad_arg("amc3d_s3dis_part_batch: bad argument");
    const PartForm form = {mode == 1 ? kColourS3disVal : kColourS3disTest, mode == 0, true};
    const PartArgs a = {rows, n, npts, gravity_dim, nseg, seg_kinds, idx, coord, colour, label, color_mean, color_std, centre_in,
                        pos_out, x_out, heights, y_out, centre_out, workspace, workspace_bytes, (hipStream_t)stream_};
    if (int e = part_check(form, a, "amc3d_s3dis_part_batch")) return e;
    if (mode == 1 && coord_f64) return bad_arg("amc3d_s3dis_part_batch: the val item is float32 (s3dis.py:99)");
    return part_batch(form, coord_f64 != 0, a, "amc3d_s3dis_part_batch");
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
