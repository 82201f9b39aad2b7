// S3DISSphere on the device (gfx950): spheres of radius in_radius cut out of whole voxel-subsampled Areas, their centres picked
// by a running potential (dataset/s3dis/s3dis_sphere.py:214-247 the schedule, :288-347 the item).  The clouds are one
// concatenated array -- cloud c is points [cloud_off[c], cloud_off[c+1]) -- and every index below is an int.
//   pick      argmin(min_potentials), then argmin(potentials[cloud]), first minimum in both: the lexicographic (value, global
//             index) minimum over all clouds (the first cloud that holds the smallest value, and its first point that does).
//             It runs over a table of per-block minima, kPotBlock points per entry, in one workgroup; the centre stays on the
//             device as (cloud, point)
//   keys      pick = sub_points[point] + noise in float64 (the reference reads the coordinates back from the KD-tree, which holds
//             them as float64); per point of the cloud the KD-tree's reduced distance ((dx*dx + dy*dy) + dz*dz) in float64, no
//             contraction; key = its bit pattern where d2 <= r*r, all ones elsewhere; value = the point.  One streaming pass
//             over the largest cloud's size
//   order     one stable device-wide radix sort of the (key, point) pairs: the input is in point order, so equal distances
//             come out in ascending point order (sklearn leaves that order unspecified), and the survivors come first
//   finish    cur = the number of survivors (a binary search for the first all-ones key), count = min(cur, num_points), the
//             first num_points points -> order; in the schedule also the Tukey update potentials[q] += (1 - d32 / r^2)^2 with
//             d32 the float32 sum of squares of the float64 differences rounded to float32, and the rest in float64 (numpy >= 2
//             promotes there).  Points inside one sphere are distinct: plain read-modify-write, the same bits on every run.  It
//             marks the touched blocks
//   minima    the table's entries: all of them once, afterwards the marked ones of the picked cloud
//   tail      one launch for B spheres: slot k <- order[perm[k]] below count, order[perm[pad[k]]] above, then input_inds, mask,
//             pos = point - pick in float64 rounded to float32, colours, label, heights = the absolute gravity coordinate
// Launches: a schedule step is pick, keys, the library sort, finish, minima; a query of a given centre is keys, the sort, finish.
// Nothing allocates, synchronises or reads back; the sort goes through cub_kernel_memset.h, so no memset node is captured.
#include "cub_kernel_memset.h"  // hipCUB with its memsets as kernels (graph-safe)

#include "room_common.h"

namespace amc {

constexpr int kPotBlock = 1024;  // points per entry of the minima table
constexpr int kPotShift = 10;
constexpr int kSphThreads = 256;
constexpr unsigned long long kOutside = ~0ULL;  // the key of a point outside the sphere (a NaN pattern: no distance has it)

struct PotMin {
    double v;
    int i;
};

__device__ __forceinline__ void pot_min(PotMin &a, double v, int i)
{
    if (v < a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; }
}

// the workgroup's lexicographic minimum, valid in thread 0.  s: blockDim.x / 64 entries of LDS
__device__ __forceinline__ PotMin block_pot_min(PotMin m, PotMin *s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) pot_min(m, __shfl_xor(m.v, d, 64), __shfl_xor(m.i, d, 64));
    if (lane == 0) s[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < waves; ++w) pot_min(m, s[w].v, s[w].i);
    return m;
}

__device__ __forceinline__ PotMin pot_none() { return PotMin{__longlong_as_double(0x7ff0000000000000LL), 0x7fffffff}; }

// entry g of the table: the first minimum of potentials [g * kPotBlock, (g + 1) * kPotBlock).  cloud == NULL: every entry;
// else the marked entries of cloud *cloud, whose marks are cleared
__global__ __launch_bounds__(kSphThreads) void sphere_minima_kernel(int total, int clouds, const int *__restrict__ cloud_off,
                                                                    const int *__restrict__ cloud, const double *__restrict__ pot,
                                                                    double *__restrict__ blk_val, int *__restrict__ blk_idx,
                                                                    int *__restrict__ touched)
{
    __shared__ PotMin s[kSphThreads / 64];
    int g = blockIdx.x;
    if (cloud) {
        const int c = min(max(*cloud, 0), clouds - 1);
        const int lo = cloud_off[c], hi = cloud_off[c + 1];
        if (hi <= lo) return;
        g += lo >> kPotShift;
        if (g > ((hi - 1) >> kPotShift) || !touched[g]) return;  // (uniform over the workgroup)
    }
    const int base = g << kPotShift;
    if (base >= total) return;
    PotMin m = pot_none();
    for (int i = base + threadIdx.x; i < min(base + kPotBlock, total); i += kSphThreads) pot_min(m, pot[i], i);
    m = block_pot_min(m, s);
    if (threadIdx.x == 0) {
        blk_val[g] = m.v;
        blk_idx[g] = m.i == 0x7fffffff ? base : m.i;  // (a block of NaNs: any point of it)
        touched[g] = 0;
    }
}

__global__ __launch_bounds__(1024) void sphere_pick_kernel(int clouds, int nblk, const int *__restrict__ cloud_off,
                                                           const double *__restrict__ blk_val, const int *__restrict__ blk_idx,
                                                           int *__restrict__ cloud_out, int *__restrict__ point_out)
{
    __shared__ PotMin s[16];
    PotMin m = pot_none();
    for (int b = threadIdx.x; b < nblk; b += 1024) pot_min(m, blk_val[b], blk_idx[b]);
    m = block_pot_min(m, s);
    if (threadIdx.x == 0) {
        const int g = m.i == 0x7fffffff ? 0 : m.i;
        const int c = room_seg<int>(clouds, cloud_off, g);
        *cloud_out = c;
        *point_out = g - cloud_off[c];
    }
}

// the sphere's cloud [lo, lo + n) and its centre point, both clamped to what exists
__device__ __forceinline__ void sphere_cloud(int clouds, const int *__restrict__ cloud_off, int cloud, int point, int &lo, int &n,
                                             int &p)
{
    const int c = min(max(cloud, 0), clouds - 1);
    lo = cloud_off[c];
    n = cloud_off[c + 1] - lo;
    p = min(max(point, 0), max(n - 1, 0));
}

__global__ __launch_bounds__(kSphThreads) void sphere_keys_kernel(int clouds, int n_max, double r2, const float *__restrict__ pts,
                                                                  const int *__restrict__ cloud_off, const int *__restrict__ cloud,
                                                                  const int *__restrict__ point, const double *__restrict__ noise,
                                                                  double *__restrict__ centre, unsigned long long *__restrict__ key,
                                                                  int *__restrict__ val)
{
    const int i = blockIdx.x * kSphThreads + threadIdx.x;
    int lo, n, p;
    sphere_cloud(clouds, cloud_off, *cloud, *point, lo, n, p);
    double c[3] = {0.0, 0.0, 0.0};
    if (n > 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = __dadd_rn((double)pts[(size_t)(lo + p) * 3 + j], noise[j]);  // s3dis_sphere.py:232
    }
    if (i == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) centre[j] = c[j];
    }
    if (i >= n_max) return;
    unsigned long long k = kOutside;
    if (i < n) {
        const size_t q = (size_t)(lo + i) * 3;
        const double d2 = dist2_ref((double)pts[q], (double)pts[q + 1], (double)pts[q + 2], c[0], c[1], c[2]);
        if (d2 <= r2) k = order_bits(d2);
    }
    key[i] = k;
    val[i] = i;
}

// s3dis_sphere.py:241-245 for one point of the list: the weight its potential gains
__device__ __forceinline__ double tukey(const float *__restrict__ p, const double *__restrict__ c, double r2)
{
    const float dx = (float)__dsub_rn((double)p[0], c[0]), dy = (float)__dsub_rn((double)p[1], c[1]),
                dz = (float)__dsub_rn((double)p[2], c[2]);
    const double d = (double)__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    const double u = __dsub_rn(1.0, __ddiv_rn(d, r2));
    return d > r2 ? 0.0 : __dmul_rn(u, u);
}

// order NULL: not wanted; pot NULL: no update
__global__ __launch_bounds__(kSphThreads) void sphere_finish_kernel(int clouds, int n_max, int num_points, double r2,
                                                                    const float *__restrict__ pts, const int *__restrict__ cloud_off,
                                                                    const int *__restrict__ cloud, const double *__restrict__ centre,
                                                                    const unsigned long long *__restrict__ key_s,
                                                                    const int *__restrict__ val_s, int *__restrict__ order,
                                                                    int *__restrict__ cur, int *__restrict__ count,
                                                                    double *__restrict__ pot, int *__restrict__ touched)
{
    const int k = blockIdx.x * kSphThreads + threadIdx.x;
    if (k == 0) {  // the survivors sort before every kOutside key
        int lo = 0, hi = n_max;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key_s[mid] != kOutside) lo = mid + 1; else hi = mid;
        }
        *cur = lo;
        *count = min(lo, num_points);
    }
    if (k >= num_points) return;
    int lo, n, p;
    sphere_cloud(clouds, cloud_off, *cloud, 0, lo, n, p);
    int idx = -1;
    if (k < n_max && key_s[k] != kOutside) {
        idx = val_s[k];
        if (idx < 0 || idx >= n) idx = -1;
    }
    if (order) order[k] = idx;
    if (pot && idx >= 0) {
        const int g = lo + idx;
        pot[g] = __dadd_rn(pot[g], tukey(pts + (size_t)g * 3, centre, r2));
        touched[g >> kPotShift] = 1;
    }
}

// s3dis_sphere.py:303-347 for B spheres.  perm NULL: no shuffle; pad >= 0, or floor(pad_u * count) where it is negative or NULL
__global__ __launch_bounds__(kSphThreads) void sphere_tail_kernel(int clouds, int num_points, int g, const float *__restrict__ pts,
                                                                  const float *__restrict__ colour, const long long *__restrict__ label,
                                                                  const int *__restrict__ cloud_off, const int *__restrict__ cloud,
                                                                  const int *__restrict__ point, const double *__restrict__ centre,
                                                                  const int *__restrict__ order, const int *__restrict__ count,
                                                                  const int *__restrict__ perm, const int *__restrict__ pad,
                                                                  const double *__restrict__ pad_u, long long *__restrict__ inds_out,
                                                                  int *__restrict__ mask_out, float *__restrict__ pos_out,
                                                                  float *__restrict__ x_out, long long *__restrict__ y_out,
                                                                  float *__restrict__ heights)
{
    const int b = blockIdx.y, k = blockIdx.x * kSphThreads + threadIdx.x;
    if (k >= num_points) return;
    int lo, n, p;
    sphere_cloud(clouds, cloud_off, cloud[b], point[b], lo, n, p);
    const size_t row = (size_t)b * num_points, o = row + k;
    const int cnt = min(max(count[b], 0), num_points);
    int idx = p;  // an empty sphere: the centre's own point in every slot, mask 0
    if (cnt > 0) {
        int j = k;
        if (k >= cnt) {
            j = pad ? pad[o] : -1;
            if (j < 0) j = pad_u ? (int)__dmul_rn(pad_u[o], (double)cnt) : 0;
            j = min(max(j, 0), cnt - 1);
        }
        if (perm) j = min(max(perm[row + j], 0), cnt - 1);
        idx = min(max(order[row + j], 0), max(n - 1, 0));
    }
    inds_out[o] = idx;
    mask_out[o] = k < cnt ? 1 : 0;
    if (n <= 0) return;
    const size_t q = (size_t)(lo + idx) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        pos_out[o * 3 + j] = (float)__dsub_rn((double)pts[q + j], centre[b * 3 + j]);
        x_out[o * 3 + j] = colour[q + j];
    }
    y_out[o] = label[lo + idx];
    heights[o] = pts[q + g];
}

static size_t sphere_sort_temp(int n)
{
    size_t a = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const int *)nullptr, (int *)nullptr, n);
    return align256(a);
}

static size_t sphere_workspace(int n_max)
{
    if (n_max <= 0) return 0;
    // keys | sorted keys | points | sorted points | the sort's temp
    return 2 * align256((size_t)n_max * 8) + 2 * align256((size_t)n_max * 4) + sphere_sort_temp(n_max) + 256;
}

// keys, the sort and finish for the sphere whose record is (*cloud, *point, noise[0..2])
static int sphere_one(const char *what, int clouds, int n_max, int num_points, double r2, const float *pts, const int *cloud_off,
                      const int *cloud, const int *point, const double *noise, double *centre, int *order, int *cur, int *count,
                      double *pot, int *touched, void *workspace, hipStream_t stream)
{
    char *w = (char *)workspace;
    unsigned long long *key = (unsigned long long *)w; w += align256((size_t)n_max * 8);
    unsigned long long *key_s = (unsigned long long *)w; w += align256((size_t)n_max * 8);
    int *val = (int *)w; w += align256((size_t)n_max * 4);
    int *val_s = (int *)w; w += align256((size_t)n_max * 4);
    hipLaunchKernelGGL(sphere_keys_kernel, dim3(div_up(n_max, kSphThreads)), dim3(kSphThreads), 0, stream, clouds, n_max, r2, pts,
                       cloud_off, cloud, point, noise, centre, key, val);
    size_t temp = sphere_sort_temp(n_max);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(w, temp, (const unsigned long long *)key, key_s, (const int *)val, val_s, n_max,
                                                      0, 64, stream);
    if (e != hipSuccess) { set_error("%s: radix sort: %s", what, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(sphere_finish_kernel, dim3(div_up(num_points, kSphThreads)), dim3(kSphThreads), 0, stream, clouds, n_max,
                       num_points, r2, pts, cloud_off, cloud, (const double *)centre, (const unsigned long long *)key_s,
                       (const int *)val_s, order, cur, count, pot, touched);
    return 0;
}

static bool sphere_sizes_ok(int clouds, int total, int n_max, int count, int num_points, double radius)
{
    return clouds > 0 && total > 0 && n_max > 0 && n_max <= total && count >= 0 && num_points > 0 && radius > 0.0 &&
           (long long)count * num_points <= 0x7fffffffLL;
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_sphere_workspace_bytes(int n_max) { return sphere_workspace(n_max); }

AMC_API int amc3d_sphere_minima(int total, const double *potentials, double *blk_val, int *blk_idx, int *touched, void *stream)
{
    if (total <= 0) return 0;
    if (!potentials || !blk_val || !blk_idx || !touched) return bad_arg("amc3d_sphere_minima: bad argument");
    hipLaunchKernelGGL(sphere_minima_kernel, dim3(div_up(total, kPotBlock)), dim3(kSphThreads), 0, (hipStream_t)stream, total, 0,
                       (const int *)nullptr, (const int *)nullptr, potentials, blk_val, blk_idx, touched);
    return launch_status("amc3d_sphere_minima");
}

AMC_API int amc3d_sphere_schedule(int clouds, int total, int n_max, int nb_max, int steps, int num_points, double radius,
                                  const float *points, const int *cloud_off, double *potentials, double *blk_val, int *blk_idx,
                                  int *touched, const double *noise, int *cloud_ind, int *point_ind, double *centre, int *order,
                                  int *cur, int *count, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *what = "amc3d_sphere_schedule";
    if (steps == 0) return 0;
    if (!sphere_sizes_ok(clouds, total, n_max, steps, num_points, radius) || nb_max <= 0 || !points || !cloud_off || !potentials ||
        !blk_val || !blk_idx || !touched || !noise || !cloud_ind || !point_ind || !centre || !cur || !count || !workspace ||
        workspace_bytes < sphere_workspace(n_max))
        return bad_arg("amc3d_sphere_schedule: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const double r2 = radius * radius;
    const int nblk = div_up(total, kPotBlock);
    for (int s = 0; s < steps; ++s) {
        hipLaunchKernelGGL(sphere_pick_kernel, dim3(1), dim3(1024), 0, stream, clouds, nblk, cloud_off, (const double *)blk_val,
                           (const int *)blk_idx, cloud_ind + s, point_ind + s);
        int rc = sphere_one(what, clouds, n_max, num_points, r2, points, cloud_off, cloud_ind + s, point_ind + s, noise + (size_t)s * 3,
                            centre + (size_t)s * 3, order ? order + (size_t)s * num_points : nullptr, cur + s, count + s, potentials,
                            touched, workspace, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(sphere_minima_kernel, dim3(nb_max), dim3(kSphThreads), 0, stream, total, clouds, cloud_off,
                           (const int *)(cloud_ind + s), (const double *)potentials, blk_val, blk_idx, touched);
    }
    return launch_status(what);
}

AMC_API int amc3d_sphere_query(int clouds, int total, int n_max, int spheres, int num_points, double radius, const float *points,
                               const int *cloud_off, const int *cloud_ind, const int *point_ind, const double *noise, double *centre,
                               int *order, int *cur, int *count, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "amc3d_sphere_query";
    if (spheres == 0) return 0;
    if (!sphere_sizes_ok(clouds, total, n_max, spheres, num_points, radius) || !points || !cloud_off || !cloud_ind || !point_ind ||
        !noise || !centre || !order || !cur || !count || !workspace || workspace_bytes < sphere_workspace(n_max))
        return bad_arg("amc3d_sphere_query: bad argument");
    const double r2 = radius * radius;
    for (int s = 0; s < spheres; ++s) {
        int rc = sphere_one(what, clouds, n_max, num_points, r2, points, cloud_off, cloud_ind + s, point_ind + s, noise + (size_t)s * 3,
                            centre + (size_t)s * 3, order + (size_t)s * num_points, cur + s, count + s, nullptr, nullptr, workspace,
                            (hipStream_t)stream);
        if (rc) return rc;
    }
    return launch_status(what);
}

AMC_API int amc3d_sphere_tail(int clouds, int spheres, int num_points, int gravity_dim, const float *points, const float *colours,
                              const long long *labels, const int *cloud_off, const int *cloud_ind, const int *point_ind,
                              const double *centre, const int *order, const int *count, const int *perm, const int *pad,
                              const double *pad_u, long long *input_inds, int *mask, float *pos, float *x, long long *y,
                              float *heights, void *stream)
{
    if (spheres == 0) return 0;
    if (clouds <= 0 || spheres < 0 || spheres > 65535 || num_points <= 0 || gravity_dim < 0 || gravity_dim > 2 ||
        (long long)spheres * num_points > 0x7fffffffLL || !points || !colours || !labels || !cloud_off || !cloud_ind || !point_ind ||
        !centre || !order || !count || !input_inds || !mask || !pos || !x || !y || !heights)
        return bad_arg("amc3d_sphere_tail: bad argument");
    hipLaunchKernelGGL(sphere_tail_kernel, dim3(div_up(num_points, kSphThreads), spheres), dim3(kSphThreads), 0, (hipStream_t)stream,
                       clouds, num_points, gravity_dim, points, colours, labels, cloud_off, cloud_ind, point_ind, centre, order, count,
                       perm, pad, pad_u, input_inds, mask, pos, x, y, heights);
    return launch_status("amc3d_sphere_tail");
}
