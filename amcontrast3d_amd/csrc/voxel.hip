// Input pipeline of the S3DIS / ScanNet loaders on the device:
//   voxelize   openpoints/dataset/data_util.py:92-141  floor(coord / voxel) -> FNV-1a 64-bit hash of the three cell
//              coordinates -> argsort -> unique / counts (one random or every point per voxel)
//   crop_pc    :146-174  the voxel_max points nearest to a seed point: argsort of the squared distances
// The reference does this in numpy inside 6 loader workers; at > 18 M points/s per GPU that is the bottleneck.
// Here: one kernel for the keys, a stable LSD radix sort of (key, index) pairs (hipCUB / rocPRIM device primitive --
// a plain library sort, as rocBLAS is for plain GEMMs), run-length kernels for voxel ids / starts / counts, and the
// same for the crop with the distance bits as keys.  numpy's argsort is NOT stable: which order the points of one
// voxel (or two equidistant points) come in is unspecified by the reference; a stable order is one valid choice.
// Arithmetic as numpy does it under numpy 2 (the container's): coord (float32) / np.array(voxel_size) is a float64
// division (a 0-d array is not a weak scalar), floor in float64, cast to uint64; squared distances in float32 without
// contraction, ((dx^2 + dy^2) + dz^2).
// ScanNet's chain (dataset/scannetv2/scannet.py:140-176) rotates the raw room with np.dot(pos_f32, R_f64) before crop_pc, so
// its coordinates reach voxelize and the crop as float64: the *_f64 entry points take double coordinates (same hash of
// floor(coord / voxel), distances ((dx^2 + dy^2) + dz^2) in double, sorted on their 64-bit patterns).
#include "cub_kernel_memset.h"  // hipCUB with its memsets as kernels (graph-safe)

#include "room_common.h"

namespace amc {

// T = float (S3DIS) or double (ScanNet): the division and floor are float64 either way
template <typename T>
__global__ void voxel_key_kernel(int n, const T *__restrict__ coord, double voxel, unsigned long long *__restrict__ key,
                                 int *__restrict__ iota)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long h = 14695981039346656037ULL;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double c = floor((double)coord[(size_t)i * 3 + j] / voxel);
        h *= 1099511628211ULL;
        h ^= (unsigned long long)(long long)c;  // non-negative by contract (the cloud is shifted to its min corner first)
    }
    key[i] = h;
    iota[i] = i;
}

// head[i] = 1 where a new voxel starts in the sorted key sequence
__global__ void voxel_head_kernel(int n, const unsigned long long *__restrict__ ks, int *__restrict__ head)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = (i == 0 || ks[i] != ks[i - 1]) ? 1 : 0;
}

// incl = inclusive scan of head: voxel id of sorted position i is incl[i] - 1
__global__ void voxel_start_kernel(int n, const int *__restrict__ head, const int *__restrict__ incl, int *__restrict__ voxel_idx,
                                   int *__restrict__ start, int *__restrict__ nvox)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = incl[i] - 1;
    voxel_idx[i] = v;
    if (head[i]) start[v] = i;
    if (i == n - 1) { *nvox = v + 1; start[v + 1] = n; }
}

__global__ void voxel_count_kernel(int n, const int *__restrict__ nvox, const int *__restrict__ start, int *__restrict__ count)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) count[v] = v < *nvox ? start[v + 1] - start[v] : 0;
}

__global__ void voxel_select_kernel(int nvox, const int *__restrict__ start, const int *__restrict__ count,
                                    const int *__restrict__ idx_sort, const int *__restrict__ rnd, int *__restrict__ out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nvox) out[v] = idx_sort[start[v] + rnd[v] % count[v]];
}

// C = float or double: distances in C, their bit patterns (non-negative values order like them) as 32- or 64-bit keys
template <typename C, typename K>
__global__ void crop_d2_kernel(int n, const C *__restrict__ coord, int init, C *__restrict__ d2, K *__restrict__ bits,
                               int *__restrict__ iota)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t p = (size_t)i * 3, q = (size_t)init * 3;
    const C d = dist2_ref(coord[p], coord[p + 1], coord[p + 2], coord[q], coord[q + 1], coord[q + 2]);
    d2[i] = d;
    bits[i] = order_bits(d);
    iota[i] = i;
}

__global__ void copy_i32_kernel(int n, const int *__restrict__ src, int *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

static size_t sort64_temp(int n)
{
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                       (const int *)nullptr, (int *)nullptr, n);
    size_t s = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, s, (const int *)nullptr, (int *)nullptr, n);
    return align256(t > s ? t : s);
}

static size_t sort32_temp(int n)
{
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const unsigned *)nullptr, (unsigned *)nullptr, (const int *)nullptr,
                                       (int *)nullptr, n);
    return align256(t);
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_voxelize_workspace_bytes(int n)
{
    if (n <= 0) return 0;
    // sorted keys | iota | head | incl | sort / scan temp
    return align256((size_t)n * 8) + 3 * align256((size_t)n * 4) + sort64_temp(n) + 256;
}

template <typename T>
static int voxelize_impl(const char *what, int n, const T *coord, double voxel_size, unsigned long long *key, int *idx_sort,
                         int *voxel_idx, int *start, int *count, int *nvox, void *workspace, size_t workspace_bytes,
                         hipStream_t stream)
{
    if (n <= 0) return 0;
    if (!coord || !(voxel_size > 0.0) || !key || !idx_sort || !voxel_idx || !start || !count || !nvox || !workspace ||
        workspace_bytes < amc3d_voxelize_workspace_bytes(n)) {
        set_error("%s: bad argument", what);
        return (int)hipErrorInvalidValue;
    }
    char *w = (char *)workspace;
    unsigned long long *ks = (unsigned long long *)w; w += align256((size_t)n * 8);
    int *iota = (int *)w; w += align256((size_t)n * 4);
    int *head = (int *)w; w += align256((size_t)n * 4);
    int *incl = (int *)w; w += align256((size_t)n * 4);
    size_t temp = sort64_temp(n);
    const int blocks = div_up(n, 256);
    hipLaunchKernelGGL(voxel_key_kernel<T>, dim3(blocks), dim3(256), 0, stream, n, coord, voxel_size, key, iota);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(w, temp, (const unsigned long long *)key, ks, (const int *)iota, idx_sort, n, 0, 64, stream);
    if (e != hipSuccess) { set_error("%s: radix sort: %s", what, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(voxel_head_kernel, dim3(blocks), dim3(256), 0, stream, n, (const unsigned long long *)ks, head);
    temp = sort64_temp(n);
    e = hipcub::DeviceScan::InclusiveSum(w, temp, (const int *)head, incl, n, stream);
    if (e != hipSuccess) { set_error("%s: scan: %s", what, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(voxel_start_kernel, dim3(blocks), dim3(256), 0, stream, n, (const int *)head, (const int *)incl, voxel_idx, start,
                       nvox);
    hipLaunchKernelGGL(voxel_count_kernel, dim3(blocks), dim3(256), 0, stream, n, (const int *)nvox, (const int *)start, count);
    return launch_status(what);
}

// coord (n,3) fp32, shifted to its min corner.  key (n): the FNV-1a hash of every point's cell (as fnv_hash_vec);
// idx_sort (n): point indices ordered by key (stable); voxel_idx (n): voxel id of sorted position i; start (n+1):
// first sorted position of every voxel (start[nvox] = n); count (n): points per voxel (0 beyond nvox); nvox (1).
AMC_API int amc3d_voxelize(int n, const float *coord, double voxel_size, unsigned long long *key, int *idx_sort, int *voxel_idx,
                           int *start, int *count, int *nvox, void *workspace, size_t workspace_bytes, void *stream_)
{
    return voxelize_impl("amc3d_voxelize", n, coord, voxel_size, key, idx_sort, voxel_idx, start, count, nvox, workspace,
                         workspace_bytes, (hipStream_t)stream_);
}

// the same for float64 coordinates (ScanNet's rotated rooms); workspace: amc3d_voxelize_workspace_bytes(n)
AMC_API int amc3d_voxelize_f64(int n, const double *coord, double voxel_size, unsigned long long *key, int *idx_sort,
                               int *voxel_idx, int *start, int *count, int *nvox, void *workspace, size_t workspace_bytes,
                               void *stream_)
{
    return voxelize_impl("amc3d_voxelize_f64", n, coord, voxel_size, key, idx_sort, voxel_idx, start, count, nvox, workspace,
                         workspace_bytes, (hipStream_t)stream_);
}

// train mode of voxelize (data_util.py:136-140): one point per voxel, idx_unique[v] = idx_sort[start[v] + rnd[v] % count[v]]
AMC_API int amc3d_voxel_select(int nvox, const int *start, const int *count, const int *idx_sort, const int *rnd, int *idx_unique,
                               void *stream)
{
    if (nvox <= 0) return 0;
    if (!start || !count || !idx_sort || !rnd || !idx_unique) return bad_arg("amc3d_voxel_select: null pointer");
    hipLaunchKernelGGL(voxel_select_kernel, dim3(div_up(nvox, 256)), dim3(256), 0, (hipStream_t)stream, nvox, start, count, idx_sort,
                       rnd, idx_unique);
    return launch_status("amc3d_voxel_select");
}

AMC_API size_t amc3d_crop_nearest_workspace_bytes(int n)
{
    if (n <= 0) return 0;
    return 4 * align256((size_t)n * 4) + sort32_temp(n) + 256;  // bits | sorted bits | iota | sorted idx | temp
}

AMC_API size_t amc3d_crop_nearest_f64_workspace_bytes(int n)
{
    if (n <= 0) return 0;
    // bits | sorted bits (8 B each) | iota | sorted idx | temp
    return 2 * align256((size_t)n * 8) + 2 * align256((size_t)n * 4) + sort64_temp(n) + 256;
}

// K: the key type, unsigned for float and unsigned long long for double coordinates
template <typename C, typename K>
static int crop_nearest_impl(const char *what, int n, const C *coord, int init_idx, int keep, C *d2, int *crop_idx, void *workspace,
                             size_t workspace_bytes, hipStream_t stream)
{
    if (n <= 0 || keep <= 0) return 0;
    const bool k32 = sizeof(K) == 4;
    const size_t need = k32 ? amc3d_crop_nearest_workspace_bytes(n) : amc3d_crop_nearest_f64_workspace_bytes(n);
    size_t temp = k32 ? sort32_temp(n) : sort64_temp(n);
    if (!coord || init_idx < 0 || init_idx >= n || keep > n || !d2 || !crop_idx || !workspace || workspace_bytes < need) {
        set_error("%s: bad argument", what);
        return (int)hipErrorInvalidValue;
    }
    char *w = (char *)workspace;
    K *bits = (K *)w; w += align256((size_t)n * sizeof(K));
    K *sbits = (K *)w; w += align256((size_t)n * sizeof(K));
    int *iota = (int *)w; w += align256((size_t)n * 4);
    int *sidx = (int *)w; w += align256((size_t)n * 4);
    hipLaunchKernelGGL((crop_d2_kernel<C, K>), dim3(div_up(n, 256)), dim3(256), 0, stream, n, coord, init_idx, d2, bits, iota);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(w, temp, (const K *)bits, sbits, (const int *)iota, sidx, n, 0,
                                                      8 * (int)sizeof(K), stream);
    if (e != hipSuccess) { set_error("%s: radix sort: %s", what, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(copy_i32_kernel, dim3(div_up(keep, 256)), dim3(256), 0, stream, keep, (const int *)sidx, crop_idx);
    return launch_status(what);
}

// crop_pc's nearest-N crop (data_util.py:157-160): d2 (n) = squared distance of every point to coord[init_idx];
// crop_idx (keep) = the keep nearest points in ascending distance (stable among equal distances)
AMC_API int amc3d_crop_nearest(int n, const float *coord, int init_idx, int keep, float *d2, int *crop_idx, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return crop_nearest_impl<float, unsigned>("amc3d_crop_nearest", n, coord, init_idx, keep, d2, crop_idx, workspace, workspace_bytes,
                                              (hipStream_t)stream);
}

// crop_pc's crop on float64 coordinates: d2 (n) double, crop_idx (keep) as amc3d_crop_nearest
AMC_API int amc3d_crop_nearest_f64(int n, const double *coord, int init_idx, int keep, double *d2, int *crop_idx, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return crop_nearest_impl<double, unsigned long long>("amc3d_crop_nearest_f64", n, coord, init_idx, keep, d2, crop_idx, workspace,
                                                         workspace_bytes, (hipStream_t)stream);
}
