// S3DIS training input on the device (gfx950): S3DIS.__getitem__ with presample=False (dataset/s3dis/s3dis.py:122-144) up to
// the transform chain, plus the collate, for a whole batch of RAW rooms per call.
//
// The reference, per room and in numpy: np.load(...).astype(float32); xyz -= xyz.min(0); crop_pc (dataset/data_util.py:146-174:
// min-corner shift, voxelize mode 0, nearest-voxel_max crop or padding by repetition, shuffle, min-corner shift, cast).
// voxel.hip does that for one room per call, and the caller reads the voxel count, count.max() and the crop centre back for
// every room.  Here the rooms are one ragged batch -- rows of one (rows,7) array {xyz, rgb 0..255, label}, fp32 or fp64; room r
// is rows [src[r], src[r] + offsets[r+1] - offsets[r]) and points [offsets[r], offsets[r+1]) of the batch -- and every stage is
// one launch (or one library sort) for all of them:
//   min corner   kMinBlocks workgroups per room, then a fold; min is exact, so any order gives the same corner
//   keys         coord = fl32(xyz) - corner in fp32, FNV-1a of floor(coord / voxel) in fp64: voxel.hip's voxel_key_kernel
//   order        by (room, key), stable.  rocPRIM's segmented radix sort gives a long segment to ONE workgroup
//                (device_segmented_radix_sort.hpp launches dim3(segments), or dim3(large_segment_count) after partitioning
//                by length), so eight million-point rooms would sort on eight CUs.  Instead: one device-wide stable sort of
//                (key, point) over all 64 key bits, then one device-wide stable pass over the ceil(log2 rooms) bits of the
//                room id -- LSD order, so the order inside a room is the first sort's
//   voxels       heads (a room boundary is a head even between equal keys), one scan, starts, counts; per-room first voxel
//                (vbase) and count.max() (cmax) stay on the device
//   select       sel[v] = idx_sort[start[v] + rnd[v] % count[v]], rnd given or floor(u * count.max()) of a fp64 uniform
//   crop         d2 of every representative to its own room's centre, fp32 ((dx^2 + dy^2) + dz^2) as crop_d2_kernel; one
//                device-wide stable sort on (room << 32) | bits(d2); a room's first voxel_max sorted entries are its crop
//   tail         one workgroup per room: slot k <- representative crop[perm[k]] (rooms below voxel_max: identity + pad), minus
//                the cropped cloud's fp32 min corner; colours and label cast from the raw row
// All arithmetic is exact by construction (fp32 subtract, fp64 divide and floor, integer hash, non-contracted fp32 distance), so
// the result equals the per-room route's bit for bit.  Random draws are the caller's: the library has no generator.
#include "cub_kernel_memset.h"  // hipCUB with its memsets as kernels (graph-safe)

#include "common.h"

namespace amc {

constexpr int kMinBlocks = 64;  // workgroups per room in the strided per-room passes
constexpr int kMinThreads = 256;

// the last room whose first element is <= i (tab: rooms + 1 ascending entries)
template <typename I>
__device__ __forceinline__ int seg_of(int rooms, const I *__restrict__ tab, I i)
{
    int lo = 0, hi = rooms - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// per (room, workgroup) partial minimum of fl32(xyz) -> part[(r * kMinBlocks + blk) * 3 + j]
template <typename T>
__global__ __launch_bounds__(kMinThreads) void s3dis_min_kernel(const T *__restrict__ raw, const long long *__restrict__ src,
                                                                const long long *__restrict__ off, float *__restrict__ part)
{
    __shared__ float s[kMinThreads / 64][3];
    const int r = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = off[r + 1] - off[r], row0 = src[r];
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f};
    for (long long i = (long long)blk * kMinThreads + threadIdx.x; i < n; i += (long long)kMinBlocks * kMinThreads) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fminf(mn[j], (float)raw[(size_t)(row0 + i) * 7 + j]);
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fminf(mn[j], __shfl_xor(mn[j], d, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s[wave][j] = mn[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = s[0][threadIdx.x];
        for (int w = 1; w < kMinThreads / 64; ++w) v = fminf(v, s[w][threadIdx.x]);
        part[((size_t)r * kMinBlocks + blk) * 3 + threadIdx.x] = v;
    }
}

// corner (rooms,3) from the partials; cmax zeroed for the atomic maximum of s3dis_count_kernel
__global__ void s3dis_corner_kernel(int rooms, const float *__restrict__ part, float *__restrict__ corner, int *__restrict__ cmax)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rooms * 3) return;
    const int r = t / 3, j = t - r * 3;
    float v = part[(size_t)r * kMinBlocks * 3 + j];
    for (int k = 1; k < kMinBlocks; ++k) v = fminf(v, part[((size_t)r * kMinBlocks + k) * 3 + j]);
    corner[t] = v;
    if (j == 0) cmax[r] = 0;
}

// s3dis.py:129-130 and crop_pc's own shift (of a cloud whose minimum is then exactly 0: it changes nothing), then the cell hash
template <typename T>
__global__ __launch_bounds__(256) void s3dis_key_kernel(int rooms, long long total, const T *__restrict__ raw,
                                                        const long long *__restrict__ src, const long long *__restrict__ off,
                                                        const float *__restrict__ corner, double voxel, float *__restrict__ coord,
                                                        unsigned long long *__restrict__ key, int *__restrict__ iota)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int r = seg_of<long long>(rooms, off, i);
    const size_t row = (size_t)(src[r] + (i - off[r]));
    unsigned long long h = 14695981039346656037ULL;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float c = __fsub_rn((float)raw[row * 7 + j], corner[r * 3 + j]);
        coord[(size_t)i * 3 + j] = c;
        h *= 1099511628211ULL;
        h ^= (unsigned long long)(long long)floor((double)c / voxel);  // c >= 0: the cloud sits at its min corner
    }
    key[i] = h;
    iota[i] = (int)i;
}

__global__ void s3dis_room_id_kernel(int rooms, int total, const long long *__restrict__ off, const int *__restrict__ idx,
                                     unsigned *__restrict__ room)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) room[i] = (unsigned)seg_of<long long>(rooms, off, (long long)idx[i]);
}

// room: the room of every sorted position (NULL: one room)
__global__ void s3dis_head_kernel(int total, const unsigned long long *__restrict__ key, const int *__restrict__ idx_sort,
                                  const unsigned *__restrict__ room, int *__restrict__ head)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    head[i] = (i == 0 || (room && room[i] != room[i - 1]) || key[idx_sort[i]] != key[idx_sort[i - 1]]) ? 1 : 0;
}

__global__ void s3dis_start_kernel(int rooms, int total, const int *__restrict__ head, const int *__restrict__ incl,
                                   const unsigned *__restrict__ room, int *__restrict__ start, int *__restrict__ vbase)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int v = incl[i] - 1;
    if (head[i]) start[v] = i;
    if (i == 0) vbase[0] = 0;
    else if (room && room[i] != room[i - 1]) vbase[room[i]] = v;
    if (i == total - 1) { vbase[rooms] = v + 1; start[v + 1] = total; }
}

// count[v] of the room's voxels and the room's count.max()
__global__ __launch_bounds__(kMinThreads) void s3dis_count_kernel(const int *__restrict__ vbase, const int *__restrict__ start,
                                                                  int *__restrict__ count, int *__restrict__ cmax)
{
    __shared__ int s[kMinThreads / 64];
    const int r = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int end = vbase[r + 1];
    int m = 0;
    for (int v = vbase[r] + blockIdx.x * kMinThreads + threadIdx.x; v < end; v += kMinBlocks * kMinThreads) {
        const int c = start[v + 1] - start[v];
        count[v] = c;
        m = max(m, c);
    }
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
    if (lane == 0) s[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMinThreads / 64; ++w) m = max(m, s[w]);
        if (m > 0) atomicMax(&cmax[r], m);
    }
}

// voxelize mode 0 (data_util.py:137-140); rnd[v] < 0 or rnd NULL: floor(u[v] * count.max()) of the voxel's room
__global__ void s3dis_select_kernel(int rooms, int nvox, const int *__restrict__ vbase, const int *__restrict__ cmax,
                                    const int *__restrict__ start, const int *__restrict__ count, const int *__restrict__ idx_sort,
                                    const int *__restrict__ rnd, const double *__restrict__ u, int *__restrict__ sel)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvox) return;
    int r = rnd ? rnd[v] : -1;
    if (r < 0) r = u ? (int)__dmul_rn(u[v], (double)cmax[seg_of<int>(rooms, vbase, v)]) : 0;
    sel[v] = idx_sort[start[v] + r % count[v]];
}

// the crop centre of room r: init[r] >= 0, or min(floor(init_u[r] * nv), nv - 1)
__device__ __forceinline__ int crop_centre(int r, int nv, const int *__restrict__ init, const double *__restrict__ init_u)
{
    int c = init ? init[r] : -1;
    if (c < 0) c = init_u ? (int)__dmul_rn(init_u[r], (double)nv) : 0;
    return min(max(c, 0), nv - 1);
}

// data_util.py:158-160 for every room with at least voxel_max voxels; the others keep their order (key = local voxel id)
__global__ void s3dis_d2_kernel(int rooms, int nvox, int voxel_max, const int *__restrict__ vbase, const float *__restrict__ coord,
                                const int *__restrict__ sel, const int *__restrict__ init, const double *__restrict__ init_u,
                                float *__restrict__ d2, unsigned long long *__restrict__ ckey, int *__restrict__ iota)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvox) return;
    const int r = seg_of<int>(rooms, vbase, v);
    const int nv = vbase[r + 1] - vbase[r];
    unsigned low = (unsigned)(v - vbase[r]);
    float d = 0.f;
    if (nv >= voxel_max) {
        const size_t p = (size_t)sel[v], q = (size_t)sel[vbase[r] + crop_centre(r, nv, init, init_u)];
        d = dist2_ref(coord[p * 3], coord[p * 3 + 1], coord[p * 3 + 2], coord[q * 3], coord[q * 3 + 1], coord[q * 3 + 2]);
        low = __float_as_uint(d);  // non-negative floats order like their bit patterns
    }
    d2[v] = d;
    ckey[v] = ((unsigned long long)r << 32) | low;
    iota[v] = v;
}

// slot k of room r -> its voxel: crop order for a room with >= voxel_max voxels, else identity, then the padding draws
__device__ __forceinline__ int tail_voxel(int k, int n, int nv, int vb, int voxel_max, const int *__restrict__ order,
                                          const int *__restrict__ pad, const int *__restrict__ perm)
{
    int c = perm ? perm[k] : k;
    c = min(max(c, 0), n - 1);
    if (nv >= voxel_max && order) return order[vb + min(c, nv - 1)];
    if (c >= nv) c = pad ? min(max(pad[c], 0), nv - 1) : nv - 1;
    return vb + c;
}

template <typename T>
__global__ __launch_bounds__(1024) void s3dis_tail_kernel(int n, int voxel_max, const T *__restrict__ raw,
                                                          const long long *__restrict__ src, const long long *__restrict__ off,
                                                          const float *__restrict__ coord, const int *__restrict__ vbase,
                                                          const int *__restrict__ sel, const int *__restrict__ order,
                                                          const int *__restrict__ pad, const int *__restrict__ perm,
                                                          float *__restrict__ pos_out, float *__restrict__ col_out,
                                                          long long *__restrict__ y_out)
{
    __shared__ float s_mn[16][3];
    __shared__ float s_corner[3];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int vb = vbase[r], nv = vbase[r + 1] - vb;
    const int *pd = pad ? pad + (size_t)r * n : nullptr, *pm = perm ? perm + (size_t)r * n : nullptr;
    // crop_pc's last `coord -= coord.min(0)` (data_util.py:173); the shuffle does not change the set
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f};
    for (int k = threadIdx.x; k < n; k += 1024) {
        const size_t p = (size_t)sel[tail_voxel(k, n, nv, vb, voxel_max, order, pd, nullptr)];
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fminf(mn[j], coord[p * 3 + j]);
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fminf(mn[j], __shfl_xor(mn[j], d, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s_mn[wave][j] = mn[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = s_mn[0][threadIdx.x];
        for (int w = 1; w < 16; ++w) v = fminf(v, s_mn[w][threadIdx.x]);
        s_corner[threadIdx.x] = v;
    }
    __syncthreads();
    const long long row0 = src[r] - off[r];
    for (int k = threadIdx.x; k < n; k += 1024) {
        const size_t p = (size_t)sel[tail_voxel(k, n, nv, vb, voxel_max, order, pd, pm)];
        const size_t row = (size_t)(row0 + (long long)p), o = (size_t)r * n + k;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pos_out[o * 3 + j] = __fsub_rn(coord[p * 3 + j], s_corner[j]);
            col_out[o * 3 + j] = (float)raw[row * 7 + 3 + j];
        }
        y_out[o] = (long long)(float)raw[row * 7 + 6];
    }
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static int room_bits(int rooms)
{
    int bits = 0;
    while ((1 << bits) < rooms) ++bits;
    return bits;
}

static size_t voxelize_temp(int n)
{
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const int *)nullptr, (int *)nullptr, n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const unsigned *)nullptr, (unsigned *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, c, (const int *)nullptr, (int *)nullptr, n);
    return align256(a > b ? (a > c ? a : c) : (b > c ? b : c));
}

static size_t crop_temp(int n)
{
    size_t a = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const int *)nullptr, (int *)nullptr, n);
    return align256(a);
}

template <typename T>
static int voxelize_rooms(int rooms, int n, const T *raw, const long long *src, const long long *off, double voxel, float *coord,
                          unsigned long long *key, int *idx_sort, int *start, int *count, int *vbase, int *cmax, float *corner,
                          char *w, hipStream_t stream)
{
    unsigned long long *ks = (unsigned long long *)w; w += align256((size_t)n * 8);  // the first sort's keys
    int *iota = (int *)w; w += align256((size_t)n * 4);                              // then head
    int *idx1 = (int *)w; w += align256((size_t)n * 4);
    unsigned *rm = (unsigned *)w; w += align256((size_t)n * 4);                      // then incl
    unsigned *rms = (unsigned *)w; w += align256((size_t)n * 4);
    float *part = (float *)w; w += align256((size_t)rooms * kMinBlocks * 3 * sizeof(float));
    const int bits = room_bits(rooms), blocks = div_up(n, 256);
    size_t temp = voxelize_temp(n);
    hipLaunchKernelGGL(s3dis_min_kernel<T>, dim3(kMinBlocks, rooms), dim3(kMinThreads), 0, stream, raw, src, off, part);
    hipLaunchKernelGGL(s3dis_corner_kernel, dim3(div_up(rooms * 3, 64)), dim3(64), 0, stream, rooms, (const float *)part, corner, cmax);
    hipLaunchKernelGGL(s3dis_key_kernel<T>, dim3(blocks), dim3(256), 0, stream, rooms, (long long)n, raw, src, off,
                       (const float *)corner, voxel, coord, key, iota);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(w, temp, (const unsigned long long *)key, ks, (const int *)iota,
                                                      bits ? idx1 : idx_sort, n, 0, 64, stream);
    if (e != hipSuccess) { set_error("amc3d_s3dis_voxelize_rooms: radix sort: %s", hipGetErrorString(e)); return (int)e; }
    if (bits) {
        hipLaunchKernelGGL(s3dis_room_id_kernel, dim3(blocks), dim3(256), 0, stream, rooms, n, off, (const int *)idx1, rm);
        temp = voxelize_temp(n);
        e = hipcub::DeviceRadixSort::SortPairs(w, temp, (const unsigned *)rm, rms, (const int *)idx1, idx_sort, n, 0, bits, stream);
        if (e != hipSuccess) { set_error("amc3d_s3dis_voxelize_rooms: room sort: %s", hipGetErrorString(e)); return (int)e; }
    }
    const unsigned *room = bits ? rms : nullptr;
    int *head = iota, *incl = (int *)rm;
    hipLaunchKernelGGL(s3dis_head_kernel, dim3(blocks), dim3(256), 0, stream, n, (const unsigned long long *)key,
                       (const int *)idx_sort, room, head);
    temp = voxelize_temp(n);
    e = hipcub::DeviceScan::InclusiveSum(w, temp, (const int *)head, incl, n, stream);
    if (e != hipSuccess) { set_error("amc3d_s3dis_voxelize_rooms: scan: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(s3dis_start_kernel, dim3(blocks), dim3(256), 0, stream, rooms, n, (const int *)head, (const int *)incl, room,
                       start, vbase);
    hipLaunchKernelGGL(s3dis_count_kernel, dim3(kMinBlocks, rooms), dim3(kMinThreads), 0, stream, (const int *)vbase,
                       (const int *)start, count, cmax);
    return launch_status("amc3d_s3dis_voxelize_rooms");
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_s3dis_voxelize_workspace_bytes(int rooms, long long total)
{
    if (rooms <= 0 || total <= 0 || total > 0x7fffffffLL) return 0;
    const int n = (int)total;
    return align256((size_t)n * 8) + 4 * align256((size_t)n * 4) + align256((size_t)rooms * kMinBlocks * 3 * sizeof(float)) +
           voxelize_temp(n) + 256;
}

AMC_API int amc3d_s3dis_voxelize_rooms(int rooms, long long total, int raw_f64, const void *raw, const long long *src,
                                       const long long *offsets, double voxel_size, float *coord, unsigned long long *key,
                                       int *idx_sort, int *start, int *count, int *vbase, int *cmax, float *corner,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (rooms <= 0 || total <= 0) return 0;
    if (rooms > 1024 || total > 0x7fffffffLL) return bad_arg("amc3d_s3dis_voxelize_rooms: at most 1024 rooms and 2^31 - 1 points");
    if (!raw || !src || !offsets || !(voxel_size > 0.0) || !coord || !key || !idx_sort || !start || !count || !vbase || !cmax ||
        !corner || !workspace || workspace_bytes < amc3d_s3dis_voxelize_workspace_bytes(rooms, total))
        return bad_arg("amc3d_s3dis_voxelize_rooms: bad argument");
    if (raw_f64)
        return voxelize_rooms<double>(rooms, (int)total, (const double *)raw, src, offsets, voxel_size, coord, key, idx_sort, start,
                                      count, vbase, cmax, corner, (char *)workspace, (hipStream_t)stream);
    return voxelize_rooms<float>(rooms, (int)total, (const float *)raw, src, offsets, voxel_size, coord, key, idx_sort, start, count,
                                 vbase, cmax, corner, (char *)workspace, (hipStream_t)stream);
}

AMC_API size_t amc3d_s3dis_crop_workspace_bytes(int nvox)
{
    if (nvox <= 0) return 0;
    return 2 * align256((size_t)nvox * 8) + align256((size_t)nvox * 4) + crop_temp(nvox) + 256;  // keys | sorted keys | iota | temp
}

AMC_API int amc3d_s3dis_select_crop(int rooms, int nvox, int voxel_max, int any_crop, const float *coord, const int *idx_sort,
                                    const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd,
                                    const double *rnd_u, const int *init, const double *init_u, int *sel, float *d2, int *order,
                                    void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rooms <= 0 || nvox <= 0) return 0;
    if (rooms > 1024 || voxel_max <= 0 || !coord || !idx_sort || !start || !count || !vbase || !cmax || !sel ||
        (any_crop && (!d2 || !order || !workspace || workspace_bytes < amc3d_s3dis_crop_workspace_bytes(nvox))))
        return bad_arg("amc3d_s3dis_select_crop: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = div_up(nvox, 256);
    hipLaunchKernelGGL(s3dis_select_kernel, dim3(blocks), dim3(256), 0, stream, rooms, nvox, vbase, cmax, start, count, idx_sort, rnd,
                       rnd_u, sel);
    if (any_crop) {
        char *w = (char *)workspace;
        unsigned long long *ckey = (unsigned long long *)w; w += align256((size_t)nvox * 8);
        unsigned long long *skey = (unsigned long long *)w; w += align256((size_t)nvox * 8);
        int *iota = (int *)w; w += align256((size_t)nvox * 4);
        size_t temp = crop_temp(nvox);
        hipLaunchKernelGGL(s3dis_d2_kernel, dim3(blocks), dim3(256), 0, stream, rooms, nvox, voxel_max, vbase, coord, (const int *)sel,
                           init, init_u, d2, ckey, iota);
        hipError_t e = hipcub::DeviceRadixSort::SortPairs(w, temp, (const unsigned long long *)ckey, skey, (const int *)iota, order,
                                                          nvox, 0, 32 + room_bits(rooms), stream);
        if (e != hipSuccess) { set_error("amc3d_s3dis_select_crop: radix sort: %s", hipGetErrorString(e)); return (int)e; }
    }
    return launch_status("amc3d_s3dis_select_crop");
}

AMC_API int amc3d_s3dis_crop_tail(int rooms, int n, int voxel_max, int raw_f64, const void *raw, const long long *src,
                                  const long long *offsets, const float *coord, const int *vbase, const int *sel, const int *order,
                                  const int *pad, const int *perm, float *pos_out, float *colour_out, long long *y_out,
                                  void *stream)
{
    if (rooms <= 0 || n <= 0) return 0;
    if (voxel_max <= 0 || !raw || !src || !offsets || !coord || !vbase || !sel || !pos_out || !colour_out || !y_out)
        return bad_arg("amc3d_s3dis_crop_tail: bad argument");
    if (raw_f64)
        hipLaunchKernelGGL(s3dis_tail_kernel<double>, dim3(rooms), dim3(1024), 0, (hipStream_t)stream, n, voxel_max,
                           (const double *)raw, src, offsets, coord, vbase, sel, order, pad, perm, pos_out, colour_out, y_out);
    else
        hipLaunchKernelGGL(s3dis_tail_kernel<float>, dim3(rooms), dim3(1024), 0, (hipStream_t)stream, n, voxel_max,
                           (const float *)raw, src, offsets, coord, vbase, sel, order, pad, perm, pos_out, colour_out, y_out);
    return launch_status("amc3d_s3dis_crop_tail");
}
