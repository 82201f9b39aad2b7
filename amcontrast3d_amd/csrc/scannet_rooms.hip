// ScanNet training input on the device (gfx950), the part after the transform chain, for a whole batch of rooms per call:
// crop_pc (dataset/data_util.py:146-174) in float64 -- min-corner shift, voxelize mode 0, nearest-voxel_max crop or padding by
// repetition, shuffle, min-corner shift, cast -- and `heights` (dataset/scannetv2/scannet.py:168-176), plus the collate.
//
// scannet_input.hip transforms all rooms of a batch in one pass; what followed was voxel.hip's *_f64 entry points and one
// amc3d_scannet_crop_tail launch room by room, with the voxel count of every room read back in between.  This file is the
// float64 sibling of s3dis_input.hip: the rooms are one ragged batch -- pos (total,3) double, x (total,3) fp32 and y (total) int64
// as ScanNetTrainAugment leaves them, room r being points [offsets[r], offsets[r+1]) -- and every stage is one launch (or one
// library sort) for all of them:
//   min corner   kRoomBlocks workgroups per room, then a fold; min is exact, so any order gives the same corner
//   keys         coord = pos - corner in fp64, FNV-1a of floor(coord / voxel) in fp64: voxel.hip's voxel_key_kernel<double>
//   order        by (room, key), stable.  No segmented sort (rocPRIM gives a long segment to ONE workgroup, s3dis_input.hip):
//                one device-wide stable sort of (key, point) over all 64 key bits, then one device-wide stable pass over the
//                ceil(log2 rooms) bits of the room id -- LSD order, so the order inside a room is the first sort's.  One room
//                has no room bits: the second pass does not run
//   voxels       heads (a room boundary is a head even between equal keys), one scan, starts, counts; per-room first voxel
//                (vbase) and count.max() (cmax) stay on the device
//   select       sel[v] = idx_sort[start[v] + rnd[v] % count[v]], rnd given or floor(u * count.max()) of a fp64 uniform
//   crop         d2 of every representative to its own room's centre, fp64 ((dx^2 + dy^2) + dz^2) as crop_d2_f64_kernel.  The
//                composite key (room, 64 bits of d2) is wider than a radix key, so it is sorted as the voxel order is: one
//                stable sort over the 64 bits of d2 (>= +0: the pattern order is the value order), then the stable pass over
//                the room bits; a room's first voxel_max sorted entries are its crop
//   tail         kTailBlocks workgroups per room: partial fp64 minima of the room's n slots, then every gathering workgroup
//                folds its room's partials and writes slot k <- representative crop[perm[k]] (rooms below voxel_max: identity
//                + pad) minus that corner, cast to fp32; colours, label, heights = the gravity column
// All arithmetic is exact by construction (fp64 subtract, divide and floor, integer hash, non-contracted fp64 distance), so the
// result equals the per-room route's bit for bit.  Random draws are the caller's: the library has no generator.
#include "cub_kernel_memset.h"  // hipCUB with its memsets as kernels (graph-safe)

#include "common.h"

namespace amc {

constexpr int kRoomBlocks = 64;   // workgroups per room in the strided per-room passes over the raw points
constexpr int kRoomThreads = 256;
constexpr int kTailBlocks = 32;   // workgroups per room in the tail (64000 slots: 8 per thread)
constexpr int kTailThreads = 256;

// the last room whose first element is <= i (tab: rooms + 1 ascending entries)
template <typename I>
__device__ __forceinline__ int room_seg(int rooms, const I *__restrict__ tab, I i)
{
    int lo = 0, hi = rooms - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// three fp64 minima of a workgroup of kThreads threads -> out[0..2] (written by threads 0..2)
template <int kThreads>
__device__ __forceinline__ void block_min3(double mn[3], double (*s)[3], double *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fmin(mn[j], __shfl_xor(mn[j], d, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s[wave][j] = mn[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = s[0][threadIdx.x];
        for (int w = 1; w < kThreads / 64; ++w) v = fmin(v, s[w][threadIdx.x]);
        out[threadIdx.x] = v;
    }
}

// per (room, workgroup) partial minimum of pos -> part[(r * kRoomBlocks + blk) * 3 + j]
__global__ __launch_bounds__(kRoomThreads) void scannet_rooms_min_kernel(const double *__restrict__ pos,
                                                                         const long long *__restrict__ off,
                                                                         double *__restrict__ part)
{
    __shared__ double s[kRoomThreads / 64][3];
    const int r = blockIdx.y, blk = blockIdx.x;
    double mn[3] = {1.7e308, 1.7e308, 1.7e308};
    for (long long i = off[r] + (long long)blk * kRoomThreads + threadIdx.x; i < off[r + 1]; i += (long long)kRoomBlocks * kRoomThreads) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fmin(mn[j], pos[(size_t)i * 3 + j]);
    }
    block_min3<kRoomThreads>(mn, s, part + ((size_t)r * kRoomBlocks + blk) * 3);
}

// corner (rooms,3) from the partials; cmax zeroed for the atomic maximum of scannet_rooms_count_kernel
__global__ void scannet_rooms_corner_kernel(int rooms, const double *__restrict__ part, double *__restrict__ corner,
                                            int *__restrict__ cmax)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rooms * 3) return;
    const int r = t / 3, j = t - r * 3;
    double v = part[(size_t)r * kRoomBlocks * 3 + j];
    for (int k = 1; k < kRoomBlocks; ++k) v = fmin(v, part[((size_t)r * kRoomBlocks + k) * 3 + j]);
    corner[t] = v;
    if (j == 0) cmax[r] = 0;
}

// crop_pc's `coord -= coord.min(0)` (data_util.py:150) in fp64, then the cell hash
__global__ __launch_bounds__(256) void scannet_rooms_key_kernel(int rooms, int total, const double *__restrict__ pos,
                                                                const long long *__restrict__ off, const double *__restrict__ corner,
                                                                double voxel, double *__restrict__ coord,
                                                                unsigned long long *__restrict__ key, int *__restrict__ iota)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int r = room_seg<long long>(rooms, off, i);
    unsigned long long h = 14695981039346656037ULL;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double c = __dsub_rn(pos[(size_t)i * 3 + j], corner[r * 3 + j]);
        coord[(size_t)i * 3 + j] = c;
        h *= 1099511628211ULL;
        h ^= (unsigned long long)(long long)floor(c / voxel);  // c >= 0: the cloud sits at its min corner
    }
    key[i] = h;
    iota[i] = (int)i;
}

// the room of every entry of idx, looked up in tab (rooms + 1 ascending entries): points in offsets, voxels in vbase
template <typename I>
__global__ void scannet_rooms_id_kernel(int rooms, int n, const I *__restrict__ tab, const int *__restrict__ idx,
                                        unsigned *__restrict__ room)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) room[i] = (unsigned)room_seg<I>(rooms, tab, (I)idx[i]);
}

// room: the room of every sorted position (NULL: one room)
__global__ void scannet_rooms_head_kernel(int total, const unsigned long long *__restrict__ key, const int *__restrict__ idx_sort,
                                          const unsigned *__restrict__ room, int *__restrict__ head)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    head[i] = (i == 0 || (room && room[i] != room[i - 1]) || key[idx_sort[i]] != key[idx_sort[i - 1]]) ? 1 : 0;
}

__global__ void scannet_rooms_start_kernel(int rooms, int total, const int *__restrict__ head, const int *__restrict__ incl,
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
__global__ __launch_bounds__(kRoomThreads) void scannet_rooms_count_kernel(const int *__restrict__ vbase, const int *__restrict__ start,
                                                                           int *__restrict__ count, int *__restrict__ cmax)
{
    __shared__ int s[kRoomThreads / 64];
    const int r = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int end = vbase[r + 1];
    int m = 0;
    for (int v = vbase[r] + blockIdx.x * kRoomThreads + threadIdx.x; v < end; v += kRoomBlocks * kRoomThreads) {
        const int c = start[v + 1] - start[v];
        count[v] = c;
        m = max(m, c);
    }
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
    if (lane == 0) s[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRoomThreads / 64; ++w) m = max(m, s[w]);
        if (m > 0) atomicMax(&cmax[r], m);
    }
}

// voxelize mode 0 (data_util.py:137-140); rnd[v] < 0 or rnd NULL: floor(u[v] * count.max()) of the voxel's room
__global__ void scannet_rooms_select_kernel(int rooms, int nvox, const int *__restrict__ vbase, const int *__restrict__ cmax,
                                            const int *__restrict__ start, const int *__restrict__ count,
                                            const int *__restrict__ idx_sort, const int *__restrict__ rnd,
                                            const double *__restrict__ u, int *__restrict__ sel)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvox) return;
    int r = rnd ? rnd[v] : -1;
    if (r < 0) r = u ? (int)__dmul_rn(u[v], (double)cmax[room_seg<int>(rooms, vbase, v)]) : 0;
    sel[v] = idx_sort[start[v] + r % count[v]];
}

// the crop centre of room r: init[r] >= 0, or min(floor(init_u[r] * nv), nv - 1)
__device__ __forceinline__ int rooms_crop_centre(int r, int nv, const int *__restrict__ init, const double *__restrict__ init_u)
{
    int c = init ? init[r] : -1;
    if (c < 0) c = init_u ? (int)__dmul_rn(init_u[r], (double)nv) : 0;
    return min(max(c, 0), nv - 1);
}

// data_util.py:158-160 in fp64 for every room with at least voxel_max voxels; the others keep their order (key = local voxel id)
__global__ void scannet_rooms_d2_kernel(int rooms, int nvox, int voxel_max, const int *__restrict__ vbase,
                                        const double *__restrict__ coord, const int *__restrict__ sel, const int *__restrict__ init,
                                        const double *__restrict__ init_u, double *__restrict__ d2,
                                        unsigned long long *__restrict__ ckey, int *__restrict__ iota)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvox) return;
    const int r = room_seg<int>(rooms, vbase, v);
    const int nv = vbase[r + 1] - vbase[r];
    unsigned long long k = (unsigned long long)(v - vbase[r]);
    double d = 0.0;
    if (nv >= voxel_max) {
        const size_t p = (size_t)sel[v], q = (size_t)sel[vbase[r] + rooms_crop_centre(r, nv, init, init_u)];
        const double dx = __dsub_rn(coord[p * 3], coord[q * 3]);
        const double dy = __dsub_rn(coord[p * 3 + 1], coord[q * 3 + 1]);
        const double dz = __dsub_rn(coord[p * 3 + 2], coord[q * 3 + 2]);
        d = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        k = (unsigned long long)__double_as_longlong(d);  // non-negative doubles order like their bit patterns
    }
    d2[v] = d;
    ckey[v] = k;
    iota[v] = v;
}

// slot k of room r -> its voxel: crop order for a room with >= voxel_max voxels, else identity, then the padding draws
__device__ __forceinline__ int rooms_tail_voxel(int k, int n, int nv, int vb, int voxel_max, const int *__restrict__ order,
                                                const int *__restrict__ pad, const int *__restrict__ perm)
{
    int c = perm ? perm[k] : k;
    c = min(max(c, 0), n - 1);
    if (nv >= voxel_max && order) return order[vb + min(c, nv - 1)];
    if (c >= nv) c = pad ? min(max(pad[c], 0), nv - 1) : nv - 1;
    return vb + c;
}

// crop_pc's last `coord -= coord.min(0)` (data_util.py:173): per (room, workgroup) partial fp64 minimum of the room's n slots
// (the shuffle does not change the set, so the loop runs in crop order) -> part[(r * kTailBlocks + blk) * 3 + j]
__global__ __launch_bounds__(kTailThreads) void scannet_rooms_tail_min_kernel(int n, int voxel_max, const double *__restrict__ coord,
                                                                              const int *__restrict__ vbase, const int *__restrict__ sel,
                                                                              const int *__restrict__ order, const int *__restrict__ pad,
                                                                              double *__restrict__ part)
{
    __shared__ double s[kTailThreads / 64][3];
    const int r = blockIdx.y, blk = blockIdx.x;
    const int vb = vbase[r], nv = vbase[r + 1] - vb;
    const int *pd = pad ? pad + (size_t)r * n : nullptr;
    double mn[3] = {1.7e308, 1.7e308, 1.7e308};
    for (int k = blk * kTailThreads + threadIdx.x; k < n; k += kTailBlocks * kTailThreads) {
        const size_t p = (size_t)sel[rooms_tail_voxel(k, n, nv, vb, voxel_max, order, pd, nullptr)];
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = fmin(mn[j], coord[p * 3 + j]);
    }
    block_min3<kTailThreads>(mn, s, part + ((size_t)r * kTailBlocks + blk) * 3);
}

__global__ __launch_bounds__(kTailThreads) void scannet_rooms_tail_kernel(int n, int voxel_max, int g, const double *__restrict__ coord,
                                                                          const float *__restrict__ x, const long long *__restrict__ y,
                                                                          const int *__restrict__ vbase, const int *__restrict__ sel,
                                                                          const int *__restrict__ order, const int *__restrict__ pad,
                                                                          const int *__restrict__ perm, const double *__restrict__ part,
                                                                          float *__restrict__ pos_out, float *__restrict__ x_out,
                                                                          float *__restrict__ heights, long long *__restrict__ y_out)
{
    __shared__ double s_corner[3];
    const int r = blockIdx.y, blk = blockIdx.x;
    if (threadIdx.x < 3) {
        const double *P = part + (size_t)r * kTailBlocks * 3;
        double v = P[threadIdx.x];
        for (int k = 1; k < kTailBlocks; ++k) v = fmin(v, P[k * 3 + threadIdx.x]);
        s_corner[threadIdx.x] = v;
    }
    __syncthreads();
    const double c0 = s_corner[0], c1 = s_corner[1], c2 = s_corner[2];
    const int vb = vbase[r], nv = vbase[r + 1] - vb;
    const int *pd = pad ? pad + (size_t)r * n : nullptr, *pm = perm ? perm + (size_t)r * n : nullptr;
    for (int k = blk * kTailThreads + threadIdx.x; k < n; k += kTailBlocks * kTailThreads) {
        const size_t p = (size_t)sel[rooms_tail_voxel(k, n, nv, vb, voxel_max, order, pd, pm)], o = (size_t)r * n + k;
        const float q[3] = {(float)__dsub_rn(coord[p * 3], c0), (float)__dsub_rn(coord[p * 3 + 1], c1),
                            (float)__dsub_rn(coord[p * 3 + 2], c2)};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pos_out[o * 3 + j] = q[j];
            x_out[o * 3 + j] = x[p * 3 + j];
        }
        heights[o] = q[g];  // scannet.py:174-175: the shifted cloud's gravity minimum is exactly 0 (scannet_input.hip)
        y_out[o] = y[p];
    }
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static int room_bits(int rooms)
{
    int bits = 0;
    while ((1 << bits) < rooms) ++bits;
    return bits;
}

// the temporary storage of the 64-bit pair sort, the room-bit pair sort and the scan, whichever is largest
static size_t rooms_temp(int n)
{
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const int *)nullptr, (int *)nullptr, n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const unsigned *)nullptr, (unsigned *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, c, (const int *)nullptr, (int *)nullptr, n);
    return align256(a > b ? (a > c ? a : c) : (b > c ? b : c));
}

// stable order of n (key, value) pairs by (room of the value, key): LSD, the 64 key bits first, then the room bits.  tab: the
// rooms' first values (rooms + 1 ascending).  ks / v1 / rm / rms: n-element scratch; rms holds the sorted room ids afterwards
// (when rooms > 1)
template <typename I>
static hipError_t sort_by_room_then_key(int rooms, int n, const I *tab, const unsigned long long *key, unsigned long long *ks,
                                        const int *val, int *v1, unsigned *rm, unsigned *rms, int *out, void *temp_ptr,
                                        hipStream_t stream)
{
    const int bits = room_bits(rooms);
    size_t temp = rooms_temp(n);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp_ptr, temp, key, ks, val, bits ? v1 : out, n, 0, 64, stream);
    if (e != hipSuccess || !bits) return e;
    hipLaunchKernelGGL(scannet_rooms_id_kernel<I>, dim3(div_up(n, 256)), dim3(256), 0, stream, rooms, n, tab, (const int *)v1, rm);
    temp = rooms_temp(n);
    return hipcub::DeviceRadixSort::SortPairs(temp_ptr, temp, (const unsigned *)rm, rms, (const int *)v1, out, n, 0, bits, stream);
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_scannet_voxelize_workspace_bytes(int rooms, long long total)
{
    if (rooms <= 0 || total <= 0 || total > 0x7fffffffLL) return 0;
    const int n = (int)total;
    // sorted keys | iota, then head | first order | room ids, then incl | sorted room ids | min partials | sort / scan temp
    return align256((size_t)n * 8) + 4 * align256((size_t)n * 4) + align256((size_t)rooms * kRoomBlocks * 3 * sizeof(double)) +
           rooms_temp(n) + 256;
}

AMC_API int amc3d_scannet_voxelize_rooms(int rooms, long long total, const double *pos, const long long *offsets, double voxel_size,
                                         double *coord, unsigned long long *key, int *idx_sort, int *start, int *count, int *vbase,
                                         int *cmax, double *corner, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rooms <= 0 || total <= 0) return 0;
    if (rooms > 1024 || total > 0x7fffffffLL) return bad_arg("amc3d_scannet_voxelize_rooms: at most 1024 rooms and 2^31 - 1 points");
    if (!pos || !offsets || !(voxel_size > 0.0) || !coord || !key || !idx_sort || !start || !count || !vbase || !cmax || !corner ||
        !workspace || workspace_bytes < amc3d_scannet_voxelize_workspace_bytes(rooms, total))
        return bad_arg("amc3d_scannet_voxelize_rooms: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int n = (int)total;
    char *w = (char *)workspace;
    unsigned long long *ks = (unsigned long long *)w; w += align256((size_t)n * 8);  // the first sort's keys
    int *iota = (int *)w; w += align256((size_t)n * 4);                              // then head
    int *idx1 = (int *)w; w += align256((size_t)n * 4);
    unsigned *rm = (unsigned *)w; w += align256((size_t)n * 4);                      // then incl
    unsigned *rms = (unsigned *)w; w += align256((size_t)n * 4);
    double *part = (double *)w; w += align256((size_t)rooms * kRoomBlocks * 3 * sizeof(double));
    const int blocks = div_up(n, 256);
    hipLaunchKernelGGL(scannet_rooms_min_kernel, dim3(kRoomBlocks, rooms), dim3(kRoomThreads), 0, stream, pos, offsets, part);
    hipLaunchKernelGGL(scannet_rooms_corner_kernel, dim3(div_up(rooms * 3, 64)), dim3(64), 0, stream, rooms, (const double *)part,
                       corner, cmax);
    hipLaunchKernelGGL(scannet_rooms_key_kernel, dim3(blocks), dim3(256), 0, stream, rooms, n, pos, offsets, (const double *)corner,
                       voxel_size, coord, key, iota);
    hipError_t e = sort_by_room_then_key<long long>(rooms, n, offsets, key, ks, iota, idx1, rm, rms, idx_sort, w, stream);
    if (e != hipSuccess) { set_error("amc3d_scannet_voxelize_rooms: radix sort: %s", hipGetErrorString(e)); return (int)e; }
    const unsigned *room = rooms > 1 ? rms : nullptr;
    int *head = iota, *incl = (int *)rm;
    hipLaunchKernelGGL(scannet_rooms_head_kernel, dim3(blocks), dim3(256), 0, stream, n, (const unsigned long long *)key,
                       (const int *)idx_sort, room, head);
    size_t temp = rooms_temp(n);
    e = hipcub::DeviceScan::InclusiveSum(w, temp, (const int *)head, incl, n, stream);
    if (e != hipSuccess) { set_error("amc3d_scannet_voxelize_rooms: scan: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(scannet_rooms_start_kernel, dim3(blocks), dim3(256), 0, stream, rooms, n, (const int *)head, (const int *)incl,
                       room, start, vbase);
    hipLaunchKernelGGL(scannet_rooms_count_kernel, dim3(kRoomBlocks, rooms), dim3(kRoomThreads), 0, stream, (const int *)vbase,
                       (const int *)start, count, cmax);
    return launch_status("amc3d_scannet_voxelize_rooms");
}

AMC_API size_t amc3d_scannet_crop_workspace_bytes(int nvox)
{
    if (nvox <= 0) return 0;
    // keys | sorted keys | iota | first order | room ids | sorted room ids | sort temp
    return 2 * align256((size_t)nvox * 8) + 4 * align256((size_t)nvox * 4) + rooms_temp(nvox) + 256;
}

AMC_API int amc3d_scannet_select_crop(int rooms, int nvox, int voxel_max, int any_crop, const double *coord, const int *idx_sort,
                                      const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd,
                                      const double *rnd_u, const int *init, const double *init_u, int *sel, double *d2, int *order,
                                      void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rooms <= 0 || nvox <= 0) return 0;
    if (rooms > 1024 || voxel_max <= 0 || !coord || !idx_sort || !start || !count || !vbase || !cmax || !sel ||
        (any_crop && (!d2 || !order || !workspace || workspace_bytes < amc3d_scannet_crop_workspace_bytes(nvox))))
        return bad_arg("amc3d_scannet_select_crop: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = div_up(nvox, 256);
    hipLaunchKernelGGL(scannet_rooms_select_kernel, dim3(blocks), dim3(256), 0, stream, rooms, nvox, vbase, cmax, start, count,
                       idx_sort, rnd, rnd_u, sel);
    if (any_crop) {
        char *w = (char *)workspace;
        unsigned long long *ckey = (unsigned long long *)w; w += align256((size_t)nvox * 8);
        unsigned long long *skey = (unsigned long long *)w; w += align256((size_t)nvox * 8);
        int *iota = (int *)w; w += align256((size_t)nvox * 4);
        int *ord1 = (int *)w; w += align256((size_t)nvox * 4);
        unsigned *rm = (unsigned *)w; w += align256((size_t)nvox * 4);
        unsigned *rms = (unsigned *)w; w += align256((size_t)nvox * 4);
        hipLaunchKernelGGL(scannet_rooms_d2_kernel, dim3(blocks), dim3(256), 0, stream, rooms, nvox, voxel_max, vbase, coord,
                           (const int *)sel, init, init_u, d2, ckey, iota);
        hipError_t e = sort_by_room_then_key<int>(rooms, nvox, vbase, ckey, skey, iota, ord1, rm, rms, order, w, stream);
        if (e != hipSuccess) { set_error("amc3d_scannet_select_crop: radix sort: %s", hipGetErrorString(e)); return (int)e; }
    }
    return launch_status("amc3d_scannet_select_crop");
}

AMC_API size_t amc3d_scannet_crop_tail_workspace_bytes(int rooms)
{
    if (rooms <= 0) return 0;
    return align256((size_t)rooms * kTailBlocks * 3 * sizeof(double));
}

AMC_API int amc3d_scannet_crop_tail_rooms(int rooms, int n, int voxel_max, int gravity_dim, const double *coord, const float *x,
                                          const long long *y, const int *vbase, const int *sel, const int *order, const int *pad,
                                          const int *perm, float *pos_out, float *x_out, float *heights, long long *y_out,
                                          void *workspace, size_t workspace_bytes, void *stream_)
{
    if (rooms <= 0 || n <= 0) return 0;
    if (rooms > 65535 || voxel_max <= 0 || gravity_dim < 0 || gravity_dim > 2 || !coord || !x || !y || !vbase || !sel || !pos_out ||
        !x_out || !heights || !y_out || !workspace || workspace_bytes < amc3d_scannet_crop_tail_workspace_bytes(rooms))
        return bad_arg("amc3d_scannet_crop_tail_rooms: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    double *part = (double *)workspace;
    hipLaunchKernelGGL(scannet_rooms_tail_min_kernel, dim3(kTailBlocks, rooms), dim3(kTailThreads), 0, stream, n, voxel_max, coord,
                       vbase, sel, order, pad, part);
    hipLaunchKernelGGL(scannet_rooms_tail_kernel, dim3(kTailBlocks, rooms), dim3(kTailThreads), 0, stream, n, voxel_max, gravity_dim,
                       coord, x, y, vbase, sel, order, pad, perm, (const double *)part, pos_out, x_out, heights, y_out);
    return launch_status("amc3d_scannet_crop_tail_rooms");
}
