// Training input on the device (gfx950) for a whole batch of rooms per call: crop_pc (dataset/data_util.py:146-174: min-corner
// shift, voxelize mode 0, nearest-voxel_max crop or padding by repetition, shuffle, min-corner shift, cast) plus the collate.
// voxel.hip does that for one room per call, and the caller reads the voxel count, count.max() and the crop centre back for
// every room.  Here the rooms are one ragged batch -- room r is points [offsets[r], offsets[r+1]) -- and every stage is one
// launch (or one library sort) for all of them:
//   min corner   kRoomBlocks workgroups per room, then a fold; min is exact, so any order gives the same corner
//   keys         coord = point - corner in C, FNV-1a of floor(coord / voxel) in fp64: voxel.hip's voxel_key_kernel
//   order        by (room, key), stable (sort_by_room_then_key).  rocPRIM's segmented radix sort gives a long segment to ONE
//                workgroup (device_segmented_radix_sort.hpp launches dim3(segments), or dim3(large_segment_count) after
//                partitioning by length), so eight million-point rooms would sort on eight CUs.  Instead: one device-wide
//                stable sort of (key, point) over all 64 key bits, then one device-wide stable pass over the ceil(log2 rooms)
//                bits of the room id -- LSD order, so the order inside a room is the first sort's
//   voxels       heads (a room boundary is a head even between equal keys), one scan, starts, counts; per-room first voxel
//                (vbase) and count.max() (cmax) stay on the device
//   select       sel[v] = idx_sort[start[v] + rnd[v] % count[v]], rnd given or floor(u * count.max()) of a fp64 uniform
//   crop         d2 of every representative to its own room's centre, ((dx^2 + dy^2) + dz^2) in C as voxel.hip's crop_d2_kernel,
//                ordered by (room, bits of d2) with the same helper; a room's first voxel_max sorted entries are its crop
//   tail         slot k <- representative crop[perm[k]] (rooms below voxel_max: identity + pad) minus the cropped cloud's min
//                corner in C, cast to fp32
// All arithmetic is exact by construction (subtract in C, fp64 divide and floor, integer hash, non-contracted distance in C), so
// the result equals the per-room route's bit for bit.  Random draws are the caller's: the library has no generator.
//
// Two instantiations:
//                   S3DIS (amc3d_s3dis_*)                                      ScanNet (amc3d_scannet_*_rooms, _select_crop)
//   source          rows [src[r], ...) of one (rows,7) array {xyz, rgb 0..255,   pos (total,3) double as ScanNetTrainAugment
//                   label}, fp32 or fp64, cast to fp32 first (s3dis.py:122-144)   leaves it, x (total,3) fp32, y (total) int64
//   C               float                                                      double
//   crop key        32 bits of d2: the room rides above them, one sort         64 bits of d2: two passes, as the voxel order
//   tail            one 1024-thread workgroup per room, the min inside;         kTailBlocks workgroups per room behind a launch
//                   colours and label cast from the raw row                    of partial minima; x, y gathered, `heights`
//                                                                              (scannet.py:168-176) = the gravity column
#include "cub_kernel_memset.h"  // hipCUB with its memsets as kernels (graph-safe)

#include "room_common.h"

namespace amc {

constexpr int kRoomBlocks = 64;   // workgroups per room in the strided per-room passes over points and voxels
constexpr int kRoomThreads = 256;
constexpr int kTailBlocks = 32;   // workgroups per room in ScanNet's tail (64000 slots: 8 per thread)
constexpr int kTailThreads = 256;
constexpr int kMaxRooms = 1024, kMaxRoomBits = 10;

// Point sources: at(row, j) is column j of a row, and point i of the batch (in room r) is row shift(r) + i.
template <typename T>
struct RawRows {  // S3DIS: T = float or double
    using coord_t = float;
    const T *raw;
    const long long *src, *off;
    bool ok() const { return raw && src; }
    __device__ __forceinline__ long long shift(int r) const { return src[r] - off[r]; }
    __device__ __forceinline__ float at(long long row, int j) const { return (float)raw[(size_t)row * 7 + j]; }
};

struct DensePos {  // ScanNet
    using coord_t = double;
    const double *pos;
    bool ok() const { return pos != nullptr; }
    __device__ __forceinline__ long long shift(int) const { return 0; }
    __device__ __forceinline__ double at(long long row, int j) const { return pos[(size_t)row * 3 + j]; }
};

// per (room, workgroup) partial minimum of the room's points -> part[(r * kRoomBlocks + blk) * 3 + j]
template <typename S>
__global__ __launch_bounds__(kRoomThreads) void room_min_kernel(S pts, const long long *__restrict__ off,
                                                                typename S::coord_t *__restrict__ part)
{
    using C = typename S::coord_t;
    __shared__ C s[kRoomThreads / 64][3];
    const int r = blockIdx.y, blk = blockIdx.x;
    const long long sh = pts.shift(r), end = off[r + 1];
    C mn[3] = {kHuge<C>, kHuge<C>, kHuge<C>};
    for (long long i = off[r] + (long long)blk * kRoomThreads + threadIdx.x; i < end; i += (long long)kRoomBlocks * kRoomThreads) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = min_c(mn[j], pts.at(sh + i, j));
    }
    block_min3<C, kRoomThreads>(mn, s, part + ((size_t)r * kRoomBlocks + blk) * 3);
}

// corner (rooms,3) from the partials; cmax zeroed for the atomic maximum of room_count_kernel
template <typename C>
__global__ void room_corner_kernel(int rooms, const C *__restrict__ part, C *__restrict__ corner, int *__restrict__ cmax)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rooms * 3) return;
    const int r = t / 3, j = t - r * 3;
    C v = part[(size_t)r * kRoomBlocks * 3 + j];
    for (int k = 1; k < kRoomBlocks; ++k) v = min_c(v, part[((size_t)r * kRoomBlocks + k) * 3 + j]);
    corner[t] = v;
    if (j == 0) cmax[r] = 0;
}

// crop_pc's `coord -= coord.min(0)` (data_util.py:150; for S3DIS also s3dis.py:129-130, after which crop_pc's own shift is of a
// cloud whose minimum is exactly 0 and changes nothing), then the cell hash
template <typename S>
__global__ __launch_bounds__(256) void room_key_kernel(int rooms, int total, S pts, const long long *__restrict__ off,
                                                       const typename S::coord_t *__restrict__ corner, double voxel,
                                                       typename S::coord_t *__restrict__ coord,
                                                       unsigned long long *__restrict__ key, int *__restrict__ iota)
{
    using C = typename S::coord_t;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int r = room_seg<long long>(rooms, off, i);
    const long long row = pts.shift(r) + i;
    const C p[3] = {pts.at(row, 0), pts.at(row, 1), pts.at(row, 2)};
    unsigned long long h = 14695981039346656037ULL;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const C c = sub_rn(p[j], corner[r * 3 + j]);
        coord[(size_t)i * 3 + j] = c;
        h *= 1099511628211ULL;
        h ^= (unsigned long long)(long long)floor((double)c / voxel);  // c >= 0: the cloud sits at its min corner
    }
    key[i] = h;
    iota[i] = (int)i;
}

// the room of every entry of idx, looked up in tab (rooms + 1 ascending entries): points in offsets, voxels in vbase
template <typename I>
__global__ void room_id_kernel(int rooms, int n, const I *__restrict__ tab, const int *__restrict__ idx, unsigned *__restrict__ room)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) room[i] = (unsigned)room_seg<I>(rooms, tab, (I)idx[i]);
}

// room: the room of every sorted position (NULL: one room)
__global__ void room_head_kernel(int total, const unsigned long long *__restrict__ key, const int *__restrict__ idx_sort,
                                 const unsigned *__restrict__ room, int *__restrict__ head)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    head[i] = (i == 0 || (room && room[i] != room[i - 1]) || key[idx_sort[i]] != key[idx_sort[i - 1]]) ? 1 : 0;
}

__global__ void room_start_kernel(int rooms, int total, const int *__restrict__ head, const int *__restrict__ incl,
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
__global__ __launch_bounds__(kRoomThreads) void room_count_kernel(const int *__restrict__ vbase, const int *__restrict__ start,
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
__global__ void room_select_kernel(int rooms, int nvox, const int *__restrict__ vbase, const int *__restrict__ cmax,
                                   const int *__restrict__ start, const int *__restrict__ count, const int *__restrict__ idx_sort,
                                   const int *__restrict__ rnd, const double *__restrict__ u, int *__restrict__ sel)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvox) return;
    int r = rnd ? rnd[v] : -1;
    if (r < 0) r = u ? (int)__dmul_rn(u[v], (double)cmax[room_seg<int>(rooms, vbase, v)]) : 0;
    sel[v] = idx_sort[start[v] + r % count[v]];
}

// the crop centre of room r: init[r] >= 0, or min(floor(init_u[r] * nv), nv - 1)
__device__ __forceinline__ int crop_centre(int r, int nv, const int *__restrict__ init, const double *__restrict__ init_u)
{
    int c = init ? init[r] : -1;
    if (c < 0) c = init_u ? (int)__dmul_rn(init_u[r], (double)nv) : 0;
    return min(max(c, 0), nv - 1);
}

// The order of (room, key) pairs, stated once: when the key's bits and the room's fit in 64 together, the room rides in the
// key's high bits and one sort does it (fp32 distances); otherwise the key is sorted first and the room in a second, stable
// pass (the 64-bit cell hashes, fp64 distances).  sort_by_room_then_key issues the sorts.
template <typename C>
constexpr bool kRoomInKey = 8 * (int)sizeof(C) + kMaxRoomBits <= 64;

// data_util.py:158-160 for every room with at least voxel_max voxels; the others keep their order (key = local voxel id)
template <typename C>
__global__ void room_d2_kernel(int rooms, int nvox, int voxel_max, const int *__restrict__ vbase, const C *__restrict__ coord,
                               const int *__restrict__ sel, const int *__restrict__ init, const double *__restrict__ init_u,
                               C *__restrict__ d2, unsigned long long *__restrict__ ckey, int *__restrict__ iota)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvox) return;
    const int r = room_seg<int>(rooms, vbase, v);
    const int nv = vbase[r + 1] - vbase[r];
    unsigned long long k = (unsigned long long)(v - vbase[r]);
    C d = 0;
    if (nv >= voxel_max) {
        const size_t p = (size_t)sel[v], q = (size_t)sel[vbase[r] + crop_centre(r, nv, init, init_u)];
        d = dist2_ref(coord[p * 3], coord[p * 3 + 1], coord[p * 3 + 2], coord[q * 3], coord[q * 3 + 1], coord[q * 3 + 2]);
        k = order_bits(d);
    }
    d2[v] = d;
    ckey[v] = kRoomInKey<C> ? ((unsigned long long)r << 32) | k : k;
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

// crop_pc's last `coord -= coord.min(0)` (data_util.py:173): this thread's minimum over slots k0, k0 + stride, ... of room r's
// n slots (the shuffle does not change the set, so the loop runs in crop order)
template <typename C>
__device__ __forceinline__ void slot_min3(C mn[3], int k0, int stride, int r, int n, int voxel_max, const C *__restrict__ coord,
                                          const int *__restrict__ vbase, const int *__restrict__ sel,
                                          const int *__restrict__ order, const int *__restrict__ pad)
{
    const int vb = vbase[r], nv = vbase[r + 1] - vb;
    const int *pd = pad ? pad + (size_t)r * n : nullptr;
    for (int k = k0; k < n; k += stride) {
        const size_t p = (size_t)sel[tail_voxel(k, n, nv, vb, voxel_max, order, pd, nullptr)];
#pragma unroll
        for (int j = 0; j < 3; ++j) mn[j] = min_c(mn[j], coord[p * 3 + j]);
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void s3dis_tail_kernel(int n, int voxel_max, RawRows<T> pts, const float *__restrict__ coord,
                                                          const int *__restrict__ vbase, const int *__restrict__ sel,
                                                          const int *__restrict__ order, const int *__restrict__ pad,
                                                          const int *__restrict__ perm, float *__restrict__ pos_out,
                                                          float *__restrict__ col_out, long long *__restrict__ y_out)
{
    __shared__ float s_mn[16][3];
    __shared__ float s_corner[3];
    const int r = blockIdx.x;
    float mn[3] = {kHuge<float>, kHuge<float>, kHuge<float>};
    slot_min3<float>(mn, threadIdx.x, 1024, r, n, voxel_max, coord, vbase, sel, order, pad);
    block_min3<float, 1024>(mn, s_mn, s_corner);
    __syncthreads();
    const int vb = vbase[r], nv = vbase[r + 1] - vb;
    const int *pd = pad ? pad + (size_t)r * n : nullptr, *pm = perm ? perm + (size_t)r * n : nullptr;
    const long long sh = pts.shift(r);
    for (int k = threadIdx.x; k < n; k += 1024) {
        const size_t p = (size_t)sel[tail_voxel(k, n, nv, vb, voxel_max, order, pd, pm)], o = (size_t)r * n + k;
        const long long row = sh + (long long)p;
        const float c[4] = {pts.at(row, 3), pts.at(row, 4), pts.at(row, 5), pts.at(row, 6)};  // rgb, label
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pos_out[o * 3 + j] = sub_rn(coord[p * 3 + j], s_corner[j]);
            col_out[o * 3 + j] = c[j];
        }
        y_out[o] = (long long)c[3];
    }
}

// ScanNet's partial minima -> part[(r * kTailBlocks + blk) * 3 + j]
__global__ __launch_bounds__(kTailThreads) void scannet_tail_min_kernel(int n, int voxel_max, const double *__restrict__ coord,
                                                                        const int *__restrict__ vbase, const int *__restrict__ sel,
                                                                        const int *__restrict__ order, const int *__restrict__ pad,
                                                                        double *__restrict__ part)
{
    __shared__ double s[kTailThreads / 64][3];
    const int r = blockIdx.y, blk = blockIdx.x;
    double mn[3] = {kHuge<double>, kHuge<double>, kHuge<double>};
    slot_min3<double>(mn, blk * kTailThreads + threadIdx.x, kTailBlocks * kTailThreads, r, n, voxel_max, coord, vbase, sel, order, pad);
    block_min3<double, kTailThreads>(mn, s, part + ((size_t)r * kTailBlocks + blk) * 3);
}

// every gathering workgroup folds its room's partials first
__global__ __launch_bounds__(kTailThreads) void scannet_tail_kernel(int n, int voxel_max, int g, const double *__restrict__ coord,
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
        const size_t p = (size_t)sel[tail_voxel(k, n, nv, vb, voxel_max, order, pd, pm)], o = (size_t)r * n + k;
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

static int room_bits(int rooms)
{
    int bits = 0;
    while ((1 << bits) < rooms) ++bits;
    return bits;
}

// hipCUB's temporary storage for n elements: the 64-bit pair sort alone (one_sort), or the largest of it, the room-bit pair sort
// and the scan
static size_t room_temp(int n, bool one_sort)
{
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const int *)nullptr, (int *)nullptr, n);
    if (one_sort) return align256(a);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const unsigned *)nullptr, (unsigned *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, c, (const int *)nullptr, (int *)nullptr, n);
    return align256(a > b ? (a > c ? a : c) : (b > c ? b : c));
}

// stable order of n (key, value) pairs by (room of the value, key), the rule of kRoomInKey at work: keys of key_bits bits that
// leave room for the room bits carry the room above them (the caller put it there) and one sort over both does it; 64-bit
// keys are sorted first, then the rooms in a second, stable pass -- LSD order.  One room has no room bits: no second pass.
// tab: the rooms' first values (rooms + 1 ascending); v1 / rm / rms: n-element scratch of the second pass, rms holding the
// sorted room ids afterwards
template <typename I>
static int sort_by_room_then_key(const char *what, int key_bits, int rooms, int n, const I *tab, const unsigned long long *key,
                                 unsigned long long *ks, const int *val, int *v1, unsigned *rm, unsigned *rms, int *out,
                                 void *temp_ptr, size_t temp_bytes, hipStream_t stream)
{
    const int bits = room_bits(rooms);
    const bool one = key_bits + bits <= 64;
    size_t temp = temp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp_ptr, temp, key, ks, val, one ? out : v1, n, 0, one ? key_bits + bits : 64,
                                                      stream);
    if (e != hipSuccess) { set_error("%s: radix sort: %s", what, hipGetErrorString(e)); return (int)e; }
    if (one) return 0;
    hipLaunchKernelGGL(room_id_kernel<I>, dim3(div_up(n, 256)), dim3(256), 0, stream, rooms, n, tab, (const int *)v1, rm);
    temp = temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(temp_ptr, temp, (const unsigned *)rm, rms, (const int *)v1, out, n, 0, bits, stream);
    if (e != hipSuccess) { set_error("%s: room sort: %s", what, hipGetErrorString(e)); return (int)e; }
    return 0;
}

static int bad(const char *what, const char *why)
{
    set_error("%s: %s", what, why);
    return (int)hipErrorInvalidValue;
}

template <typename C>
static size_t voxelize_workspace(int rooms, long long total)
{
    if (rooms <= 0 || total <= 0 || total > 0x7fffffffLL) return 0;
    const int n = (int)total;
    // sorted keys | iota, then head | first order | room ids, then incl | sorted room ids | min partials | sort / scan temp
    return align256((size_t)n * 8) + 4 * align256((size_t)n * 4) + align256((size_t)rooms * kRoomBlocks * 3 * sizeof(C)) +
           room_temp(n, false) + 256;
}

template <typename S>
static int voxelize_rooms(const char *what, int rooms, long long total, S pts, const long long *off, double voxel,
                          typename S::coord_t *coord, unsigned long long *key, int *idx_sort, int *start, int *count, int *vbase,
                          int *cmax, typename S::coord_t *corner, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    using C = typename S::coord_t;
    if (rooms <= 0 || total <= 0) return 0;
    if (rooms > kMaxRooms || total > 0x7fffffffLL) return bad(what, "at most 1024 rooms and 2^31 - 1 points");
    if (!pts.ok() || !off || !(voxel > 0.0) || !coord || !key || !idx_sort || !start || !count || !vbase || !cmax || !corner ||
        !workspace || workspace_bytes < voxelize_workspace<C>(rooms, total))
        return bad(what, "bad argument");
    const int n = (int)total, blocks = div_up(n, 256);
    char *w = (char *)workspace;
    unsigned long long *ks = (unsigned long long *)w; w += align256((size_t)n * 8);  // the first sort's keys
    int *iota = (int *)w; w += align256((size_t)n * 4);                              // then head
    int *idx1 = (int *)w; w += align256((size_t)n * 4);
    unsigned *rm = (unsigned *)w; w += align256((size_t)n * 4);                      // then incl
    unsigned *rms = (unsigned *)w; w += align256((size_t)n * 4);
    C *part = (C *)w; w += align256((size_t)rooms * kRoomBlocks * 3 * sizeof(C));
    hipLaunchKernelGGL(room_min_kernel<S>, dim3(kRoomBlocks, rooms), dim3(kRoomThreads), 0, stream, pts, off, part);
    hipLaunchKernelGGL(room_corner_kernel<C>, dim3(div_up(rooms * 3, 64)), dim3(64), 0, stream, rooms, (const C *)part, corner, cmax);
    hipLaunchKernelGGL(room_key_kernel<S>, dim3(blocks), dim3(256), 0, stream, rooms, n, pts, off, (const C *)corner, voxel, coord,
                       key, iota);
    const size_t temp_bytes = room_temp(n, false);
    int rc = sort_by_room_then_key<long long>(what, 64, rooms, n, off, key, ks, iota, idx1, rm, rms, idx_sort, w, temp_bytes, stream);
    if (rc) return rc;
    const unsigned *room = rooms > 1 ? rms : nullptr;
    int *head = iota, *incl = (int *)rm;
    hipLaunchKernelGGL(room_head_kernel, dim3(blocks), dim3(256), 0, stream, n, (const unsigned long long *)key,
                       (const int *)idx_sort, room, head);
    size_t temp = temp_bytes;
    hipError_t e = hipcub::DeviceScan::InclusiveSum(w, temp, (const int *)head, incl, n, stream);
    if (e != hipSuccess) { set_error("%s: scan: %s", what, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(room_start_kernel, dim3(blocks), dim3(256), 0, stream, rooms, n, (const int *)head, (const int *)incl, room,
                       start, vbase);
    hipLaunchKernelGGL(room_count_kernel, dim3(kRoomBlocks, rooms), dim3(kRoomThreads), 0, stream, (const int *)vbase,
                       (const int *)start, count, cmax);
    return launch_status(what);
}

template <typename C>
static size_t crop_workspace(int nvox)
{
    if (nvox <= 0) return 0;
    // keys | sorted keys | iota, and for two passes | first order | room ids | sorted room ids, then the sort temp
    return 2 * align256((size_t)nvox * 8) + (kRoomInKey<C> ? 1 : 4) * align256((size_t)nvox * 4) + room_temp(nvox, kRoomInKey<C>) +
           256;
}

template <typename C>
static int select_crop(const char *what, int rooms, int nvox, int voxel_max, int any_crop, const C *coord, const int *idx_sort,
                       const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd, const double *rnd_u,
                       const int *init, const double *init_u, int *sel, C *d2, int *order, void *workspace, size_t workspace_bytes,
                       hipStream_t stream)
{
    if (rooms <= 0 || nvox <= 0) return 0;
    if (rooms > kMaxRooms || voxel_max <= 0 || !coord || !idx_sort || !start || !count || !vbase || !cmax || !sel ||
        (any_crop && (!d2 || !order || !workspace || workspace_bytes < crop_workspace<C>(nvox))))
        return bad(what, "bad argument");
    const int blocks = div_up(nvox, 256);
    hipLaunchKernelGGL(room_select_kernel, dim3(blocks), dim3(256), 0, stream, rooms, nvox, vbase, cmax, start, count, idx_sort, rnd,
                       rnd_u, sel);
    if (any_crop) {
        char *w = (char *)workspace;
        unsigned long long *ckey = (unsigned long long *)w; w += align256((size_t)nvox * 8);
        unsigned long long *skey = (unsigned long long *)w; w += align256((size_t)nvox * 8);
        int *iota = (int *)w; w += align256((size_t)nvox * 4);
        int *ord1 = nullptr;
        unsigned *rm = nullptr, *rms = nullptr;
        if (!kRoomInKey<C>) {
            ord1 = (int *)w; w += align256((size_t)nvox * 4);
            rm = (unsigned *)w; w += align256((size_t)nvox * 4);
            rms = (unsigned *)w; w += align256((size_t)nvox * 4);
        }
        hipLaunchKernelGGL(room_d2_kernel<C>, dim3(blocks), dim3(256), 0, stream, rooms, nvox, voxel_max, vbase, coord,
                           (const int *)sel, init, init_u, d2, ckey, iota);
        int rc = sort_by_room_then_key<int>(what, 8 * (int)sizeof(C), rooms, nvox, vbase, ckey, skey, iota, ord1, rm, rms, order, w,
                                            room_temp(nvox, kRoomInKey<C>), stream);
        if (rc) return rc;
    }
    return launch_status(what);
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_s3dis_voxelize_workspace_bytes(int rooms, long long total) { return voxelize_workspace<float>(rooms, total); }

AMC_API int amc3d_s3dis_voxelize_rooms(int rooms, long long total, int raw_f64, const void *raw, const long long *src,
                                       const long long *offsets, double voxel_size, float *coord, unsigned long long *key,
                                       int *idx_sort, int *start, int *count, int *vbase, int *cmax, float *corner,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "amc3d_s3dis_voxelize_rooms";
    const RawRows<double> r64{(const double *)raw, src, offsets};
    const RawRows<float> r32{(const float *)raw, src, offsets};
    if (raw_f64)
        return voxelize_rooms(what, rooms, total, r64, offsets, voxel_size, coord, key, idx_sort, start, count, vbase, cmax, corner,
                              workspace, workspace_bytes, (hipStream_t)stream);
    return voxelize_rooms(what, rooms, total, r32, offsets, voxel_size, coord, key, idx_sort, start, count, vbase, cmax, corner,
                          workspace, workspace_bytes, (hipStream_t)stream);
}

AMC_API size_t amc3d_s3dis_crop_workspace_bytes(int nvox) { return crop_workspace<float>(nvox); }

AMC_API int amc3d_s3dis_select_crop(int rooms, int nvox, int voxel_max, int any_crop, const float *coord, const int *idx_sort,
                                    const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd,
                                    const double *rnd_u, const int *init, const double *init_u, int *sel, float *d2, int *order,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    return select_crop<float>("amc3d_s3dis_select_crop", rooms, nvox, voxel_max, any_crop, coord, idx_sort, start, count, vbase,
                              cmax, rnd, rnd_u, init, init_u, sel, d2, order, workspace, workspace_bytes, (hipStream_t)stream);
}

AMC_API int amc3d_s3dis_crop_tail(int rooms, int n, int voxel_max, int raw_f64, const void *raw, const long long *src,
                                  const long long *offsets, const float *coord, const int *vbase, const int *sel, const int *order,
                                  const int *pad, const int *perm, float *pos_out, float *colour_out, long long *y_out,
                                  void *stream)
{
    if (rooms <= 0 || n <= 0) return 0;
    if (voxel_max <= 0 || !raw || !src || !offsets || !coord || !vbase || !sel || !pos_out || !colour_out || !y_out)
        return bad_arg("amc3d_s3dis_crop_tail: bad argument");
    const RawRows<double> r64{(const double *)raw, src, offsets};
    const RawRows<float> r32{(const float *)raw, src, offsets};
    if (raw_f64)
        hipLaunchKernelGGL(s3dis_tail_kernel<double>, dim3(rooms), dim3(1024), 0, (hipStream_t)stream, n, voxel_max, r64, coord,
                           vbase, sel, order, pad, perm, pos_out, colour_out, y_out);
    else
        hipLaunchKernelGGL(s3dis_tail_kernel<float>, dim3(rooms), dim3(1024), 0, (hipStream_t)stream, n, voxel_max, r32, coord,
                           vbase, sel, order, pad, perm, pos_out, colour_out, y_out);
    return launch_status("amc3d_s3dis_crop_tail");
}

AMC_API size_t amc3d_scannet_voxelize_workspace_bytes(int rooms, long long total) { return voxelize_workspace<double>(rooms, total); }

AMC_API int amc3d_scannet_voxelize_rooms(int rooms, long long total, const double *pos, const long long *offsets, double voxel_size,
                                         double *coord, unsigned long long *key, int *idx_sort, int *start, int *count, int *vbase,
                                         int *cmax, double *corner, void *workspace, size_t workspace_bytes, void *stream)
{
    return voxelize_rooms("amc3d_scannet_voxelize_rooms", rooms, total, DensePos{pos}, offsets, voxel_size, coord, key, idx_sort,
                          start, count, vbase, cmax, corner, workspace, workspace_bytes, (hipStream_t)stream);
}

AMC_API size_t amc3d_scannet_crop_workspace_bytes(int nvox) { return crop_workspace<double>(nvox); }

AMC_API int amc3d_scannet_select_crop(int rooms, int nvox, int voxel_max, int any_crop, const double *coord, const int *idx_sort,
                                      const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd,
                                      const double *rnd_u, const int *init, const double *init_u, int *sel, double *d2, int *order,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    return select_crop<double>("amc3d_scannet_select_crop", rooms, nvox, voxel_max, any_crop, coord, idx_sort, start, count, vbase,
                               cmax, rnd, rnd_u, init, init_u, sel, d2, order, workspace, workspace_bytes, (hipStream_t)stream);
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
    hipLaunchKernelGGL(scannet_tail_min_kernel, dim3(kTailBlocks, rooms), dim3(kTailThreads), 0, stream, n, voxel_max, coord, vbase,
                       sel, order, pad, part);
    hipLaunchKernelGGL(scannet_tail_kernel, dim3(kTailBlocks, rooms), dim3(kTailThreads), 0, stream, n, voxel_max, gravity_dim, coord,
                       x, y, vbase, sel, order, pad, perm, (const double *)part, pos_out, x_out, heights, y_out);
    return launch_status("amc3d_scannet_crop_tail_rooms");
}
