// k-nearest-neighbour query over "offset" segments for gfx950.
//
// Reference: pointops/src/knnquery/knnquery_cuda_kernel.cu:65-108 -- one thread
// per query scans its whole segment in index order, keeping a max-heap of
// `nsample` (<= 100) entries in per-thread scratch: a candidate replaces the
// root iff d2 < root (strict), then `reheap` (:21-36) sifts down; `heap_sort`
// (:39-48) finally emits ascending distance.  How equal distances are ordered
// (and which of several equal maxima is evicted) is a property of that heap
// history, so "bit-exact indices" means reproducing it.
//
// knn_exact_kernel: one WAVEFRONT per query replays exactly that heap, but scans
// 64 candidates per step: lanes compute d2 for 64 consecutive indices, a ballot
// selects those below the current root, and only those are fed -- in ascending
// index order, re-checked against the updated root -- to the heap, which lives
// in LDS.  A candidate that fails `d2 < root` at ballot time can never pass
// later (the root only decreases), so the heap sees the same insert sequence as
// the reference's sequential scan.  The 16 waves of a workgroup share LDS tiles
// of the support cloud.

#include "common.h"

namespace amc {

constexpr int KNN_TILE = 1024;
constexpr int KNN_WAVES = 16;
constexpr int KNN_MAXK = 100;  // reference: float best_dist[100] (knnquery_cuda_kernel.cu:86)

// knnquery_cuda_kernel.cu:21-36
__device__ __forceinline__ void reheap(float *dist, int *idx, int k)
{
    int root = 0;
    int child = 1;
    while (child < k) {
        if (child + 1 < k && dist[child + 1] > dist[child]) child++;
        if (dist[root] > dist[child]) return;
        const float tf = dist[root]; dist[root] = dist[child]; dist[child] = tf;
        const int ti = idx[root]; idx[root] = idx[child]; idx[child] = ti;
        root = child;
        child = root * 2 + 1;
    }
}

// segment of point/query `i` given cumulative ends (knnquery_cuda_kernel.cu:51-62,74-80)
__device__ __forceinline__ int seg_of(int i, const int *__restrict__ ends, int nb)
{
    int s = 0;
    while (s < nb - 1 && !(i < ends[s])) ++s;
    return s;
}

// queries: either all of 0..m-1 (qlist == nullptr) or the first *qcount entries of qlist
__global__ __launch_bounds__(KNN_WAVES * 64) void knn_exact_kernel(
    int m, int nsample, int nbatch, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const int *__restrict__ offset, const int *__restrict__ new_offset, int *__restrict__ idx,
    float *__restrict__ dist2, const int *__restrict__ qlist, const int *__restrict__ qcount)
{
    __shared__ float sx[KNN_TILE], sy[KNN_TILE], sz[KNN_TILE];
    __shared__ float hd[KNN_WAVES][KNN_MAXK];
    __shared__ int hi[KNN_WAVES][KNN_MAXK];
    __shared__ int s_lo[KNN_WAVES], s_hi[KNN_WAVES];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = qlist ? *qcount : m;

    for (int base = blockIdx.x * KNN_WAVES; base < total; base += gridDim.x * KNN_WAVES) {
        const int qi = base + wave;
        const bool live = qi < total;
        const int pt = live ? (qlist ? qlist[qi] : qi) : 0;
        int start = 0, end = 0;
        if (live) {
            const int bt = seg_of(pt, new_offset, nbatch);
            start = bt == 0 ? 0 : offset[bt - 1];
            end = offset[bt];
        }
        const float qx = new_xyz[(size_t)pt * 3], qy = new_xyz[(size_t)pt * 3 + 1], qz = new_xyz[(size_t)pt * 3 + 2];
        float *mydist = hd[wave];
        int *myidx = hi[wave];
        for (int i = lane; i < nsample; i += 64) { mydist[i] = 1e10f; myidx[i] = start; }
        float root = 1e10f;

        __syncthreads();  // previous round's readers of s_lo/s_hi and tiles are done
        if (lane == 0) { s_lo[wave] = live ? start : 0x7fffffff; s_hi[wave] = live ? end : 0; }
        __syncthreads();
        int lo = 0x7fffffff, hi_ = 0;
        for (int w = 0; w < KNN_WAVES; ++w) { lo = min(lo, s_lo[w]); hi_ = max(hi_, s_hi[w]); }

        for (int t0 = lo; t0 < hi_; t0 += KNN_TILE) {
            const int tn = min(KNN_TILE, hi_ - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < tn * 3; i += KNN_WAVES * 64) {
                const float v = xyz[(size_t)t0 * 3 + i];
                const int p = i / 3, c = i - p * 3;
                (c == 0 ? sx : c == 1 ? sy : sz)[p] = v;
            }
            __syncthreads();
            if (!live || t0 >= end || t0 + tn <= start) continue;  // wave-uniform
            for (int k0 = 0; k0 < tn; k0 += 64) {
                const int kl = k0 + lane, gi = t0 + kl;
                const bool valid = kl < tn && gi >= start && gi < end;
                const float d2 = dist2_ref(qx, qy, qz, sx[kl < tn ? kl : 0], sy[kl < tn ? kl : 0], sz[kl < tn ? kl : 0]);
                unsigned long long mask = __ballot(valid && d2 < root);
                while (mask) {
                    const int bpos = (int)__builtin_ctzll(mask);
                    mask &= mask - 1;
                    const float cd = __shfl(d2, bpos, 64);
                    if (cd < root) {  // knnquery_cuda_kernel.cu:97-101
                        mydist[0] = cd;
                        myidx[0] = t0 + k0 + bpos;
                        reheap(mydist, myidx, nsample);
                        root = mydist[0];
                    }
                }
            }
        }
        if (live) {
            // knnquery_cuda_kernel.cu:39-48
            for (int i = nsample - 1; i > 0; i--) {
                const float tf = mydist[0]; mydist[0] = mydist[i]; mydist[i] = tf;
                const int ti = myidx[0]; myidx[0] = myidx[i]; myidx[i] = ti;
                reheap(mydist, myidx, i);
            }
            for (int i = lane; i < nsample; i += 64) {
                idx[(size_t)pt * nsample + i] = myidx[i];
                dist2[(size_t)pt * nsample + i] = mydist[i];
            }
        }
    }
}


// =============================================================================================
// Grid-accelerated path (k <= 64).
//
// Brute force is O(m*n): 5.1e10 distance evaluations per training step at the benchmark shape.
// The same answers come from a uniform grid over the support cloud: bin the support points into
// cells of edge h (counting sort, x fastest), then each query scans the 3x3x3 block of cells
// around it, then shells of growing Chebyshev radius R, until its current k-th distance is
// provably smaller than the distance to anything outside the scanned block.
//
// The walk (QueryCell, shell_pair_runs).  A query's cell (cx,cy,cz) is its clamped cell coordinate in its
// segment's grid.  Shell R is walked as its (2R+1)^2 (dz,dy) pairs; x is the fastest cell axis, so a pair's cells
// are one run [b, e) of sorted[].  A pair on the shell's rim contributes the full x-run [cx-R, cx+R], an interior
// pair only its two end cells (the cells between belong to smaller shells); for R == 1 every pair contributes the
// full run: the whole 3x3x3 block.  Rows outside the grid contribute nothing.  The replay's pruning set and ball
// query take the whole (2R+1)^3 block at once: the full run of every pair.
//
// The stop rule (shell_unseen_bound, shell_closed).  After shell R everything unseen lies beyond one of the six faces
// of the block [c-R, c+R]^3; a face that coincides with the grid's boundary imposes nothing (there are no points
// beyond it), and a block that covers the whole grid ends the search.  The nearest remaining face is `dmin` away;
// cell coordinates are formed in fp32, so `margin` (kg_params_kernel) is taken off, and the search ends once
// k-th < (dmin - margin)^2 * 0.99999.  Every kernel that walks shells takes both from these helpers: exactness
// rests on this arithmetic.
//
// Exactness.  kg_query_kernel (k in 33..64): one wavefront owns one query and keeps its k best candidates in lanes
// 0..k-1, sorted ascending (insertion = one ballot + a lane shift).  kg_query_group_kernel<32> (k <= 32): a wavefront
// serves two queries, 32 lanes each: same search, same lists.  When the k+1 smallest distances of a
// query are pairwise different, the reference's max-heap + heap-sort output is fully determined:
// those k indices in ascending distance -- independent of scan order -- which is what the lane
// list holds.  When two of them are EQUAL the reference's output depends on its heap history
// (index scan order); such queries are detected (list_tied: adjacent equal values in the list, or the best
// rejected distance equal to the k-th), listed, and recomputed by knn_exact_list_kernel, which replays the
// reference's heap over a prefix of the segment that the grid prunes.  (knn_exact_kernel, the all-pairs replay,
// answers the calls that build no grid: k > 64 and small problems.)  Distances are always the reference's
// expression (dist2_ref).
//
// Cell size.  h is calibrated on the data, per call: 64 sample queries get an estimate of their k-th
// neighbour distance from a brute-force scan of every 4th support point (one workgroup each), and
// h = 0.7 * the 80th percentile, so that the 3x3x3 block holds a few k candidates whatever the density or
// dimensionality of the cloud (surfaces, volumes, 8 overlapping clouds in one segment...); queries whose k-th
// neighbour lies beyond the block go on to the next shell.  (Sub-sampling step 4 and scale 0.7 came out of a sweep
// of both over the loss's seven searches at 8 x 24000 points, the shape of tools/knn_bench.py; the sweep script is
// not kept.)  h steers speed only; any h gives the same results.
// =============================================================================================
constexpr int KG_SAMPLES = 64;
constexpr int KG_MAXK = 64;
constexpr int KGG_MAXK = 32;  // up to here a wavefront serves two queries (kg_query_group_kernel<32>)
constexpr int KG_SCAN_TILE = 4096;  // cells per workgroup of the cell-count scan (256 threads x 16)

struct GridParams {
    float minx, miny, minz, h, inv_h, margin;
    int nx, ny, nz, ncell;  // per segment
};

constexpr int KG_MAX_BATCH = 64;  // segments of a grid search (amc3d_knnquery_uses_grid, grid_search_pays)

struct KnnWorkspace {           // byte offsets into the caller's workspace
    size_t params, bbox, samples, off_s, fb_count, tile_sums, off_q, cell_start, cursor, sorted, fb_list, total;
};

__host__ __device__ inline int knn_cell_cap(int n)
{
    long c = 8L * n;
    if (c < 4096) c = 4096;
    if (c > (1L << 22)) c = 1L << 22;
    return (int)c;
}

static KnnWorkspace knn_layout(int n, int m)
{
    KnnWorkspace w;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t cap = (size_t)knn_cell_cap(n);
    // the fixed head; off_s / off_q (ball query's and 3-NN's uniform segment ends, KG_MAX_BATCH ints each) sit in
    // the gaps behind samples and tile_sums
    constexpr size_t samples = 512, off_s = 768, fb_count = 1024, tile_sums = 2048, off_q = 6400, cell_start = 8192;
    constexpr size_t max_tiles = ((size_t)1 << 22) / KG_SCAN_TILE;  // knn_cell_cap: at most 2^22 cells
    static_assert(samples + KG_SAMPLES * 4 <= off_s && off_s + KG_MAX_BATCH * 4 <= fb_count, "knn_layout: off_s");
    static_assert(tile_sums + (max_tiles + 1) * 4 <= off_q && off_q + KG_MAX_BATCH * 4 <= cell_start, "knn_layout: off_q");
    static_assert(fb_count == AMC_KNN_FALLBACK_COUNT_OFFSET, "knn_layout: fb_count");
    w.params = 0;
    w.bbox = 256;
    w.samples = samples;
    w.off_s = off_s;
    w.fb_count = fb_count;
    w.tile_sums = tile_sums;
    w.off_q = off_q;
    w.cell_start = cell_start;
    w.cursor = up(w.cell_start + (cap + 1) * 4);
    w.sorted = up(w.cursor + (cap + 1) * 4);
    w.fb_list = up(w.sorted + (size_t)n * 16);
    w.total = up(w.fb_list + (size_t)m * 4);
    return w;
}

// order-preserving float <-> int for atomicMin/Max
__device__ __forceinline__ int f2ord(float f)
{
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void kg_init_kernel(int *bbox, int *fb_count)
{
    if (threadIdx.x < 3) bbox[threadIdx.x] = 0x7fffffff;          // min
    else if (threadIdx.x < 6) bbox[threadIdx.x] = (int)0x80000000;  // max
    if (threadIdx.x == 6) *fb_count = 0;
}

__global__ __launch_bounds__(256) void kg_bbox_kernel(int n, const float *__restrict__ xyz, int *__restrict__ bbox)
{
    __shared__ float s_lo[4][3], s_hi[4][3];
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = xyz[(size_t)i * 3 + c];
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int s = 32; s >= 1; s >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], s, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], s, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_lo[threadIdx.x >> 6][c] = lo[c]; s_hi[threadIdx.x >> 6][c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {  // one atomic pair per workgroup and axis
        const int c = threadIdx.x;
        const float l = fminf(fminf(s_lo[0][c], s_lo[1][c]), fminf(s_lo[2][c], s_lo[3][c]));
        const float h = fmaxf(fmaxf(s_hi[0][c], s_hi[1][c]), fmaxf(s_hi[2][c], s_hi[3][c]));
        atomicMin(bbox + c, f2ord(l));
        atomicMax(bbox + 3 + c, f2ord(h));
    }
}

// ---- a wavefront's sorted list of its k best candidates (lanes 0..k-1) ---------------------------
struct LaneList {
    float v;    // this lane's distance (ascending with lane id); 1e10 = the reference's placeholder
    int id;     // this lane's point index
    float tau;  // wave-uniform copy of the k-th (worst kept) distance
};

__device__ __forceinline__ void ll_init(LaneList &l, int start)
{
    l.v = 1e10f;
    l.id = start;
    l.tau = 1e10f;
}

// value of the lane below (lane 0 keeps its own): ONE v_mov_b32_dpp wave_shr:1 (the gfx9 whole-wave shift),
// not a ds_bpermute round trip through the LDS crossbar -- the insertion below is a dependent chain
__device__ __forceinline__ int lane_below_i32(int x)
{
    return __builtin_amdgcn_update_dpp(x, x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ float lane_below_f32(float x) { return __int_as_float(lane_below_i32(__float_as_int(x))); }

// insert (cd, ci), cd < tau, keeping ascending order; returns the evicted k-th value
__device__ __forceinline__ float ll_insert(LaneList &l, int k, int lane, float cd, int ci)
{
    const float evicted = l.tau;
    const int p = (int)__popcll(__ballot(lane < k && l.v <= cd));  // first lane with v > cd
    const float upv = lane_below_f32(l.v);
    const int upi = lane_below_i32(l.id);
    if (lane > p) { l.v = upv; l.id = upi; }
    if (lane == p) { l.v = cd; l.id = ci; }
    l.tau = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l.v), k - 1));
    return evicted;
}

// feed one chunk of up to 64 candidates (one per lane) to the list; rej tracks rejected distances
__device__ __forceinline__ void ll_feed(LaneList &l, int k, int lane, bool valid, float d2, int ci, float &rej_lane,
                                        float &rej_uni)
{
    const bool pass = valid && d2 < l.tau;
    rej_lane = fminf(rej_lane, (valid && !pass) ? d2 : 3.4e38f);
    unsigned long long mask = __ballot(pass);
    while (mask) {
        const int b = (int)__builtin_ctzll(mask);
        mask &= mask - 1;
        const float cd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d2), b));  // wave-uniform (SGPR)
        const int cc = __builtin_amdgcn_readlane(ci, b);
        if (cd < l.tau) rej_uni = fminf(rej_uni, ll_insert(l, k, lane, cd, cc));
        else rej_uni = fminf(rej_uni, cd);
    }
}

// The first 64 candidates of a query go through a bitonic sorting network instead of up to 64 list insertions
// (21 compare-exchange stages ~ 200 instructions, against ~23 per insertion and ~45 insertions): afterwards the
// list is exact for those candidates and tau is already close to final, so few later candidates pass.
// Lanes without a candidate carry the reference's placeholder (1e10, start) and sort to the tail.
__device__ __forceinline__ void ll_sort_first(LaneList &l, int k, int lane, bool valid, float d2, int ci, int start,
                                              float &rej_uni)
{
    float v = valid ? d2 : 1e10f;
    int id = valid ? ci : start;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const float ov = __shfl_xor(v, stride, 64);
            const int oi = __shfl_xor(id, stride, 64);
            const bool take_min = ((lane & stride) == 0) == ((lane & size) == 0);
            const bool swap = take_min ? (ov < v) : (ov > v);
            v = swap ? ov : v;
            id = swap ? oi : id;
        }
    }
    l.v = v;
    l.id = id;
    l.tau = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k - 1));
    if (k < 64) rej_uni = fminf(rej_uni, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)));  // best dropped
}

// Ties among the k+1 smallest distances of a finished list of G lanes (gl: the lane within it) -> the reference's order
// depends on its heap history.  Two adjacent equal values in the list, or the best rejected distance (rl per lane,
// ru list-uniform) equal to the k-th.  True in the lane that sees the tie: the caller ballots.
template <int G>
__device__ __forceinline__ bool list_tied(const LaneList &l, int k, int gl, float rl, float ru)
{
#pragma unroll
    for (int s = G / 2; s >= 1; s >>= 1) rl = fminf(rl, __shfl_xor(rl, s, 64));
    const float rej = fminf(rl, ru);
    const float nextv = __shfl_down(l.v, 1, G);
    const bool tie_in = gl < k - 1 && l.v == nextv && l.v < 1e10f;
    const bool tie_edge = gl == k - 1 && l.v < 1e10f && rej == l.v;
    return tie_in || tie_edge;
}

// ---- calibration: k-th neighbour distance of KG_SAMPLES queries, estimated on every 8th support point
// (the (k/8)-th neighbour among 1/8 of the points sits at about the same radius; h only steers speed,
// never results, so an estimate is enough) -----------------------------------------------------------
__global__ __launch_bounds__(1024) void kg_sample_kernel(int m, int k, int nb, int KG_SUB, const float *__restrict__ xyz,
                                                         const float *__restrict__ new_xyz,
                                                         const int *__restrict__ offset,
                                                         const int *__restrict__ new_offset, float *__restrict__ samples)
{
    __shared__ float vals[16 * KG_MAXK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = (int)(((long)blockIdx.x * m) / KG_SAMPLES);
    const int s = seg_of(q, new_offset, nb);
    const int start = s == 0 ? 0 : offset[s - 1], end = offset[s];
    const float qx = new_xyz[(size_t)q * 3], qy = new_xyz[(size_t)q * 3 + 1], qz = new_xyz[(size_t)q * 3 + 2];
    LaneList l;
    ll_init(l, start);
    float rl = 3.4e38f, ru = 3.4e38f;
    const int nsub = (end - start + KG_SUB - 1) / KG_SUB;  // sub-sampled points start, start+8, ...
    const int span = (nsub + 15) / 16;
    const int lo = wave * span, hi = min(nsub, lo + span);
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < hi;
        const int ii = start + (valid ? i : lo) * KG_SUB;
        const float d2 = dist2_ref(qx, qy, qz, xyz[(size_t)ii * 3], xyz[(size_t)ii * 3 + 1], xyz[(size_t)ii * 3 + 2]);
        ll_feed(l, k, lane, valid, d2, ii, rl, ru);
    }
    if (lane < k) vals[wave * k + lane] = l.v;
    __syncthreads();
    // the k-th smallest of the 16*k kept values: rank by counting
    const int total = 16 * k;
    if ((int)threadIdx.x < total) {
        const float mine = vals[threadIdx.x];
        int rank = 0;
        for (int j = 0; j < total; ++j) {
            const float o = vals[j];
            rank += (o < mine || (o == mine && j < (int)threadIdx.x)) ? 1 : 0;
        }
        if (rank == k - 1) samples[blockIdx.x] = mine;
    }
}

__global__ __launch_bounds__(64) void kg_params_kernel(int n, int nb, float hscale, float fixed_h, const int *__restrict__ bbox,
                                                       const float *__restrict__ samples, GridParams *__restrict__ gp)
{
    const int lane = threadIdx.x;
    const float mine = samples[lane];
    int rank = 0;
    for (int j = 0; j < KG_SAMPLES; ++j) {
        const float o = __shfl(mine, j, 64);
        rank += (o < mine || (o == mine && j < lane)) ? 1 : 0;
    }
    const unsigned long long pick = __ballot(rank == (KG_SAMPLES * 4) / 5);
    const float r2 = __shfl(mine, (int)__builtin_ctzll(pick), 64);
    if (lane != 0) return;
    const float minx = ord2f(bbox[0]), miny = ord2f(bbox[1]), minz = ord2f(bbox[2]);
    const float ex = fmaxf(ord2f(bbox[3]) - minx, 0.f), ey = fmaxf(ord2f(bbox[4]) - miny, 0.f),
                ez = fmaxf(ord2f(bbox[5]) - minz, 0.f);
    const float emax = fmaxf(fmaxf(ex, ey), fmaxf(ez, 1e-30f));
    float h = hscale * sqrtf(r2);
    if (!(r2 < 1e9f) || !(h > emax * 1e-6f)) h = emax;  // fewer than k points, or all points coincide
    if (fixed_h > 0.f) h = fixed_h;                      // radius searches bring their own cell size (a lower bound)
    const float cap = (float)(knn_cell_cap(n) / (nb > 0 ? nb : 1));
    // grow h until the grid fits the cell budget (float arithmetic: no int overflow on huge extents)
    for (int it = 0; it < 400 && (ex / h + 1.f) * (ey / h + 1.f) * (ez / h + 1.f) > cap; ++it) h *= 1.26f;
    const int nx = (int)(ex / h) + 1, ny = (int)(ey / h) + 1, nz = (int)(ez / h) + 1;
    gp->minx = minx; gp->miny = miny; gp->minz = minz;
    gp->h = h;
    gp->inv_h = 1.f / h;
    // fp32 rounding of (x - min) * inv_h is below 2^-22 * (cells along the axis): stay clear of it
    gp->margin = h * (1e-3f + 4e-7f * (float)max(nx, max(ny, nz)));
    gp->nx = nx; gp->ny = ny; gp->nz = nz;
    gp->ncell = nx * ny * nz;
}

__device__ __forceinline__ int cell_coord(float v, float mn, float inv_h, int dim)
{
    const int c = (int)floorf((v - mn) * inv_h);
    return min(max(c, 0), dim - 1);
}

// ---- the walk and the stop rule ("Grid-accelerated path" above), shared by every kernel that searches the grid ----
struct QueryCell {
    float qx, qy, qz;  // the query
    int cx, cy, cz;    // its (clamped) cell
    const int *cs;     // cell_start of its segment's grid
};

__device__ __forceinline__ QueryCell query_cell(const GridParams &g, const float *__restrict__ new_xyz, int q, int seg,
                                                const int *__restrict__ cell_start)
{
    QueryCell h;
    h.qx = new_xyz[(size_t)q * 3]; h.qy = new_xyz[(size_t)q * 3 + 1]; h.qz = new_xyz[(size_t)q * 3 + 2];
    h.cx = cell_coord(h.qx, g.minx, g.inv_h, g.nx);
    h.cy = cell_coord(h.qy, g.miny, g.inv_h, g.ny);
    h.cz = cell_coord(h.qz, g.minz, g.inv_h, g.nz);
    h.cs = cell_start + (size_t)seg * g.ncell;
    return h;
}

// The x-runs [bA, eA) and [bB, eB) of sorted[] that row (dz,dy) of shell R contributes: the full run where the row is
// on the rim (or R == 1, or the caller wants the whole block), else the two end cells; empty outside the grid.
__device__ __forceinline__ void shell_row_runs(const GridParams &g, const int *__restrict__ cs, int cx, int cy, int cz, int R,
                                               int dz, int dy, bool whole_block, int &bA, int &eA, int &bB, int &eB)
{
    bA = 0; eA = 0; bB = 0; eB = 0;
    const int z = cz + dz, y = cy + dy;
    if (z < 0 || z >= g.nz || y < 0 || y >= g.ny) return;
    const int row = (z * g.ny + y) * g.nx;
    if (whole_block || R == 1 || dz == -R || dz == R || dy == -R || dy == R) {
        bA = cs[row + max(cx - R, 0)];
        eA = cs[row + min(cx + R, g.nx - 1) + 1];
    } else {
        if (cx - R >= 0) { bA = cs[row + cx - R]; eA = cs[row + cx - R + 1]; }
        if (cx + R < g.nx) { bB = cs[row + cx + R]; eB = cs[row + cx + R + 1]; }
    }
}

// the same for pair pi = (dz + R) * (2R+1) + (dy + R) of the shell; pi >= (2R+1)^2 gives empty runs
__device__ __forceinline__ void shell_pair_runs(const GridParams &g, const int *__restrict__ cs, int cx, int cy, int cz, int R,
                                                int pi, bool whole_block, int &bA, int &eA, int &bB, int &eB)
{
    const int side = 2 * R + 1;
    if (pi < side * side) shell_row_runs(g, cs, cx, cy, cz, R, pi / side - R, pi % side - R, whole_block, bA, eA, bB, eB);
    else { bA = 0; eA = 0; bB = 0; eB = 0; }
}

// dmin - margin: nothing outside the block [c-R, c+R]^3 is nearer to the query; `whole`: the block covers the grid
__device__ __forceinline__ float shell_unseen_bound(const GridParams &g, const QueryCell &h, int R, bool &whole)
{
    float dmin = 3.4e38f;
    whole = true;
    if (h.cx - R > 0) { dmin = fminf(dmin, h.qx - (g.minx + (float)(h.cx - R) * g.h)); whole = false; }
    if (h.cx + R + 1 < g.nx) { dmin = fminf(dmin, (g.minx + (float)(h.cx + R + 1) * g.h) - h.qx); whole = false; }
    if (h.cy - R > 0) { dmin = fminf(dmin, h.qy - (g.miny + (float)(h.cy - R) * g.h)); whole = false; }
    if (h.cy + R + 1 < g.ny) { dmin = fminf(dmin, (g.miny + (float)(h.cy + R + 1) * g.h) - h.qy); whole = false; }
    if (h.cz - R > 0) { dmin = fminf(dmin, h.qz - (g.minz + (float)(h.cz - R) * g.h)); whole = false; }
    if (h.cz + R + 1 < g.nz) { dmin = fminf(dmin, (g.minz + (float)(h.cz + R + 1) * g.h) - h.qz); whole = false; }
    return dmin - g.margin;
}

// squared distance below which a candidate is strictly nearer than anything unseen (0: no such distance)
__device__ __forceinline__ float shell_safe_d2(float bound) { return bound > 0.f ? bound * bound * 0.99999f : 0.f; }

// the search may end: the k-th (worst kept) squared distance `kth` is strictly nearer than anything unseen
__device__ __forceinline__ bool shell_closed(float bound, bool whole, float kth)
{
    return whole || kth < shell_safe_d2(bound);  // (kth >= 0: a bound <= 0 closes nothing)
}

__global__ void kg_count_kernel(int n, int nb, const float *__restrict__ xyz, const int *__restrict__ offset,
                                const GridParams *__restrict__ gp, int *__restrict__ cell_count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GridParams g = *gp;
    const int cx = cell_coord(xyz[(size_t)i * 3], g.minx, g.inv_h, g.nx);
    const int cy = cell_coord(xyz[(size_t)i * 3 + 1], g.miny, g.inv_h, g.ny);
    const int cz = cell_coord(xyz[(size_t)i * 3 + 2], g.minz, g.inv_h, g.nz);
    const int seg = nb > 1 ? seg_of(i, offset, nb) : 0;
    atomicAdd(cell_count + (size_t)seg * g.ncell + ((size_t)cz * g.ny + cy) * g.nx + cx, 1);
}

// In-place exclusive scan of cell_count[0 .. nb*ncell] in three coalesced phases over tiles of
// KG_SCAN_TILE cells: per-tile sums, scan of the (<= 1024) tile sums, per-tile scan + offset.
// The cell count is only known on the device, so the grid is sized for the cell budget and
// surplus workgroups return.
__device__ __forceinline__ int block_excl_scan_256(int v, int *s_part, int &block_total)
{
    // exclusive scan of one int per thread across a 256-thread workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(inc, s, 64);
        if (lane >= s) inc += o;
    }
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_part[w];
    block_total = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(256) void kg_scan_sums_kernel(int nb, const GridParams *__restrict__ gp,
                                                           const int *__restrict__ cells, int *__restrict__ tile_sums)
{
    __shared__ int s_part[4];
    const int total = nb * gp->ncell;
    const int t0 = blockIdx.x * KG_SCAN_TILE;
    if (t0 >= total) { if (threadIdx.x == 0) tile_sums[blockIdx.x] = 0; return; }
    int sum = 0;
    for (int i = t0 + threadIdx.x; i < min(t0 + KG_SCAN_TILE, total); i += 256) sum += cells[i];
    int tot;
    block_excl_scan_256(sum, s_part, tot);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void kg_scan_tiles_kernel(int ntiles, int *__restrict__ tile_sums)
{
    __shared__ int part[1024];
    const int v = (int)threadIdx.x < ntiles ? tile_sums[threadIdx.x] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const int o = threadIdx.x >= s ? part[threadIdx.x - s] : 0;
        __syncthreads();
        part[threadIdx.x] += o;
        __syncthreads();
    }
    if ((int)threadIdx.x < ntiles) tile_sums[threadIdx.x] = part[threadIdx.x] - v;  // exclusive
    if (threadIdx.x == 1023) tile_sums[ntiles] = part[1023];
}

__global__ __launch_bounds__(256) void kg_scan_apply_kernel(int nb, const GridParams *__restrict__ gp,
                                                            int *__restrict__ cells, const int *__restrict__ tile_sums,
                                                            int ntiles)
{
    __shared__ int s_part[4];
    const int total = nb * gp->ncell;
    const int t0 = blockIdx.x * KG_SCAN_TILE;
    if (t0 >= total) return;
    int run = tile_sums[blockIdx.x];
    for (int c0 = t0; c0 < min(t0 + KG_SCAN_TILE, total); c0 += 256) {
        const int i = c0 + threadIdx.x;
        const int v = i < total ? cells[i] : 0;
        int tot;
        const int ex = block_excl_scan_256(v, s_part, tot);
        if (i < total) cells[i] = run + ex;
        run += tot;
    }
    if (t0 + KG_SCAN_TILE >= total && threadIdx.x == 0) cells[total] = tile_sums[ntiles];
}

__global__ void kg_scatter_kernel(int n, int nb, const float *__restrict__ xyz, const int *__restrict__ offset,
                                  const GridParams *__restrict__ gp, const int *__restrict__ cell_start,
                                  int *__restrict__ cursor, float4 *__restrict__ sorted)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GridParams g = *gp;
    const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    const int cx = cell_coord(x, g.minx, g.inv_h, g.nx), cy = cell_coord(y, g.miny, g.inv_h, g.ny),
              cz = cell_coord(z, g.minz, g.inv_h, g.nz);
    const int seg = nb > 1 ? seg_of(i, offset, nb) : 0;
    const size_t cell = (size_t)seg * g.ncell + ((size_t)cz * g.ny + cy) * g.nx + cx;
    const int pos = cell_start[cell] + atomicAdd(cursor + cell, 1);
    if (pos >= 0 && pos < n) sorted[pos] = make_float4(x, y, z, __int_as_float(i));  // guard: never write outside
}

// ---- queries --------------------------------------------------------------------------------------
// Packed runs.  The x-runs of a shell are short (a few points per cell), so a wavefront feeds them PACKED, 64 candidates
// per step, instead of one partly filled step per run: lane r owns run [b, b + len) of sorted[], an exclusive scan of
// the run lengths gives every candidate slot c its run (the last non-empty one whose first slot is <= c) and its
// place in it.
// -> number of slots (wave-uniform); excl: this lane's first slot
__device__ __forceinline__ int packed_scan(int len, int lane, int &excl)
{
    int incl = len;
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(incl, s, 64);
        if (lane >= s) incl += o;
    }
    excl = incl - len;
    return __builtin_amdgcn_readlane(incl, 63);
}

// position in sorted[] of slot c of the step [c0, c0 + 64); runs = __ballot(len > 0)
__device__ __forceinline__ int packed_slot_source(int c, int c0, unsigned long long runs, int excl, int b)
{
    int base = 0;
    while (runs) {
        const int src = (int)__builtin_ctzll(runs);
        runs &= runs - 1;
        const int e0 = __builtin_amdgcn_readlane(excl, src);
        if (e0 >= c0 + 64) break;  // later runs start beyond this step (wave-uniform)
        const int b0 = __builtin_amdgcn_readlane(b, src);
        base = c >= e0 ? b0 - e0 : base;
    }
    return base + c;
}

// `fresh`: nothing is in the list yet (wave-uniform)
__device__ __forceinline__ void kg_scan_packed(LaneList &l, int k, int lane, int b, int len, float qx, float qy, float qz,
                                               const float4 *__restrict__ sorted, float &rl, float &ru, bool &fresh,
                                               int start)
{
    int excl;
    const int total = packed_scan(len, lane, excl);
    const unsigned long long runs = __ballot(len > 0);
    for (int c0 = 0; c0 < total; c0 += 64) {
        const int c = c0 + lane;
        const int src = packed_slot_source(c, c0, runs, excl, b);
        const bool valid = c < total;
        const float4 p = sorted[valid ? src : __builtin_amdgcn_readfirstlane(src)];
        const float d2 = dist2_ref(qx, qy, qz, p.x, p.y, p.z);
        if (fresh) {  // wave-uniform: nothing in the list yet
            ll_sort_first(l, k, lane, valid, d2, __float_as_int(p.w), start, ru);
            fresh = false;
        } else {
            ll_feed(l, k, lane, valid, d2, __float_as_int(p.w), rl, ru);
        }
    }
}

__global__ __launch_bounds__(256) void kg_query_kernel(int m, int k, int nb, int self, const float *__restrict__ new_xyz,
                                                       const int *__restrict__ offset,
                                                       const int *__restrict__ new_offset,
                                                       const GridParams *__restrict__ gp,
                                                       const int *__restrict__ cell_start,
                                                       const float4 *__restrict__ sorted, int *__restrict__ idx,
                                                       float *__restrict__ dist2, int *__restrict__ fb_list,
                                                       int *__restrict__ fb_count)
{
    const int lane = threadIdx.x & 63;
    const GridParams g = *gp;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < m; t += gridDim.x * 4) {
        // when the queries are the support points themselves they are taken in cell order: the waves of a
        // workgroup then walk the same cells and share their candidates' cache lines
        const int q = self ? __float_as_int(sorted[t].w) : t;
        const int seg = nb > 1 ? seg_of(q, new_offset, nb) : 0;
        const int start = seg == 0 ? 0 : offset[seg - 1];
        const QueryCell h = query_cell(g, new_xyz, q, seg, cell_start);
        LaneList l;
        ll_init(l, start);
        float rl = 3.4e38f, ru = 3.4e38f;
        bool fresh = true;

        for (int R = 1;; ++R) {
            // the shell's (dz,dy) pairs, one per lane, in batches of 64
            const int npairs = (2 * R + 1) * (2 * R + 1);
            for (int p0 = 0; p0 < npairs; p0 += 64) {
                int bA, eA, bB, eB;
                shell_pair_runs(g, h.cs, h.cx, h.cy, h.cz, R, p0 + lane, false, bA, eA, bB, eB);
                kg_scan_packed(l, k, lane, bA, eA - bA, h.qx, h.qy, h.qz, sorted, rl, ru, fresh, start);
                if (R > 1) kg_scan_packed(l, k, lane, bB, eB - bB, h.qx, h.qy, h.qz, sorted, rl, ru, fresh, start);
            }
            bool whole;
            const float bound = shell_unseen_bound(g, h, R, whole);
            if (shell_closed(bound, whole, l.tau)) break;
        }

        if (__ballot(list_tied<64>(l, k, lane, rl, ru))) {
            if (lane == 0) fb_list[atomicAdd(fb_count, 1)] = q;
        } else if (lane < k) {
            idx[(size_t)q * k + lane] = l.id;
            dist2[(size_t)q * k + lane] = l.v;
        }
    }
}

// ---- several queries per wavefront (k <= G) ----------------------------------------------------------------
// kg_query_kernel holds a 64-lane wave slot per query although at most k lanes carry list entries.  Here a wave is
// cut into 64/G groups of G lanes and every group runs kg_query_kernel's search for a query of its own: same
// shells, same packed candidate steps (G wide), same sorted lane list (lanes 0..k-1 of the GROUP; steps with many
// passing candidates enter it by a sort and merge, see gl_merge), same two tie conditions and the same replay list.
// What a non-tied query stores is determined by the input alone (the k nearest in ascending distance), so both
// kernels store the same bits.
//
// Every cross-lane operation stays wave-wide and every branch around one is wave-uniform (exec is always full):
// ballots are taken over the wave and a group reads its own G bits; values that kg_query_kernel keeps wave-uniform
// in SGPRs (tau, the rejected minimum, the query and its cell) are group-uniform VGPRs here, broadcast with
// __shfl(x, src, G); loops run while ANY group of the wave has work and a group without work is predicated off
// (`act`, zero-length runs, an empty pass mask), which leaves its list and its rejected minimum untouched.
template <int G>
__device__ __forceinline__ unsigned grp_bits(unsigned long long wave_mask, int lane)
{
    static_assert(G == 16 || G == 32, "group width");
    return (unsigned)(wave_mask >> (lane & ~(G - 1))) & (G == 32 ? 0xffffffffu : 0xffffu);
}

// insert (cd, ci) into the lists of the groups with `ins` set (there cd < tau); the others keep theirs
template <int G>
__device__ __forceinline__ void gl_insert(LaneList &l, int k, int lane, int gl, bool ins, float cd, int ci)
{
    const int p = (int)__popc(grp_bits<G>(__ballot(gl < k && l.v <= cd), lane));  // first lane of the group with v > cd
    // wave_shr:1 hands a group's lane 0 the value of the previous group's last lane; lane 0 never takes the
    // shifted value (gl > p fails there: p >= 0), so nothing crosses from one query's list into another's
    const float upv = lane_below_f32(l.v);
    const int upi = lane_below_i32(l.id);
    if (ins && gl > p) { l.v = upv; l.id = upi; }
    if (ins && gl == p) { l.v = cd; l.id = ci; }
    l.tau = __shfl(l.v, k - 1, G);
}

// the candidates in `mine` (this group's G bits of the pass ballot), one after the other in lane order;
// ru / rl track rejected distances as in ll_feed
template <int G>
__device__ __forceinline__ void gl_feed(LaneList &l, int k, int lane, int gl, unsigned mine, float d2, int ci, float &rej_uni)
{
    while (__ballot(mine != 0)) {  // wave-uniform: some group still has a candidate
        const bool has = mine != 0;
        const int b = has ? (int)__builtin_ctz(mine) : 0;
        mine &= mine - 1;
        const float cd = __shfl(d2, b, G);
        const int cc = __shfl(ci, b, G);
        const bool ins = has && cd < l.tau;  // tau may have dropped below it since the ballot
        const float evicted = l.tau;
        gl_insert<G>(l, k, lane, gl, ins, cd, cc);
        rej_uni = fminf(rej_uni, has ? (ins ? evicted : cd) : 3.4e38f);
    }
}

// one compare-exchange stage of a bitonic network inside the groups (stride < G: the partner is in the same group).
// The keys are the bit patterns of non-negative floats, which order as integers do: integer min / max, no branch.
__device__ __forceinline__ void gl_cmpx(int &key, int &id, int stride, bool take_min)
{
    const int ok = __shfl_xor(key, stride, 64), oi = __shfl_xor(id, stride, 64);
    const int nk = take_min ? min(key, ok) : max(key, ok);
    id = nk != key ? oi : id;  // equal keys: both lanes keep their own entry
    key = nk;
}

// All passing candidates of a step at once, where one-by-one insertion (kg_query_kernel's way: ~45 instructions and
// two cross-lane round trips each here) would take longer: with G candidates per step the first steps of a query
// pass most of theirs (the first one all).  The group's candidates are sorted DESCENDING (bitonic network, lanes
// without a passing candidate carry 3.4e38), set against the ascending list lane by lane -- the smaller of each
// pair are the G smallest of both and form a bitonic sequence, the larger are dropped -- and one bitonic merge
// sorts them.  This is ll_sort_first for a list that may already hold entries: an empty list (placeholders 1e10,
// start) needs no case of its own.  Entries beyond the k-th are dropped as well; every dropped distance goes to
// the lane's rejected minimum, as ll_feed's rejected and evicted ones do.
template <int G>
__device__ __forceinline__ void gl_merge(LaneList &l, int k, int gl, bool pass, float d2, int ci, float &rej_lane)
{
    const int far = __float_as_int(3.4e38f);
    int key = pass ? __float_as_int(d2) : far, id = ci;
#pragma unroll
    for (int size = 2; size <= G; size <<= 1) {
        const bool up = size < G && (gl & size) == 0;  // alternating below G, the whole group descending
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) gl_cmpx(key, id, stride, ((gl & stride) == 0) == up);
    }
    const int lk = gl < k ? __float_as_int(l.v) : far;  // lanes beyond the list hold nothing
    const bool cand = key < lk;
    rej_lane = fminf(rej_lane, __int_as_float(cand ? lk : key));
    key = cand ? key : lk;
    id = cand ? id : l.id;
#pragma unroll
    for (int stride = G / 2; stride > 0; stride >>= 1) gl_cmpx(key, id, stride, (gl & stride) == 0);
    l.v = __int_as_float(key);
    l.id = id;
    if (gl >= k) rej_lane = fminf(rej_lane, l.v);
    l.tau = __shfl(l.v, k - 1, G);
}

constexpr int KGG_MERGE_FROM = 4;  // passing candidates of a step (the fuller group's) from which gl_merge is used

// kg_scan_packed for groups: lane gl of a group owns run [b, b + len) of that group's query (len == 0 where the
// group is finished or the lane has no run); G candidates per group and step
template <int G>
__device__ __forceinline__ void gl_scan_packed(LaneList &l, int k, int lane, int gl, int b, int len, float qx, float qy,
                                               float qz, const float4 *__restrict__ sorted, float &rl, float &ru)
{
    int incl = len;
#pragma unroll
    for (int s = 1; s < G; s <<= 1) {
        const int o = __shfl_up(incl, s, G);
        if (gl >= s) incl += o;
    }
    const int total = __shfl(incl, G - 1, G);  // group-uniform
    const int boff = b - (incl - len);         // run start minus the run's first candidate slot
    int wtotal = 0;                            // wave-uniform loop bound: the longest group
#pragma unroll
    for (int gq = 0; gq < 64 / G; ++gq) wtotal = max(wtotal, __builtin_amdgcn_readlane(incl, gq * G + G - 1));
    for (int c0 = 0; c0 < wtotal; c0 += G) {
        const int c = c0 + gl;
        const bool valid = c < total;  // a group that has run out of candidates feeds nothing
        // the run of slot c is the first lane of the group whose inclusive sum exceeds c (an empty run never is):
        // binary search over the non-decreasing sums
        int j = 0;
#pragma unroll
        for (int s = G / 2; s >= 1; s >>= 1) j += __shfl(incl, j + s - 1, G) <= c ? s : 0;
        const int src = __shfl(boff, j, G) + c;  // j <= G - 1 where valid
        const float4 p = sorted[valid ? src : 0];
        const float d2 = dist2_ref(qx, qy, qz, p.x, p.y, p.z);
        const bool pass = valid && d2 < l.tau;
        rl = fminf(rl, (valid && !pass) ? d2 : 3.4e38f);
        const unsigned long long wpass = __ballot(pass);
        int most = 0;  // wave-uniform: passing candidates of the fullest group
#pragma unroll
        for (int gq = 0; gq < 64 / G; ++gq) most = max(most, (int)__popc(grp_bits<G>(wpass, gq * G)));
        if (most >= KGG_MERGE_FROM) gl_merge<G>(l, k, gl, pass, d2, __float_as_int(p.w), rl);
        else if (most > 0) gl_feed<G>(l, k, lane, gl, grp_bits<G>(wpass, lane), d2, __float_as_int(p.w), ru);
    }
}

// (waves_per_eu: left alone the compiler takes 65 registers, one over what eight waves per SIMD allow; held to eight
// it takes 62 and spills nothing)
template <int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void kg_query_group_kernel(
                                                             int m, int k, int nb, int self,
                                                             const float *__restrict__ new_xyz,
                                                             const int *__restrict__ offset,
                                                             const int *__restrict__ new_offset,
                                                             const GridParams *__restrict__ gp,
                                                             const int *__restrict__ cell_start,
                                                             const float4 *__restrict__ sorted, int *__restrict__ idx,
                                                             float *__restrict__ dist2, int *__restrict__ fb_list,
                                                             int *__restrict__ fb_count)
{
    constexpr int NG = 64 / G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1);
    const GridParams g = *gp;
    for (int t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NG; t0 < m; t0 += gridDim.x * 4 * NG) {
        // self searches: the wave's queries are consecutive entries of sorted[], i.e. the groups walk the same cells.
        // The last wave's missing queries (m % NG != 0) shadow the wave's first one in lockstep and store nothing.
        const int t = t0 + lane / G;
        const bool live = t < m;
        const int tq = live ? t : t0;
        const int q = self ? __float_as_int(sorted[tq].w) : tq;
        const int seg = nb > 1 ? seg_of(q, new_offset, nb) : 0;
        const int start = seg == 0 ? 0 : offset[seg - 1];
        const QueryCell h = query_cell(g, new_xyz, q, seg, cell_start);
        LaneList l;
        ll_init(l, start);  // a segment with fewer than k points leaves the placeholders (1e10, start) at the tail
        float rl = 3.4e38f, ru = 3.4e38f;
        bool act = true;  // group-uniform: this group's search goes on

        for (int R = 1;; ++R) {
            // the shell's (dz,dy) pairs, G per batch: the 9 pairs of R == 1 and the 25 of R == 2 fit one batch of 32;
            // a finished group asks for the pair past the last, which has no runs
            const int npairs = (2 * R + 1) * (2 * R + 1);
            for (int p0 = 0; p0 < npairs; p0 += G) {
                int bA, eA, bB, eB;
                shell_pair_runs(g, h.cs, h.cx, h.cy, h.cz, R, act ? p0 + gl : npairs, false, bA, eA, bB, eB);
                gl_scan_packed<G>(l, k, lane, gl, bA, eA - bA, h.qx, h.qy, h.qz, sorted, rl, ru);
                if (R > 1) gl_scan_packed<G>(l, k, lane, gl, bB, eB - bB, h.qx, h.qy, h.qz, sorted, rl, ru);
            }
            bool whole;
            const float bound = shell_unseen_bound(g, h, R, whole);
            if (shell_closed(bound, whole, l.tau)) act = false;
            if (!__ballot(act)) break;  // the wave goes on while any of its groups does
        }

        const bool tied = grp_bits<G>(__ballot(list_tied<G>(l, k, gl, rl, ru)), lane) != 0;
        if (live) {
            if (tied) {
                if (gl == 0) fb_list[atomicAdd(fb_count, 1)] = q;
            } else if (gl < k) {
                idx[(size_t)q * k + gl] = l.id;
                dist2[(size_t)q * k + gl] = l.v;
            }
        }
    }
}

// One WORKGROUP per listed query (the grid path's tie fallback: a handful of queries per call).  The reference's
// output for such a query depends on its heap history, i.e. on every ACCEPTED candidate of an ascending index scan
// (a candidate is accepted iff fewer than k earlier candidates are at most as far).  Two things keep the replay
// short:
//  * Pruning by the grid.  Let S be the points of the query's 3x3x3 cell block nearer than the block's
//    boundary (nothing outside the block is that near), and T the k-th smallest INDEX in S.  Beyond T every
//    point outside S already has k nearer predecessors and is rejected, so the replay is: all of [start, T) in
//    index order, then the members of S with index >= T in index order.  T is ~ k/|S| of the segment.
//  * The prefix [start, T) is consumed in steps whose size doubles from 64 up to 4096 candidates (4 per
//    thread): every thread tests its candidates against the heap root as it was at the start of the step
//    (conservative: the root only decreases), and only the survivors (~k per doubling) are replayed by wave 0
//    against the heap in LDS; the loads of the next step are issued before the barriers of the current one.
// The replayed max-heap of wave 0 lives in LANES (node i in lane i; the grid path has k <= 64).  Replacing the
// root is then mostly lane-parallel: every lane finds its larger child (two cross-lane reads), the sift-down path
// is walked with one v_readlane per level, and all nodes on the path take their child's entry at once.
// Same result as the reference's reheap (knnquery_cuda_kernel.cu:21-36) after `dist[0] = cd; idx[0] = ci`:
// the right child is preferred only when strictly larger; the moving value stops when it is strictly larger
// than the larger child.
struct LaneHeap {
    float d;
    int id;
};
__device__ __forceinline__ float lh_root(const LaneHeap &h) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h.d), 0)); }

__device__ __forceinline__ void lh_replace_root(LaneHeap &h, int k, int lane, float cd, int ci)
{
    const int c1 = 2 * lane + 1, c2 = 2 * lane + 2;
    const float d1 = __shfl(h.d, c1 & 63, 64), d2 = __shfl(h.d, c2 & 63, 64);
    const bool right = c2 < k && d2 > d1;
    const int big = right ? c2 : c1;      // meaningful where c1 < k
    const float dbig = right ? d2 : d1;
    int p = 0;
    unsigned long long path = 0;          // nodes that take their larger child's entry
    while (2 * p + 1 < k) {
        const float dc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dbig), p));
        if (cd > dc) break;
        path |= 1ull << p;
        p = __builtin_amdgcn_readlane(big, p);
    }
    const int ibig = __shfl(h.id, big & 63, 64);
    const bool on = (path >> lane) & 1ull;
    h.d = on ? dbig : h.d;
    h.id = on ? ibig : h.id;
    if (lane == p) { h.d = cd; h.id = ci; }
}

constexpr int KXL_PER = 8;   // candidates per thread and step
constexpr int KXL_MAXR = 2;  // largest cell block (2R+1)^3 tried for the pruning set
__global__ __launch_bounds__(1024) void knn_exact_list_kernel(
    int nsample, int nbatch, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const int *__restrict__ offset, const int *__restrict__ new_offset, int *__restrict__ idx,
    float *__restrict__ dist2, const int *__restrict__ qlist, const int *__restrict__ qcount,
    const GridParams *__restrict__ gp, const int *__restrict__ cell_start, const float4 *__restrict__ sorted)
{
    __shared__ float s_d2[1024 * KXL_PER];
    __shared__ float s_rd[1024];  // S by index rank: distance
    __shared__ int s_ri[1024];    //                  index
    __shared__ unsigned long long s_mask[KXL_PER][16];
    __shared__ float s_root;
    __shared__ int s_run_b[(2 * KXL_MAXR + 1) * (2 * KXL_MAXR + 1)], s_run_e[(2 * KXL_MAXR + 1) * (2 * KXL_MAXR + 1)], s_T, s_cnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = *qcount;
    for (int qi = blockIdx.x; qi < total; qi += gridDim.x) {
        const int pt = qlist[qi];
        const int bt = seg_of(pt, new_offset, nbatch);
        const int start = bt == 0 ? 0 : offset[bt - 1], seg_end = offset[bt];
        const float qx = new_xyz[(size_t)pt * 3], qy = new_xyz[(size_t)pt * 3 + 1], qz = new_xyz[(size_t)pt * 3 + 2];
        __syncthreads();
        LaneHeap hp;  // used by wave 0 only
        hp.d = 1e10f;
        hp.id = start;
        if (threadIdx.x == 0) { s_root = 1e10f; s_T = seg_end; s_cnt = 0; }
        __syncthreads();

        // ---- grid pruning: S and T -------------------------------------------------------------------
        int *s_si = (int *)(s_d2 + 1024);      // S by candidate slot: index      (s_d2[0..1023]: distance)
        int ns = 0;                            // |S| when the pruning applies, else 0
        if (gp) {  // (every caller brings a grid; unguarded, the loads move above the barriers and cost six registers)
            const GridParams g = *gp;
            const QueryCell h = query_cell(g, new_xyz, pt, bt, cell_start);
            // the (2R+1)^3 block for R = 1, then 2: the first whose S holds at least k points is used
            for (int R = 1; R <= KXL_MAXR && ns == 0; ++R) {
                const int nruns = (2 * R + 1) * (2 * R + 1);
                __syncthreads();
                if ((int)threadIdx.x < nruns) {
                    int b, e, bB, eB;  // whole block: every pair gives its full x-run, no second run
                    shell_pair_runs(g, h.cs, h.cx, h.cy, h.cz, R, (int)threadIdx.x, true, b, e, bB, eB);
                    s_run_b[threadIdx.x] = b;
                    s_run_e[threadIdx.x] = e;
                }
                if (threadIdx.x == 0) s_cnt = 0;
                __syncthreads();
                bool whole;
                const float r0 = shell_safe_d2(shell_unseen_bound(g, h, R, whole));  // nothing outside the block is nearer
                int tot = 0;
                for (int r = 0; r < nruns; ++r) tot += s_run_e[r] - s_run_b[r];
                if (tot > 1024 * KXL_PER) break;  // workgroup-uniform: too dense for the LDS staging -> full scan
                // up to KXL_PER block candidates per thread; members of S are appended to the slot arrays
                float cd[KXL_PER];
                int ci[KXL_PER];
                bool in_s[KXL_PER];
#pragma unroll
                for (int u = 0; u < KXL_PER; ++u) {
                    const int c = u * 1024 + (int)threadIdx.x;
                    in_s[u] = false;
                    cd[u] = 0.f;
                    ci[u] = 0;
                    if (c < tot) {
                        int acc = 0, src = 0;
                        for (int r = 0; r < nruns; ++r) {
                            const int len = s_run_e[r] - s_run_b[r];
                            if (c >= acc && c < acc + len) src = s_run_b[r] + (c - acc);
                            acc += len;
                        }
                        const float4 p = sorted[src];
                        cd[u] = dist2_ref(qx, qy, qz, p.x, p.y, p.z);
                        ci[u] = __float_as_int(p.w);
                        in_s[u] = cd[u] < r0;
                    }
                    if (in_s[u]) {
                        const int slot = atomicAdd(&s_cnt, 1);
                        if (slot < 1024) { s_d2[slot] = cd[u]; s_si[slot] = ci[u]; }
                    }
                }
                __syncthreads();
                const int cnt = s_cnt;
                if (cnt >= nsample && cnt <= 1024) {
                    // rank of every member's index within S (indices are distinct)
#pragma unroll
                    for (int u = 0; u < KXL_PER; ++u) {
                        if (in_s[u]) {
                            int rank = 0;
                            for (int j = 0; j < cnt; ++j) rank += s_si[j] < ci[u] ? 1 : 0;
                            s_rd[rank] = cd[u];
                            s_ri[rank] = ci[u];
                            if (rank == nsample - 1) s_T = ci[u] + 1;  // the k-th smallest index of S closes the prefix
                        }
                    }
                    ns = cnt;
                }
                __syncthreads();
            }
        }
        const int end = s_T;  // == seg_end without pruning

        auto step_len = [&](int pos) { return min(1024 * KXL_PER, max(64, pos - start)); };
        float px[KXL_PER], py[KXL_PER], pz[KXL_PER];
        auto load = [&](int pos, int len) {
#pragma unroll
            for (int j = 0; j < KXL_PER; ++j) {
                const int o = j * 1024 + (int)threadIdx.x;
                const int i = (o < len && pos + o < end) ? pos + o : start;
                px[j] = xyz[(size_t)i * 3]; py[j] = xyz[(size_t)i * 3 + 1]; pz[j] = xyz[(size_t)i * 3 + 2];
            }
        };
        constexpr int per = KXL_PER;
        auto step_len2 = [&](int pos) { return step_len(pos); };
        int pos = start, len = step_len2(start);
        if (pos < end) load(pos, len);
        while (pos < end) {
            const float root0 = s_root;
            float d2[KXL_PER];
            bool pass[KXL_PER], any = false;
#pragma unroll
            for (int j = 0; j < KXL_PER; ++j) {
                const int o = j * 1024 + (int)threadIdx.x;
                d2[j] = dist2_ref(qx, qy, qz, px[j], py[j], pz[j]);
                pass[j] = o < len && pos + o < end && d2[j] < root0;
                any |= pass[j];
            }
            const int npos = pos + len, nlen = step_len2(npos);
            if (npos < end) load(npos, nlen);  // in flight across the barriers below
            if (__syncthreads_or(any)) {
#pragma unroll
                for (int j = 0; j < KXL_PER; ++j) {
                    if (j < per) s_d2[j * 1024 + threadIdx.x] = d2[j];
                    const unsigned long long mk = __ballot(pass[j]);
                    if (lane == 0) s_mask[j][wave] = mk;
                }
                __syncthreads();
                if (wave == 0) {  // ascending index order: slab by slab, wave by wave, bit by bit
                    float root = root0;
                    // lane (j*16 + w) fetches mask word (j, w); only the non-empty words are visited
                    // (KXL_PER * 16 = 128 words: two per lane, slabs 0-3 then 4-7)
                  for (int half = 0; half < KXL_PER / 4; ++half) {
                    const unsigned long long mine = s_mask[half * 4 + (lane >> 4)][lane & 15];
                    unsigned long long words = __ballot(mine != 0);
                    while (words) {
                        const int wsel = (int)__builtin_ctzll(words);
                        words &= words - 1;
                        unsigned long long mm = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(mine >> 32), wsel) << 32) |
                                                (unsigned)__builtin_amdgcn_readlane((int)(mine & 0xffffffffu), wsel);
                        while (mm) {
                            const int b = (int)__builtin_ctzll(mm);
                            mm &= mm - 1;
                            const int o = half * 4096 + wsel * 64 + b;  // == j*1024 + w*64 + b
                            const float cd = s_d2[o];
                            if (cd < root) {  // knnquery_cuda_kernel.cu:97-101
                                lh_replace_root(hp, nsample, lane, cd, pos + o);
                                root = lh_root(hp);
                            }
                        }
                    }
                  }
                    if (lane == 0) s_root = root;
                }
                __syncthreads();
            }
            pos = npos;
            len = nlen;
        }
        if (wave == 0) {
            // the members of S beyond the prefix, in index order (ranks nsample.. hold the indices >= T)
            float root = s_root;
            for (int r = nsample; r < ns; ++r) {
                const float cd = s_rd[r];
                if (cd < root) {
                    lh_replace_root(hp, nsample, lane, cd, s_ri[r]);
                    root = lh_root(hp);
                }
            }
            for (int i = nsample - 1; i > 0; i--) {  // knnquery_cuda_kernel.cu:39-48: swap(0, i); reheap(i)
                const float d0 = lh_root(hp), di = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hp.d), i));
                const int j0 = __builtin_amdgcn_readlane(hp.id, 0), ji = __builtin_amdgcn_readlane(hp.id, i);
                if (lane == i) { hp.d = d0; hp.id = j0; }
                lh_replace_root(hp, i, lane, di, ji);
            }
            if (lane < nsample) {
                idx[(size_t)pt * nsample + lane] = hp.id;
                if (dist2) dist2[(size_t)pt * nsample + lane] = hp.d;  // (amc3d_knn_prefix: the caller may not want them)
            }
        }
    }
}

// ---- k nearest as the PREFIX of a finished row (amc3d_knn_prefix) -------------------------------------------------
// The loss votes the labels of its coarser stages over the kr = 4 / 16 nearest full-resolution points of every stage
// point -- and a stage point IS a full-resolution point, whose 24 nearest the stage-0 self search has just stored in
// ascending distance.  Where the first kr + 1 distances of that row are pairwise different (strictly ascending) the
// reference's kr-heap output is determined by the distances alone (see "Exactness" above): columns 0..kr-1 of the row,
// whichever of the search kernels or the replay wrote it.  The distances of the row are dist2_ref of the same bits.
// 32 lanes per query: they scan the query's own grid cell for the support points with equal coordinates (exactly one
// must match: with coincident points the row found need not be the query's in the reference's tie order, and the rows
// of both carry a zero-distance tie anyway), check the row, and copy; everything else goes to the replay list.
// Every cross-lane operation is wave-wide; a group without a query is predicated off.
__global__ __launch_bounds__(256) void kg_prefix_kernel(int m, int kr, int nb, int row_stride, const float *__restrict__ new_xyz,
                                                        const int *__restrict__ new_offset, const GridParams *__restrict__ gp,
                                                        const int *__restrict__ cell_start, const float4 *__restrict__ sorted,
                                                        const int *__restrict__ rows_idx, const float *__restrict__ rows_d2,
                                                        int *__restrict__ idx, float *__restrict__ dist2,
                                                        int *__restrict__ fb_list, int *__restrict__ fb_count)
{
    const int lane = threadIdx.x & 63, gl = lane & 31;
    const long qg = ((long)blockIdx.x * 256 + threadIdx.x) >> 5;
    const bool act = qg < m;
    const int q = act ? (int)qg : 0;
    const GridParams g = *gp;
    const int seg = nb > 1 ? seg_of(q, new_offset, nb) : 0;
    const QueryCell h = query_cell(g, new_xyz, q, seg, cell_start);
    const float qx = h.qx, qy = h.qy, qz = h.qz;
    const size_t cell = ((size_t)h.cz * g.ny + h.cy) * g.nx + h.cx;
    const int b = h.cs[cell];
    const int len = act ? h.cs[cell + 1] - b : 0;
    const int wave_len = max(len, __shfl_xor(len, 32, 64));
    int found = 0, cnt = 0;
    for (int c0 = 0; c0 < wave_len; c0 += 32) {  // (a few points per cell)
        const int c = c0 + gl;
        const bool valid = c < len;
        const float4 pt = sorted[valid ? b + c : 0];
        const bool match = valid && pt.x == qx && pt.y == qy && pt.z == qz;
        const unsigned bits = grp_bits<32>(__ballot(match), lane);
        cnt += (int)__popc(bits);
        const int v = __shfl(__float_as_int(pt.w), (lane & 32) + (bits ? (int)__builtin_ctz(bits) : 0), 64);
        if (bits) found = v;
    }
    const bool one = act && cnt == 1;
    const size_t row = one ? (size_t)found * row_stride : 0;
    const float d = gl <= kr ? rows_d2[row + gl] : 0.f;  // kr <= 31: columns 0..kr sit in the group's lanes
    const float dnext = __shfl_down(d, 1, 64);
    const bool bad = (gl < kr && !(d < dnext)) || (gl == kr && !(d < 1e10f));
    const bool use = one && grp_bits<32>(__ballot(bad), lane) == 0;
    if (use) {
        if (gl < kr) {
            idx[(size_t)q * kr + gl] = rows_idx[row + gl];
            if (dist2) dist2[(size_t)q * kr + gl] = d;
        }
    } else if (act && gl == 0) {
        fb_list[atomicAdd(fb_count, 1)] = q;
    }
}

// ---- host side: the workspace as typed pointers ------------------------------------------------------------
struct GridView {
    GridParams *gp;
    int *bbox;
    float *samples;
    int *off_s, *off_q;  // uniform segment ends of the batched (B, N, 3) searches
    int *fb_count;       // number of entries of fb_list (AMC_KNN_FALLBACK_COUNT_OFFSET)
    int *tile_sums, *cell_start, *cursor;
    float4 *sorted;
    int *fb_list;        // queries handed to the replay
};

static GridView grid_view(const KnnWorkspace &w, void *workspace)
{
    char *base = (char *)workspace;
    GridView v;
    v.gp = (GridParams *)(base + w.params);
    v.bbox = (int *)(base + w.bbox);
    v.samples = (float *)(base + w.samples);
    v.off_s = (int *)(base + w.off_s);
    v.off_q = (int *)(base + w.off_q);
    v.fb_count = (int *)(base + w.fb_count);
    v.tile_sums = (int *)(base + w.tile_sums);
    v.cell_start = (int *)(base + w.cell_start);
    v.cursor = (int *)(base + w.cursor);
    v.sorted = (float4 *)(base + w.sorted);
    v.fb_list = (int *)(base + w.fb_list);
    return v;
}

// Grid construction shared by the k-NN, ball-query and 3-NN searches: bounding box, cell size (calibrated on
// `ksample`-th neighbour distances of 64 sample queries, or `fixed_h` when > 0), counting sort of the support
// points into cell order.  Leaves GridParams, cell_start[] and sorted[] in the workspace.
static int kg_build(const GridView &v, int n, int m, int nbatch, const float *xyz, const float *new_xyz, const int *offset,
                    const int *new_offset, int ksample, int sub, float hscale, float fixed_h, hipStream_t stream)
{
    const size_t cells = (size_t)knn_cell_cap(n) + 1;
    // cell_start and cursor are neighbours in the workspace (knn_layout): one launch zeroes both and the padding between
    if (int st = fill_i32(v.cell_start, 0, (size_t)(v.cursor - v.cell_start) + cells, stream)) return st;
    hipLaunchKernelGGL(kg_init_kernel, dim3(1), dim3(64), 0, stream, v.bbox, v.fb_count);
    hipLaunchKernelGGL(kg_bbox_kernel, dim3(min(div_up(n, 256), 64)), dim3(256), 0, stream, n, xyz, v.bbox);
    if (!(fixed_h > 0.f))
        hipLaunchKernelGGL(kg_sample_kernel, dim3(KG_SAMPLES), dim3(1024), 0, stream, m, ksample, nbatch, sub, xyz, new_xyz,
                           offset, new_offset, v.samples);
    hipLaunchKernelGGL(kg_params_kernel, dim3(1), dim3(64), 0, stream, n, nbatch, hscale, fixed_h, v.bbox, v.samples, v.gp);
    hipLaunchKernelGGL(kg_count_kernel, dim3(div_up(n, 256)), dim3(256), 0, stream, n, nbatch, xyz, offset, v.gp,
                       v.cell_start);
    const int ntiles = div_up(knn_cell_cap(n), KG_SCAN_TILE);  // <= 1024
    hipLaunchKernelGGL(kg_scan_sums_kernel, dim3(ntiles), dim3(256), 0, stream, nbatch, v.gp, v.cell_start, v.tile_sums);
    hipLaunchKernelGGL(kg_scan_tiles_kernel, dim3(1), dim3(1024), 0, stream, ntiles, v.tile_sums);
    hipLaunchKernelGGL(kg_scan_apply_kernel, dim3(ntiles), dim3(256), 0, stream, nbatch, v.gp, v.cell_start, v.tile_sums,
                       ntiles);
    hipLaunchKernelGGL(kg_scatter_kernel, dim3(div_up(n, 256)), dim3(256), 0, stream, n, nbatch, xyz, offset, v.gp,
                       v.cell_start, v.cursor, v.sorted);
    return launch_status("grid build");
}

// The grid of a k-NN call, its replay list empty.  reuse_grid: the workspace still holds the grid of this very support
// set (xyz, offset) from an earlier call -- its cell size was calibrated for that call's k, which only steers speed --
// and only the replay counter is reset.  Else the grid is built with cell edge = 0.7 x p80 of the ceil(k/4)-th
// neighbour distance among every 4th support point (see "Cell size" above).
static int grid_prepare(const GridView &v, int reuse_grid, int n, int m, int nbatch, const float *xyz, const float *new_xyz,
                        const int *offset, const int *new_offset, int k, hipStream_t stream)
{
    if (reuse_grid) {
        hipLaunchKernelGGL(kg_init_kernel, dim3(1), dim3(64), 0, stream, v.bbox, v.fb_count);
        return 0;
    }
    const int kg_sub = 4;
    const float kg_scale = 0.7f;
    return kg_build(v, n, m, nbatch, xyz, new_xyz, offset, new_offset, (k + kg_sub - 1) / kg_sub, kg_sub, kg_scale, 0.f, stream);
}

// ---- batched (B, N, 3) searches on the same grid: ball query and 3-NN --------------------------------
// cumulative ends of the uniform segments of a (B, N, 3) / (B, M, 3) pair
__global__ void kg_uniform_offsets_kernel(int nb, int n_per, int m_per, int *__restrict__ off_s, int *__restrict__ off_q)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) { off_s[i] = (i + 1) * n_per; off_q[i] = (i + 1) * m_per; }
}

// Ball query (ball_query_gpu.cu:15-51) on the grid, cell edge >= radius: every point within the radius of a query
// lies in the 3x3x3 block around the query's cell.  One wavefront per query keeps the `nsample` SMALLEST hit
// indices sorted in its lanes (the reference returns the first nsample hits of an ascending index scan), then
// pads with the first hit exactly as the reference does; a query without a hit yields zeros.
__global__ __launch_bounds__(256) void bq_grid_kernel(int nq, int n, int m, float radius2, int nsample,
                                                      const float *__restrict__ new_xyz,
                                                      const GridParams *__restrict__ gp,
                                                      const int *__restrict__ cell_start,
                                                      const float4 *__restrict__ sorted, int *__restrict__ idx)
{
    const int lane = threadIdx.x & 63;
    const GridParams g = *gp;
    for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += gridDim.x * 4) {
        const int bs = q / m;
        const QueryCell h = query_cell(g, new_xyz, q, bs, cell_start);
        int b, e, bB, eB;  // the whole 3x3x3 block: lanes 0..8 own its nine full x-runs
        shell_pair_runs(g, h.cs, h.cx, h.cy, h.cz, 1, lane, true, b, e, bB, eB);
        int excl;
        const int total = packed_scan(e - b, lane, excl);
        const unsigned long long runs = __ballot(e > b);
        int key = 0x7fffffff;  // this lane's entry of the ascending list of the smallest hit indices
        int tau = 0x7fffffff;  // its nsample-th entry (wave-uniform)
        int have = 0;
        for (int c0 = 0; c0 < total; c0 += 64) {
            const int c = c0 + lane;
            const int src = packed_slot_source(c, c0, runs, excl, b);
            const bool valid = c < total;
            const float4 p = sorted[valid ? src : __builtin_amdgcn_readfirstlane(src)];
            const float d2 = dist2_ref(h.qx, h.qy, h.qz, p.x, p.y, p.z);
            const int pi = __float_as_int(p.w);
            unsigned long long hits = __ballot(valid && d2 < radius2 && pi < tau);
            while (hits) {
                const int src = (int)__builtin_ctzll(hits);
                hits &= hits - 1;
                const int ci = __builtin_amdgcn_readlane(pi, src);
                if (ci < tau) {
                    const int pos = (int)__popcll(__ballot(lane < nsample && key < ci));
                    const int up = lane_below_i32(key);
                    if (lane > pos) key = up;
                    if (lane == pos) key = ci;
                    tau = __builtin_amdgcn_readlane(key, nsample - 1);
                    have = min(have + 1, nsample);
                }
            }
        }
        const int first = have > 0 ? __builtin_amdgcn_readlane(key, 0) - bs * n : 0;
        if (lane < nsample) idx[(size_t)q * nsample + lane] = lane < have ? key - bs * n : first;
    }
}

// three_nn (interpolate_gpu.cu:16-59) on the grid: the 3 nearest known points of every unknown point, ties
// resolved as the reference's ascending strict-'<' scan does (the lower index ranks first), i.e. the list is
// ordered by (distance, index) -- exact without a replay.  The walk and the stop rule of "Grid-accelerated path".
// One THREAD per query: a 3-NN query meets a dozen candidates in its 27 cells, so a wave per query (the first version of
// this kernel: 275 us for the 192000 queries of the finest FeaturePropagation level, 104 us now) spends its time in
// cross-lane bookkeeping; a thread keeps the three best in registers and walks the nine x-runs of its neighbourhood itself,
// four candidates in flight.  Larger or smaller cells are slower (0.7 x / 1.4 x the calibrated edge: 121 us).
__global__ __launch_bounds__(256) void nn3_grid_thread_kernel(int nq, int n, int m, const float *__restrict__ unknown,
                                                              const GridParams *__restrict__ gp,
                                                              const int *__restrict__ cell_start,
                                                              const float4 *__restrict__ sorted, float *__restrict__ dist2,
                                                              int *__restrict__ idx)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const GridParams g = *gp;
    const float inf = __builtin_inff();
    const int bs = q / n;
    const QueryCell h = query_cell(g, unknown, q, bs, cell_start);
    float d0 = inf, d1 = inf, d2 = inf;
    int i0 = bs * m, i1 = bs * m, i2 = bs * m;  // local index 0: the reference's initial besti
    auto consider = [&](const float4 p) {
        const float cd = dist2_ref(h.qx, h.qy, h.qz, p.x, p.y, p.z);
        const int ci = __float_as_int(p.w);
        if (cd < d2 || (cd == d2 && ci < i2)) {
            if (cd < d1 || (cd == d1 && ci < i1)) {
                d2 = d1; i2 = i1;
                if (cd < d0 || (cd == d0 && ci < i0)) { d1 = d0; i1 = i0; d0 = cd; i0 = ci; }
                else { d1 = cd; i1 = ci; }
            } else { d2 = cd; i2 = ci; }
        }
    };
    auto run = [&](int b0, int e0) {  // four candidates in flight: the walk is a chain of cache latencies otherwise
        for (int c = b0; c < e0; c += 4) {
            const int last = e0 - 1;
            const float4 p0 = sorted[c], p1 = sorted[min(c + 1, last)], p2 = sorted[min(c + 2, last)],
                         p3 = sorted[min(c + 3, last)];
            consider(p0);
            if (c + 1 < e0) consider(p1);
            if (c + 2 < e0) consider(p2);
            if (c + 3 < e0) consider(p3);
        }
    };
    {   // first shell: the bounds of its nine x-runs as one batch of loads (18 in flight), then the runs
        int rb[9], re[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            int bB, eB;  // R == 1: every pair is one full run
            shell_pair_runs(g, h.cs, h.cx, h.cy, h.cz, 1, t, false, rb[t], re[t], bB, eB);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) run(rb[t], re[t]);
    }
    for (int R = 1;; ++R) {
        for (int dz = -R; R > 1 && dz <= R; ++dz) {
            // a thin grid (nz == 1) is crossed in hundreds of rings: a z-row outside it must cost nothing
            if (h.cz + dz < 0 || h.cz + dz >= g.nz) continue;
            for (int dy = -R; dy <= R; ++dy) {  // (dz, dy) as they are: decoding a pair number costs two divisions
                int bA, eA, bB, eB;
                shell_row_runs(g, h.cs, h.cx, h.cy, h.cz, R, dz, dy, false, bA, eA, bB, eB);
                run(bA, eA);
                run(bB, eB);
            }
        }
        bool whole;
        const float bound = shell_unseen_bound(g, h, R, whole);
        if (shell_closed(bound, whole, d2)) break;  // the third is strictly nearer than anything unseen
    }
    dist2[(size_t)q * 3] = d0; dist2[(size_t)q * 3 + 1] = d1; dist2[(size_t)q * 3 + 2] = d2;
    idx[(size_t)q * 3] = i0 - bs * m; idx[(size_t)q * 3 + 1] = i1 - bs * m; idx[(size_t)q * 3 + 2] = i2 - bs * m;
}

bool grid_search_pays(int b, int n, int m) { return b <= KG_MAX_BATCH && (long)n * m >= (1L << 21) && (long)b * n >= 4 * KG_SAMPLES; }

size_t grid_search_workspace_bytes(int b, int n, int m) { return knn_layout(b * n, b * m).total; }

// xyz (b,n,3) support, new_xyz (b,m,3) queries
int ball_query_grid(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                    void *workspace, hipStream_t stream)
{
    const GridView v = grid_view(knn_layout(b * n, b * m), workspace);
    hipLaunchKernelGGL(kg_uniform_offsets_kernel, dim3(1), dim3(64), 0, stream, b, n, m, v.off_s, v.off_q);
    // cell edge 1 % above the radius: a point within the radius is at most one cell away whatever fp32 does
    if (int st = kg_build(v, b * n, b * m, b, xyz, new_xyz, v.off_s, v.off_q, 1, 1, 1.f, radius * 1.01f + 1e-30f, stream))
        return st;
    hipLaunchKernelGGL(bq_grid_kernel, dim3(min(div_up((long)b * m, 4), 256 * 32)), dim3(256), 0, stream, b * m, n, m,
                       radius * radius, nsample, new_xyz, (const GridParams *)v.gp, (const int *)v.cell_start,
                       (const float4 *)v.sorted, idx);
    return launch_status("amc3d_ball_query");
}

// unknown (b,n,3) queries, known (b,m,3) support
int three_nn_grid(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, void *workspace,
                  hipStream_t stream)
{
    const GridView v = grid_view(knn_layout(b * m, b * n), workspace);
    hipLaunchKernelGGL(kg_uniform_offsets_kernel, dim3(1), dim3(64), 0, stream, b, m, n, v.off_s, v.off_q);
    // cell edge = p80 of the 2nd-neighbour distance among every 2nd known point (~ the 4th neighbour).  Scales of 0.7,
    // 1.0 and 1.4 x that were timed on the finest FeaturePropagation level (nn3_grid_thread_kernel's comment): 1.0 x
    // is the fastest; the sweep script is not kept.
    if (int st = kg_build(v, b * m, b * n, b, known, unknown, v.off_s, v.off_q, 2, 2, 1.0f, 0.f, stream)) return st;
    hipLaunchKernelGGL(nn3_grid_thread_kernel, dim3(div_up((long)b * n, 256)), dim3(256), 0, stream, b * n, n, m,
                       unknown, (const GridParams *)v.gp, (const int *)v.cell_start, (const float4 *)v.sorted, dist2, idx);
    return launch_status("amc3d_three_nn");
}

}  // namespace amc

using namespace amc;

AMC_API size_t amc3d_knnquery_workspace_bytes(int n, int m, int nsample, int nbatch)
{
    (void)nsample; (void)nbatch;
    return knn_layout(n > 0 ? n : 1, m > 0 ? m : 1).total;
}

// 1 when amc3d_knnquery builds (or, with reuse_grid, expects) the cell grid for this problem size, 0 when it
// answers with the all-pairs heap kernel and leaves the workspace untouched
AMC_API int amc3d_knnquery_uses_grid(int m, int nsample, int n, int nbatch)
{
    return (nsample <= KG_MAXK && (long)n * m >= (1L << 22) && n >= 4 * KG_SAMPLES && nbatch <= KG_MAX_BATCH) ? 1 : 0;
}

// 1 when amc3d_ball_query (support n, queries m) / amc3d_three_nn (support = known) search the cell grid, given a workspace
AMC_API int amc3d_grid_search_pays(int b, int n, int m) { return grid_search_pays(b, n, m) ? 1 : 0; }

// The search behind amc3d_knnquery and amc3d_knn_batch: argument checks, route (all-pairs heap or cell grid), launches.
static int knn_search(int m, int nsample, int n, int nbatch, const float *xyz, const float *new_xyz,
                      const int *offset, const int *new_offset, int *idx, float *dist2, void *workspace,
                      size_t workspace_bytes, int reuse_grid, void *stream_)
{
    if (m <= 0) return 0;
    if (nsample <= 0 || nsample > KNN_MAXK) return bad_arg("amc3d_knnquery: nsample must be in 1..100");
    if (nbatch <= 0 || n < 0 || !xyz || !new_xyz || !offset || !new_offset || !idx || !dist2)
        return bad_arg("amc3d_knnquery: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int exact_blocks = min(div_up(m, KNN_WAVES), 256 * 8);
    // small problems and k > 64: the heap replay alone (it is exact for every input)
    const bool grid = amc3d_knnquery_uses_grid(m, nsample, n, nbatch) != 0;
    if (!grid) {
        hipLaunchKernelGGL(knn_exact_kernel, dim3(exact_blocks), dim3(KNN_WAVES * 64), 0, stream, m, nsample, nbatch,
                           xyz, new_xyz, offset, new_offset, idx, dist2, (const int *)nullptr, (const int *)nullptr);
        return launch_status("amc3d_knnquery");
    }
    const KnnWorkspace w = knn_layout(n, m);
    if (!workspace || workspace_bytes < w.total) return bad_arg("amc3d_knnquery: workspace too small");
    const GridView v = grid_view(w, workspace);
    if (int st = grid_prepare(v, reuse_grid, n, m, nbatch, xyz, new_xyz, offset, new_offset, nsample, stream)) return st;
    const GridParams *gp = v.gp;
    const int *cell_start = v.cell_start;
    const float4 *sorted = v.sorted;
    const int self = (new_xyz == xyz && m == n && new_offset == offset) ? 1 : 0;
    if (nsample <= KGG_MAXK) {
        // Two queries per wavefront, 32 lanes each, for every k <= 32 whatever m: the rule is the input's k alone.
        // Query kernel alone on the whole chip, the loss's searches at 8 x 24000 points (tools/knn_bench.py, us,
        // wave per query -> two per wave): self k = 24 over m = 192000 / 48000 / 12000 / 3000: 416 -> 218, 103 -> 57,
        // 44 -> 29, 27 -> 19; votes over the 192000-point grid, k = 4 m = 48000: 64 -> 45, k = 16 m = 12000: 38 -> 30.
        // No shape class measured slower, so none keeps the wave-per-query kernel; k in 33..64 has no other.
        constexpr int per_wg = 4 * (64 / KGG_MAXK);
        hipLaunchKernelGGL(kg_query_group_kernel<KGG_MAXK>, dim3(min(div_up(m, per_wg), 256 * 32)), dim3(256), 0, stream, m,
                           nsample, nbatch, self, new_xyz, offset, new_offset, gp, cell_start, sorted, idx, dist2, v.fb_list,
                           v.fb_count);
    } else {
        hipLaunchKernelGGL(kg_query_kernel, dim3(min(div_up(m, 4), 256 * 32)), dim3(256), 0, stream, m, nsample, nbatch, self,
                           new_xyz, offset, new_offset, gp, cell_start, sorted, idx, dist2, v.fb_list, v.fb_count);
    }
    // queries with equal distances among their k+1 nearest: replay the reference's heap
    hipLaunchKernelGGL(knn_exact_list_kernel, dim3(256), dim3(1024), 0, stream, nsample, nbatch, xyz, new_xyz, offset,
                       new_offset, idx, dist2, (const int *)v.fb_list, (const int *)v.fb_count, gp, cell_start, sorted);
    return launch_status("amc3d_knnquery");
}

AMC_API int amc3d_knnquery(int m, int nsample, int n, int nbatch, const float *xyz, const float *new_xyz,
                           const int *offset, const int *new_offset, int *idx, float *dist2, void *workspace,
                           size_t workspace_bytes, int reuse_grid, void *stream_)
{
    return knn_search(m, nsample, n, nbatch, xyz, new_xyz, offset, new_offset, idx, dist2, workspace, workspace_bytes,
                      reuse_grid, stream_);
}

AMC_API int amc3d_knn_prefix(int m, int kr, int n, int nbatch, const float *xyz, const float *new_xyz, const int *offset,
                             const int *new_offset, int k0, int row_stride, const int *rows_idx, const float *rows_d2,
                             int *idx, float *dist2, void *workspace, size_t workspace_bytes, int reuse_grid, void *stream_)
{
    if (m <= 0) return 0;
    if (kr <= 0 || kr >= k0 || kr >= 32 || row_stride < k0 || nbatch <= 0 || nbatch > KG_MAX_BATCH || n <= 0 || !xyz || !new_xyz ||
        !offset || !new_offset || !rows_idx || !rows_d2 || !idx)
        return bad_arg("amc3d_knn_prefix: bad argument (0 < kr < k0 <= row_stride, kr <= 31, nbatch <= 64)");
    if (!reuse_grid && n < 4 * KG_SAMPLES) return bad_arg("amc3d_knn_prefix: too few support points to build a grid");
    hipStream_t stream = (hipStream_t)stream_;
    const KnnWorkspace w = knn_layout(n, m);
    if (!workspace || workspace_bytes < w.total) return bad_arg("amc3d_knn_prefix: workspace too small");
    const GridView v = grid_view(w, workspace);
    if (int st = grid_prepare(v, reuse_grid, n, m, nbatch, xyz, new_xyz, offset, new_offset, kr, stream)) return st;
    const GridParams *gp = v.gp;
    const int *cell_start = v.cell_start;
    const float4 *sorted = v.sorted;
    hipLaunchKernelGGL(kg_prefix_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, kr, nbatch, row_stride, new_xyz,
                       new_offset, gp, cell_start, sorted, rows_idx, rows_d2, idx, dist2, v.fb_list, v.fb_count);
    hipLaunchKernelGGL(knn_exact_list_kernel, dim3(256), dim3(1024), 0, stream, kr, nbatch, xyz, new_xyz, offset, new_offset,
                       idx, dist2, (const int *)v.fb_list, (const int *)v.fb_count, gp, cell_start, sorted);
    return launch_status("amc3d_knn_prefix");
}

// ---- batched (B, N, 3) k-NN around the same search -----------------------------------------------------
namespace amc {

constexpr int KB_QT = 64;  // queries per workgroup of the epilogue

struct KnnBatchWorkspace {  // the search's own layout first (so a kept grid stays where it was), then this entry's
    size_t grid_bytes, off_s, off_q, idx, dist2, total;
};

static KnnBatchWorkspace knn_batch_layout(int b, int n, int m, int ksearch)
{
    KnnBatchWorkspace w;
    w.grid_bytes = knn_layout(b * n, b * m).total;
    w.off_s = w.grid_bytes;
    w.off_q = align256(w.off_s + (size_t)b * 4);
    w.idx = align256(w.off_q + (size_t)b * 4);
    w.dist2 = align256(w.idx + (size_t)b * m * ksearch * 4);
    w.total = align256(w.dist2 + (size_t)b * m * ksearch * 4);
    return w;
}

// Epilogue of amc3d_knn_batch.  The search leaves (b*m, ksearch) rows of global support rows and squared distances; this
// keeps columns 0, d, 2d, ... of them, makes the indices cloud-local and takes the root.  A workgroup serves KB_QT
// consecutive queries of one cloud.  idx and the (b,m,k) distances are row-major in the query, so the lanes run along
// the flattened (query, column) pair and a wave stores 64 consecutive words.  The (b,k,m) layout is contiguous in the
// query instead: its roots go through an LDS tile (row stride odd: conflict-free both ways) and are stored with the lanes
// running along the queries, again 64 consecutive words per wave.
__global__ __launch_bounds__(256) void knn_batch_epilogue_kernel(int n, int m, int ksearch, int dilation, int kout,
                                                                 const int *__restrict__ raw_idx,
                                                                 const float *__restrict__ raw_d2, int *__restrict__ idx,
                                                                 float *__restrict__ dist, int dist_layout)
{
    extern __shared__ float kb_tile[];  // KB_QT x (kout | 1), only for the (b,k,m) layout
    const int bi = blockIdx.y;
    const int q0 = blockIdx.x * KB_QT;
    const int nq = min(KB_QT, m - q0);
    const int ld = kout | 1;
    const size_t row0 = (size_t)bi * m + q0;
    const int first = bi * n;
    for (int e = threadIdx.x; e < nq * kout; e += 256) {
        const int ql = e / kout, j = e - ql * kout;
        const size_t src = (row0 + ql) * ksearch + (size_t)j * dilation;
        idx[row0 * kout + e] = raw_idx[src] - first;
        if (dist) {
            const float v = sqrtf(raw_d2[src]);  // IEEE: hipcc rounds sqrtf correctly by default, __fsqrt_rn is the native approximation
            if (dist_layout == AMC_KNN_DIST_BMK) dist[row0 * kout + e] = v;
            else kb_tile[ql * ld + j] = v;
        }
    }
    if (!dist || dist_layout == AMC_KNN_DIST_BMK) return;  // uniform over the workgroup
    __syncthreads();
    for (int e = threadIdx.x; e < kout * KB_QT; e += 256) {
        const int j = e / KB_QT, ql = e % KB_QT;
        if (ql < nq) dist[((size_t)bi * kout + j) * m + q0 + ql] = kb_tile[ql * ld + j];
    }
}

}  // namespace amc

static bool knn_batch_sizes_ok(int b, int n, int m, int ksearch)
{
    const long lim = 0x7fffffffL;
    return b > 0 && n > 0 && m > 0 && ksearch > 0 && ksearch <= KNN_MAXK && (long)b * n <= lim && (long)b * m <= lim &&
           (long)b * m * ksearch <= lim && b <= 65535;
}

AMC_API size_t amc3d_knn_batch_workspace_bytes(int b, int n, int m, int ksearch)
{
    if (!knn_batch_sizes_ok(b, n, m, ksearch)) return 0;
    return knn_batch_layout(b, n, m, ksearch).total;
}

AMC_API int amc3d_knn_batch(int b, int n, int m, int ksearch, int dilation, const float *support, const float *query,
                            int *idx, float *dist, int dist_layout, void *workspace, size_t workspace_bytes,
                            int reuse_grid, void *stream_)
{
    if (b <= 0 || m <= 0) return 0;
    if (!knn_batch_sizes_ok(b, n, m, ksearch)) return bad_arg("amc3d_knn_batch: sizes out of range (ksearch in 1..100, int32 products)");
    if (ksearch > n) return bad_arg("amc3d_knn_batch: ksearch exceeds the number of support points");
    if (dilation <= 0 || ksearch % dilation != 0) return bad_arg("amc3d_knn_batch: dilation must divide ksearch");
    if (!support || !query || !idx) return bad_arg("amc3d_knn_batch: null pointer");
    if (dist && dist_layout != AMC_KNN_DIST_BMK && dist_layout != AMC_KNN_DIST_BKM)
        return bad_arg("amc3d_knn_batch: unknown dist_layout");
    const KnnBatchWorkspace w = knn_batch_layout(b, n, m, ksearch);
    if (!workspace || workspace_bytes < w.total) return bad_arg("amc3d_knn_batch: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)workspace;
    int *off_s = (int *)(base + w.off_s);
    // one tensor for both clouds: one offset array too, which is what the search takes for its self-search path
    int *off_q = (query == support && m == n) ? off_s : (int *)(base + w.off_q);
    int *raw_idx = (int *)(base + w.idx);
    float *raw_d2 = (float *)(base + w.dist2);
    hipLaunchKernelGGL(kg_uniform_offsets_kernel, dim3(div_up(b, 64)), dim3(64), 0, stream, b, n, m, off_s, off_q);
    if (int st = knn_search(b * m, ksearch, b * n, b, support, query, off_s, off_q, raw_idx, raw_d2, workspace, w.grid_bytes,
                            reuse_grid, stream_))
        return st;
    const int kout = ksearch / dilation;
    const bool tile = dist && dist_layout == AMC_KNN_DIST_BKM;
    hipLaunchKernelGGL(knn_batch_epilogue_kernel, dim3(div_up(m, KB_QT), b), dim3(256),
                       tile ? (size_t)KB_QT * (kout | 1) * sizeof(float) : 0, stream, n, m, ksearch, dilation, kout,
                       (const int *)raw_idx, (const float *)raw_d2, idx, dist, dist_layout);
    return launch_status("amc3d_knn_batch");
}
