// The offset-layout ("pointops") operators for gfx950: ball query, furthest sampling, grouping, interpolation,
// subtraction and aggregation over ragged batches -- rows (n_total, .) plus cumulative segment ends.
//
// Reference semantics: openpoints/cpp/pointops/src/{ballquery,sampling,grouping,interpolation,subtraction,aggregation}.
// Features are channel-last (rows of c floats), so one thread per (row, channel) with the channel fastest makes
// every wave instruction -- load, store or float atomic -- a contiguous run of 256 bytes (several rows per wave
// when c < 64): the shape at which global float atomics run at full rate.  Row-local sums (grad_input1 of the
// subtraction, grad_weight / grad_position of the aggregation) are plain sequential sums, no atomics.  The four
// scatters have a second, atomic-free form: one gather kernel over the reverse lists of amc3d_group_csr.
#include "common.h"

namespace amc {

// ------------------------------------------------------------------------------------------ ball query
constexpr int PBQ_TILE = 1024;  // support points per LDS tile (12 KiB as three SoA planes)
constexpr int PBQ_WAVES = 4;
constexpr int PBQ_QPW = 4;  // queries per wave

// first s in [0, nbatch) with q < ends[s], clamped to the last segment: at most 32 steps, every read inside ends[0..nbatch)
__device__ __forceinline__ int segment_of(int q, const int *__restrict__ ends, int nbatch)
{
    int lo = 0, hi = nbatch - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q < ends[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The scheme of ball_query_kernel (ball_query.hip) with a per-query support range [start, end) in place of a cloud
// base: a wave owns PBQ_QPW queries and tests 64 consecutive support points per step, __ballot + mbcnt put the hits
// in index order.  The block's tiles run over the union of its queries' ranges -- [start of the first query's
// segment, end of the last one's), block-uniform -- and each query counts only indices inside its own range.
__global__ __launch_bounds__(PBQ_WAVES * 64) void pointops_ballquery_kernel(
    int m, int n, int nbatch, float radius2, int nsample, const float *__restrict__ xyz,
    const float *__restrict__ new_xyz, const int *__restrict__ offset, const int *__restrict__ new_offset,
    int *__restrict__ idx)
{
    __shared__ float sx[PBQ_TILE], sy[PBQ_TILE], sz[PBQ_TILE];
    __shared__ int s_active;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qb = blockIdx.x * PBQ_WAVES * PBQ_QPW;  // < m by the grid size
    const int q0 = qb + wave * PBQ_QPW;

    // block-uniform tile range from the block's first and last query
    int lo, hi;
    {
        const int sa = segment_of(qb, new_offset, nbatch);
        const int sb = segment_of(min(qb + PBQ_WAVES * PBQ_QPW, m) - 1, new_offset, nbatch);
        lo = sa ? offset[sa - 1] : 0;
        hi = offset[sb];
        lo = max(0, min(lo, n));
        hi = max(lo, min(hi, n));
    }

    float qx[PBQ_QPW], qy[PBQ_QPW], qz[PBQ_QPW];
    int cnt[PBQ_QPW], first[PBQ_QPW], start[PBQ_QPW], end[PBQ_QPW];
#pragma unroll
    for (int i = 0; i < PBQ_QPW; ++i) {
        const int q = q0 + i;
        const bool ok = q < m;
        const float *c = new_xyz + (size_t)(ok ? q : 0) * 3;
        qx[i] = c[0]; qy[i] = c[1]; qz[i] = c[2];
        const int s = segment_of(ok ? q : 0, new_offset, nbatch);
        const int st = s ? offset[s - 1] : 0;
        start[i] = max(lo, min(st, hi));
        end[i] = ok ? max(start[i], min(offset[s], hi)) : start[i];  // out-of-range queries have an empty range
        cnt[i] = 0;
        first[i] = 0;
    }

    for (int t0 = lo; t0 < hi; t0 += PBQ_TILE) {  // trip count and every break are block-uniform
        const int tn = min(PBQ_TILE, hi - t0);
        __syncthreads();  // previous tile fully consumed
        if (threadIdx.x == 0) s_active = 0;
        for (int i = threadIdx.x; i < tn * 3; i += PBQ_WAVES * 64) {
            const float v = xyz[(size_t)t0 * 3 + i];
            const int p = i / 3, c = i - p * 3;
            (c == 0 ? sx : c == 1 ? sy : sz)[p] = v;
        }
        __syncthreads();

        bool wave_active = false;  // wave-uniform: a query that still wants hits and whose range reaches this tile
#pragma unroll
        for (int i = 0; i < PBQ_QPW; ++i) wave_active |= cnt[i] < nsample && t0 < end[i] && start[i] < t0 + tn;
        if (wave_active) {
            for (int k0 = 0; k0 < tn; k0 += 64) {
                const int kl = k0 + lane;
                const bool valid = kl < tn;
                const int g = t0 + kl;
                const float x = sx[valid ? kl : 0], y = sy[valid ? kl : 0], z = sz[valid ? kl : 0];
#pragma unroll
                for (int i = 0; i < PBQ_QPW; ++i) {
                    if (cnt[i] < nsample && t0 + k0 < end[i]) {  // wave-uniform
                        const float d2 = dist2_ref(qx[i], qy[i], qz[i], x, y, z);
                        const bool hit = valid && g >= start[i] && g < end[i] && d2 < radius2;
                        const unsigned long long mask = __ballot(hit);
                        if (mask) {
                            const int pos = cnt[i] + mbcnt(mask);
                            if (hit && pos < nsample) idx[(size_t)(q0 + i) * nsample + pos] = g;
                            if (cnt[i] == 0) first[i] = t0 + k0 + (int)__builtin_ctzll(mask);
                            cnt[i] += (int)__popcll(mask);
                        }
                    }
                }
            }
        }
        bool more = false;  // a query of this wave still needs a later tile
#pragma unroll
        for (int i = 0; i < PBQ_QPW; ++i) more |= cnt[i] < nsample && end[i] > t0 + tn;
        if (more && lane == 0) s_active = 1;
        __syncthreads();
        if (!s_active) break;  // block-uniform
    }

    // pad the tail of each row with the first hit (zeros -- global row 0 -- when there was none)
#pragma unroll
    for (int i = 0; i < PBQ_QPW; ++i) {
        const int q = q0 + i;
        if (q < m) {
            const int have = min(cnt[i], nsample);
            for (int l = have + lane; l < nsample; l += 64) idx[(size_t)q * nsample + l] = first[i];
        }
    }
}

// ------------------------------------------------------------------------------------- furthest sampling
constexpr int PFPS_THREADS = 1024;
// points per thread whose coordinates and running minima stay in registers: the launch picks the variant from n_max
// (4 floats per point; 1024 threads leave 128 registers per thread, and 16 points with a candidate in flight spill), a longer segment keeps its
// minima in tmp
constexpr int PFPS_PPT_MAX = 12;

struct PCand {
    float v;
    int key;  // bit-reversed (k - start) mod 1024: smaller wins on equal v
    int k;    // lower wins on equal v and key
};
__device__ __forceinline__ PCand pbetter(PCand a, PCand b)
{
    const bool take_b = (b.v > a.v) || (b.v == a.v && (b.key < a.key || (b.key == a.key && b.k < a.k)));
    // field by field: `take_b ? b : a` on the struct is compiled as two stores to scratch and an indexed load, a round
    // trip through memory in each of the ten reduction steps of a pick
    PCand r;
    r.v = take_b ? b.v : a.v;
    r.key = take_b ? b.key : a.key;
    r.k = take_b ? b.k : a.k;
    return r;
}
__device__ __forceinline__ PCand pshfl_xor(PCand c, int m)
{
    PCand r;
    r.v = __shfl_xor(c.v, m, 64);
    r.key = __shfl_xor(c.key, m, 64);
    r.k = __shfl_xor(c.k, m, 64);
    return r;
}

// One workgroup of 1024 threads per segment; thread t owns k = start + t, start + t + 1024, ... as the reference's
// 1024-thread block does, keeps the first strict maximum of its points, and the workgroup keeps the candidate with
// the smallest bit-reversed t among equal maxima: the reference's tree.  For a segment shorter than 1024 the
// reference runs a smaller block; the order over 10 bits refines the order over fewer, so the picks are the same.
// One LDS-only barrier per pick (two LDS buffers); the trip count is the segment's sample count, workgroup-uniform.
template <int PFPS_PPT>
__global__ __launch_bounds__(PFPS_THREADS) void pointops_fps_kernel(
    int n, const float *__restrict__ xyz, const int *__restrict__ offset, const int *__restrict__ new_offset,
    float *__restrict__ tmp, int *__restrict__ idx)
{
    __shared__ float s_v[2][16];
    __shared__ int s_key[2][16], s_k[2][16];
    __shared__ float s_x[2][16], s_y[2][16], s_z[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = blockIdx.x;
    int start = bid ? offset[bid - 1] : 0, end = offset[bid];
    const int ms = bid ? new_offset[bid - 1] : 0, me = new_offset[bid];
    start = max(0, min(start, n));
    end = min(end, n);
    if (end <= start || me <= ms || ms < 0) return;  // empty segment or no sample asked for: before any barrier
    const int nseg = end - start;
    const bool in_regs = nseg <= PFPS_THREADS * PFPS_PPT;  // workgroup-uniform
    const int key = (int)(__brev((unsigned)tid) >> 22);

    float px[PFPS_PPT], py[PFPS_PPT], pz[PFPS_PPT], pd[PFPS_PPT];
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < PFPS_PPT; ++j) {
            const int k = start + tid + j * PFPS_THREADS;
            const bool ok = k < end;
            px[j] = ok ? xyz[(size_t)k * 3] : 0.f;
            py[j] = ok ? xyz[(size_t)k * 3 + 1] : 0.f;
            pz[j] = ok ? xyz[(size_t)k * 3 + 2] : 0.f;
            pd[j] = ok ? tmp[k] : 0.f;
        }
    }

    int old = start;
    if (tid == 0) idx[ms] = start;
    float x1 = xyz[(size_t)start * 3], y1 = xyz[(size_t)start * 3 + 1], z1 = xyz[(size_t)start * 3 + 2];
    for (int it = 1; it < me - ms; ++it) {
        float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;  // the thread's candidate and its coordinates
        int besti = start;
        if (in_regs) {
#pragma unroll
            for (int j = 0; j < PFPS_PPT; ++j) {
                const int k = start + tid + j * PFPS_THREADS;
                if (k < end) {
                    const float d2 = fminf(dist2_ref(px[j], py[j], pz[j], x1, y1, z1), pd[j]);
                    pd[j] = d2;
                    const bool up = d2 > best;
                    besti = up ? k : besti;
                    bx = up ? px[j] : bx; by = up ? py[j] : by; bz = up ? pz[j] : bz;
                    best = up ? d2 : best;
                }
            }
        } else {
            for (int k = start + tid; k < end; k += PFPS_THREADS) {
                const float xk = xyz[(size_t)k * 3], yk = xyz[(size_t)k * 3 + 1], zk = xyz[(size_t)k * 3 + 2];
                const float d2 = fminf(dist2_ref(xk, yk, zk, x1, y1, z1), tmp[k]);
                tmp[k] = d2;
                const bool up = d2 > best;
                besti = up ? k : besti;
                bx = up ? xk : bx; by = up ? yk : by; bz = up ? zk : bz;
                best = up ? d2 : best;
            }
        }
        PCand c{best, key, besti};
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c = pbetter(c, pshfl_xor(c, s));
        const int buf = it & 1;  // the other buffer's readers are one barrier behind
        // the wave's record is written by the lane that owns its winner (residue of k), with the winner's coordinates, so
        // the next pick starts without a dependent global load; a wave without points writes a record that never wins
        if (lane == ((c.k - start) & 63)) {
            s_v[buf][wave] = c.v; s_key[buf][wave] = c.key; s_k[buf][wave] = c.k;
            s_x[buf][wave] = bx; s_y[buf][wave] = by; s_z[buf][wave] = bz;
        }
        // LDS-only barrier: threads exchange nothing through global memory inside the loop (each reads and writes its
        // own tmp entries only), and __syncthreads() would also wait for the previous pick's store to idx
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        PCand w{-3.f, 0x7fffffff, 0x7fffffff};
        if (lane < 16) { w.v = s_v[buf][lane]; w.key = s_key[buf][lane]; w.k = s_k[buf][lane]; }
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1) w = pbetter(w, pshfl_xor(w, s));
        old = __builtin_amdgcn_readfirstlane(w.k);
        const int ww = ((old - start) & (PFPS_THREADS - 1)) >> 6;  // the wave that owns the pick
        x1 = s_x[buf][ww]; y1 = s_y[buf][ww]; z1 = s_z[buf][ww];
        if (tid == 0) idx[ms + it] = old;
    }
    if (in_regs && me - ms > 1) {
#pragma unroll
        for (int j = 0; j < PFPS_PPT; ++j) {
            const int k = start + tid + j * PFPS_THREADS;
            if (k < end) tmp[k] = pd[j];
        }
    }
}

// ------------------------------------------------------------------------- gathers and their gradients
// every kernel below: one thread per element, channel fastest; `total` < 2^31 is checked by the entry point

__global__ void pointops_grouping_forward_kernel(int total, int c, const float *__restrict__ input,
                                                 const int *__restrict__ idx, float *__restrict__ output)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int p = e / c, ch = e - p * c;
    output[e] = input[(size_t)idx[p] * c + ch];
}

__global__ void pointops_grouping_backward_kernel(int total, int c, const float *__restrict__ grad_output,
                                                  const int *__restrict__ idx, float *__restrict__ grad_input)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int p = e / c, ch = e - p * c;
    atomicAdd(grad_input + (size_t)idx[p] * c + ch, grad_output[e]);
}

__global__ void pointops_interpolation_forward_kernel(int total, int c, int k, int accumulate,
                                                      const float *__restrict__ input, const int *__restrict__ idx,
                                                      const float *__restrict__ weight, float *__restrict__ output)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = e / c, ch = e - i * c;
    float acc = accumulate ? output[e] : 0.f;
    for (int t = 0; t < k; ++t) {
        const size_t ii = (size_t)i * k + t;
        acc = __fadd_rn(acc, __fmul_rn(input[(size_t)idx[ii] * c + ch], weight[ii]));
    }
    output[e] = acc;
}

__global__ void pointops_interpolation_backward_kernel(int total, int c, int k, const float *__restrict__ grad_output,
                                                       const int *__restrict__ idx, const float *__restrict__ weight,
                                                       float *__restrict__ grad_input)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = e / c, ch = e - i * c;
    const float g = grad_output[e];
    for (int t = 0; t < k; ++t) {
        const size_t ii = (size_t)i * k + t;
        atomicAdd(grad_input + (size_t)idx[ii] * c + ch, __fmul_rn(g, weight[ii]));
    }
}

__global__ void pointops_subtraction_forward_kernel(int total, int nsample, int c, const float *__restrict__ input1,
                                                    const float *__restrict__ input2, const int *__restrict__ idx,
                                                    float *__restrict__ output)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int p = e / c, ch = e - p * c, i = p / nsample;
    output[e] = __fsub_rn(input1[(size_t)i * c + ch], input2[(size_t)idx[p] * c + ch]);
}

// thread (i, ch): grad_input1 as the sequential sum over j; with SCATTER also the atomics into grad_input2
template <bool SCATTER>
__global__ void pointops_subtraction_backward_kernel(int total, int nsample, int c, const int *__restrict__ idx,
                                                     const float *__restrict__ grad_output,
                                                     float *__restrict__ grad_input1, float *__restrict__ grad_input2)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = e / c, ch = e - i * c;
    float acc = 0.f;
    for (int j = 0; j < nsample; ++j) {
        const size_t p = (size_t)i * nsample + j;
        const float g = grad_output[p * c + ch];
        acc = __fadd_rn(acc, g);
        if constexpr (SCATTER) atomicAdd(grad_input2 + (size_t)idx[p] * c + ch, -g);
    }
    grad_input1[e] = acc;
}

__global__ void pointops_aggregation_forward_kernel(int total, int nsample, int c, int w_c, int accumulate,
                                                    const float *__restrict__ input, const float *__restrict__ position,
                                                    const float *__restrict__ weight, const int *__restrict__ idx,
                                                    float *__restrict__ output)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = e / c, ch = e - i * c, wc = ch % w_c;
    float acc = accumulate ? output[e] : 0.f;
    for (int j = 0; j < nsample; ++j) {
        const size_t p = (size_t)i * nsample + j;
        const float s = __fadd_rn(input[(size_t)idx[p] * c + ch], position[p * c + ch]);
        acc = __fadd_rn(acc, __fmul_rn(s, weight[p * w_c + wc]));
    }
    output[e] = acc;
}

// thread (i, ch): grad_position stored; with SCATTER also the atomics into grad_input
template <bool SCATTER>
__global__ void pointops_aggregation_backward_kernel(int total, int nsample, int c, int w_c,
                                                     const float *__restrict__ weight, const int *__restrict__ idx,
                                                     const float *__restrict__ grad_output,
                                                     float *__restrict__ grad_input, float *__restrict__ grad_position)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = e / c, ch = e - i * c, wc = ch % w_c;
    const float g = grad_output[e];
    for (int j = 0; j < nsample; ++j) {
        const size_t p = (size_t)i * nsample + j;
        const float t = __fmul_rn(g, weight[p * w_c + wc]);
        grad_position[p * c + ch] = t;
        if constexpr (SCATTER) atomicAdd(grad_input + (size_t)idx[p] * c + ch, t);
    }
}

// thread (p = i*nsample + j, wc): grad_weight as the sequential sum over the channels ch = wc, wc + w_c, ...
__global__ void pointops_aggregation_grad_weight_kernel(int total, int nsample, int c, int w_c,
                                                        const float *__restrict__ input,
                                                        const float *__restrict__ position,
                                                        const int *__restrict__ idx,
                                                        const float *__restrict__ grad_output,
                                                        float *__restrict__ grad_weight)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int p = e / w_c, wc = e - p * w_c, i = p / nsample;
    const float *in = input + (size_t)idx[p] * c, *pos = position + (size_t)p * c, *go = grad_output + (size_t)i * c;
    float acc = 0.f;
    for (int ch = wc; ch < c; ch += w_c) acc = __fadd_rn(acc, __fmul_rn(go[ch], __fadd_rn(in[ch], pos[ch])));
    grad_weight[e] = acc;
}

// The four scatters as gathers over reverse lists: thread (target, ch) adds the terms of the target's incoming
// positions in list order.  KIND 0: g[p,ch]   1: g[p/per,ch] * w[p]   2: -g[p,ch]   3: g[p/per,ch] * w[p, ch % w_c]
template <int KIND>
__global__ void pointops_scatter_csr_kernel(int total, int c, int per, int w_c, const float *__restrict__ g,
                                            const float *__restrict__ w, const int *__restrict__ rev_start,
                                            const int *__restrict__ rev_edge, float *__restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int t = e / c, ch = e - t * c;
    const int wc = KIND == 3 ? ch % w_c : 0;
    float acc = 0.f;
    const int e1 = rev_start[t + 1];
    for (int l = rev_start[t]; l < e1; ++l) {
        const int p = rev_edge[l];
        float term;
        if constexpr (KIND == 0) term = g[(size_t)p * c + ch];
        else if constexpr (KIND == 1) term = __fmul_rn(g[(size_t)(p / per) * c + ch], w[p]);
        else if constexpr (KIND == 2) term = -g[(size_t)p * c + ch];
        else term = __fmul_rn(g[(size_t)(p / per) * c + ch], w[(size_t)p * w_c + wc]);
        acc = __fadd_rn(acc, term);
    }
    out[e] = acc;
}

// a * b * c as an element count the int32 thread ids can hold; 0 when a factor is not positive
static bool fits31(long a, long b, long c, int *total)
{
    if (a <= 0 || b <= 0 || c <= 0) { *total = 0; return true; }
    const __int128 t = (__int128)a * b * c;
    if (t > 0x7fffffffL) return false;
    *total = (int)t;
    return true;
}

constexpr int PO_THREADS = 256;
#define PO_LAUNCH(kernel, total, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3(div_up(total, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)(stream), total, __VA_ARGS__)

}  // namespace amc

using namespace amc;

AMC_API int amc3d_pointops_ballquery(int m, float radius, int nsample, int n, int nbatch, const float *xyz,
                                     const float *new_xyz, const int *offset, const int *new_offset, int *idx,
                                     void *stream)
{
    if (m <= 0) return 0;
    int total;
    if (n < 0 || nbatch <= 0 || nsample <= 0 || !xyz || !new_xyz || !offset || !new_offset || !idx)
        return bad_arg("amc3d_pointops_ballquery: bad argument");
    if (!fits31(m, nsample, 1, &total) || !fits31(n, 3, 1, &total) || !fits31(m, 3, 1, &total))
        return bad_arg("amc3d_pointops_ballquery: m * nsample or 3 * n does not fit in 31 bits");
    const float radius2 = radius * radius;  // ballquery_cuda_kernel.cu:50
    hipLaunchKernelGGL(pointops_ballquery_kernel, dim3(div_up(m, PBQ_WAVES * PBQ_QPW)), dim3(PBQ_WAVES * 64), 0,
                       (hipStream_t)stream, m, n, nbatch, radius2, nsample, xyz, new_xyz, offset, new_offset, idx);
    return launch_status("amc3d_pointops_ballquery");
}

AMC_API int amc3d_pointops_furthestsampling(int nbatch, int n_max, int n, const float *xyz, const int *offset,
                                            const int *new_offset, float *tmp, int *idx, void *stream)
{
    if (nbatch <= 0 || n <= 0) return 0;
    int total;
    if (n_max < 0 || !xyz || !offset || !new_offset || !tmp || !idx)
        return bad_arg("amc3d_pointops_furthestsampling: bad argument");
    if (!fits31(n, 3, 1, &total)) return bad_arg("amc3d_pointops_furthestsampling: 3 * n does not fit in 31 bits");
    if (n_max <= 4 * PFPS_THREADS)
        hipLaunchKernelGGL(pointops_fps_kernel<4>, dim3(nbatch), dim3(PFPS_THREADS), 0, (hipStream_t)stream, n, xyz, offset,
                           new_offset, tmp, idx);
    else if (n_max <= 8 * PFPS_THREADS)
        hipLaunchKernelGGL(pointops_fps_kernel<8>, dim3(nbatch), dim3(PFPS_THREADS), 0, (hipStream_t)stream, n, xyz, offset,
                           new_offset, tmp, idx);
    else
        hipLaunchKernelGGL(pointops_fps_kernel<PFPS_PPT_MAX>, dim3(nbatch), dim3(PFPS_THREADS), 0, (hipStream_t)stream, n, xyz,
                           offset, new_offset, tmp, idx);
    return launch_status("amc3d_pointops_furthestsampling");
}

AMC_API int amc3d_pointops_grouping_forward(int m, int nsample, int c, int n, const float *input, const int *idx,
                                            float *output, void *stream)
{
    int total, rows;
    if (!fits31(m, nsample, c, &total) || !fits31(n, c, 1, &rows))
        return bad_arg("amc3d_pointops_grouping_forward: m * nsample * c or n * c does not fit in 31 bits");
    if (!total) return 0;
    if (!input || !idx || !output) return bad_arg("amc3d_pointops_grouping_forward: null pointer");
    PO_LAUNCH(pointops_grouping_forward_kernel, total, stream, c, input, idx, output);
    return launch_status("amc3d_pointops_grouping_forward");
}

AMC_API int amc3d_pointops_grouping_backward(int m, int nsample, int c, int n, const float *grad_output,
                                             const int *idx, float *grad_input, void *stream)
{
    int total, rows;
    if (!fits31(m, nsample, c, &total) || !fits31(n, c, 1, &rows))
        return bad_arg("amc3d_pointops_grouping_backward: m * nsample * c or n * c does not fit in 31 bits");
    if (!total) return 0;
    if (!grad_output || !idx || !grad_input) return bad_arg("amc3d_pointops_grouping_backward: null pointer");
    PO_LAUNCH(pointops_grouping_backward_kernel, total, stream, c, grad_output, idx, grad_input);
    return launch_status("amc3d_pointops_grouping_backward");
}

AMC_API int amc3d_pointops_interpolation_forward(int n, int c, int k, int m, int accumulate, const float *input,
                                                 const int *idx, const float *weight, float *output, void *stream)
{
    int total, rows, terms;
    if (k < 0 || !fits31(n, c, 1, &total) || !fits31(m, c, 1, &rows) || !fits31(n, k, 1, &terms))
        return bad_arg("amc3d_pointops_interpolation_forward: n * c, m * c or n * k does not fit in 31 bits");
    if (!total) return 0;
    if (!input || !idx || !weight || !output) return bad_arg("amc3d_pointops_interpolation_forward: null pointer");
    PO_LAUNCH(pointops_interpolation_forward_kernel, total, stream, c, k, accumulate, input, idx, weight, output);
    return launch_status("amc3d_pointops_interpolation_forward");
}

AMC_API int amc3d_pointops_interpolation_backward(int n, int c, int k, int m, const float *grad_output, const int *idx,
                                                  const float *weight, float *grad_input, void *stream)
{
    int total, rows, terms;
    if (k < 0 || !fits31(n, c, 1, &total) || !fits31(m, c, 1, &rows) || !fits31(n, k, 1, &terms))
        return bad_arg("amc3d_pointops_interpolation_backward: n * c, m * c or n * k does not fit in 31 bits");
    if (!total) return 0;
    if (!grad_output || !idx || !weight || !grad_input)
        return bad_arg("amc3d_pointops_interpolation_backward: null pointer");
    PO_LAUNCH(pointops_interpolation_backward_kernel, total, stream, c, k, grad_output, idx, weight, grad_input);
    return launch_status("amc3d_pointops_interpolation_backward");
}

AMC_API int amc3d_pointops_subtraction_forward(int n, int nsample, int c, const float *input1, const float *input2,
                                               const int *idx, float *output, void *stream)
{
    int total;
    if (!fits31(n, nsample, c, &total))
        return bad_arg("amc3d_pointops_subtraction_forward: n * nsample * c does not fit in 31 bits");
    if (!total) return 0;
    if (!input1 || !input2 || !idx || !output) return bad_arg("amc3d_pointops_subtraction_forward: null pointer");
    PO_LAUNCH(pointops_subtraction_forward_kernel, total, stream, nsample, c, input1, input2, idx, output);
    return launch_status("amc3d_pointops_subtraction_forward");
}

AMC_API int amc3d_pointops_subtraction_backward(int n, int nsample, int c, const int *idx, const float *grad_output,
                                                float *grad_input1, float *grad_input2, void *stream)
{
    int total, rows;
    if (nsample < 0 || !fits31(n, nsample, c, &total) || !fits31(n, c, 1, &rows))
        return bad_arg("amc3d_pointops_subtraction_backward: n * nsample * c does not fit in 31 bits");
    if (!rows) return 0;
    if (!idx || !grad_output || !grad_input1) return bad_arg("amc3d_pointops_subtraction_backward: null pointer");
    if (grad_input2)
        PO_LAUNCH(pointops_subtraction_backward_kernel<true>, rows, stream, nsample, c, idx, grad_output, grad_input1,
                  grad_input2);
    else  // deterministic mode: grad_input2 comes from amc3d_pointops_scatter_csr
        PO_LAUNCH(pointops_subtraction_backward_kernel<false>, rows, stream, nsample, c, idx, grad_output, grad_input1,
                  grad_input2);
    return launch_status("amc3d_pointops_subtraction_backward");
}

AMC_API int amc3d_pointops_aggregation_forward(int n, int nsample, int c, int w_c, int accumulate, const float *input,
                                               const float *position, const float *weight, const int *idx,
                                               float *output, void *stream)
{
    int total, terms, wts;
    if (nsample < 0 || w_c <= 0 || !fits31(n, c, 1, &total) || !fits31(n, nsample, c, &terms) ||
        !fits31(n, nsample, w_c, &wts))
        return bad_arg("amc3d_pointops_aggregation_forward: w_c <= 0, or n * nsample * max(c, w_c) does not fit in 31 bits");
    if (!total) return 0;
    if (!input || !position || !weight || !idx || !output)
        return bad_arg("amc3d_pointops_aggregation_forward: null pointer");
    PO_LAUNCH(pointops_aggregation_forward_kernel, total, stream, nsample, c, w_c, accumulate, input, position, weight,
              idx, output);
    return launch_status("amc3d_pointops_aggregation_forward");
}

AMC_API int amc3d_pointops_aggregation_backward(int n, int nsample, int c, int w_c, const float *input,
                                                const float *position, const float *weight, const int *idx,
                                                const float *grad_output, float *grad_input, float *grad_position,
                                                float *grad_weight, void *stream)
{
    int total, terms, wts;
    if (w_c <= 0 || !fits31(n, c, 1, &total) || !fits31(n, nsample, c, &terms) || !fits31(n, nsample, w_c, &wts))
        return bad_arg("amc3d_pointops_aggregation_backward: w_c <= 0, or n * nsample * max(c, w_c) does not fit in 31 bits");
    if (!terms) return 0;
    if (!input || !position || !weight || !idx || !grad_output || !grad_position || !grad_weight)
        return bad_arg("amc3d_pointops_aggregation_backward: null pointer");
    if (grad_input)
        PO_LAUNCH(pointops_aggregation_backward_kernel<true>, total, stream, nsample, c, w_c, weight, idx, grad_output,
                  grad_input, grad_position);
    else  // deterministic mode: grad_input comes from amc3d_pointops_scatter_csr
        PO_LAUNCH(pointops_aggregation_backward_kernel<false>, total, stream, nsample, c, w_c, weight, idx, grad_output,
                  grad_input, grad_position);
    int st = launch_status("amc3d_pointops_aggregation_backward");
    if (st) return st;
    PO_LAUNCH(pointops_aggregation_grad_weight_kernel, wts, stream, nsample, c, w_c, input, position, idx, grad_output,
              grad_weight);
    return launch_status("amc3d_pointops_aggregation_backward");
}

AMC_API int amc3d_pointops_scatter_csr(int kind, int n_targets, int c, int per, int w_c, const float *g, const float *w,
                                       const int *rev_start, const int *rev_edge, float *out, void *stream)
{
    int total;
    if (kind < 0 || kind > 3 || !fits31(n_targets, c, 1, &total))
        return bad_arg("amc3d_pointops_scatter_csr: kind outside 0..3, or n_targets * c does not fit in 31 bits");
    if (!total) return 0;
    if (!g || !rev_start || !rev_edge || !out || ((kind & 1) && (!w || per <= 0)) || (kind == 3 && w_c <= 0))
        return bad_arg("amc3d_pointops_scatter_csr: bad argument");
    switch (kind) {
    case 0: PO_LAUNCH(pointops_scatter_csr_kernel<0>, total, stream, c, per, w_c, g, w, rev_start, rev_edge, out); break;
    case 1: PO_LAUNCH(pointops_scatter_csr_kernel<1>, total, stream, c, per, w_c, g, w, rev_start, rev_edge, out); break;
    case 2: PO_LAUNCH(pointops_scatter_csr_kernel<2>, total, stream, c, per, w_c, g, w, rev_start, rev_edge, out); break;
    default: PO_LAUNCH(pointops_scatter_csr_kernel<3>, total, stream, c, per, w_c, g, w, rev_start, rev_edge, out); break;
    }
    return launch_status("amc3d_pointops_scatter_csr");
}
