// Neighbourhood aggregation with ONE grouped convolution -- every LocalAggregation of the InvResMLP blocks and every
// single-layer SetAbstraction of PointNeXt-B/L/XL -- as "convolve first, gather after" (gfx950).
//
// Reference (pointnext_AA.py:57-63, 139-170; group.py:244-255, 323-325): ball query -> grouping_operation gathers the
// neighbours' features into (B,C,M,32) -> cat with the relative positions dp (B,3,M,32) -> Conv2d 1x1 (C+3 -> C') ->
// BatchNorm2d (batch statistics) -> ReLU -> max over the 32 neighbours.  Every one of those tensors is 32x the size
// of the layer's input and output; the conv runs on M*32 positions.
//
// The conv is linear and the gather only selects columns, so  W . [dp ; f[idx]] = (W_f . f)[idx] + W_dp . dp :
//   G (B,C',N) = W_f . f                       one pointwise conv on the N source points (32x fewer positions)
//   y[b,c,m,k] = G[b,c,idx[b,m,k]] + W_dp[c] . dp[b,:,m,k]
// and the BatchNorm statistics of y over all B*M*32 positions follow from N-sized sums and three geometry moments
//   cnt[n] = #{(m,k): idx[m,k] = n},   D[n] = sum of dp over those positions,   S1 = sum_p dp_p,  S2 = sum_p dp_p dp_p^T :
//   sum_p y_p   = sum_n cnt[n] G[n] + W_dp . S1
//   sum_p y_p^2 = sum_n cnt[n] G[n]^2 + 2 sum_n G[n] (W_dp . D[n]) + W_dp^T S2 W_dp
// (accumulated in fp64).  The only pass over M*32 positions is the max-pool itself: gather 32 rows of G per centroid,
// add the 3-term dp product, normalise, keep the first maximum (torch.max's rule).  Nothing of size (B,C,M,32) exists.
//
// Backward.  The gradient of the pooled output reaches ONE neighbour per (b,c,m); BatchNorm's backward then makes
// it dense again, dz_p = g*is*(dq_p - mean(dq) - xhat_p*mean(dq*xhat)), but what the layer needs is only
//   dG[n] = sum_{p -> n} dz_p = g*is*( Q[n] - cnt[n]*ma - mb*is*( cnt[n]*(G[n] - mu) + W_dp . D[n] ) ),
// with Q[n] the scattered sparse gradients (M*C' atomics instead of M*32*C'), and dW_dp, dgamma, dbeta from the same
// M-sized and N-sized sums.  df = W_f^T dG and dW_f = dG f^T are the pointwise conv's backward on N points.
// The geometry moments depend on coordinates only and are part of the geometry plan (computed ahead, shared by all
// blocks of a stage).

#include "bn_math.h"

namespace amc {

constexpr double LAGG_FX_D = 68719476736.0;   // 2^36: fixed point of the per-point dp sums (|dp| <= radius or 1)
constexpr double LAGG_FX_M = 1073741824.0;    // 2^30: fixed point of the global moments (block partials in double)
constexpr int LAGG_MT = 32;                   // centroids per workgroup tile (8 per wave)
constexpr int LAGG_CT = 128;                  // channels per workgroup (pool / scatter kernels)
constexpr int LAGG_TILES = 4;                 // tiles per workgroup of the backward scatter kernel on large grids

struct LaggMoments {  // views into the opaque moments buffer of amc3d_group_moments
    const long long *mom;   // [9 (+7 pad)] S1[3], S2[(0,0),(0,1),(0,2),(1,1),(1,2),(2,2)]
    const int *cnt;         // (b, n)
    const long long *dfx;   // (b, n, 3)
};

static size_t lagg_moments_bytes(int b, int n) { return 16 * 8 + (size_t)b * n * 4 + (((size_t)b * n) & 1) * 4 + (size_t)b * n * 24; }

static LaggMoments lagg_views(const void *buf, int b, int n)
{
    LaggMoments v;
    const char *p = (const char *)buf;
    v.mom = (const long long *)p;
    v.cnt = (const int *)(p + 16 * 8);
    v.dfx = (const long long *)(p + 16 * 8 + (size_t)b * n * 4 + (((size_t)b * n) & 1) * 4);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------
// geometry moments: integer / fixed-point atomics, so the result does not depend on the order of arrival
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lagg_geom_kernel(int n, long P, const int *__restrict__ idx, const float *__restrict__ dp,
                                                        int *__restrict__ cnt, unsigned long long *__restrict__ dfx,
                                                        unsigned long long *__restrict__ mom)
{
    __shared__ double red[4][9];
    const int b = blockIdx.y;
    const int *ib = idx + (size_t)b * P;
    const float *d0 = dp + (size_t)b * 3 * P, *d1 = d0 + P, *d2 = d1 + P;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const int id = ib[p];
        const float x = d0[p], y = d1[p], z = d2[p];
        if (id >= 0 && id < n) {
            atomicAdd(cnt + (size_t)b * n + id, 1);
            unsigned long long *t = dfx + ((size_t)b * n + id) * 3;
            atomicAdd(t + 0, (unsigned long long)__double2ll_rn((double)x * LAGG_FX_D));
            atomicAdd(t + 1, (unsigned long long)__double2ll_rn((double)y * LAGG_FX_D));
            atomicAdd(t + 2, (unsigned long long)__double2ll_rn((double)z * LAGG_FX_D));
        }
        const double dx = x, dy = y, dz = z;
        s[0] += dx; s[1] += dy; s[2] += dz;
        s[3] += dx * dx; s[4] += dx * dy; s[5] += dx * dz; s[6] += dy * dy; s[7] += dy * dz; s[8] += dz * dz;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        double v = s[j];
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const double v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        atomicAdd(mom + threadIdx.x, (unsigned long long)__double2ll_rn(v * LAGG_FX_M));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// forward statistics: per channel  sum_n cnt G,  sum_n cnt G^2,  sum_n G D_j  (j = 0..2)  from the rows of G (b*n, C)
// grid (point ranges, channel chunks of 4 * LPR <= 64).  The b*n points are one axis.  LPR lanes share a row, 16 bytes (four
// channels) each, so a wave instruction fetches 64 / LPR rows -- no idle lanes at 8, 16 or 32 channels -- and up to four such
// instructions are in flight before the first is used.  A wave takes 64 points at a time: lane l loads and converts cnt / D of
// point l once and leaves them in LDS for the row phase.  The partial sums go out as partial[channel][workgroup][5]: a fixed
// partition of the points and a fixed order inside it, so the sums have the same bits on every run.
// ---------------------------------------------------------------------------------------------------------------
constexpr int LAGG_SP = 256;  // points per workgroup pass (64 per wave)

template <int LPR>
__global__ __launch_bounds__(256) void lagg_stats_rows_kernel(int C, long G, const float *__restrict__ g_pm, LaggMoments gm,
                                                              double *__restrict__ partial, int pts_per_wg)
{
    constexpr int CT = 4 * LPR, R = 64 / LPR, U = LPR < 4 ? LPR : 4;
    __shared__ double pt[4][64][4];  // cnt, D_x, D_y, D_z of the wave's 64 points
    __shared__ double red[4][CT][5];
    const int c0 = blockIdx.y * CT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % LPR, r = lane / LPR;
    double a[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int v = 0; v < 5; ++v) a[j][v] = 0.0;
    const long gbeg = (long)blockIdx.x * pts_per_wg, gend = min(G, gbeg + pts_per_wg);
    for (long g0 = gbeg; g0 < gend; g0 += LAGG_SP) {  // (the trip count is the same for the four waves)
        const long gw = g0 + wave * 64;
        __syncthreads();
        {
            double cn = 0.0, dx = 0.0, dy = 0.0, dz = 0.0;
            if (gw + lane < gend) {
                const long long *df = gm.dfx + (size_t)(gw + lane) * 3;
                const long long fx = df[0], fy = df[1], fz = df[2];
                cn = (double)gm.cnt[gw + lane];
                dx = (double)fx * (1.0 / LAGG_FX_D); dy = (double)fy * (1.0 / LAGG_FX_D); dz = (double)fz * (1.0 / LAGG_FX_D);
            }
            pt[wave][lane][0] = cn; pt[wave][lane][1] = dx; pt[wave][lane][2] = dy; pt[wave][lane][3] = dz;
        }
        __syncthreads();
#pragma unroll 1  // (unrolled, the 16-step form held every step's point values at once: 314 registers)
        for (int i0 = 0; i0 < LPR; i0 += U) {
            float4 g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long gg = gw + (i0 + u) * R + r;
                g[u] = gg < gend ? *reinterpret_cast<const float4 *>(g_pm + (size_t)gg * C + c0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double *pp = pt[wave][(i0 + u) * R + r];  // (zeros past the end of the range)
                const double cn = pp[0], dx = pp[1], dy = pp[2], dz = pp[3];
                const float gs[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double gd = gs[j], cg = cn * gd;
                    a[j][0] += cg; a[j][1] += cg * gd; a[j][2] += gd * dx; a[j][3] += gd * dy; a[j][4] += gd * dz;
                }
            }
        }
    }
    // combine the row slots (lanes q, q + LPR, ...), then the four waves
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            double x = a[j][v];
#pragma unroll
            for (int s = LPR; s < 64; s <<= 1) x += __shfl_xor(x, s, 64);
            a[j][v] = x;
        }
    if (r == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int v = 0; v < 5; ++v) red[wave][4 * q + j][v] = a[j][v];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < CT * 5; t += 256) {
        const int cl = t / 5, v = t - cl * 5;
        partial[((size_t)(c0 + cl) * gridDim.x + blockIdx.x) * 5 + v] = (red[0][cl][v] + red[1][cl][v]) + (red[2][cl][v] + red[3][cl][v]);
    }
}

// The sum of one channel's partial records rec[nparts][5] (contiguous doubles) by a workgroup of LAGG_FT threads, left in
// red[0..4].  LAGG_FT is a multiple of 5, so thread t only ever meets sum t % 5: its loads are 8 bytes, contiguous over the
// workgroup, eight of them in flight; the sub-sums are then added in a fixed tree whose strides are multiples of 5 too.
// (One record per thread at a stride of C * 40 bytes, one or four in flight, took 8-24 us for 3000-8192 partials.)
constexpr int LAGG_FT = 640;
constexpr int LAGG_FU = 8;  // loads in flight per thread: one pass of the unrolled loop consumes LAGG_FT * LAGG_FU / 5 = 1024 records

__device__ __forceinline__ void lagg_sum_records(const double *__restrict__ rec, int nparts, double *red)
{
    const int total = nparts * 5, t = threadIdx.x;
    double s[LAGG_FU];
#pragma unroll
    for (int u = 0; u < LAGG_FU; ++u) s[u] = 0.0;
    int i = t;
    for (; i + (LAGG_FU - 1) * LAGG_FT < total; i += LAGG_FU * LAGG_FT) {
#pragma unroll
        for (int u = 0; u < LAGG_FU; ++u) s[u] += rec[i + u * LAGG_FT];
    }
    for (; i < total; i += LAGG_FT) s[0] += rec[i];
    red[t] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
#pragma unroll
    for (int h = LAGG_FT / 2; h >= 5; h >>= 1) {  // 320, 160, ..., 5
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
}

// mean / invstd / unbiased variance of y from the partials and the geometry moments; gd[c][3] = sum_n G D (kept for backward)
// mode 0: everything from this rank's sums.  Statistics over several ranks (torch.nn.SyncBatchNorm semantics,
// main_AA.py:146-148): mode 1 writes this rank's {sum y, sum y^2} per channel and its position count to sums (2C + 1
// doubles) for the caller to all-reduce, mode 2 derives mean / invstd from the reduced sums.
__global__ __launch_bounds__(LAGG_FT) void lagg_stats_finalize_kernel(int C, int nparts, double count, float eps, float momentum,
                                                                  const double *__restrict__ partial, const long long *__restrict__ mom,
                                                                  WDp w_dp, float *__restrict__ mean,
                                                                  float *__restrict__ invstd, float *__restrict__ var_unbiased,
                                                                  double *__restrict__ gd, float *__restrict__ running_mean,
                                                                  float *__restrict__ running_var, long long *__restrict__ tracked,
                                                                  int mode, double *__restrict__ sums)
{
    __shared__ double red[LAGG_FT];
    const int c = blockIdx.x;
    // what thread 0's formula reads besides the sums: requested before the records, so it arrives behind them
    long long mi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) mi[j] = mom[j];
        w0 = w_dp.at(c, 0); w1 = w_dp.at(c, 1); w2 = w_dp.at(c, 2);
    }
    double a[5] = {0, 0, 0, 0, 0};
    if (mode != 2) lagg_sum_records(partial + (size_t)c * nparts * 5, nparts, red);  // (mode is the same for every thread)
    if (threadIdx.x != 0) return;
    if (mode != 2) {
#pragma unroll
        for (int j = 0; j < 5; ++j) a[j] = red[j];
    }
    double m[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) m[j] = (double)mi[j] * (1.0 / LAGG_FX_M);
    const double sy = a[0] + w0 * m[0] + w1 * m[1] + w2 * m[2];
    const double quad = w0 * w0 * m[3] + w1 * w1 * m[6] + w2 * w2 * m[8] + 2.0 * (w0 * w1 * m[4] + w0 * w2 * m[5] + w1 * w2 * m[7]);
    double sy2 = a[1] + 2.0 * (w0 * a[2] + w1 * a[3] + w2 * a[4]) + quad, sy1 = sy;
    if (mode != 2) { gd[c * 3 + 0] = a[2]; gd[c * 3 + 1] = a[3]; gd[c * 3 + 2] = a[4]; }
    if (mode == 1) {
        sums[2 * c] = sy1; sums[2 * c + 1] = sy2;
        if (c == 0) sums[2 * C] = count;
        return;
    }
    if (mode == 2) { sy1 = sums[2 * c]; sy2 = sums[2 * c + 1]; count = sums[2 * C]; }
    float mf, isf, vu;
    bn_moments(sy1, sy2, count, eps, mf, isf, vu);
    mean[c] = mf; invstd[c] = isf; var_unbiased[c] = vu;
    bn_running_update(c, momentum, mf, vu, running_mean, running_var, tracked);
}

// ---------------------------------------------------------------------------------------------------------------
// forward max-pool: pooled[b,c,m] = max_k [relu](bn(G[b, idx[b,m,k], c] + W_dp[c] . dp[b,:,m,k])), arg = first k, ystar = raw y there
// grid (m tiles of 32, channel chunks of <= 128, b); a wave owns 8 centroids; LPR lanes share one gathered row
// (16 bytes each), 64/LPR rows per load instruction
// ---------------------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void lagg_pool_kernel(int C, int n, int M, int K, int cpw, int relu,
                                                        const float *__restrict__ g_pm, const int *__restrict__ idx,
                                                        const float *__restrict__ dp, WDp w_dp,
                                                        const float *__restrict__ mean, const float *__restrict__ invstd,
                                                        const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        float *__restrict__ pooled, unsigned char *__restrict__ arg,
                                                        float *__restrict__ ystar)
{
    extern __shared__ float lagg_smem[];
    constexpr int ct = 4 * LPR, rpi = 64 / LPR;   // channels of this chunk; gathered rows per load instruction
    const int MT = 4 * cpw;                        // centroids per workgroup (cpw per wave)
    float *sp = lagg_smem;                         // [ct][MT + 1] pooled
    float *sy = sp + ct * (MT + 1);                // ystar
    float *sa = sy + ct * (MT + 1);                // arg (as float bits of an int)
    const int b = blockIdx.z, c0 = blockIdx.y * ct, m0 = blockIdx.x * MT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % LPR, r = lane / LPR;
    const int cq = c0 + 4 * q;
    float w[4][3], mu[4], is[4], ga[4], be[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cq + j;
        w[j][0] = w_dp.at(c, 0); w[j][1] = w_dp.at(c, 1); w[j][2] = w_dp.at(c, 2);
        mu[j] = mean[c]; is[j] = invstd[c]; ga[j] = gamma[c]; be[j] = beta[c];
    }
    const long P = (long)M * K;
    // a centroid's indices and relative positions (lane = neighbour) are fetched while the centroid before it is pooled: the
    // gathers of a centroid wait for its indices, and a wave walks its centroids one after the other
    int id_n = 0;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    auto fetch = [&](int m_) {
        id_n = 0; n0 = n1 = n2 = 0.f;
        if (lane < K && m_ < M) {
            const size_t p = (size_t)m_ * K + lane;
            id_n = idx[(size_t)b * P + p];
            n0 = dp[((size_t)b * 3 + 0) * P + p]; n1 = dp[((size_t)b * 3 + 1) * P + p]; n2 = dp[((size_t)b * 3 + 2) * P + p];
        }
    };
    fetch(m0 + wave * cpw);
    for (int i = 0; i < cpw; ++i) {
        const int ml = wave * cpw + i, m = m0 + ml;
        if (m >= M) break;  // wave-uniform
        const int id_l = id_n;
        const float d0 = n0, d1 = n1, d2 = n2;
        if (i + 1 < cpw) fetch(m + 1);
        float best[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        float by[4] = {0.f, 0.f, 0.f, 0.f};
        int bk[4] = {0, 0, 0, 0};
        auto visit = [&](int k0) {
            const int k = k0 + r;
            const int ks = k < K ? k : K - 1;
            const int id = __shfl(id_l, ks, 64);
            const float e0 = __shfl(d0, ks, 64), e1 = __shfl(d1, ks, 64), e2 = __shfl(d2, ks, 64);
            const float4 g = *reinterpret_cast<const float4 *>(g_pm + ((size_t)b * n + id) * C + cq);
            const float gs[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = __fmaf_rn(w[j][0], e0, __fmaf_rn(w[j][1], e1, __fmaf_rn(w[j][2], e2, gs[j])));
                float v = bn_val(y, mu[j], is[j], ga[j], be[j]);
                if (relu) v = fmaxf(v, 0.f);
                if (k < K && v > best[j]) { best[j] = v; bk[j] = k; by[j] = y; }
            }
        };
        if (K == 32) {  // the configured neighbourhood size: fully unrolled, all gathers of a centroid in flight together
#pragma unroll
            for (int k0 = 0; k0 < 32; k0 += rpi) visit(k0);
        } else {
            for (int k0 = 0; k0 < K; k0 += rpi) visit(k0);
        }
#pragma unroll
        for (int s = LPR; s < 64; s <<= 1) {  // combine the row slots, first index wins among equal values
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ov = __shfl_xor(best[j], s, 64), oy = __shfl_xor(by[j], s, 64);
                const int ok = __shfl_xor(bk[j], s, 64);
                if (ov > best[j] || (ov == best[j] && ok < bk[j])) { best[j] = ov; bk[j] = ok; by[j] = oy; }
            }
        }
        if (r == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cl = 4 * q + j;
                sp[cl * (MT + 1) + ml] = best[j];
                sy[cl * (MT + 1) + ml] = by[j];
                sa[cl * (MT + 1) + ml] = __int_as_float(bk[j]);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ct * MT; t += 256) {
        const int cl = t / MT, ml = t - cl * MT, m = m0 + ml;
        if (m < M) {
            const size_t o = ((size_t)b * C + c0 + cl) * M + m;
            pooled[o] = sp[cl * (MT + 1) + ml];
            ystar[o] = sy[cl * (MT + 1) + ml];
            arg[o] = (unsigned char)__float_as_int(sa[cl * (MT + 1) + ml]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// backward 1: per (b,c,m): dq = dpooled * [relu: bn(ystar) > 0], scatter into Q[b, idx[b,m,arg], c]; per-channel partial sums
//   {sum dq, sum dq xhat, sum dq dp_j}.  grid (m-tile groups, channel chunks of 128, b)
// ---------------------------------------------------------------------------------------------------------------
// LISTS: the deterministic form (amc3d_local_aggregation_backward with rev_start).  No atomics: the masked gradient dq and its arg go out
// point-major -- dq_pm (b, M, C) floats behind Q, arg_pm (b, M, C) bytes -- for lagg_bwd_gather_kernel, which forms Q from the
// reverse lists; the tile is already transposed in LDS here, so both stores are contiguous over the channels of a wave.
template <bool LISTS>
__global__ __launch_bounds__(256) void lagg_bwd_scatter_kernel(int C, int n, int M, int K, int relu,
                                                               const float *__restrict__ dpooled, const float *__restrict__ ystar,
                                                               const unsigned char *__restrict__ arg, const int *__restrict__ idx,
                                                               const float *__restrict__ dp, const float *__restrict__ mean,
                                                               const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, float *__restrict__ Q,
                                                               double *__restrict__ partial, int nparts_per_b, int tiles_per_wg,
                                                               float *__restrict__ dq_pm, unsigned char *__restrict__ arg_pm)
{
    extern __shared__ float lagg_smem[];
    const int ct = min(LAGG_CT, C - (int)blockIdx.y * LAGG_CT);
    float *sd = lagg_smem;                        // [ct][LAGG_MT + 1] dpooled
    float *sy = sd + ct * (LAGG_MT + 1);          // ystar
    float *sa = sy + ct * (LAGG_MT + 1);          // arg
    int *sidx = reinterpret_cast<int *>(sa + ct * (LAGG_MT + 1));  // [LAGG_MT][K]     neighbour indices of the tile's centroids
    float *sdp = reinterpret_cast<float *>(sidx + LAGG_MT * K);    // [3][LAGG_MT][K]  their relative positions
    const int b = blockIdx.z, c0 = blockIdx.y * LAGG_CT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long P = (long)M * K;
    double acc[2][5];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[h][j] = 0.0;
    float mu[2], is[2], ga[2], be[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cl = lane + 64 * h, c = cl < ct ? c0 + cl : c0;
        mu[h] = mean[c]; is[h] = invstd[c]; ga[h] = gamma[c]; be[h] = beta[c];
    }
    for (int tt = 0; tt < tiles_per_wg; ++tt) {
        const int m0 = (blockIdx.x * tiles_per_wg + tt) * LAGG_MT;
        if (m0 >= M) break;
        __syncthreads();
        for (int t = threadIdx.x; t < ct * LAGG_MT; t += 256) {
            const int cl = t / LAGG_MT, ml = t - cl * LAGG_MT, m = m0 + ml;
            float d = 0.f, y = 0.f;
            int a = 0;
            if (m < M) {
                const size_t o = ((size_t)b * C + c0 + cl) * M + m;
                d = dpooled[o]; y = ystar[o]; a = arg[o];
            }
            sd[cl * (LAGG_MT + 1) + ml] = d; sy[cl * (LAGG_MT + 1) + ml] = y; sa[cl * (LAGG_MT + 1) + ml] = __int_as_float(a);
        }
        // the tile's rows of idx and dp (contiguous: LAGG_MT * K positions), read once for all channels -- every routed
        // gradient used to fetch its own index and, behind it, three floats of dp: two dependent round trips per element
        for (int t = threadIdx.x; t < LAGG_MT * K; t += 256) {
            const long pos = (long)m0 * K + t;
            const bool in = pos < P;
            sidx[t] = in ? idx[(size_t)b * P + pos] : 0;
            const size_t pd = (size_t)b * 3 * P + pos;
            sdp[t] = in ? dp[pd] : 0.f;
            sdp[LAGG_MT * K + t] = in ? dp[pd + P] : 0.f;
            sdp[2 * LAGG_MT * K + t] = in ? dp[pd + 2 * P] : 0.f;
        }
        __syncthreads();
        for (int i = 0; i < LAGG_MT / 4; ++i) {
            const int ml = wave * (LAGG_MT / 4) + i, m = m0 + ml;
            if (m >= M) break;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int cl = lane + 64 * h;
                if (cl >= ct) continue;
                float dq = sd[cl * (LAGG_MT + 1) + ml];
                const float y = sy[cl * (LAGG_MT + 1) + ml];
                const int k = __float_as_int(sa[cl * (LAGG_MT + 1) + ml]);
                const float xh = __fmul_rn(__fsub_rn(y, mu[h]), is[h]);
                if (relu && !(__fadd_rn(__fmul_rn(xh, ga[h]), be[h]) > 0.f)) dq = 0.f;
                if constexpr (LISTS) {
                    const size_t o = ((size_t)b * M + m) * C + c0 + cl;
                    dq_pm[o] = dq;
                    arg_pm[o] = (unsigned char)k;
                }
                if (dq != 0.f) {
                    const int slot = ml * K + k;
                    const int id = sidx[slot];
                    const double dd = dq;
                    acc[h][0] += dd; acc[h][1] += dd * (double)xh;
                    acc[h][2] += dd * (double)sdp[slot]; acc[h][3] += dd * (double)sdp[LAGG_MT * K + slot];
                    acc[h][4] += dd * (double)sdp[2 * LAGG_MT * K + slot];
                    if constexpr (!LISTS) atomicAdd(Q + ((size_t)b * n + id) * C + c0 + cl, dq);
                }
            }
        }
    }
    __syncthreads();
    double *red = reinterpret_cast<double *>(lagg_smem);  // [4][ct][5] doubles
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (lane + 64 * h < ct) {
#pragma unroll
            for (int j = 0; j < 5; ++j) red[((size_t)wave * ct + lane + 64 * h) * 5 + j] = acc[h][j];
        }
    __syncthreads();
    for (int t = threadIdx.x; t < ct * 5; t += 256) {
        const int cl = t / 5, j = t - cl * 5;
        const double v = (red[((size_t)0 * ct + cl) * 5 + j] + red[((size_t)1 * ct + cl) * 5 + j]) +
                         (red[((size_t)2 * ct + cl) * 5 + j] + red[((size_t)3 * ct + cl) * 5 + j]);
        partial[((size_t)(c0 + cl) * gridDim.z * nparts_per_b + (size_t)b * nparts_per_b + blockIdx.x) * 5 + j] = v;
    }
}

// Q from the reverse lists (amc3d_group_csr), no atomics: Q[b,j,c] = the sum of dq[b,c,m] over the positions (m,k) of j's list
// with arg[b,c,m] == k, taken in list order (ascending position) by sequential fp32 adds from +0.0f.  A thread per (source
// point, channel), the channel on the lane: the list entries are wave-wide broadcasts, dq_pm / arg_pm rows contiguous reads.
// A padded ball-query row holds j at several k of one m: only the position that equals arg carries the gradient.  Every
// element of Q is written (an empty list: +0.0f).
__global__ __launch_bounds__(256) void lagg_bwd_gather_kernel(int C, int n, int M, int K, long total,
                                                              const float *__restrict__ dq_pm,
                                                              const unsigned char *__restrict__ arg_pm,
                                                              const int *__restrict__ rev_start, const int *__restrict__ rev_edge,
                                                              float *__restrict__ Q)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long g = t / C;
    const int c = (int)(t - g * C);
    const long b = g / n;
    const int s = rev_start[g], e = rev_start[g + 1];
    const float *drow = dq_pm + (size_t)b * M * C + c;
    const unsigned char *arow = arg_pm + (size_t)b * M * C + c;
    float q = 0.f;
    for (int i = s; i < e; i += 4) {  // four positions' loads in flight; the adds keep the list order
        int m[4], k[4], a[4];
        float d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = rev_edge[min(i + u, e - 1)];
            m[u] = p / K;
            k[u] = p - m[u] * K;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = arow[(size_t)m[u] * C]; d[u] = drow[(size_t)m[u] * C]; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u < e && a[u] == k[u]) q = __fadd_rn(q, d[u]);
    }
    Q[t] = q;
}

// dgamma, dbeta, dW_dp and the per-channel coefficients of dG: coef[c] = {g*is, ma, mb*is, mu}
// mode 0: one rank.  mode 1: reduce this rank's partials, publish {sum dq, sum dq xhat} to dsums (2C doubles) for the
// all-reduce, keep the five local sums in the channel's first record; mode 2 (same nparts): coefficients from the reduced dsums
// and the global count (*count_dev), dW_dp from the local sums (parameter gradients stay rank-local, as torch's SyncBatchNorm
// leaves them).  partial[channel][nparts][5], summed by lagg_sum_records.
__global__ __launch_bounds__(LAGG_FT) void lagg_bwd_finalize_kernel(int C, int nparts, double count, double *__restrict__ partial,
                                                                const long long *__restrict__ mom, const double *__restrict__ gd,
                                                                WDp w_dp, const float *__restrict__ mean,
                                                                const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                                float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                                float *__restrict__ dw_dp, long lddw, float *__restrict__ coef, int mode,
                                                                double *__restrict__ dsums, const double *__restrict__ count_dev)
{
    __shared__ double red[LAGG_FT];
    const int c = blockIdx.x;
    double *rec = partial + (size_t)c * nparts * 5;  // this channel's records; the first holds the rank's reduced sums after mode 1
    // what thread 0's formula reads besides the sums: requested before the records, so it arrives behind them
    long long mi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double w[3] = {0, 0, 0}, gdc[3] = {0, 0, 0}, mu = 0.0, is = 0.0, g = 0.0, sa2 = 0.0, sb2 = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) mi[j] = mom[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) { w[j] = w_dp.at(c, j); gdc[j] = gd[c * 3 + j]; }
        mu = mean[c]; is = invstd[c]; g = gamma[c];
        if (mode == 2) { sa2 = dsums[2 * c]; sb2 = dsums[2 * c + 1]; count = *count_dev; }
    }
    lagg_sum_records(rec, mode == 2 ? 1 : nparts, red);
    if (threadIdx.x != 0) return;
    double a[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) a[j] = red[j];
    double m[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) m[j] = (double)mi[j] * (1.0 / LAGG_FX_M);
    const double S2[3][3] = {{m[3], m[4], m[5]}, {m[4], m[6], m[7]}, {m[5], m[7], m[8]}};
    if (mode != 2) { dbeta[c] = (float)a[0]; dgamma[c] = (float)a[1]; }
    if (mode == 1) {
#pragma unroll
        for (int j = 0; j < 5; ++j) rec[j] = a[j];
        dsums[2 * c] = a[0]; dsums[2 * c + 1] = a[1];
        return;
    }
    double sa = a[0], sb = a[1];
    if (mode == 2) { sa = sa2; sb = sb2; }
    const double ma = sa / count, mb = sb / count, gi = g * is;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        // sum_p xhat_p dp_p[j] = is * ( sum_n G D_j + sum_j' w_j' S2[j'][j] - mu S1[j] )
        const double sxd = is * (gdc[j] + w[0] * S2[0][j] + w[1] * S2[1][j] + w[2] * S2[2][j] - mu * m[j]);
        dw_dp[c * lddw + j] = (float)(gi * (a[2 + j] - ma * m[j] - mb * sxd));
    }
    coef[c * 4 + 0] = (float)gi; coef[c * 4 + 1] = (float)ma; coef[c * 4 + 2] = (float)(mb * is); coef[c * 4 + 3] = (float)mu;
}

// ---------------------------------------------------------------------------------------------------------------
// backward 2: dG[b,c,n] = gi * ( Q - cnt*ma - mbis * ( cnt*(G - mu) + W_dp . D ) ), written channel-major
// grid (n tiles of NT, channel chunks of CT = 4 * LPR <= 64, b), NT = 4096 / CT up to 256.  Rows as in lagg_stats_rows_kernel:
// LPR lanes share a row of Q and of G, 16 bytes each, 64 / LPR rows per wave instruction, all of a wave's loads (at most four
// instructions per operand) in flight at once; cnt / D of a point are loaded and converted by one thread and read from LDS.
// The tile is turned in LDS; a wave then stores 256 contiguous bytes of one channel row.
// ---------------------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void lagg_bwd_apply_kernel(int C, int n, const float *__restrict__ Q, const float *__restrict__ g_pm,
                                                             LaggMoments gm, WDp w_dp,
                                                             const float *__restrict__ coef, float *__restrict__ dg_cm)
{
    constexpr int CT = 4 * LPR, R = 64 / LPR, NT = 4096 / CT < 256 ? 4096 / CT : 256, STEPS = NT / 4 / R;
    __shared__ float tile[CT][NT + 1];  // odd stride: the (channel quad, point) writes are at most 2-way
    __shared__ float4 pt[NT];           // cnt, D_x, D_y, D_z of the tile's points
    const int b = blockIdx.z, c0 = blockIdx.y * CT, n0 = blockIdx.x * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % LPR, r = lane / LPR;
    const int cq = c0 + 4 * q;
    for (int t = threadIdx.x; t < NT; t += 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 + t < n) {
            const size_t gg = (size_t)b * n + n0 + t;
            const long long *df = gm.dfx + gg * 3;
            const long long fx = df[0], fy = df[1], fz = df[2];
            v.x = (float)gm.cnt[gg];
            v.y = (float)((double)fx * (1.0 / LAGG_FX_D)); v.z = (float)((double)fy * (1.0 / LAGG_FX_D));
            v.w = (float)((double)fz * (1.0 / LAGG_FX_D));
        }
        pt[t] = v;
    }
    float gi[4], ma[4], mbis[4], mu[4], w[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cq + j;
        gi[j] = coef[c * 4 + 0]; ma[j] = coef[c * 4 + 1]; mbis[j] = coef[c * 4 + 2]; mu[j] = coef[c * 4 + 3];
        w[j][0] = w_dp.at(c, 0); w[j][1] = w_dp.at(c, 1); w[j][2] = w_dp.at(c, 2);
    }
    float4 qv[STEPS], gv[STEPS];
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        const int nl = wave * (NT / 4) + i * R + r;
        qv[i] = gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 + nl < n) {
            const size_t o = ((size_t)b * n + n0 + nl) * C + cq;
            qv[i] = *reinterpret_cast<const float4 *>(Q + o);
            gv[i] = *reinterpret_cast<const float4 *>(g_pm + o);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        const int nl = wave * (NT / 4) + i * R + r;
        const float4 p = pt[nl];
        const float cn = p.x, dx = p.y, dy = p.z, dz = p.w;
        const float qs[4] = {qv[i].x, qv[i].y, qv[i].z, qv[i].w}, gs[4] = {gv[i].x, gv[i].y, gv[i].z, gv[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float wd = w[j][0] * dx + w[j][1] * dy + w[j][2] * dz;
            tile[4 * q + j][nl] = gi[j] * (qs[j] - cn * ma[j] - mbis[j] * (cn * (gs[j] - mu[j]) + wd));
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < CT * NT; t += 256) {
        const int cl = t / NT, pp = t - cl * NT;
        if (n0 + pp < n) dg_cm[((size_t)b * C + c0 + cl) * n + n0 + pp] = tile[cl][pp];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// First layer of a multi-layer SetAbstraction MLP (PointNeXt-S: sa_layers = 2): the same convolve-before-gather
// conv + BatchNorm + ReLU, but the activation x1 (B,C,M,K) is materialised for the layers that follow
//   expand    x1[b,c,m,k] = [relu](bn(G[b, idx[b,m,k], c] + W_dp[c] . dp[b,:,m,k]))       one gather pass, one write
//   collapse  from dx1 (B,C,M,K): d = dx1 * [relu mask], scattered into Q[b, idx, c] (row-contiguous float atomics, zeros
//             skipped) + the per-channel sums {sum d, sum d xhat, sum d dp_j}: BatchNorm's backward then needs nothing
//             else of size M*K (lagg_bwd_finalize / lagg_bwd_apply turn Q into dG on the N source points).
// One pass over dx1 replaces BN-backward statistics, BN-backward apply, the conv's backward-data product + scatter and
// its backward-weight product.  grid (position-tile groups, channel chunks of 64, b); a tile = 128 positions.
// ---------------------------------------------------------------------------------------------------------------
constexpr int LAGG_PT = 128;  // positions per tile
constexpr int LAGG_XC = 64;   // channels per workgroup

template <int LPR>
__global__ __launch_bounds__(256) void lagg_expand_kernel(int C, int n, long P, int relu, const float *__restrict__ g_pm,
                                                          const int *__restrict__ idx, const float *__restrict__ dp,
                                                          WDp w_dp, const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float *__restrict__ x1)
{
    __shared__ float tile[LAGG_XC][LAGG_PT + 1];  // odd stride: the (channel quad, position) writes are at most 2-way
    const int b = blockIdx.z, c0 = blockIdx.y * LAGG_XC;
    const int ct = min(LAGG_XC, C - c0);
    const long p0 = (long)blockIdx.x * LAGG_PT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int rpi = 64 / LPR;
    const int q = lane % LPR, r = lane / LPR;
    const int cq = c0 + 4 * q;
    float w[4][3], mu[4], is[4], ga[4], be[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cq + j;
        w[j][0] = w_dp.at(c, 0); w[j][1] = w_dp.at(c, 1); w[j][2] = w_dp.at(c, 2);
        mu[j] = mean[c]; is[j] = invstd[c]; ga[j] = gamma[c]; be[j] = beta[c];
    }
    // this wave's 32 positions: lane l < 32 fetches index and dp of position wave*32 + l
    const long pw = p0 + wave * 32;
    int id_l = 0;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (lane < 32 && pw + lane < P) {
        id_l = idx[(size_t)b * P + pw + lane];
        d0 = dp[((size_t)b * 3 + 0) * P + pw + lane]; d1 = dp[((size_t)b * 3 + 1) * P + pw + lane]; d2 = dp[((size_t)b * 3 + 2) * P + pw + lane];
    }
#pragma unroll
    for (int k0 = 0; k0 < 32; k0 += rpi) {
        const int k = k0 + r;
        const int id = __shfl(id_l, k, 64);
        const float e0 = __shfl(d0, k, 64), e1 = __shfl(d1, k, 64), e2 = __shfl(d2, k, 64);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pw + k < P) g = *reinterpret_cast<const float4 *>(g_pm + ((size_t)b * n + id) * C + cq);
        const float gs[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = __fmaf_rn(w[j][0], e0, __fmaf_rn(w[j][1], e1, __fmaf_rn(w[j][2], e2, gs[j])));
            float v = bn_val(y, mu[j], is[j], ga[j], be[j]);
            if (relu) v = fmaxf(v, 0.f);
            tile[4 * q + j][wave * 32 + k] = v;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ct * LAGG_PT; t += 256) {  // a wave stores 256 contiguous bytes of one channel row
        const int cl = t / LAGG_PT, pp = t - cl * LAGG_PT;
        if (p0 + pp < P) x1[((size_t)b * C + c0 + cl) * P + p0 + pp] = tile[cl][pp];
    }
}

template <int LPR>
__global__ __launch_bounds__(256) void lagg_collapse_kernel(int C, int n, long P, int relu, const float *__restrict__ dx1,
                                                            const float *__restrict__ g_pm, const int *__restrict__ idx,
                                                            const float *__restrict__ dp, WDp w_dp,
                                                            const float *__restrict__ mean, const float *__restrict__ invstd,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            float *__restrict__ Q, double *__restrict__ partial, int nparts_per_b,
                                                            int tiles_per_wg)
{
    __shared__ float tile[LAGG_XC][LAGG_PT + 1];
    double(*red)[LAGG_XC][5] = reinterpret_cast<double(*)[LAGG_XC][5]>(&tile[0][0]);  // reused after the last tile (10 KiB of 33)
    constexpr int rpi = 64 / LPR, CT = 4 * LPR;  // channels of this workgroup's chunk
    const int b = blockIdx.z, c0 = blockIdx.y * LAGG_XC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % LPR, r = lane / LPR;
    const int cq = c0 + 4 * q;
    float w[4][3], mu[4], is[4], ga[4], be[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cq + j;
        w[j][0] = w_dp.at(c, 0); w[j][1] = w_dp.at(c, 1); w[j][2] = w_dp.at(c, 2);
        mu[j] = mean[c]; is[j] = invstd[c]; ga[j] = gamma[c]; be[j] = beta[c];
    }
    double acc[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int v = 0; v < 5; ++v) acc[j][v] = 0.0;
    for (int tt = 0; tt < tiles_per_wg; ++tt) {
        const long p0 = ((long)blockIdx.x * tiles_per_wg + tt) * LAGG_PT;
        if (p0 >= P) break;
        __syncthreads();
        for (int t = threadIdx.x; t < CT * LAGG_PT; t += 256) {
            const int cl = t / LAGG_PT, pp = t - cl * LAGG_PT;
            tile[cl][pp] = (p0 + pp < P) ? dx1[((size_t)b * C + c0 + cl) * P + p0 + pp] : 0.f;
        }
        __syncthreads();
        const long pw = p0 + wave * 32;
        int id_l = 0;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (lane < 32 && pw + lane < P) {
            id_l = idx[(size_t)b * P + pw + lane];
            d0 = dp[((size_t)b * 3 + 0) * P + pw + lane]; d1 = dp[((size_t)b * 3 + 1) * P + pw + lane]; d2 = dp[((size_t)b * 3 + 2) * P + pw + lane];
        }
        // phase A: 16-byte gathers of the G rows; mask the ReLU, accumulate the sums, leave the masked gradient in the tile
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += rpi) {
            const int k = k0 + r;
            const int id = __shfl(id_l, k, 64);
            const float e0 = __shfl(d0, k, 64), e1 = __shfl(d1, k, 64), e2 = __shfl(d2, k, 64);
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pw + k < P) g = *reinterpret_cast<const float4 *>(g_pm + ((size_t)b * n + id) * C + cq);
            const float gs[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = __fmaf_rn(w[j][0], e0, __fmaf_rn(w[j][1], e1, __fmaf_rn(w[j][2], e2, gs[j])));
                const float xh = __fmul_rn(__fsub_rn(y, mu[j]), is[j]);
                float d = tile[4 * q + j][wave * 32 + k];
                if (relu && !(__fadd_rn(__fmul_rn(xh, ga[j]), be[j]) > 0.f)) d = 0.f;
                tile[4 * q + j][wave * 32 + k] = d;  // (this lane is the only reader and writer of the element)
                const double dd = d;
                acc[j][0] += dd; acc[j][1] += dd * (double)xh;
                acc[j][2] += dd * (double)e0; acc[j][3] += dd * (double)e1; acc[j][4] += dd * (double)e2;
            }
        }
        // phase B: scatter with one lane per channel: a wave-instruction adds 64 / CT whole rows of CT contiguous floats
        // (each wave reads back only what it wrote itself: its own 32 positions)
        constexpr int ppi = 64 / CT > 0 ? 64 / CT : 1;  // positions per instruction
        const int cl = lane % CT, sub = lane / CT;
        for (int k0 = 0; k0 < 32; k0 += ppi) {
            const int k = k0 + sub;
            const int id = __shfl(id_l, k & 31, 64);
            if (sub < ppi && pw + k < P) {
                const float d = tile[cl][wave * 32 + k];
                if (d != 0.f) atomicAdd(Q + ((size_t)b * n + id) * C + c0 + cl, d);
            }
        }
    }
    // combine the row slots (lanes q, q + LPR, ...), then the four waves
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            double x = acc[j][v];
#pragma unroll
            for (int s = LPR; s < 64; s <<= 1) x += __shfl_xor(x, s, 64);
            acc[j][v] = x;
        }
    __syncthreads();  // the tile is no longer read: its memory holds the cross-wave reduction
    if (r == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int v = 0; v < 5; ++v) red[wave][4 * q + j][v] = acc[j][v];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < CT * 5; t += 256) {
        const int cl2 = t / 5, v = t - cl2 * 5;
        partial[((size_t)(c0 + cl2) * gridDim.z * nparts_per_b + (size_t)b * nparts_per_b + blockIdx.x) * 5 + v] =
            (red[0][cl2][v] + red[1][cl2][v]) + (red[2][cl2][v] + red[3][cl2][v]);
    }
}

static bool lagg_supported(int C, int K)
{
    if (C < 8 || C % 4 || K < 1 || K > 64) return false;
    const int ct = C < LAGG_CT ? C : LAGG_CT;
    const int lpr = ct / 4;
    return (lpr & (lpr - 1)) == 0 && C % ct == 0;  // 8,16,32,64,128 and multiples of 128
}

// tiles per workgroup of the backward scatter kernel: one while that still leaves the grid small (its workgroups walk their
// centroids serially: a few dozen of them took 50-100 us on the coarse stages of PointNeXt-L)
static int lagg_scatter_tiles(int b, int C, int M)
{
    const long wgs1 = (long)b * div_up(M, LAGG_MT) * div_up(C, LAGG_CT);
    return wgs1 <= 8192 ? 1 : LAGG_TILES;
}

// centroids per wave of the max-pool kernel: 8, fewer where that leaves the chip with under ~2 workgroups per CU (the coarse stages)
static int lagg_pool_cpw(int b, int cout, int npoints)
{
    const int ct = cout < LAGG_CT ? cout : LAGG_CT;
    int cpw = 8;
    while (cpw > 1 && (long)div_up(npoints, 4 * cpw) * (cout / ct) * b < 1024) cpw >>= 1;
    return cpw;
}

static size_t lagg_partial_bytes(int b, int C, int n, int M)
{
    const size_t pf = (size_t)b * div_up(n, LAGG_SP),  // the statistics: at most one partial per 256-point pass (lagg_stats_pts)
                 pb = (size_t)b * div_up(div_up(M, LAGG_MT), lagg_scatter_tiles(b, C, M));
    const size_t pc = (size_t)b * div_up((long)M * 32, LAGG_PT);  // collapse kernel (K = 32), at most one partial per tile
    size_t m = pf > pb ? pf : pb;
    if (pc > m) m = pc;
    return m * C * 5 * sizeof(double);
}

// the materialising first layer: K = 32, channel chunks of 64 (or the whole of C in {8, 16, 32})
static bool lagg_expand_supported(int C, int K)
{
    if (K != 32 || C < 8 || C % 4) return false;
    const int ct = C < LAGG_XC ? C : LAGG_XC;
    const int lpr = ct / 4;
    return (lpr & (lpr - 1)) == 0 && C % ct == 0;
}

size_t csr_partials(int b, int cout, int n);  // csr.hip
constexpr int LAGG_CTILES = 2;  // tiles per workgroup of lagg_collapse_kernel (1, 2, 4 measured alike: the kernel runs at the float-atomic rate)

// points per workgroup of lagg_stats_rows_kernel: whole 256-point passes, about 1024 workgroups over the chip.  At most
// ceil(b * n / 256) partials per channel, which lagg_partial_bytes() reserves
static int lagg_stats_pts(long G, int C)
{
    const int chunks = C <= 64 ? 1 : C / 64;
    const long target = 1024 / chunks > 1 ? 1024 / chunks : 1;
    const long passes = (G + LAGG_SP - 1) / LAGG_SP;
    return (int)((passes + target - 1) / target) * LAGG_SP;
}

// batch statistics of the layer from the rows of G: the partial sums (phases 0, 1), then mean / invstd / gd / running buffers
static int lagg_statistics(int b, int cout, int n, int npoints, int nsample, float eps, float momentum, const float *g_pm,
                           const LaggMoments &gm, WDp w_dp, float *mean, float *invstd, float *var_unbiased, double *gd,
                           float *running_mean, float *running_var, long long *num_batches_tracked, int phase, double *sums,
                           double *partial, hipStream_t stream)
{
    const long G = (long)b * n;
    const int ct = cout < 64 ? cout : 64;
    const int per = lagg_stats_pts(G, cout), nparts = div_up(G, per);
    if (phase != 2) {
#define AMC_STATS(L)                                                                                                           \
    hipLaunchKernelGGL(lagg_stats_rows_kernel<L>, dim3(nparts, cout / ct), dim3(256), 0, stream, cout, G, g_pm, gm, partial, per)
        switch (ct / 4) { case 2: AMC_STATS(2); break; case 4: AMC_STATS(4); break; case 8: AMC_STATS(8); break; default: AMC_STATS(16); }
#undef AMC_STATS
    }
    hipLaunchKernelGGL(lagg_stats_finalize_kernel, dim3(cout), dim3(LAGG_FT), 0, stream, cout, nparts,
                       (double)b * (double)npoints * (double)nsample, eps, momentum, (const double *)partial, gm.mom, w_dp, mean,
                       invstd, var_unbiased, gd, running_mean, running_var, num_batches_tracked, phase, sums);
    return 0;
}

// dG (b, cout, n) channel-major from Q, the rows of G and the coefficients of lagg_bwd_finalize_kernel
static void lagg_apply(int b, int cout, int n, const float *Q, const float *g_pm, const LaggMoments &gm, WDp w_dp, const float *coef,
                       float *dg_cm, hipStream_t stream)
{
    const int ct = cout < 64 ? cout : 64;
    const int nt = 4096 / ct < 256 ? 4096 / ct : 256;
#define AMC_APPLY(L)                                                                                                           \
    hipLaunchKernelGGL(lagg_bwd_apply_kernel<L>, dim3(div_up(n, nt), cout / ct, b), dim3(256), 0, stream, cout, n, Q, g_pm, gm,  \
                       w_dp, coef, dg_cm)
    switch (ct / 4) { case 2: AMC_APPLY(2); break; case 4: AMC_APPLY(4); break; case 8: AMC_APPLY(8); break; default: AMC_APPLY(16); }
#undef AMC_APPLY
}

}  // namespace amc

using namespace amc;

AMC_API int amc3d_local_aggregation_supported(int cout, int nsample) { return lagg_supported(cout, nsample) ? 1 : 0; }

AMC_API size_t amc3d_group_moments_bytes(int b, int n) { return (b <= 0 || n <= 0) ? 0 : lagg_moments_bytes(b, n); }

// moments (opaque, amc3d_group_moments_bytes): in-degree and dp sum of every support point, global dp moments
AMC_API int amc3d_group_moments(int b, int n, int npoints, int nsample, const int *idx, const float *dp, void *moments,
                                size_t moments_bytes, void *stream_)
{
    if (b <= 0 || n <= 0) return 0;
    if (!idx || !dp || !moments || moments_bytes < lagg_moments_bytes(b, n) || npoints <= 0 || nsample <= 0)
        return bad_arg("amc3d_group_moments: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    if (int st = fill_i32((int *)moments, 0, lagg_moments_bytes(b, n) / 4, stream)) return st;
    const LaggMoments v = lagg_views(moments, b, n);
    const long P = (long)npoints * nsample;
    const int blocks = (int)(div_up(P, 256 * 4) < 1024 ? div_up(P, 256 * 4) : 1024);
    hipLaunchKernelGGL(lagg_geom_kernel, dim3(blocks, b), dim3(256), 0, stream, n, P, idx, dp, (int *)v.cnt,
                       (unsigned long long *)v.dfx, (unsigned long long *)v.mom);
    return launch_status("amc3d_group_moments");
}

// coef (cout, 4) floats, rounded up so that what follows it in the workspace stays 16-byte aligned
static size_t lagg_coef_floats(int cout) { return ((size_t)cout * 4 + 3) & ~(size_t)3; }

// the workspace of amc3d_local_aggregation_backward with lists: that of the atomic form | dq_pm (b, npoints, cout) floats | arg_pm bytes
AMC_API size_t amc3d_local_aggregation_csr_workspace_bytes(int b, int cout, int n, int npoints)
{
    if (b <= 0 || cout <= 0 || n <= 0 || npoints <= 0) return 0;
    return lagg_partial_bytes(b, cout, n, npoints) + (size_t)b * n * cout * sizeof(float) + lagg_coef_floats(cout) * sizeof(float) +
           (size_t)b * npoints * cout * 5 + 64;
}

// where both backward forms leave Q (b, n, cout) in their workspace, in bytes (tests and tools check the summation order on it)
AMC_API size_t amc3d_local_aggregation_workspace_q_offset(int b, int cout, int n, int npoints)
{
    if (b <= 0 || cout <= 0 || n <= 0 || npoints <= 0) return 0;
    return lagg_partial_bytes(b, cout, n, npoints);
}

// how many partial records per channel each producer leaves for the finalize kernels at this shape (tests and tools):
// counts[0] the forward statistics, [1] the pooled layer's backward scatter, [2] the atomic collapse, [3] the reverse-list collapse
AMC_API int amc3d_local_aggregation_partial_counts(int b, int cout, int n, int npoints, int nsample, int *counts)
{
    if (!counts || b <= 0 || cout <= 0 || n <= 0 || npoints <= 0 || nsample <= 0)
        return bad_arg("amc3d_local_aggregation_partial_counts: bad argument");
    counts[0] = div_up((long)b * n, lagg_stats_pts((long)b * n, cout));
    counts[1] = b * div_up(div_up(npoints, LAGG_MT), lagg_scatter_tiles(b, cout, npoints));
    counts[2] = b * div_up(div_up((long)npoints * nsample, LAGG_PT), LAGG_CTILES);
    counts[3] = (int)csr_partials(b, cout, n);
    return 0;
}

// centroids per wave the forward's max-pool launch takes at this shape (8, 4, 2 or 1: a workgroup pools 4 times as many); -1:
// not a shape of the layer (tests and tools)
AMC_API int amc3d_local_aggregation_pool_centroids(int b, int cout, int npoints)
{
    if (b <= 0 || npoints <= 0 || !lagg_supported(cout, 1)) return -1;
    return lagg_pool_cpw(b, cout, npoints);
}

AMC_API size_t amc3d_local_aggregation_workspace_bytes(int b, int cout, int n, int npoints)
{
    if (b <= 0 || cout <= 0 || n <= 0 || npoints <= 0) return 0;
    // partial sums | Q (b, n, cout) | coef (cout, 4)
    return lagg_partial_bytes(b, cout, n, npoints) + (size_t)b * n * cout * sizeof(float) + (size_t)cout * 4 * sizeof(float) + 64;
}

static int lagg_bad(const char *entry, const char *what)
{
    set_error("%s: %s", entry, what);
    return (int)hipErrorInvalidValue;
}

// What both layers' forwards do before their own launch.  G = W_f . f comes from the caller: as rows g_pm (b,n,cout)
// (g_cm == NULL: amc3d_pointwise_conv_forward_rows wrote them), or channel-major g_cm (b,cout,n), which is first turned into
// g_pm.  g_pm is kept for backward.  Then the batch statistics: mean / invstd / var_unbiased (cout), gd (cout,3) doubles.
// training == 0: mean / invstd are INPUTS (running statistics), no statistics pass.
// *done: the caller launches nothing more (an empty batch; phase 1, which ends with this rank's sums)
static int lagg_forward_begin(const char *entry, bool (*supported)(int, int), int b, int cout, int n, int npoints, int nsample,
                              int training, float eps, float momentum, const float *g_cm, const int *idx, const float *dp,
                              WDp w_dp, const void *moments, const float *gamma, const float *beta, float *g_pm, float *mean,
                              float *invstd, float *var_unbiased, double *gd, float *running_mean, float *running_var,
                              long long *num_batches_tracked, int phase, double *sums, void *workspace, size_t workspace_bytes,
                              void *stream_, bool *done)
{
    *done = true;
    if (w_dp.ld < 3) return lagg_bad(entry, "row stride below 3");
    if (training && phase != 0 && !sums) return lagg_bad(entry, "phase 1 / 2 need the sums buffer");
    if (b <= 0 || npoints <= 0) return 0;
    if (!supported(cout, nsample) || n <= 0 || !idx || !dp || !w_dp || !gamma || !beta || !g_pm || ((uintptr_t)g_pm & 15) ||
        !mean || !invstd || (training && (!moments || !var_unbiased || !gd || !workspace ||
        workspace_bytes < amc3d_local_aggregation_workspace_bytes(b, cout, n, npoints))) ||
        (running_mean && (!running_var || !num_batches_tracked)))
        return lagg_bad(entry, "unsupported shape, null or misaligned pointer or workspace too small");
    LaggMoments gm{};
    if (moments) gm = lagg_views(moments, b, n);
    // G channel-major: its rows first (phase 2 finds them where phase 1 left them)
    if (g_cm && !(training && phase == 2))
        if (int st = amc3d_transpose_cn(b, cout, n, g_cm, g_pm, stream_)) return st;
    if (training) {
        if (int st = lagg_statistics(b, cout, n, npoints, nsample, eps, momentum, g_pm, gm, w_dp, mean, invstd, var_unbiased, gd,
                                     running_mean, running_var, num_batches_tracked, phase, sums, (double *)workspace,
                                     (hipStream_t)stream_))
            return st;
        if (phase == 1) return launch_status(entry);
    }
    *done = false;
    return 0;
}

// The checks both layers' backwards share; dy is the incoming gradient, need_bytes the workspace of the form that runs.
// *done: an empty batch, nothing to launch
static int lagg_backward_begin(const char *entry, bool (*supported)(int, int), int b, int cout, int n, int npoints, int nsample,
                               const float *dy, const float *g_pm, const float *dp, WDp w_dp, const void *moments,
                               const double *gd, const float *mean, const float *invstd, const float *gamma, const float *beta,
                               const float *dg_cm, const float *dw_dp, long lddw, const float *dgamma, const float *dbeta,
                               int phase, const double *dsums, const double *count_dev, const void *workspace,
                               size_t workspace_bytes, size_t need_bytes, bool *done)
{
    *done = true;
    if (w_dp.ld < 3 || lddw < 3) return lagg_bad(entry, "row stride below 3");
    if (b <= 0 || npoints <= 0) return 0;
    if (phase != 0 && (!dsums || (phase == 2 && !count_dev))) return lagg_bad(entry, "phase 1 / 2 need dsums (and the count)");
    if (!supported(cout, nsample) || n <= 0 || !dy || !g_pm || !dp || !w_dp || !moments || !gd || !mean || !invstd || !gamma ||
        !beta || !dg_cm || !dw_dp || !dgamma || !dbeta || !workspace || (((uintptr_t)workspace | (uintptr_t)g_pm) & 15) ||
        workspace_bytes < need_bytes)
        return lagg_bad(entry, "unsupported shape, null pointer or workspace too small");
    *done = false;
    return 0;
}

// The end of both layers' backwards, from what the first stage left: `nparts` partial records per channel and Q (b,n,cout).
// BatchNorm's coefficients and dw_dp (cout,3 at lddw), dgamma, dbeta (cout); phase 1 ends there, with this rank's dsums.  Then
// dg_cm (b,cout,n), the gradient w.r.t. G = W_f . f (the caller runs the pointwise conv's backward on it)
static int lagg_backward_finish(const char *entry, int b, int cout, int n, int npoints, int nsample, int nparts,
                                double *partial, const float *Q, float *coef, const float *g_pm, const void *moments,
                                const double *gd, WDp w_dp, const float *mean, const float *invstd, const float *gamma,
                                float *dg_cm, float *dw_dp, long lddw, float *dgamma, float *dbeta, int phase, double *dsums,
                                const double *count_dev, hipStream_t stream)
{
    const LaggMoments gm = lagg_views(moments, b, n);
    hipLaunchKernelGGL(lagg_bwd_finalize_kernel, dim3(cout), dim3(LAGG_FT), 0, stream, cout, nparts,
                       (double)b * (double)npoints * (double)nsample, partial, gm.mom, gd, w_dp, mean, invstd,
                       gamma, dgamma, dbeta, dw_dp, lddw, coef, phase, dsums, count_dev);
    if (phase == 1) return launch_status(entry);
    lagg_apply(b, cout, n, Q, g_pm, gm, w_dp, coef, dg_cm, stream);
    return launch_status(entry);
}

// Outputs besides those of lagg_forward_begin: pooled / ystar (b,cout,npoints) fp32, arg (b,cout,npoints) bytes
AMC_API int amc3d_local_aggregation_forward(int b, int cout, int n, int npoints, int nsample, int training, int relu, float eps,
                                            float momentum, const float *g_cm, const int *idx, const float *dp,
                                            const float *w_dp_, long ldw, const void *moments, const float *gamma,
                                            const float *beta, float *g_pm, float *pooled, unsigned char *arg, float *ystar,
                                            float *mean, float *invstd, float *var_unbiased, double *gd, float *running_mean,
                                            float *running_var, long long *num_batches_tracked, int phase, double *sums,
                                            void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *entry = "amc3d_local_aggregation_forward";
    const WDp w_dp{w_dp_, ldw};
    if (b > 0 && npoints > 0 && (!pooled || !arg || !ystar)) return lagg_bad(entry, "null output");
    bool done;
    if (int st = lagg_forward_begin(entry, lagg_supported, b, cout, n, npoints, nsample, training, eps, momentum, g_cm, idx, dp, w_dp,
                                    moments, gamma, beta, g_pm, mean, invstd, var_unbiased, gd, running_mean, running_var,
                                    num_batches_tracked, phase, sums, workspace, workspace_bytes, stream_, &done))
        return st;
    if (done) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const int ct = cout < LAGG_CT ? cout : LAGG_CT;
    const int cpw = lagg_pool_cpw(b, cout, npoints);
    const size_t lds = (size_t)3 * ct * (4 * cpw + 1) * sizeof(float);
#define AMC_POOL(L)                                                                                                            \
    hipLaunchKernelGGL(lagg_pool_kernel<L>, dim3(div_up(npoints, 4 * cpw), cout / ct, b), dim3(256), lds, stream, cout, n, npoints, \
                       nsample, cpw, relu, (const float *)g_pm, idx, dp, w_dp, (const float *)mean, (const float *)invstd, gamma,  \
                       beta, pooled, arg, ystar)
    switch (ct / 4) { case 2: AMC_POOL(2); break; case 4: AMC_POOL(4); break; case 8: AMC_POOL(8); break; case 16: AMC_POOL(16); break;
                      default: AMC_POOL(32); }
#undef AMC_POOL
    return launch_status(entry);
}

// Q by float atomics (rev_start == NULL), or from the reverse lists of idx (amc3d_group_csr): bit-reproducible.  Summation
// order of Q: see lagg_bwd_gather_kernel and include/amc3d.h
AMC_API int amc3d_local_aggregation_backward(int b, int cout, int n, int npoints, int nsample, int relu, const float *dpooled,
                                             const float *ystar, const unsigned char *arg, const float *g_pm, const int *idx,
                                             const float *dp, const float *w_dp_, long ldw, const void *moments,
                                             const double *gd, const float *mean, const float *invstd, const float *gamma,
                                             const float *beta, const int *rev_start, const int *rev_edge, float *dg_cm,
                                             float *dw_dp, long lddw, float *dgamma, float *dbeta, int phase, double *dsums,
                                             const double *count_dev, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *entry = "amc3d_local_aggregation_backward";
    const WDp w_dp{w_dp_, ldw};
    const bool lists = rev_start != nullptr;
    bool done;
    if (int st = lagg_backward_begin(entry, lagg_supported, b, cout, n, npoints, nsample, dpooled, g_pm, dp, w_dp, moments, gd, mean,
                                     invstd, gamma, beta, dg_cm, dw_dp, lddw, dgamma, dbeta, phase, dsums, count_dev, workspace,
                                     workspace_bytes,
                                     lists ? amc3d_local_aggregation_csr_workspace_bytes(b, cout, n, npoints)
                                           : amc3d_local_aggregation_workspace_bytes(b, cout, n, npoints), &done))
        return st;
    if (done) return 0;
    if (!ystar || !arg || !idx || (lists && (!rev_edge || (long)b * n * cout >= (1L << 39) || (long)npoints * nsample >= (1L << 31))))
        return lagg_bad(entry, "null pointer, or a shape beyond the reverse-list form");
    hipStream_t stream = (hipStream_t)stream_;
    double *partial = (double *)workspace;
    float *Q = (float *)((char *)workspace + lagg_partial_bytes(b, cout, n, npoints));
    float *coef = Q + (size_t)b * n * cout;
    const int ct = cout < LAGG_CT ? cout : LAGG_CT;
    const int stiles = lagg_scatter_tiles(b, cout, npoints);
    const int nparts_b = div_up(div_up(npoints, LAGG_MT), stiles);
    if (phase != 2) {
        size_t lds = ((size_t)3 * ct * (LAGG_MT + 1) + (size_t)4 * LAGG_MT * nsample) * sizeof(float);
        const size_t red = (size_t)4 * ct * 5 * sizeof(double);
        if (lds < red) lds = red;
        if (lists) {  // no atomics, no zero fill: the gather writes every element of Q
            float *dq_pm = coef + lagg_coef_floats(cout);
            unsigned char *arg_pm = (unsigned char *)(dq_pm + (size_t)b * npoints * cout);
            if (lds > 65536)
                (void)hipFuncSetAttribute((const void *)lagg_bwd_scatter_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(lagg_bwd_scatter_kernel<true>, dim3(nparts_b, cout / ct, b), dim3(256), lds, stream, cout, n, npoints,
                               nsample, relu, dpooled, ystar, arg, idx, dp, mean, invstd, gamma, beta, Q, partial, nparts_b, stiles,
                               dq_pm, arg_pm);
            const long total = (long)b * n * cout;
            hipLaunchKernelGGL(lagg_bwd_gather_kernel, dim3((unsigned)div_up(total, 256L)), dim3(256), 0, stream, cout, n, npoints,
                               nsample, total, (const float *)dq_pm, (const unsigned char *)arg_pm, rev_start, rev_edge, Q);
        } else {
            if (int st = fill_i32((int *)Q, 0, (size_t)b * n * cout, stream)) return st;
            if (lds > 65536)  // (128 channels x 33 x 3 images + the idx / dp rows: 67 KB; gfx950 has 160 KB per workgroup)
                (void)hipFuncSetAttribute((const void *)lagg_bwd_scatter_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(lagg_bwd_scatter_kernel<false>, dim3(nparts_b, cout / ct, b), dim3(256), lds, stream, cout, n, npoints,
                               nsample, relu, dpooled, ystar, arg, idx, dp, mean, invstd, gamma, beta, Q, partial, nparts_b, stiles,
                               (float *)nullptr, (unsigned char *)nullptr);
        }
    }
    return lagg_backward_finish(entry, b, cout, n, npoints, nsample, nparts_b * b, partial, Q, coef, g_pm, moments, gd, w_dp, mean,
                                invstd, gamma, dg_cm, dw_dp, lddw, dgamma, dbeta, phase, dsums, count_dev, stream);
}

// ---- first layer of a multi-layer SetAbstraction MLP: conv (before the gather) + BatchNorm + ReLU, x1 materialised ----
AMC_API int amc3d_grouped_conv_bn_supported(int cout, int nsample) { return lagg_expand_supported(cout, nsample) ? 1 : 0; }

// x1 (b,cout,npoints,32) = [relu](bn(G[idx] + W_dp . dp)); other arguments as amc3d_local_aggregation_forward
AMC_API int amc3d_grouped_conv_bn_forward(int b, int cout, int n, int npoints, int nsample, int training, int relu, float eps,
                                          float momentum, const float *g_cm, const int *idx, const float *dp, const float *w_dp_,
                                          long ldw, const void *moments, const float *gamma, const float *beta, float *g_pm,
                                          float *x1, float *mean, float *invstd, float *var_unbiased, double *gd,
                                          float *running_mean, float *running_var, long long *num_batches_tracked, int phase,
                                          double *sums, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *entry = "amc3d_grouped_conv_bn_forward";
    const WDp w_dp{w_dp_, ldw};
    if (b > 0 && npoints > 0 && !x1) return lagg_bad(entry, "null output");
    bool done;
    if (int st = lagg_forward_begin(entry, lagg_expand_supported, b, cout, n, npoints, nsample, training, eps, momentum, g_cm, idx, dp,
                                    w_dp, moments, gamma, beta, g_pm, mean, invstd, var_unbiased, gd, running_mean, running_var,
                                    num_batches_tracked, phase, sums, workspace, workspace_bytes, stream_, &done))
        return st;
    if (done) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const long P = (long)npoints * nsample;
    const int ct = cout < LAGG_XC ? cout : LAGG_XC;
#define AMC_EXPAND(L)                                                                                                          \
    hipLaunchKernelGGL(lagg_expand_kernel<L>, dim3(div_up(P, LAGG_PT), cout / ct, b), dim3(256), 0, stream, cout, n, P, relu, \
                       (const float *)g_pm, idx, dp, w_dp, (const float *)mean, (const float *)invstd, gamma, beta, x1)
    switch (ct / 4) { case 2: AMC_EXPAND(2); break; case 4: AMC_EXPAND(4); break; case 8: AMC_EXPAND(8); break; default: AMC_EXPAND(16); }
#undef AMC_EXPAND
    return launch_status(entry);
}

namespace amc {
int csr_collapse(int b, int cout, int n, int npoints, int nsample, int relu, const float *dx1_pm, const float *g_pm,
                 const int *rev_start, const int *rev_edge, const float *rev_dp, const float *dp, WDp w_dp,
                 const float *mean, const float *invstd, const float *gamma, const float *beta, float *Q, double *partial,
                 int *nparts, hipStream_t stream);
size_t csr_partials(int b, int cout, int n);
}

AMC_API size_t amc3d_grouped_conv_bn_csr_workspace_bytes(int b, int cout, int n, int npoints, int nsample)
{
    if (b <= 0 || cout <= 0 || n <= 0 || npoints <= 0) return 0;
    const size_t parts = csr_partials(b, cout, n);
    // partial sums | Q (b, n, cout) | coef (cout, 4) | dx1 position-major (b, P, cout)
    return parts * cout * 5 * sizeof(double) + (size_t)b * n * cout * sizeof(float) + (size_t)cout * 4 * sizeof(float) + 256 +
           (size_t)b * npoints * nsample * cout * sizeof(float);
}

// from dx1 (b,cout,npoints,32): dg_cm (b,cout,n), dw_dp (cout,3), dgamma, dbeta.  rev_start == NULL: one pass over dx1 collapses
// it into Q with float atomics.  With the reverse lists rev_start / rev_edge of amc3d_group_csr there are none: dx1 is first
// transposed to position-major (workspace) unless it comes that way, then every source point sums its incoming positions in
// list order (csrc/csr.hip): deterministic, and ~2.5x faster than the atomic scatter
AMC_API int amc3d_grouped_conv_bn_backward(int b, int cout, int n, int npoints, int nsample, int relu, const float *dx1,
                                           int dx1_position_major, const float *g_pm, const int *idx, const int *rev_start,
                                           const int *rev_edge, const float *rev_dp, const float *dp, const float *w_dp_,
                                           long ldw, const void *moments, const double *gd, const float *mean,
                                           const float *invstd, const float *gamma, const float *beta, float *dg_cm,
                                           float *dw_dp, long lddw, float *dgamma, float *dbeta, int phase, double *dsums,
                                           const double *count_dev, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *entry = "amc3d_grouped_conv_bn_backward";
    const WDp w_dp{w_dp_, ldw};
    const bool lists = rev_start != nullptr;
    bool done;
    if (int st = lagg_backward_begin(entry, lagg_expand_supported, b, cout, n, npoints, nsample, dx1, g_pm, dp, w_dp, moments, gd,
                                     mean, invstd, gamma, beta, dg_cm, dw_dp, lddw, dgamma, dbeta, phase, dsums, count_dev,
                                     workspace, workspace_bytes,
                                     lists ? amc3d_grouped_conv_bn_csr_workspace_bytes(b, cout, n, npoints, nsample)
                                           : amc3d_local_aggregation_workspace_bytes(b, cout, n, npoints), &done))
        return st;
    if (done) return 0;
    if (lists ? !rev_edge : (!idx || dx1_position_major || rev_dp))
        return lagg_bad(entry, "lists need rev_edge; without them idx, a channel-major dx1 and no rev_dp");
    hipStream_t stream = (hipStream_t)stream_;
    const long P = (long)npoints * nsample;
    const size_t parts = lists ? csr_partials(b, cout, n) : 0;
    char *w = (char *)workspace;
    double *partial = (double *)w; w += lists ? parts * cout * 5 * sizeof(double) : lagg_partial_bytes(b, cout, n, npoints);
    float *Q = (float *)w; w += (size_t)b * n * cout * sizeof(float);
    float *coef = (float *)w; w += (size_t)cout * 4 * sizeof(float);
    int nparts;
    if (lists) {
        if (P >= (1L << 31)) return lagg_bad(entry, "too many positions");
        nparts = (int)parts;
        if (phase != 2) {
            float *dx1_pm = (float *)(((uintptr_t)w + 255) & ~(uintptr_t)255);
            if (dx1_position_major) {
                if ((uintptr_t)dx1 & 15) return lagg_bad(entry, "position-major dx1 must be 16-byte aligned");
                dx1_pm = const_cast<float *>(dx1);  // read only
            } else if (int st = amc3d_transpose_cn(b, cout, (int)P, dx1, dx1_pm, stream_)) return st;  // (b, cout, P) -> (b, P, cout)
            if (rev_dp && ((uintptr_t)rev_dp & 15)) return lagg_bad(entry, "rev_dp must be 16-byte aligned");
            if (int st = csr_collapse(b, cout, n, npoints, nsample, relu, dx1_pm, g_pm, rev_start, rev_edge, rev_dp, dp, w_dp, mean,
                                      invstd, gamma, beta, Q, partial, &nparts, stream))
                return st;
        }
    } else {
        const int ct = cout < LAGG_XC ? cout : LAGG_XC;
        const int ctiles = LAGG_CTILES;
        const int nparts_b = div_up(div_up(P, LAGG_PT), ctiles);
        nparts = nparts_b * b;
        if (phase != 2) {
            if (int st = fill_i32((int *)Q, 0, (size_t)b * n * cout, stream)) return st;
#define AMC_COLLAPSE(L)                                                                                                        \
    hipLaunchKernelGGL(lagg_collapse_kernel<L>, dim3(nparts_b, cout / ct, b), dim3(256), 0, stream, cout, n, P, relu, dx1, g_pm,  \
                       idx, dp, w_dp, mean, invstd, gamma, beta, Q, partial, nparts_b, ctiles)
            switch (ct / 4) { case 2: AMC_COLLAPSE(2); break; case 4: AMC_COLLAPSE(4); break; case 8: AMC_COLLAPSE(8); break; default: AMC_COLLAPSE(16); }
#undef AMC_COLLAPSE
        }
    }
    return lagg_backward_finish(entry, b, cout, n, npoints, nsample, nparts, partial, Q, coef, g_pm, moments, gd, w_dp, mean, invstd,
                                gamma, dg_cm, dw_dp, lddw, dgamma, dbeta, phase, dsums, count_dev, stream);
}

