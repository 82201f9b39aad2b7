// k nearest (or farthest) neighbours in FEATURE space for gfx950: the graph of DynConv / EdgeConv
// (models/layers/graph_conv.py), which the reference builds as cdist + topk over a (B, M, N) matrix.
//
// Distance.  d2(i,j) = (qq_i + ss_j) - 2 * dot_ij in fp32, where dot_ij, qq_i and ss_j are fmaf chains over the
// channels in ascending order starting from 0.  v_mfma_f32_32x32x2_f32 is bit for bit such a chain (two channels per
// instruction, chained in k order), so the dot tile comes from the matrix cores and qq / ss from explicit fmaf on the
// VALU.  Channels past C are staged as zeros: fmaf(0, 0, acc) == acc, the chain is unchanged.  In a self-search
// qq_i == ss_i == dot_ii, hence d2(i,i) = 2c - 2c = 0 exactly.
//
// Order.  The list of a query is the `ksearch` smallest pairs (key, index), key = d2 (farthest: -d2), ascending.  One
// wavefront owns a query's list for the whole search and walks the support in ascending index order; a candidate
// enters iff key < the current last key (strict), behind every entry with key <= its own.  Every entry already listed
// has a smaller index than the candidate, so that IS the comparison of pairs, and the result depends on neither the
// tile shape nor the schedule.
//
// Shape.  A workgroup of NW wavefronts owns 32 * NW queries of one cloud and walks the support in tiles of 64.  Channels
// go through LDS in chunks of 32 (query chunk and support chunk, rows padded to 33 words).  Wave w accumulates the
// 32 x 64 dot block of ITS 32 queries in two independent 32x32 accumulators, turns it into keys in a wave-private LDS
// tile and scans that tile row by row: 64 candidates per step and a ballot against the row's current last key (kept in a
// lane of a register, so a row without survivors costs one LDS read and one compare).  A row with survivors takes its
// sorted list from LDS into registers (each lane holds entries lane and lane + 64), inserts them one by one (one ballot
// finds the slot, one whole-wave DPP shift makes room) and puts the list back.  No d2 ever reaches global memory, and the
// lists are sorted when the walk ends: the epilogue only strides over them (dilation), makes the distances euclidean and
// stores.
//
// LDS (bytes): lists 32 NW * ksearch * 8, key tiles NW * 32 * 65 * 4, chunks (32 NW + 64) * 33 * 4, qq / ss 128 NW + 256.
// NW = 4, ksearch = 100: 102400 + 33280 + 25344 + 768 = 161792 of 163840.  NW = 2, ksearch = 20: 10240 + 16640 + 16896
// + 512 = 44288 (three workgroups per CU).

#include "common.h"

namespace amc {

constexpr int KF_MAXK = 100;
constexpr int KF_TS = 64;       // support points per tile
constexpr int KF_CK = 32;       // channels per chunk
constexpr int KF_LD = KF_CK + 1;
constexpr int KF_TLD = KF_TS + 1;

typedef float kf_f32x16 __attribute__((ext_vector_type(16)));

static size_t kf_lds_bytes(int nw, int ksearch)
{
    const size_t tq = 32 * (size_t)nw;
    return tq * ksearch * 8 + (size_t)nw * 32 * KF_TLD * 4 + (tq + KF_TS) * KF_LD * 4 + tq * 4 + KF_TS * 4;
}

// rows [r0, r0 + nrows) x channels [c0, c0 + KF_CK) of one cloud into dst[row][KF_LD]; rows past `rows_total` and channels past
// `c` are zeros.  The lanes run along whichever of the two strides is 1, so both layouts load whole cache lines.
template <int NT>
__device__ __forceinline__ void kf_stage(float *__restrict__ dst, const float *__restrict__ src, long row_stride, long ch_stride,
                                         int r0, int nrows, int rows_total, int c0, int c)
{
    if (ch_stride == 1) {
        for (int e = threadIdx.x; e < nrows * KF_CK; e += NT) {
            const int r = e / KF_CK, ch = e % KF_CK;
            const bool ok = r0 + r < rows_total && c0 + ch < c;
            dst[r * KF_LD + ch] = ok ? src[(long)(r0 + r) * row_stride + (c0 + ch)] : 0.0f;
        }
    } else {
        for (int e = threadIdx.x; e < nrows * KF_CK; e += NT) {
            const int ch = e / nrows, r = e % nrows;
            const bool ok = r0 + r < rows_total && c0 + ch < c;
            dst[r * KF_LD + ch] = ok ? src[(long)(r0 + r) * row_stride + (long)(c0 + ch) * ch_stride] : 0.0f;
        }
    }
}

// acc = fmaf chain of row `r` of a staged chunk with itself over its first `nc` channels, continued from `acc`
__device__ __forceinline__ float kf_self_chain(const float *__restrict__ chunk, int r, int nc, float acc)
{
    for (int ch = 0; ch < nc; ++ch) {
        const float v = chunk[r * KF_LD + ch];
        acc = fmaf(v, v, acc);
    }
    return acc;
}

// value of the lane below (lane 0 keeps its own): one v_mov_b32_dpp wave_shr:1, as the lane lists of knn.hip shift
__device__ __forceinline__ int kf_lane_below(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float kf_lane_below(float x) { return __int_as_float(kf_lane_below(__float_as_int(x))); }

template <int NW>
__global__ __launch_bounds__(NW * 64) void knn_features_kernel(int n, int m, int c, int ksearch, int dilation, int farthest,
                                                               const float *__restrict__ support, long s_row, long s_ch,
                                                               const float *__restrict__ query, long q_row, long q_ch,
                                                               int *__restrict__ idx, float *__restrict__ dist, int dist_layout)
{
    constexpr int NT = NW * 64, TQ = NW * 32;
    extern __shared__ __attribute__((aligned(16))) float kf_lds[];
    float *lkey = kf_lds;                             // [TQ][ksearch]
    int *lidx = (int *)(lkey + TQ * ksearch);         // [TQ][ksearch]
    float *tile = (float *)(lidx + TQ * ksearch);     // [NW][32][KF_TLD]
    float *qc = tile + NW * 32 * KF_TLD;              // [TQ][KF_LD]
    float *sc = qc + TQ * KF_LD;                      // [KF_TS][KF_LD]
    float *qq = sc + KF_TS * KF_LD;                   // [TQ]
    float *ss = qq + TQ;                              // [KF_TS]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bi = blockIdx.y, q0 = blockIdx.x * TQ;
    const float *sup = support + (size_t)bi * n * c;
    const float *qry = query + (size_t)bi * m * c;
    const int nchunks = (c + KF_CK - 1) / KF_CK;
    const float inf = __builtin_inff();

    for (int e = threadIdx.x; e < TQ * ksearch; e += NT) { lkey[e] = inf; lidx[e] = 0; }

    // qq of the tile's queries; a single chunk then stays in qc for the whole walk
    float chain = 0.0f;
    for (int ck = 0; ck < nchunks; ++ck) {
        __syncthreads();
        kf_stage<NT>(qc, qry, q_row, q_ch, q0, TQ, m, ck * KF_CK, c);
        __syncthreads();
        if (threadIdx.x < TQ) chain = kf_self_chain(qc, threadIdx.x, min(KF_CK, c - ck * KF_CK), chain);
    }
    if (threadIdx.x < TQ) qq[threadIdx.x] = chain;

    float *mytile = tile + wave * 32 * KF_TLD;
    const int arow = (wave * 32 + (lane & 31)) * KF_LD + (lane >> 5);
    const int brow = (lane & 31) * KF_LD + (lane >> 5);
    const int nq = min(32, m - (q0 + wave * 32));  // queries of this wave that exist (<= 0: none)
    float lastv = inf;                             // lane r: the current last key of the wave's query r

    for (int t0 = 0; t0 < n; t0 += KF_TS) {
        kf_f32x16 acc0 = {0}, acc1 = {0};
        chain = 0.0f;
        for (int ck = 0; ck < nchunks; ++ck) {
            const int nc = min(KF_CK, c - ck * KF_CK);
            __syncthreads();  // the previous chunk's readers are done
            kf_stage<NT>(sc, sup, s_row, s_ch, t0, KF_TS, n, ck * KF_CK, c);
            if (nchunks > 1) kf_stage<NT>(qc, qry, q_row, q_ch, q0, TQ, m, ck * KF_CK, c);
            __syncthreads();
            if (threadIdx.x < KF_TS) {
                chain = kf_self_chain(sc, threadIdx.x, nc, chain);
                if (ck == nchunks - 1) ss[threadIdx.x] = chain;
            }
            const int steps = (nc + 1) >> 1;  // an odd tail pairs the last channel with a staged zero
            for (int kk = 0; kk < steps; ++kk) {
                const float a = qc[arow + 2 * kk];
                const float b0 = sc[brow + 2 * kk];
                const float b1 = sc[brow + 32 * KF_LD + 2 * kk];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
            }
        }
        __syncthreads();  // ss (and, before the first tile, qq) are visible
        if (nq <= 0) continue;  // uniform over the wave; the workgroup's barriers are all above

        // keys of this wave's 32 x 64 block: accumulator register r of lane l is query 4 * (l >> 5) + 8 * (r >> 2) + (r & 3),
        // support point l & 31 of its half
        {
            const int col = lane & 31;
            const float s0 = ss[col], s1 = ss[32 + col];
            const bool v0 = t0 + col < n, v1 = t0 + 32 + col < n;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 4 * (lane >> 5) + 8 * (r >> 2) + (r & 3);
                const float qv = qq[wave * 32 + row];
                const float d0 = (qv + s0) - 2.0f * acc0[r];
                const float d1 = (qv + s1) - 2.0f * acc1[r];
                mytile[row * KF_TLD + col] = v0 ? (farthest ? -d0 : d0) : inf;
                mytile[row * KF_TLD + 32 + col] = v1 ? (farthest ? -d1 : d1) : inf;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        float keyn = mytile[lane];
        for (int r = 0; r < nq; ++r) {
            const float key = keyn;
            keyn = mytile[min(r + 1, 31) * KF_TLD + lane];  // the next row is on its way while this one is fed
            float last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lastv), r));
            unsigned long long mask = __ballot(key < last);
            if (!mask) continue;
            // the row's list moves into registers for its insertions: entry `lane` in (k0, i0), entry 64 + lane in (k1, i1).
            // Slots past ksearch hold +inf and then evicted keys, all above any later candidate.
            float *keys = lkey + (wave * 32 + r) * ksearch;
            int *ids = lidx + (wave * 32 + r) * ksearch;
            const bool in0 = lane < ksearch, in1 = lane + 64 < ksearch;
            float k0 = in0 ? keys[lane] : inf, k1 = in1 ? keys[lane + 64] : inf;
            int i0 = in0 ? ids[lane] : 0, i1 = in1 ? ids[lane + 64] : 0;
            do {
                const int bpos = (int)__builtin_ctzll(mask);
                mask &= mask - 1;
                const float cand = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(key), bpos));
                if (!(cand < last)) continue;
                const int ci = t0 + bpos;
                // p0 = entries of the first 64 with key <= cand (a prefix: the list ascends); those above move up by one lane
                const int p0 = (int)__popcll(__ballot(k0 <= cand));
                if (ksearch > 64) {
                    float up1 = kf_lane_below(k1);
                    int upi1 = kf_lane_below(i1);
                    if (p0 < 64) {  // entry 63 is pushed into entry 64
                        const float top = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k0), 63));
                        const int topi = __builtin_amdgcn_readlane(i0, 63);
                        k1 = lane == 0 ? top : up1;
                        i1 = lane == 0 ? topi : upi1;
                    } else {
                        const int p1 = (int)__popcll(__ballot(k1 <= cand));
                        if (lane > p1) { k1 = up1; i1 = upi1; }
                        if (lane == p1) { k1 = cand; i1 = ci; }
                    }
                }
                const float up0 = kf_lane_below(k0);
                const int upi0 = kf_lane_below(i0);
                if (lane > p0) { k0 = up0; i0 = upi0; }
                if (lane == p0) { k0 = cand; i0 = ci; }
                last = ksearch > 64 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k1), ksearch - 65))
                                    : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k0), ksearch - 1));
            } while (mask);
            if (in0) { keys[lane] = k0; ids[lane] = i0; }
            if (in1) { keys[lane + 64] = k1; ids[lane + 64] = i1; }
            if (lane == r) lastv = last;
        }
        __builtin_amdgcn_wave_barrier();
    }

    // epilogue: columns 0, d, 2d, ... of each list; euclidean distances
    if (nq <= 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int kout = ksearch / dilation;
    const size_t row0 = (size_t)bi * m + q0 + wave * 32;
    for (int e = lane; e < nq * kout; e += 64) {
        const int r = e / kout, j = e - r * kout;
        idx[row0 * kout + e] = lidx[(wave * 32 + r) * ksearch + j * dilation];
        if (dist && dist_layout == AMC_KNN_DIST_BMK) {
            const float key = lkey[(wave * 32 + r) * ksearch + j * dilation];
            dist[row0 * kout + e] = sqrtf(fmaxf(farthest ? -key : key, 0.0f));
        }
    }
    if (dist && dist_layout == AMC_KNN_DIST_BKM) {
        for (int e = lane; e < 32 * kout; e += 64) {  // the lanes run along the queries: (b,k,m) is contiguous in them
            const int j = e >> 5, r = e & 31;
            if (r < nq) {
                const float key = lkey[(wave * 32 + r) * ksearch + j * dilation];
                dist[((size_t)bi * kout + j) * m + q0 + wave * 32 + r] = sqrtf(fmaxf(farthest ? -key : key, 0.0f));
            }
        }
    }
}

}  // namespace amc

using namespace amc;

static bool knn_features_sizes_ok(int b, int n, int m, int c, int ksearch)
{
    const long lim = 0x7fffffffL;
    return b > 0 && n > 0 && m > 0 && c > 0 && ksearch > 0 && ksearch <= KF_MAXK && (long)b * n <= lim && (long)b * m <= lim &&
           (long)b * m * ksearch <= lim && (long)n * c <= lim && (long)m * c <= lim && b <= 65535;
}

// Everything the search keeps lives in LDS.  The workspace is one reserved section, so that 0 keeps meaning "sizes out of
// range" as for the other searches and a later split of the support range has where to put its partial lists.
AMC_API size_t amc3d_knn_features_workspace_bytes(int b, int n, int m, int c, int ksearch)
{
    if (!knn_features_sizes_ok(b, n, m, c, ksearch)) return 0;
    return 256;
}

template <int NW>
static void knn_features_launch(int b, int n, int m, int c, int ksearch, int dilation, int farthest, const float *support,
                                long s_row, long s_ch, const float *query, long q_row, long q_ch, int *idx, float *dist,
                                int dist_layout, hipStream_t stream)
{
    const size_t lds = kf_lds_bytes(NW, ksearch);
    (void)hipFuncSetAttribute((const void *)knn_features_kernel<NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(knn_features_kernel<NW>, dim3(div_up(m, 32 * NW), b), dim3(NW * 64), lds, stream, n, m, c, ksearch,
                       dilation, farthest, support, s_row, s_ch, query, q_row, q_ch, idx, dist, dist_layout);
}

AMC_API int amc3d_knn_features(int b, int n, int m, int c, int ksearch, int dilation, int farthest, const float *support,
                               long s_row_stride, long s_ch_stride, const float *query, long q_row_stride, long q_ch_stride,
                               int *idx, float *dist, int dist_layout, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (b <= 0 || m <= 0) return 0;
    if (!knn_features_sizes_ok(b, n, m, c, ksearch))
        return bad_arg("amc3d_knn_features: sizes out of range (ksearch in 1..100, c >= 1, int32 products)");
    if (ksearch > n) return bad_arg("amc3d_knn_features: ksearch exceeds the number of support points");
    if (dilation <= 0 || ksearch % dilation != 0) return bad_arg("amc3d_knn_features: dilation must divide ksearch");
    if (!support || !query || !idx) return bad_arg("amc3d_knn_features: null pointer");
    // a cloud is n * c (m * c) consecutive floats in either layout: the last element read must lie inside it
    if (s_row_stride <= 0 || s_ch_stride <= 0 || q_row_stride <= 0 || q_ch_stride <= 0 ||
        (n - 1) * s_row_stride + (c - 1) * s_ch_stride >= (long)n * c || (m - 1) * q_row_stride + (c - 1) * q_ch_stride >= (long)m * c)
        return bad_arg("amc3d_knn_features: strides must be positive and stay inside a cloud of rows * c floats");
    if (dist && dist_layout != AMC_KNN_DIST_BMK && dist_layout != AMC_KNN_DIST_BKM)
        return bad_arg("amc3d_knn_features: unknown dist_layout");
    if (!workspace || workspace_bytes < amc3d_knn_features_workspace_bytes(b, n, m, c, ksearch))
        return bad_arg("amc3d_knn_features: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    // 128 queries per workgroup halve the support traffic per query; 64 keep a chip of 256 CUs filled on smaller batches
    if ((long)b * div_up(m, 128) >= 512)
        knn_features_launch<4>(b, n, m, c, ksearch, dilation, farthest, support, s_row_stride, s_ch_stride, query, q_row_stride,
                               q_ch_stride, idx, dist, dist_layout, stream);
    else
        knn_features_launch<2>(b, n, m, c, ksearch, dilation, farthest, support, s_row_stride, s_ch_stride, query, q_row_stride,
                               q_ch_stride, idx, dist, dist_layout, stream);
    return launch_status("amc3d_knn_features");
}
