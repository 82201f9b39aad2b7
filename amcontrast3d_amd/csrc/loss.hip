// Adaptive-margin contrastive loss kernels for gfx950.
//
// The reference evaluates this part of the path as a few dozen torch ops per stage plus a Python
// loop (AMContrast3D/MarginContrast.py:220-259, AEF/ambiguity.py:11-93, AEF/utils.py:11-43),
// materialising (m,23,ncls) and (m,23,C) neighbour tensors.  Here it is five kernels per stage
// that read the stage's xyz / labels / embeddings through the k-NN index and write per-point
// scalars; nothing of size m*k*C is ever stored.
//
// Arithmetic follows the reference's CPU evaluation where it is sensitive:
//  * squared distances for d+/d- use the expanded form of AEF/function.py:18-39,
//    ((-2*(x x' + y y' + z z')) + |p|^2) + |p'|^2 in fp32 without FMA and in that order --
//    the form cancels catastrophically for close points (relative error up to 1e-1), and the
//    ambiguity a_i is a steep function of it, so a "more accurate" distance would NOT match;
//  * cosine similarity is sum_c (f_i[c]/max(|f_i|,eps)) * (f_j[c]/max(|f_j|,eps)), the form
//    torch 2.x's F.cosine_similarity evaluates (MarginContrast.py:77-79).
#include "common.h"

#include <type_traits>
#include <utility>

namespace amc {

// ---------------------------------------------------------------------------------------------
// Sub-sampled stage labels: arg-max of the mean one-hot label of the kr nearest full-resolution
// points (AEF/utils.py:29-41) followed by the arg-max of MarginContrast.py:111-113 -- i.e. the
// majority class, lowest class id on equal counts.  One wavefront per point; lanes hold the
// neighbours' classes, one __ballot per class counts them.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vote_labels_kernel(int m, int kr, int ncls, const int *__restrict__ labels0,
                                                          const int *__restrict__ nbr, int *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= m) return;
    int c0 = -1, c1 = -1;  // kr <= 128
    if (lane < kr) c0 = labels0[nbr[(size_t)q * kr + lane]];
    if (lane + 64 < kr) c1 = labels0[nbr[(size_t)q * kr + lane + 64]];
    int best = -1, bestc = 0;
    for (int c = 0; c < ncls; ++c) {
        const int cnt = (int)__popcll(__ballot(c0 == c)) + (int)__popcll(__ballot(c1 == c));
        if (cnt > best) { best = cnt; bestc = c; }
    }
    if (lane == 0) out[q] = bestc;
}

// ---------------------------------------------------------------------------------------------
// Neighbourhood statistics of every point (MarginContrast.py:228-231, ambiguity.py:12,18-21,26-39):
// n+ = #neighbours of the same class, d+/d- = summed "squared distances" to the same-/other-class
// neighbours, and the global max of n+ (ambiguity.py:13 divides by it).
// nbr points at the first kept column of the (m, nbr_stride) k-NN index (the self match in
// column 0 is skipped by the caller's pointer offset, MarginContrast.py:225-226).
// ---------------------------------------------------------------------------------------------
// posmask[i,j] = (class of neighbour j) == (class of i)   (MarginContrast.py:111-115, 228-230)
__global__ void posmask_kernel(int m, int k, int nbr_stride, const int *__restrict__ labels,
                               const int *__restrict__ nbr, unsigned char *__restrict__ posmask)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)m * k) return;
    const int i = (int)(t / k), j = (int)(t - (size_t)i * k);
    posmask[t] = labels[nbr[(size_t)i * nbr_stride + j]] == labels[i] ? 1 : 0;
}

// mode: 1 = constant distance 5 (cctype Method1), 2 = "squared distance" (Method2), 3 = its root (Method3)
__global__ __launch_bounds__(256) void ambiguity_stats_kernel(int m, int k, int nbr_stride, int mode,
                                                              const float *__restrict__ p,
                                                              const unsigned char *__restrict__ posmask,
                                                              const int *__restrict__ nbr, int *__restrict__ n_pos,
                                                              float *__restrict__ d_pos, float *__restrict__ d_neg,
                                                              int *__restrict__ max_npos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int np = 0;
    if (i < m) {
        const float px = p[(size_t)i * 3], py = p[(size_t)i * 3 + 1], pz = p[(size_t)i * 3 + 2];
        const float ss = __fadd_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)), __fmul_rn(pz, pz));
        float dp = 0.f, dn = 0.f;
        for (int j = 0; j < k; ++j) {
            const int nb = nbr[(size_t)i * nbr_stride + j];
            const float qx = p[(size_t)nb * 3], qy = p[(size_t)nb * 3 + 1], qz = p[(size_t)nb * 3 + 2];
            const float dot = __fadd_rn(__fadd_rn(__fmul_rn(px, qx), __fmul_rn(py, qy)), __fmul_rn(pz, qz));
            const float sd = __fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz));
            float dd = __fadd_rn(__fadd_rn(__fmul_rn(-2.f, dot), ss), sd);
            if (mode == 3) dd = sqrtf(__fadd_rn(fabsf(dd), 1e-12f));  // ambiguity.py:49
            const bool pos = posmask[(size_t)i * k + j] != 0;
            np += pos ? 1 : 0;
            dp = __fadd_rn(dp, pos ? dd : 0.f);
            dn = __fadd_rn(dn, pos ? 0.f : dd);
        }
        n_pos[i] = np;
        d_pos[i] = mode == 1 ? 5.f : dp;  // ambiguity.py:24-25
        d_neg[i] = mode == 1 ? 5.f : dn;
    }
    // wave max, then one atomic per wave
    int w = np;
    for (int s = 32; s >= 1; s >>= 1) w = max(w, __shfl_xor(w, s, 64));
    if ((threadIdx.x & 63) == 0 && w > 0) atomicMax(max_npos, w);
}

// posmask_kernel and ambiguity_stats_kernel as ONE pass over the neighbour rows.  The stats kernel runs a thread per point:
// a wave instruction then reads 64 different rows, 96 bytes apart, and gathers 64 unrelated coordinates, k times in a row,
// after posmask_kernel has read the same rows and gathered the same neighbours' labels.  Here a workgroup takes LR_PTS
// consecutive points and the lanes run along their flattened (point, slot) pairs: a wave reads consecutive words of nbr
// (one gap per row where nbr_stride > k), gathers label and coordinates of neighbour x once, stores the mask byte and
// leaves the edge's term in LDS.  Then one lane per point adds its k terms in ascending slot order from 0.f -- the
// expressions and the order of ambiguity_stats_kernel, so n+, d+, d- and the mask carry the same bits.
constexpr int LR_PTS = 128;  // points per workgroup (LDS: 5 bytes per edge, 20 per point)

__global__ __launch_bounds__(256) void loss_rows_kernel(int m, int k, int nbr_stride, int mode, const int *__restrict__ labels,
                                                        const float *__restrict__ p, const int *__restrict__ nbr,
                                                        unsigned char *__restrict__ posmask, int *__restrict__ n_pos,
                                                        float *__restrict__ d_pos, float *__restrict__ d_neg,
                                                        int *__restrict__ max_npos)
{
    extern __shared__ float lr_lds[];  // [LR_PTS * k] edge terms | [LR_PTS * 4] x, y, z, |p|^2 | [LR_PTS] labels | mask bytes
    float *s_dd = lr_lds;
    float *s_pt = s_dd + LR_PTS * k;
    int *s_lab = (int *)(s_pt + LR_PTS * 4);
    unsigned char *s_pm = (unsigned char *)(s_lab + LR_PTS);
    const int i0 = blockIdx.x * LR_PTS;
    const int npts = min(LR_PTS, m - i0);
    if ((int)threadIdx.x < npts) {
        const size_t i = (size_t)i0 + threadIdx.x;
        const float px = p[i * 3], py = p[i * 3 + 1], pz = p[i * 3 + 2];
        s_pt[threadIdx.x * 4] = px;
        s_pt[threadIdx.x * 4 + 1] = py;
        s_pt[threadIdx.x * 4 + 2] = pz;
        s_pt[threadIdx.x * 4 + 3] = __fadd_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)), __fmul_rn(pz, pz));
        s_lab[threadIdx.x] = labels[i];
    }
    __syncthreads();
    const int nedge = npts * k;
    for (int e = threadIdx.x; e < nedge; e += 256) {
        const int il = e / k, j = e - il * k;
        const int nb = nbr[((size_t)i0 + il) * nbr_stride + j];
        const bool pos = labels[nb] == s_lab[il];
        float dd = 0.f;
        if (mode != 1) {  // (Method1 stores the constant 5: ambiguity.py:24-25)
            const float px = s_pt[il * 4], py = s_pt[il * 4 + 1], pz = s_pt[il * 4 + 2], ss = s_pt[il * 4 + 3];
            const float qx = p[(size_t)nb * 3], qy = p[(size_t)nb * 3 + 1], qz = p[(size_t)nb * 3 + 2];
            const float dot = __fadd_rn(__fadd_rn(__fmul_rn(px, qx), __fmul_rn(py, qy)), __fmul_rn(pz, qz));
            const float sd = __fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz));
            dd = __fadd_rn(__fadd_rn(__fmul_rn(-2.f, dot), ss), sd);
            if (mode == 3) dd = sqrtf(__fadd_rn(fabsf(dd), 1e-12f));  // ambiguity.py:49
        }
        posmask[(size_t)i0 * k + e] = pos ? 1 : 0;
        s_dd[e] = dd;
        s_pm[e] = pos ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x >= LR_PTS) return;  // (whole waves: LR_PTS is a multiple of 64)
    int np = 0;
    if ((int)threadIdx.x < npts) {
        const float *dd_i = s_dd + threadIdx.x * k;
        const unsigned char *pm_i = s_pm + threadIdx.x * k;
        float dp = 0.f, dn = 0.f;
        for (int j = 0; j < k; ++j) {
            const float dd = dd_i[j];
            const bool pos = pm_i[j] != 0;
            np += pos ? 1 : 0;
            dp = __fadd_rn(dp, pos ? dd : 0.f);
            dn = __fadd_rn(dn, pos ? 0.f : dd);
        }
        const size_t i = (size_t)i0 + threadIdx.x;
        n_pos[i] = np;
        d_pos[i] = mode == 1 ? 5.f : dp;
        d_neg[i] = mode == 1 ? 5.f : dn;
    }
    // wave max, then one atomic per wave
    int w = np;
    for (int s = 32; s >= 1; s >>= 1) w = max(w, __shfl_xor(w, s, 64));
    if ((threadIdx.x & 63) == 0 && w > 0) atomicMax(max_npos, w);
}

// a_i (ambiguity.py:13-14, 56-61, 71): |n+ - max|/max; for 0 < n+ < max:
// 1 / (1 + e^(beta * (n+/d+ - n-/d-)))  with e = fp32(math.e) raised by pow as torch does
__global__ void ambiguity_kernel(int m, int k, float beta, const int *__restrict__ n_pos,
                                 const float *__restrict__ d_pos, const float *__restrict__ d_neg,
                                 const int *__restrict__ max_npos, float *__restrict__ a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int top = *max_npos;
    const int np = n_pos[i];
    float v = __fdiv_rn((float)abs(np - top), (float)top);
    if (0 < np && np < top) {
        const float cc = __fsub_rn(__fdiv_rn((float)np, d_pos[i]), __fdiv_rn((float)(k - np), d_neg[i]));
        v = __fdiv_rn(1.f, __fadd_rn(1.f, powf(2.718281828459045f, __fmul_rn(beta, cc))));
    }
    a[i] = v;
}

// max(||f_i||_2, eps) per row (F.cosine_similarity's clamp_min(eps), eps = 1e-8)
__global__ __launch_bounds__(256) void row_norm_kernel(int m, int C, const float *__restrict__ f,
                                                       float *__restrict__ norm)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = f[(size_t)i * C + c];
        s += v * v;
    }
    for (int sft = 32; sft >= 1; sft >>= 1) s += __shfl_xor(s, sft, 64);
    if (lane == 0) norm[i] = fmaxf(sqrtf(s), 1e-8f);
}

// the same norm and the UNIT rows h_i = f_i / max(||f_i||, eps) (C == 4 * LPR, LPR lanes per row, 16-byte pieces).  The
// contrast kernels below gather h instead of f: the four IEEE divisions per lane and fetched row -- 40 of the ~85 VALU
// instructions a round of rows cost; the kernels were VALU-bound, not gather-bound: with every gather redirected to the
// anchor's own row they took the same time -- are done once per row here, and no neighbour norm is fetched.
template <int LPR>
__global__ __launch_bounds__(256) void row_unit_kernel(int m, const float *__restrict__ f, float *__restrict__ norm,
                                                       float *__restrict__ unit)
{
    const int q = threadIdx.x & (LPR - 1);
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) / LPR;
    if (i >= m) return;  // (whole LPR-lane groups leave together: the shuffles below stay inside a group)
    float4 v = reinterpret_cast<const float4 *>(f)[i * LPR + q];
    float s = v.x * v.x;
    s += v.y * v.y;
    s += v.z * v.z;
    s += v.w * v.w;
#pragma unroll
    for (int d = LPR / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    const float n = fmaxf(sqrtf(s), 1e-8f);
    v.x = __fdiv_rn(v.x, n); v.y = __fdiv_rn(v.y, n); v.z = __fdiv_rn(v.z, n); v.w = __fdiv_rn(v.w, n);
    reinterpret_cast<float4 *>(unit)[i * LPR + q] = v;
    if (q == 0) norm[i] = n;
}

// the same from CHANNEL-major embeddings f_cm (B, C, n), as the decoder leaves them (pointnext_AA.py:518-519 makes the
// point-major copy the loss reads with flatten(transpose)): a 64-point tile goes through LDS, the row-major f is never
// written.  Same arithmetic and summation order as row_unit_kernel.
// TP points per tile (16 at the wide, short stages: a cloud of 375 points is 24 tiles, not 6)
template <int LPR> constexpr int unit_tile_points() { return LPR >= 32 ? 16 : 64; }

// one tile: the points n0 .. n0 + TP of cloud b; s_tile = [C][TP + 1] floats of LDS
template <int LPR, int TP>
__device__ __forceinline__ void row_unit_cm_tile(float *s_tile, int n, int b, int n0, const float *__restrict__ f_cm,
                                                 float *__restrict__ norm, float *__restrict__ unit)
{
    constexpr int C = 4 * LPR, TS = TP + 1;
    for (int e = threadIdx.x; e < C * TP; e += 256) {
        const int ch = e / TP, pt = e - ch * TP;
        s_tile[ch * TS + pt] = n0 + pt < n ? f_cm[((size_t)b * C + ch) * n + n0 + pt] : 0.f;
    }
    __syncthreads();
    const int q = threadIdx.x & (LPR - 1);
    for (int pl = threadIdx.x / LPR; pl < TP; pl += 256 / LPR) {  // (the same trip count for every thread)
        float4 v = make_float4(s_tile[(4 * q) * TS + pl], s_tile[(4 * q + 1) * TS + pl], s_tile[(4 * q + 2) * TS + pl],
                               s_tile[(4 * q + 3) * TS + pl]);
        float s = v.x * v.x;
        s += v.y * v.y;
        s += v.z * v.z;
        s += v.w * v.w;
#pragma unroll
        for (int d = LPR / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        const float nv = fmaxf(sqrtf(s), 1e-8f);
        v.x = __fdiv_rn(v.x, nv); v.y = __fdiv_rn(v.y, nv); v.z = __fdiv_rn(v.z, nv); v.w = __fdiv_rn(v.w, nv);
        if (n0 + pl < n) {
            const size_t i = (size_t)b * n + n0 + pl;
            reinterpret_cast<float4 *>(unit)[i * LPR + q] = v;
            if (q == 0) norm[i] = nv;
        }
    }
}

template <int LPR, int TP>
__global__ __launch_bounds__(256) void row_unit_cm_kernel(int n, const float *__restrict__ f_cm, float *__restrict__ norm,
                                                          float *__restrict__ unit)
{
    extern __shared__ float s_tile[];  // [C][TP + 1]
    row_unit_cm_tile<LPR, TP>(s_tile, n, blockIdx.y, blockIdx.x * TP, f_cm, norm, unit);
}

// ---------------------------------------------------------------------------------------------
// What the contrast kernels share.  Several of them must agree to the bit -- contrast_sim_* with contrast_forward_*, the
// mutual backward's recomputed cosine with the forward's, the per-edge gradient expressions with each other -- so every
// expression, walk and rule below exists once and the kernels call it.  The library is built with -ffp-contract=off: what
// is written here is what runs, in this order.
// ---------------------------------------------------------------------------------------------
// the anchors that enter the loss (MarginContrast.py:250-252)
__device__ __forceinline__ bool contrast_selected(float a) { return 0.f < a && a <= 1.f; }

// Prologue of a kernel that runs one lane group per anchor: group w -> anchor i and its ambiguity ai; false past the end.
// sel = the list of select_anchors below; sel == nullptr: every anchor is visited, and the caller tests ai.
__device__ __forceinline__ bool contrast_anchor(const int *__restrict__ sel, int m, int w, const float *__restrict__ a, int &i,
                                                float &ai)
{
    if (w >= (sel ? sel[0] : m)) return false;
    i = sel ? sel[1 + w] : w;
    ai = a[i];
    return true;
}

// the default form (margin 'adaptive', db '-m', Method1, a temperature): margin of an anchor, exponential of a slot, and
// the factor of dl/ds_j common to an anchor's slots, -scale / ((r + eps) S^2 T) with r = P/S (an anchor without a positive
// neighbour, P == 0, has a constant loss and a zero gradient: the callers test that and do not use the factor)
__device__ __forceinline__ float contrast_margin(float mu, float a, float nu) { return __fadd_rn(__fmul_rn(mu, a), nu); }

__device__ __forceinline__ float contrast_exp(float s, bool pos, float margin, float temperature)
{
    return expf(__fdiv_rn(pos ? __fsub_rn(s, margin) : s, temperature));
}

__device__ __forceinline__ float contrast_coef(float scale, float psum, float tsum, float temperature)
{
    const float r = psum / tsum;
    return -scale / ((r + 1e-12f) * tsum * tsum * temperature);
}

// dL/ds_j of slot j: coef e_j N on a positive, -coef e_j P on a negative
__device__ __forceinline__ float contrast_edge_g(float coef, float e, bool pos, float nsum, float psum)
{
    return coef * e * (pos ? nsum : -psum);
}

// sum over the 32 lanes of an anchor's group (two groups per wave; xor below 32 stays inside one)
__device__ __forceinline__ float group32_sum(float v)
{
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// P, N and S of one anchor from its stored cosines, 32 lanes per anchor: slot-local sums over the rounds of 32 slots, then a
// tree over the lanes (the forward kernels fold their slots in another fixed order; any such order is within rounding of
// this one).  N = S - P is summed on its own: a positive's coefficient is proportional to it, and tsum - psum loses it to
// cancellation when the positives dominate (low temperature, r near 1).  Every lane of the group returns the same values.
struct ContrastSums { float psum, nsum, tsum; };

__device__ __forceinline__ ContrastSums contrast_sums32(int k, int sub, const unsigned char *__restrict__ pm_i,
                                                        const float *__restrict__ sim_i, float margin, float temperature)
{
    ContrastSums r{0.f, 0.f, 0.f};
    for (int j = sub; j < k; j += 32) {
        const bool pos = pm_i[j] != 0;
        const float e = contrast_exp(sim_i[j], pos, margin, temperature);
        r.psum += pos ? e : 0.f;
        r.nsum += pos ? 0.f : e;
        r.tsum += e;
    }
    for (int s = 16; s >= 1; s >>= 1) {
        r.psum += __shfl_xor(r.psum, s, 64);
        r.nsum += __shfl_xor(r.nsum, s, 64);
        r.tsum += __shfl_xor(r.tsum, s, 64);
    }
    return r;
}

// The cosine of two raw rows, sum_c (fi[c] / ni) * (fj[c] / nj), any C: four partial sums (a chain of C / 4 additions each,
// not of C: the cosine's rounding error is multiplied by 1 / T in the exponent)
__device__ __forceinline__ float row_cosine(const float *__restrict__ fi, const float *__restrict__ fj, float ni, float nj, int C)
{
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if ((C & 3) == 0) {
        for (int c = 0; c < C; c += 4) {
            const float4 u = *reinterpret_cast<const float4 *>(fi + c);
            const float4 v = *reinterpret_cast<const float4 *>(fj + c);
            a0 += __fdiv_rn(u.x, ni) * __fdiv_rn(v.x, nj);
            a1 += __fdiv_rn(u.y, ni) * __fdiv_rn(v.y, nj);
            a2 += __fdiv_rn(u.z, ni) * __fdiv_rn(v.z, nj);
            a3 += __fdiv_rn(u.w, ni) * __fdiv_rn(v.w, nj);
        }
    } else {
        int c = 0;
        for (; c + 3 < C; c += 4) {
            a0 += __fdiv_rn(fi[c], ni) * __fdiv_rn(fj[c], nj);
            a1 += __fdiv_rn(fi[c + 1], ni) * __fdiv_rn(fj[c + 1], nj);
            a2 += __fdiv_rn(fi[c + 2], ni) * __fdiv_rn(fj[c + 2], nj);
            a3 += __fdiv_rn(fi[c + 3], ni) * __fdiv_rn(fj[c + 3], nj);
        }
        for (; c < C; ++c) a0 += __fdiv_rn(fi[c], ni) * __fdiv_rn(fj[c], nj);
    }
    return (a0 + a1) + (a2 + a3);
}

// four channels of the cosine of two unit rows: one multiply and three fused multiply-adds, the same in the forward and in
// the backward that recomputes it
__device__ __forceinline__ float unit_dot4(const float4 &a, const float4 &b)
{
    return __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmul_rn(a.x, b.x))));
}

// The gather over UNIT rows (C == 4 * LPR): LPR lanes read one row as 16-byte pieces, so every wave instruction fetches
// R = 64/LPR whole rows (full 64-byte sectors), UNIT_U such rounds in flight.  The cosine of a slot is four products and a
// tree over the row's LPR lanes; every lane of the row then holds it.
constexpr int UNIT_U = 4;  // rounds in flight (LPR >= UNIT_U: lane q < UNIT_U of a row owns the row's slot of round q)

// rows x[0..UNIT_U) (-1: none) against the row whose piece q this lane holds in u: v = the fetched pieces, s = the cosines
template <int LPR>
__device__ __forceinline__ void unit_row_cosines(const float4 *__restrict__ h4, const float4 &u, int q, const int (&x)[UNIT_U],
                                                 float4 (&v)[UNIT_U], float (&s)[UNIT_U])
{
#pragma unroll
    for (int t = 0; t < UNIT_U; ++t) v[t] = x[t] >= 0 ? h4[(unsigned)x[t] * (unsigned)LPR + (unsigned)q] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < UNIT_U; ++t) {
        float acc = unit_dot4(u, v[t]);
#pragma unroll
        for (int d = LPR / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
        s[t] = acc;
    }
}

// One step of anchor i's walk over its neighbour list, in two halves so that a caller can issue its own per-slot loads
// between the index loads and the row loads (the fused forward reads the slot's mask there; the order of the loads is part
// of the generated code).  unit_gather_indices: the neighbours in the slots j0 + t * R + r of the rounds t < UNIT_U (-1 past
// the end).  unit_gather_rows: their rows fetched, -> the cosine of the slot THIS lane owns, jq = j0 + q * R + r (meaningful
// where q < UNIT_U and jq < k): a slot's exponential is then evaluated once, by lane q = t of row r, not by all LPR lanes of
// the row in every round.
template <int LPR>
__device__ __forceinline__ void unit_gather_indices(const int *__restrict__ nbr, int i, int nbr_stride, int k, int j0, int r,
                                                    int (&nb)[UNIT_U])
{
#pragma unroll
    for (int t = 0; t < UNIT_U; ++t) {
        const int j = j0 + t * (64 / LPR) + r;
        nb[t] = j < k ? nbr[(size_t)i * nbr_stride + j] : -1;
    }
}

template <int LPR>
__device__ __forceinline__ float unit_gather_rows(const float4 *__restrict__ h4, const float4 &u, int q, const int (&nb)[UNIT_U])
{
    float4 v[UNIT_U];
    float c[UNIT_U];
    unit_row_cosines<LPR>(h4, u, q, nb, v, c);
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < UNIT_U; ++t) s = q == t ? c[t] : s;
    return s;
}

// A row below the norm clamp (|f| < eps: norm[] holds eps) has fhat = f / eps, linear in f: its derivative is fhat_j / eps, with
// no projection term -- what autograd gives for x / clamp_min(|x|, eps).  All backward forms drop s_j fhat there.  They
// see the clamped norm only (the test is norm > eps), so a row whose norm is eps to the bit counts as clamped, where
// clamp_min's gradient would still pass: one fp32 value of the norm.
__device__ __forceinline__ float contrast_projection(float norm, float s) { return norm > 1e-8f ? s : 0.f; }

// The float-atomic edge walk of contrast_backward_kernel and contrast_backward_edges_kernel: LPA lanes per anchor i, lane
// `sub` owns channels sub, sub + LPA, ... (VPT of them, C <= LPA * VPT); the neighbours are walked one at a time so every
// atomic wave-instruction adds LPA contiguous floats of one row (the shape global float atomics run at full rate for), U
// neighbour rows in flight ahead of the atomics.  The caller produces a chunk of LPA neighbours -- lane `sub` holds what
// neighbour j0 + sub needs that is not a row: its index nb_l, cosine sj_l, norm nj_l and coefficient g_l = dL/ds_j, one
// round trip for the chunk -- and chunk() broadcasts those by shuffle.
//   ds_j/df_i = (fhat_j - s_j fhat_i)/|f_i|,  ds_j/df_j = (fhat_i - s_j fhat_j)/|f_j|   (contrast_projection below the clamp)
template <int LPA, int VPT>
struct EdgeWalk {
    static constexpr int U = VPT >= 8 ? 2 : (VPT >= 4 ? 4 : 8);  // neighbour rows in flight
    float fhi[VPT], gi[VPT];

    __device__ __forceinline__ void begin(int C, int sub, const float *__restrict__ f, int i, float ni)
    {
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int c = sub + v * LPA;
            fhi[v] = c < C ? __fdiv_rn(f[(size_t)i * C + c], ni) : 0.f;
            gi[v] = 0.f;
        }
    }

    // cnt = the chunk's neighbours (<= LPA)
    __device__ __forceinline__ void chunk(int C, int sub, const float *__restrict__ f, float ni, int cnt, int nb_l, float sj_l,
                                          float nj_l, float g_l, float *__restrict__ grad_f)
    {
        for (int jj = 0; jj < cnt; jj += U) {
            int nb[U];
            float fj[U][VPT];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = min(jj + u, LPA - 1);
                const int t = __shfl(nb_l, src, LPA);
                nb[u] = jj + u < cnt ? t : -1;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int c = sub + v * LPA;
                    fj[u][v] = (nb[u] >= 0 && c < C) ? f[(size_t)nb[u] * C + c] : 0.f;
                }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = min(jj + u, LPA - 1);
                const float g = __shfl(g_l, src, LPA), sj = __shfl(sj_l, src, LPA), nj = __shfl(nj_l, src, LPA);
                if (nb[u] < 0) continue;
                const float gin = g / ni, gjn = g / nj;
                const float si = contrast_projection(ni, sj), sx = contrast_projection(nj, sj);
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int c = sub + v * LPA;
                    if (c < C) {
                        const float fhj = __fdiv_rn(fj[u][v], nj);
                        gi[v] += gin * (fhj - si * fhi[v]);
                        atomicAdd(grad_f + (size_t)nb[u] * C + c, gjn * (fhi[v] - sx * fhj));
                    }
                }
            }
        }
    }

    __device__ __forceinline__ void finish(int C, int sub, int i, float *__restrict__ grad_f)
    {
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int c = sub + v * LPA;
            if (c < C) atomicAdd(grad_f + (size_t)i * C + c, gi[v]);
        }
    }
};

// The reverse-list gather of the rows kernels.  Edge t of row n: its own slot t < own (x = neighbour t of n), else entry
// t - own of its reverse list (the position i * k + j of an anchor i whose j-th neighbour is n: x = i) -> the other end x,
// g = dL/ds and s = the cosine of that edge; x = -1 past the end.
__device__ __forceinline__ void rows_edge(int t, int total, int own, int n, int k, const int *__restrict__ nbr_n,
                                          const int *__restrict__ rev_n, const float *__restrict__ gco,
                                          const float *__restrict__ sim, int &x, float &g, float &s)
{
    x = -1; g = 0.f; s = 0.f;
    if (t < total) {
        int pos;
        if (t < own) { pos = n * k + t; x = nbr_n[t]; }
        else { pos = rev_n[t - own]; x = pos / k; }
        g = gco[pos];
        s = sim[pos];
    }
}

// acc += g/|f_n| * (f_x / |f_x| - s * fhat_n) on four channels (fn = the piece of fhat_n, v of the raw row f_x)
__device__ __forceinline__ void rows_accumulate(float4 &acc, float g, float s, float nn, const float4 &fn, const float4 &v, float nx)
{
    const float gn = g / nn;
    const float sn = contrast_projection(nn, s);
    acc.x += gn * (__fdiv_rn(v.x, nx) - sn * fn.x);
    acc.y += gn * (__fdiv_rn(v.y, nx) - sn * fn.y);
    acc.z += gn * (__fdiv_rn(v.z, nx) - sn * fn.z);
    acc.w += gn * (__fdiv_rn(v.w, nx) - sn * fn.w);
}

// ---------------------------------------------------------------------------------------------
// The anchors that enter the loss, 0 < a <= 1 (MarginContrast.py:250-252), as a compact ascending list:
// sel[0] = count, sel[1..count] = anchor ids, sel[m+1..] = per-256-block counts (scratch).  The list depends on
// coordinates and labels only, so it is built with the stage's plan; the contrast kernels then run one full
// wave per SELECTED anchor instead of testing a_i per anchor (two thirds of the full-resolution points on the synthetic
// rooms, nearly all at the coarse stages).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_count_kernel(int m, const float *__restrict__ a, int *__restrict__ sel)
{
    __shared__ int s_cnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool s = i < m && contrast_selected(a[i]);
    const int c = (int)__popcll(__ballot(s));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) sel[(size_t)m + 1 + blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void select_write_kernel(int m, const float *__restrict__ a, int *__restrict__ sel)
{
    __shared__ int s_part[4], s_cnt[4];
    const int *bc = sel + (size_t)m + 1;
    int before = 0;  // selected anchors in the blocks in front of this one
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) before += bc[b];
    for (int s = 32; s >= 1; s >>= 1) before += __shfl_xor(before, s, 64);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool sl = i < m && contrast_selected(a[i]);
    const unsigned long long mask = __ballot(sl);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_part[wv] = before; s_cnt[wv] = (int)__popcll(mask); }
    __syncthreads();
    int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int w = 0; w < wv; ++w) base += s_cnt[w];
    if (sl) sel[1 + base + (int)__popcll(mask & ((1ull << lane) - 1ull))] = i;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        sel[0] = s_part[0] + s_part[1] + s_part[2] + s_part[3] + s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ---------------------------------------------------------------------------------------------
// Contrast forward, one wave per anchor (C == 4 * LPR) over the UNIT rows (unit_gather_indices / unit_gather_rows above).
// Same per-element arithmetic as contrast_forward_kernel below (u_c / n_i * (v_c / n_x), channel order of the tree).
// sel == nullptr: every anchor is visited and tested.
// ---------------------------------------------------------------------------------------------
// the wave of anchor group w (w = 4 * block + wave of the block)
template <int LPR>
__device__ __forceinline__ void contrast_forward_unit_wave(
    int w, int m, int k, int nbr_stride, const float *__restrict__ unit, const int *__restrict__ nbr,
    const unsigned char *__restrict__ posmask, const float *__restrict__ a, const int *__restrict__ sel, float mu, float nu,
    float temperature, float *__restrict__ sim, float *__restrict__ stats, float *__restrict__ loss_pt)
{
    constexpr int R = 64 / LPR;  // rows per round
    const int lane = threadIdx.x & 63, q = lane & (LPR - 1), r = lane / LPR;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, w, a, i, ai)) return;
    if (!contrast_selected(ai)) {
        if (lane == 0) loss_pt[i] = 0.f;
        return;
    }
    const float margin = contrast_margin(mu, ai, nu);
    const float4 *h4 = reinterpret_cast<const float4 *>(unit);
    const float4 u = h4[(size_t)i * LPR + q];
    float psum = 0.f, tsum = 0.f, nsum = 0.f;
    for (int j0 = 0; j0 < k; j0 += UNIT_U * R) {
        int nb[UNIT_U];
        unit_gather_indices<LPR>(nbr, i, nbr_stride, k, j0, r, nb);
        const int jq = j0 + q * R + r;  // the slot this lane evaluates
        const bool mine = q < UNIT_U && jq < k;
        const bool pos = mine ? posmask[(size_t)i * k + jq] != 0 : false;
        const float s = unit_gather_rows<LPR>(h4, u, q, nb);
        if (mine) {
            if (sim) sim[(size_t)i * k + jq] = s;
            const float e = contrast_exp(s, pos, margin, temperature);
            psum += pos ? e : 0.f;
            nsum += pos ? 0.f : e;
            tsum += e;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        psum += __shfl_xor(psum, d, 64);
        tsum += __shfl_xor(tsum, d, 64);
    }
    if (stats) {  // (kernel-uniform) the negatives' sum on its own: tsum - psum would lose it where the positives dominate
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) nsum += __shfl_xor(nsum, d, 64);
    }
    if (lane == 0) {
        loss_pt[i] = -logf(__fadd_rn(__fdiv_rn(psum, tsum), 1e-12f));
        if (stats) { stats[(size_t)i * 2] = psum; stats[(size_t)i * 2 + 1] = nsum; }  // what the backward's records need of this pass
    }
}

template <int LPR>
__global__ __launch_bounds__(256) void contrast_forward_unit_kernel(
    int m, int k, int nbr_stride, const float *__restrict__ unit, const int *__restrict__ nbr,
    const unsigned char *__restrict__ posmask, const float *__restrict__ a, const int *__restrict__ sel, float mu, float nu,
    float temperature, float *__restrict__ sim, float *__restrict__ stats, float *__restrict__ loss_pt)
{
    contrast_forward_unit_wave<LPR>(blockIdx.x * 4 + (threadIdx.x >> 6), m, k, nbr_stride, unit, nbr, posmask, a, sel, mu, nu,
                                    temperature, sim, stats, loss_pt);
}

// ---------------------------------------------------------------------------------------------
// Contrast forward (MarginContrast.py:250-257, 117-174 with margin 'adaptive', db '-m', Method1):
// 32 lanes per anchor, lane j owns neighbour j (k <= 32 per round); the anchor row is a broadcast
// load, the neighbour row a per-lane 16-byte stream that stays in L1 across the channel loop.
// Writes the cosine similarities (for the backward) and the per-anchor loss; anchors outside
// 0 < a <= 1 (perfectly consistent neighbourhoods) contribute nothing.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void contrast_forward_kernel(
    int m, int C, int k, int nbr_stride, const float *__restrict__ f, const float *__restrict__ norm,
    const int *__restrict__ nbr, const unsigned char *__restrict__ posmask, const float *__restrict__ a,
    const int *__restrict__ sel, float mu, float nu, float temperature, float *__restrict__ sim,
    float *__restrict__ loss_pt)
{
    const int sub = threadIdx.x & 31;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) >> 5, a, i, ai)) return;
    if (!contrast_selected(ai)) {
        if (sub == 0) loss_pt[i] = 0.f;
        return;
    }
    const float ni = norm[i];
    const float margin = contrast_margin(mu, ai, nu);
    const float *fi = f + (size_t)i * C;
    float psum = 0.f, tsum = 0.f;
    for (int j0 = 0; j0 < k; j0 += 32) {
        const int j = j0 + sub;
        float e = 0.f;
        bool pos = false;
        if (j < k) {
            const int nb = nbr[(size_t)i * nbr_stride + j];
            const float nj = norm[nb];
            const float acc = row_cosine(fi, f + (size_t)nb * C, ni, nj, C);
            sim[(size_t)i * k + j] = acc;
            pos = posmask[(size_t)i * k + j] != 0;
            e = contrast_exp(acc, pos, margin, temperature);
        }
        psum += pos ? e : 0.f;
        tsum += e;
    }
    for (int s = 16; s >= 1; s >>= 1) {
        psum += __shfl_xor(psum, s, 64);
        tsum += __shfl_xor(tsum, s, 64);
    }
    if (sub == 0) loss_pt[i] = -logf(__fadd_rn(__fdiv_rn(psum, tsum), 1e-12f));
}

// mean of loss_pt over the selected anchors, deterministically (one workgroup, fixed order):
// out[0] = sum / count, out[1] = count.  torch.mean of an empty selection is NaN in the
// reference; so is 0/0 here.
// (the 1024 threads of one workgroup; thread 0 returns out[0], the others 0)
__device__ __forceinline__ float masked_mean_block(double (&s_sum)[16], int (&s_cnt)[16], int m, const float *__restrict__ loss_pt,
                                                   const float *__restrict__ a, float *__restrict__ out)
{
    double sum = 0.0;
    int cnt = 0;
    // one workgroup (fixed order, no workspace): keep many 16-byte loads in flight per thread instead of a
    // dependent scalar load per element
    const int m4 = ((((uintptr_t)loss_pt | (uintptr_t)a) & 15) == 0) ? (m & ~3) : 0;
    for (int i0 = threadIdx.x * 4; i0 < m4; i0 += 4096 * 4) {
        float4 lv[4], av[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 4096;
            const bool ok = i < m4;
            lv[u] = ok ? *reinterpret_cast<const float4 *>(loss_pt + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            av[u] = ok ? *reinterpret_cast<const float4 *>(a + i) : make_float4(-1.f, -1.f, -1.f, -1.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float l4[4] = {lv[u].x, lv[u].y, lv[u].z, lv[u].w}, a4[4] = {av[u].x, av[u].y, av[u].z, av[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (contrast_selected(a4[e])) { sum += (double)l4[e]; cnt += 1; }
        }
    }
    for (int i = m4 + threadIdx.x; i < m; i += 1024) {
        const float ai = a[i];
        if (contrast_selected(ai)) { sum += (double)loss_pt[i]; cnt += 1; }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        sum += __shfl_xor(sum, s, 64);
        cnt += __shfl_xor(cnt, s, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    float mean = 0.f;
    if (threadIdx.x == 0) {
        double t = 0.0;
        int c = 0;
        for (int w = 0; w < 16; ++w) { t += s_sum[w]; c += s_cnt[w]; }
        mean = (float)(t / (double)c);
        out[0] = mean;
        out[1] = (float)c;
    }
    return mean;
}

__global__ __launch_bounds__(1024) void masked_mean_kernel(int m, const float *__restrict__ loss_pt,
                                                           const float *__restrict__ a, float *__restrict__ out)
{
    __shared__ double s_sum[16];
    __shared__ int s_cnt[16];
    masked_mean_block(s_sum, s_cnt, m, loss_pt, a, out);
}

// ---------------------------------------------------------------------------------------------
// Contrast backward: d(mean loss)/d f by float atomics (EdgeWalk above: LPA lanes per anchor, neighbours one at a time).
//   l = -log(r + eps), r = P/S, e_j = exp(s'_j / T):  dl/ds_j = -(e_j (pos_j S - P)) / ((r+eps) S^2 T)
// Where the time goes (contrast_bench.py, S3DIS-like batch, 66-99 % of the anchors listed): the
// kernel adds 387 / 229 / 134 / 73 MB of rows at the four stages in 0.33 / 0.20 / 0.12 / 0.06 ms = 1.15-1.17 TB/s, the
// chip-wide float-atomic rate (MI355X_MICROARCH.md: 1.26-1.36 TB/s); without the neighbour-row atomics it takes a third
// of that, without the gathers the same.  Splitting an anchor's neighbours over several lane groups (tried for the deep
// stages) only adds prologues: +15-25 %.
// Memory-level parallelism: lane j of the group first loads everything neighbour j needs that is not a row
// (its index, norm, similarity, mask -- one round trip for all k), the walk then broadcasts those by shuffle and
// keeps U neighbour rows in flight ahead of the atomics.  sel as in the forward.
// ---------------------------------------------------------------------------------------------
template <int LPA, int VPT>
__global__ __launch_bounds__(256) void contrast_backward_kernel(
    int m, int C, int k, int nbr_stride, const float *__restrict__ f, const float *__restrict__ norm,
    const int *__restrict__ nbr, const unsigned char *__restrict__ posmask, const float *__restrict__ a,
    const int *__restrict__ sel, float mu, float nu, float temperature, const float *__restrict__ sim,
    const float *__restrict__ mean_cnt, const float *__restrict__ grad_out, float *__restrict__ grad_f)
{
    const int sub = threadIdx.x & (LPA - 1);
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) / LPA, a, i, ai)) return;
    if (!contrast_selected(ai)) return;
    const float scale = grad_out[0] / mean_cnt[1];
    const float ni = norm[i];
    const float margin = contrast_margin(mu, ai, nu);

    EdgeWalk<LPA, VPT> walk;
    walk.begin(C, sub, f, i, ni);
    // lane `sub` holds neighbour j0 + sub of the current chunk of LPA neighbours
    int nb_l = -1;
    bool pos_l = false;
    float sj_l = 0.f, nj_l = 1.f, e_l = 0.f;
    auto load_chunk = [&](int j0) {
        const int j = j0 + sub;
        nb_l = -1; pos_l = false; sj_l = 0.f; nj_l = 1.f; e_l = 0.f;
        if (j < k) {
            nb_l = nbr[(size_t)i * nbr_stride + j];
            pos_l = posmask[(size_t)i * k + j] != 0;
            sj_l = sim[(size_t)i * k + j];
            nj_l = norm[nb_l];
            e_l = contrast_exp(sj_l, pos_l, margin, temperature);
        }
    };
    // P and S over all neighbours, and the negatives' share S - P summed on its own (see contrast_sums32)
    float psum = 0.f, tsum = 0.f, nsum = 0.f;
    for (int j0 = (k - 1) / LPA * LPA; j0 >= 0; j0 -= LPA) {  // ends on chunk 0, which the walk starts with
        load_chunk(j0);
        psum += pos_l ? e_l : 0.f;
        nsum += pos_l ? 0.f : e_l;
        tsum += e_l;
    }
#pragma unroll
    for (int s = LPA / 2; s >= 1; s >>= 1) {
        psum += __shfl_xor(psum, s, 64);
        nsum += __shfl_xor(nsum, s, 64);
        tsum += __shfl_xor(tsum, s, 64);
    }
    const float coef = contrast_coef(scale, psum, tsum, temperature);
    if (psum == 0.f) return;  // no positive neighbour: constant loss, zero gradient

    for (int j0 = 0; j0 < k; j0 += LPA) {
        if (j0 > 0) load_chunk(j0);
        const float g_l = contrast_edge_g(coef, e_l, pos_l, nsum, psum);
        walk.chunk(C, sub, f, ni, min(LPA, k - j0), nb_l, sj_l, nj_l, g_l, grad_f);
    }
    walk.finish(C, sub, i, grad_f);
}

// ---------------------------------------------------------------------------------------------
// Contrast backward as a gather (no float atomics, fixed summation order, every row of grad_f written once).
// With g_ij = dL/ds_ij (0 for anchors that are not selected or have no positive neighbour) both halves of the gradient
// have one form:   dL/df_n = sum over edges (n, x) of  g/|f_n| * (fhat_x - s * fhat_n)
//   own edges       x = neighbour j of n           (g, s) = (g_nj, s_nj)       when n is a selected anchor
//   incoming edges  x = anchor i with nbr[i,j] = n (g, s) = (g_ij, s_ij)       listed in rev (amc3d_contrast_csr)
// contrast_coef_kernel writes g for the selected anchors; contrast_backward_rows_kernel walks, one wave per row n
// (C == 4 * LPR, 64/LPR edges per round, U rounds of rows in flight), both edge sets and stores the row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void contrast_coef_kernel(
    int m, int k, const unsigned char *__restrict__ posmask, const float *__restrict__ a, const int *__restrict__ sel,
    float mu, float nu, float temperature, const float *__restrict__ sim, const float *__restrict__ mean_cnt,
    const float *__restrict__ grad_out, float *__restrict__ gco)
{
    const int sub = threadIdx.x & 31;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) >> 5, a, i, ai)) return;  // (sel: the listed are selected)
    const float scale = grad_out[0] / mean_cnt[1];
    const float margin = contrast_margin(mu, ai, nu);
    const unsigned char *pm_i = posmask + (size_t)i * k;
    const float *sim_i = sim + (size_t)i * k;
    const ContrastSums t = contrast_sums32(k, sub, pm_i, sim_i, margin, temperature);
    const float coef = t.psum == 0.f ? 0.f : contrast_coef(scale, t.psum, t.tsum, temperature);
    for (int j = sub; j < k; j += 32) {
        const bool pos = pm_i[j] != 0;
        const float e = contrast_exp(sim_i[j], pos, margin, temperature);
        gco[(size_t)i * k + j] = t.psum == 0.f ? 0.f : contrast_edge_g(coef, e, pos, t.nsum, t.psum);
    }
}

template <int LPR>
__global__ __launch_bounds__(256) void contrast_backward_rows_kernel(
    int m, int k, int nbr_stride, const float *__restrict__ f, const float *__restrict__ norm,
    const int *__restrict__ nbr, const float *__restrict__ a, const int *__restrict__ rev,
    const float *__restrict__ sim, const float *__restrict__ gco, float *__restrict__ grad_f)
{
    constexpr int R = 64 / LPR;  // edges per round
    constexpr int U = 4;         // rounds in flight
    const int lane = threadIdx.x & 63, q = lane & (LPR - 1), r = lane / LPR;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= m) return;
    const float an = a[n];
    const int own = contrast_selected(an) ? k : 0;
    const int e0 = rev[n], deg = rev[n + 1] - e0;
    const int *rev_edge = rev + m + 1;
    const int total = own + deg;
    const float4 *f4 = reinterpret_cast<const float4 *>(f);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (total > 0) {
        const float nn = norm[n];
        float4 fn = f4[(size_t)n * LPR + q];
        fn.x = __fdiv_rn(fn.x, nn); fn.y = __fdiv_rn(fn.y, nn); fn.z = __fdiv_rn(fn.z, nn); fn.w = __fdiv_rn(fn.w, nn);
        for (int t0 = 0; t0 < total; t0 += U * R) {
            int x[U];
            float g[U], sv[U], nx[U];
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                rows_edge(t0 + u * R + r, total, own, n, k, nbr + (size_t)n * nbr_stride, rev_edge + e0, gco, sim, x[u], g[u], sv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nx[u] = x[u] >= 0 ? norm[x[u]] : 1.f;
                v[u] = x[u] >= 0 ? f4[(size_t)x[u] * LPR + q] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (x[u] < 0) continue;
                rows_accumulate(acc, g[u], sv[u], nn, fn, v[u], nx[u]);
            }
        }
#pragma unroll
        for (int s = LPR; s < 64; s <<= 1) {
            acc.x += __shfl_xor(acc.x, s, 64);
            acc.y += __shfl_xor(acc.y, s, 64);
            acc.z += __shfl_xor(acc.z, s, 64);
            acc.w += __shfl_xor(acc.w, s, 64);
        }
    }
    if (r == 0) reinterpret_cast<float4 *>(grad_f)[(size_t)n * LPR + q] = acc;
}

// The wide form: any C = 4 * C4 up to 256 * P (the widths deterministic mode needs beyond the powers of two above, 512 of
// PointNeXt-XL among them).  One wave per row n, ONE edge per round, lane q owns the float4 pieces q, q + 64, .. (P of them,
// those below C4), so a wave reads a neighbour row in contiguous 1 KB pieces; U rounds of rows in flight.  No lane shares an
// element with another, so there is no cross-lane sum: each output element is the sequential fp32 sum, from +0.0f, over
// the row's own slots 0..k-1 (a selected anchor only) and then over its reverse list in list order.  Edge decode and per-edge
// expression are contrast_backward_rows_kernel's (rows_edge, rows_accumulate).
template <int P>
__global__ __launch_bounds__(256) void contrast_backward_rows_wide_kernel(
    int m, int C4, int k, int nbr_stride, const float *__restrict__ f, const float *__restrict__ norm,
    const int *__restrict__ nbr, const float *__restrict__ a, const int *__restrict__ rev,
    const float *__restrict__ sim, const float *__restrict__ gco, float *__restrict__ grad_f)
{
    constexpr int U = 4;  // rounds in flight
    const int q = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= m) return;
    const float an = a[n];
    const int own = contrast_selected(an) ? k : 0;
    const int e0 = rev[n], deg = rev[n + 1] - e0;
    const int *rev_edge = rev + m + 1;
    const int total = own + deg;
    const float4 *f4 = reinterpret_cast<const float4 *>(f);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = zero;
    if (total > 0) {
        const float nn = norm[n];
        float4 fn[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int piece = q + 64 * p;
            fn[p] = piece < C4 ? f4[(size_t)n * C4 + piece] : zero;
            fn[p].x = __fdiv_rn(fn[p].x, nn); fn[p].y = __fdiv_rn(fn[p].y, nn);
            fn[p].z = __fdiv_rn(fn[p].z, nn); fn[p].w = __fdiv_rn(fn[p].w, nn);
        }
        for (int t0 = 0; t0 < total; t0 += U) {
            int x[U];
            float g[U], sv[U], nx[U];
            float4 v[U][P];
#pragma unroll
            for (int u = 0; u < U; ++u)
                rows_edge(t0 + u, total, own, n, k, nbr + (size_t)n * nbr_stride, rev_edge + e0, gco, sim, x[u], g[u], sv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nx[u] = x[u] >= 0 ? norm[x[u]] : 1.f;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int piece = q + 64 * p;
                    v[u][p] = (x[u] >= 0 && piece < C4) ? f4[(size_t)x[u] * C4 + piece] : zero;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (x[u] < 0) continue;
#pragma unroll
                for (int p = 0; p < P; ++p) rows_accumulate(acc[p], g[u], sv[u], nn, fn[p], v[u][p], nx[u]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int piece = q + 64 * p;
        if (piece < C4) reinterpret_cast<float4 *>(grad_f)[(size_t)n * C4 + piece] = acc[p];
    }
}

// ---------------------------------------------------------------------------------------------
// Contrast backward over the MUTUAL edges (round 3; the default).  91 % of the edges of the stages' 24-NN graphs are mutual
// (x in N(n) and n in N(x)), and everything an edge contributes is symmetric in its two ends: the cosine s_nx = s_xn (the
// products commute and the channel sum runs in the same order, so even the bits agree with what the forward computed at
// the other end) and the positive mask (equal classes).  So point n, walking its OWN list once, has in registers what both
// directions of a mutual edge need:
//     dL/df_n = sum_{x in N(n)} (g_nx [n selected] + g_xn [x selected, edge mutual]) / |f_n| * (fhat_x - s_nx fhat_n)
//             + sum over the non-mutual incoming edges (x -> n), listed in rev (amc3d_contrast_mutual: a tenth of all edges)
// with g_ix = dL/ds_ix = coef_i e_ix ([pos] N_i - [neg] P_i), e_ix = exp((s - [pos] margin_i)/T), N_i = S_i - P_i the negatives'
// sum (added up on its own: the difference would cancel), from a 32-byte record per anchor (norm, coef, S, P, margin, N:
// contrast_record_kernel; the backward reads norm, coef, P, margin and N).  Every neighbour row is fetched ONCE per (n, x) pair -- the traffic of
// the forward kernel -- every gradient row is written once with a plain store, the summation order is fixed, and no float
// atomic is left (the atomic form added 387 / 229 / 134 / 73 MB of rows per step at the chip's float-atomic rate of 1.15 TB/s).
// ---------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) ContrastRecord { float norm, coef, tsum, psum, margin, nsum, pad1, pad2; };  // nsum = S - P, summed on its own

__global__ __launch_bounds__(256) void contrast_record_kernel(
    int m, int k, const float *__restrict__ norm, const unsigned char *__restrict__ posmask, const float *__restrict__ a,
    float mu, float nu, float temperature, const float *__restrict__ sim, const float *__restrict__ mean_cnt,
    const float *__restrict__ grad_out, ContrastRecord *__restrict__ rec)
{
    const int sub = threadIdx.x & 31;
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    if (i >= m) return;
    const float ai = a[i];
    const bool selected = contrast_selected(ai);
    const float margin = contrast_margin(mu, ai, nu);
    // (uniform per half-wave) sim holds values for the selected anchors only: the others sum over no slot
    const ContrastSums t = contrast_sums32(selected ? k : 0, sub, posmask + (size_t)i * k, sim + (size_t)i * k, margin, temperature);
    if (sub == 0) {
        const float scale = grad_out[0] / mean_cnt[1];
        ContrastRecord o;
        o.norm = norm[i];
        o.coef = (selected && t.psum != 0.f) ? contrast_coef(scale, t.psum, t.tsum, temperature) : 0.f;
        o.tsum = t.tsum; o.psum = t.psum; o.margin = margin; o.nsum = t.nsum; o.pad1 = o.pad2 = 0.f;
        rec[i] = o;
    }
}

// the same records from the two sums the forward pass kept per anchor (stats[2 i] = sum of the positives' exponentials,
// stats[2 i + 1] = sum of the negatives'): nothing to recompute, no similarities to read; one thread per anchor
// (the record of anchor i; g = the gradient of the stage's mean)
__device__ __forceinline__ void contrast_record_stats_anchor(int i, int m, const float *__restrict__ norm, const float *__restrict__ a,
                                                             float mu, float nu, float temperature, const float *__restrict__ stats,
                                                             const float *__restrict__ mean_cnt, float g,
                                                             ContrastRecord *__restrict__ rec)
{
    if (i >= m) return;
    const float ai = a[i];
    const bool selected = contrast_selected(ai);  // (the forward visited the selected anchors only: the others' stats are unwritten)
    const float psum = selected ? stats[(size_t)i * 2] : 0.f, nsum = selected ? stats[(size_t)i * 2 + 1] : 1.f;
    const float tsum = __fadd_rn(psum, nsum);
    const float scale = g / mean_cnt[1];
    ContrastRecord o;
    o.norm = norm[i];
    o.coef = (selected && psum != 0.f) ? contrast_coef(scale, psum, tsum, temperature) : 0.f;
    o.tsum = tsum; o.psum = psum; o.margin = contrast_margin(mu, ai, nu); o.nsum = nsum; o.pad1 = o.pad2 = 0.f;
    rec[i] = o;
}

__global__ __launch_bounds__(256) void contrast_record_stats_kernel(int m, const float *__restrict__ norm, const float *__restrict__ a,
                                                                    float mu, float nu, float temperature,
                                                                    const float *__restrict__ stats, const float *__restrict__ mean_cnt,
                                                                    const float *__restrict__ grad_out, ContrastRecord *__restrict__ rec)
{
    contrast_record_stats_anchor(blockIdx.x * 256 + threadIdx.x, m, norm, a, mu, nu, temperature, stats, mean_cnt, grad_out[0], rec);
}

// The mutual-edge gather (unit rows, see row_unit_kernel: hx = f_x / n_x is fetched, not recomputed; lane q < UNIT_U of a row
// decodes and evaluates the row's slot of round q -- index, mask, mutual count, the record of x, the two exponentials --
// once, and hands x down to / the finished coefficient back to the row's lanes by shuffles).  One wave: row n < m of the
// gradient, every lane returns piece q of it.
template <int LPR>
__device__ __forceinline__ float4 contrast_mutual_row(
    int lane, int n, int m, int k, int nbr_stride, const float *__restrict__ unit, const int *__restrict__ nbr,
    const unsigned char *__restrict__ posmask, const unsigned char *__restrict__ mutual, const int *__restrict__ rev,
    const ContrastRecord *__restrict__ rec, float temperature)
{
    constexpr int R = 64 / LPR;  // rows per round
    constexpr int U = UNIT_U;    // rounds in flight
    const int q = lane & (LPR - 1), r = lane / LPR, row0 = lane & ~(LPR - 1);
    const float4 *h4 = reinterpret_cast<const float4 *>(unit);
    const float4 *rec4 = reinterpret_cast<const float4 *>(rec);
    const float4 rn0 = rec4[(size_t)n * 2];       // norm, coef, (tsum: not read here), psum
    const float4 rn1 = rec4[(size_t)n * 2 + 1];   // margin, nsum
    const float margin_n = rn1.x, nsum_n = rn1.y;
    const float nn = rn0.x, coef_n = rn0.y, psum_n = rn0.w;
    const float4 fn = h4[(size_t)n * LPR + q];
    const int e0 = rev[n], deg = rev[n + 1] - e0;
    const int *rev_edge = rev + m + 1;
    const int total = k + deg;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < total; t0 += U * R) {
        // the slot this lane decodes and evaluates: round q, row r
        const int tq = t0 + q * R + r;
        int myx = -1;
        bool pos = false, own = false;
        float inc = 0.f;  // incoming edges x -> n met at this slot (their number: 0 or 1 in a k-NN graph)
        if (q < U) {
            if (tq < k) {  // own list: the edge n -> x, and x -> n when it is mutual
                myx = nbr[(size_t)n * nbr_stride + tq];
                pos = posmask[(size_t)n * k + tq] != 0;
                inc = (float)(mutual[(size_t)n * k + tq] & 0x7f);
                own = coef_n != 0.f;
                if (!own && inc == 0.f) myx = -1;  // nothing flows along this edge
            } else if (tq < total) {  // a non-mutual incoming edge x -> n
                const int p = rev_edge[e0 + tq - k];
                myx = p / k;
                pos = posmask[p] != 0;
                inc = 1.f;
            }
        }
        int x[U];
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = __shfl(myx, row0 | u, 64);
        const float4 rx = myx >= 0 ? rec4[(size_t)myx * 2] : make_float4(1.f, 0.f, 1.f, 0.f);  // (only coef = 0 matters for an empty slot)
        const float4 rx1 = myx >= 0 ? rec4[(size_t)myx * 2 + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float mx = rx1.x;
        float s[U], smine = 0.f;
        unit_row_cosines<LPR>(h4, fn, q, x, v, s);  // the forward's loads, products and tree: s_nx to the bit
#pragma unroll
        for (int u = 0; u < U; ++u) smine = q == u ? s[u] : smine;
        float gn = 0.f;
        if (myx >= 0) {
            float g = 0.f;
            if (own) {
                g += contrast_edge_g(coef_n, contrast_exp(smine, pos, margin_n, temperature), pos, nsum_n, psum_n);
            }
            if (inc != 0.f && rx.y != 0.f) {
                g += inc * contrast_edge_g(rx.y, contrast_exp(smine, pos, mx, temperature), pos, rx1.y, rx.w);
            }
            gn = g / nn;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float gu = __shfl(gn, row0 | u, 64);
            const float sn = contrast_projection(nn, s[u]);
            acc.x = __fmaf_rn(gu, __fmaf_rn(-sn, fn.x, v[u].x), acc.x);
            acc.y = __fmaf_rn(gu, __fmaf_rn(-sn, fn.y, v[u].y), acc.y);
            acc.z = __fmaf_rn(gu, __fmaf_rn(-sn, fn.z, v[u].z), acc.z);
            acc.w = __fmaf_rn(gu, __fmaf_rn(-sn, fn.w, v[u].w), acc.w);
        }
    }
#pragma unroll
    for (int d = LPR; d < 64; d <<= 1) {
        acc.x += __shfl_xor(acc.x, d, 64);
        acc.y += __shfl_xor(acc.y, d, 64);
        acc.z += __shfl_xor(acc.z, d, 64);
        acc.w += __shfl_xor(acc.w, d, 64);
    }
    return acc;
}

template <int LPR>
__global__ __launch_bounds__(256) void contrast_backward_mutual_kernel(
    int m, int k, int nbr_stride, const float *__restrict__ unit, const int *__restrict__ nbr,
    const unsigned char *__restrict__ posmask, const unsigned char *__restrict__ mutual, const int *__restrict__ rev,
    const ContrastRecord *__restrict__ rec, float temperature, float *__restrict__ grad_f)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= m) return;
    const float4 acc = contrast_mutual_row<LPR>(lane, n, m, k, nbr_stride, unit, nbr, posmask, mutual, rev, rec, temperature);
    if (lane < LPR) reinterpret_cast<float4 *>(grad_f)[(size_t)n * LPR + lane] = acc;
}

// ---------------------------------------------------------------------------------------------
// All stages of the loss per launch (amc3d_contrast_stages_forward_cm / _backward_cm).  The descriptors travel by value; a
// kernel's grid is the concatenation of the stages' grids, first[s] = the first block of stage s (first[nstages] = the
// grid).  A block finds its stage by a scan that is uniform across the workgroup, and its width by a switch that calls the
// body the single-stage kernel of that width calls: the arithmetic of a stage does not know which launch it runs in.
// ---------------------------------------------------------------------------------------------
struct ContrastStages {
    int nstages;
    int first[AMC_CONTRAST_MAX_STAGES + 1];
    AmcContrastStage st[AMC_CONTRAST_MAX_STAGES];
};

// -> the stage of block blk, and blk as the block's index within that stage
__device__ __forceinline__ int contrast_stage_of_block(const ContrastStages &S, int &blk)
{
    int s = 0;
    while (s + 1 < S.nstages && blk >= S.first[s + 1]) ++s;
    blk -= S.first[s];
    return s;
}

template <int N> using int_c = std::integral_constant<int, N>;

// fn(int_c<C / 4>) for the widths of amc3d_contrast_backward_csr_supported (the entry points admit no other)
template <class F>
__device__ __forceinline__ void device_with_lpr(int C, F &&fn)
{
    switch (C) {
    case 16: fn(int_c<4>{}); break;
    case 32: fn(int_c<8>{}); break;
    case 64: fn(int_c<16>{}); break;
    case 128: fn(int_c<32>{}); break;
    case 256: fn(int_c<64>{}); break;
    default: break;
    }
}

// Points per tile of the channel-major gradient store (contrast_stages_backward_kernel): a tile is [C][TP + 1] floats of
// LDS and is written as runs of TP floats.  A wave walks TP / 4 rows one after the other, and the wide stages are short (375
// points per cloud at 256 channels): the small tiles keep as many waves on their rows as the row-major kernel has, and
// that outweighs the short runs (profiles/contrast_stages_tile_sweep.txt: the best of 4 .. 64 points per width)
template <int LPR> constexpr int grad_tile_points() { return LPR >= 64 ? 4 : LPR >= 32 ? 8 : 16; }

__global__ __launch_bounds__(256) void contrast_stages_unit_kernel(const ContrastStages S)
{
    extern __shared__ float s_tile[];
    int blk = blockIdx.x;
    const AmcContrastStage &st = S.st[contrast_stage_of_block(S, blk)];
    device_with_lpr(st.C, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value, TP = unit_tile_points<LPR>();
        const int tiles = (st.n + TP - 1) / TP;
        row_unit_cm_tile<LPR, TP>(s_tile, st.n, blk / tiles, (blk % tiles) * TP, st.f_cm, st.norm, st.unit);
    });
}

__global__ __launch_bounds__(256) void contrast_stages_forward_kernel(const ContrastStages S, float mu, float nu, float temperature)
{
    int blk = blockIdx.x;
    const AmcContrastStage &st = S.st[contrast_stage_of_block(S, blk)];
    device_with_lpr(st.C, [&](auto lpr) {
        contrast_forward_unit_wave<decltype(lpr)::value>(blk * 4 + (threadIdx.x >> 6), st.b * st.n, st.k, st.nbr_stride, st.unit, st.nbr,
                                                         st.posmask, st.a, st.sel, mu, nu, temperature, nullptr, st.stats, st.loss_pt);
    });
}

// One workgroup: masked_mean_kernel's sums stage by stage, then total = scale * (((l0 + l1) + l2) + ...), the chain the
// per-stage route leaves to the caller's additions
__global__ __launch_bounds__(1024) void contrast_stages_mean_kernel(const ContrastStages S, float scale, float *__restrict__ total)
{
    __shared__ double s_sum[16];
    __shared__ int s_cnt[16];
    __shared__ float s_mean[AMC_CONTRAST_MAX_STAGES];
#pragma unroll 1
    for (int s = 0; s < S.nstages; ++s) {
        const AmcContrastStage &st = S.st[s];
        const float l = masked_mean_block(s_sum, s_cnt, st.b * st.n, st.loss_pt, st.a, st.mean_cnt);
        if (threadIdx.x == 0) s_mean[s] = l;
        __syncthreads();  // (s_sum, s_cnt are free again)
    }
    if (threadIdx.x == 0) {
        float t = s_mean[0];
        for (int s = 1; s < S.nstages; ++s) t = __fadd_rn(t, s_mean[s]);
        total[0] = __fmul_rn(scale, t);
    }
}

__global__ __launch_bounds__(256) void contrast_stages_record_kernel(const ContrastStages S, float mu, float nu, float temperature,
                                                                     float scale, const float *__restrict__ grad_out)
{
    int blk = blockIdx.x;
    const AmcContrastStage &st = S.st[contrast_stage_of_block(S, blk)];
    contrast_record_stats_anchor(blk * 256 + threadIdx.x, st.b * st.n, st.norm, st.a, mu, nu, temperature, st.stats, st.mean_cnt,
                                 __fmul_rn(grad_out[0], scale), (ContrastRecord *)st.rec);
}

// The mutual-edge gather storing CHANNEL-major: a workgroup owns the points n0 .. n0 + TP of one cloud, its waves take those
// rows in turn (contrast_mutual_row: the accumulators and their order are the single-stage kernel's), a finished row goes
// from its lanes into the tile, and after one barrier the tile leaves as runs of TP floats of grad_cm[b][c][n0 ...].
template <int LPR, int TP>
__device__ __forceinline__ void contrast_mutual_tile_cm(float *s_tile, const AmcContrastStage &st, int blk, float temperature)
{
    constexpr int C = 4 * LPR, TS = TP + 1;
    const int tiles = (st.n + TP - 1) / TP;
    const int b = blk / tiles, n0 = (blk % tiles) * TP;
    const int np = min(TP, st.n - n0);  // points of this tile
    int lane = threadIdx.x & 63;
    for (int pl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); pl < np; pl += 4) {  // (a scalar: the row is the wave's)
        asm volatile("" : "+v"(lane));  // (what derives from the lane is formed per row, not kept across the rows)
        const float4 acc = contrast_mutual_row<LPR>(lane, b * st.n + n0 + pl, st.b * st.n, st.k, st.nbr_stride, st.unit, st.nbr, st.posmask,
                                                    st.mutual, st.rev, (const ContrastRecord *)st.rec, temperature);
        if (lane < LPR) {
            s_tile[(4 * lane) * TS + pl] = acc.x;
            s_tile[(4 * lane + 1) * TS + pl] = acc.y;
            s_tile[(4 * lane + 2) * TS + pl] = acc.z;
            s_tile[(4 * lane + 3) * TS + pl] = acc.w;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * TP; e += 256) {
        const int ch = e / TP, pt = e - ch * TP;
        if (pt < np) st.grad_cm[((size_t)b * C + ch) * st.n + n0 + pt] = s_tile[ch * TS + pt];
    }
}

__global__ __launch_bounds__(256) void contrast_stages_backward_kernel(const ContrastStages S, float temperature)
{
    extern __shared__ float s_tile[];
    int blk = blockIdx.x;
    const AmcContrastStage &st = S.st[contrast_stage_of_block(S, blk)];
    device_with_lpr(st.C, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        contrast_mutual_tile_cm<LPR, grad_tile_points<LPR>()>(s_tile, st, blk, temperature);
    });
}

// ---------------------------------------------------------------------------------------------
// The other forms of contrast_softnn_margin (MarginContrast.py:117-174): margin constant / adaptive / learned, decision
// boundary none / -m / +m, Method1 / Method2, with or without a temperature.  The form is four run-time integers
// (kernel-uniform branches, no template per combination); the pieces shared with the default form's kernels
// are the helpers at the top of the contrast part.  Three steps forward -- the cosines alone (contrast_sim_*), the per-anchor loss from the
// stored cosines (contrast_variant_loss_kernel), masked_mean_kernel -- and two backward: g_ij = dL/ds_ij
// (contrast_variant_coef_kernel), then the gradient rows from g by contrast_backward_rows_kernel or its wide form (a gather over reverse
// lists, which knows nothing of the loss's form) or by contrast_backward_edges_kernel (float atomics, any C <= 512).
//
// Per anchor, with z_j = (s_j - [pos] m) / T  (-m),  (s_j + [neg] m) / T  (+m),  s_j / T  (none), e_j = exp(z_j),
// P = sum_pos e, N = sum_neg e (each summed on its own, see contrast_sums32), S = P + N, q_j = dl/dz_j:
//   Method1  l = -log(P/S + eps):       q_j = -e_j (N/S) / ((P/S + eps) S)  on positives,  +e_j (P/S) / ((P/S + eps) S)  on negatives
//   Method2  l = -log(Y / (npos + eps)),  Y = sum_j (e_j [pos] / (e_j [pos] + N) + eps)  over ALL k slots:
//            q_j = -(e_j / (e_j + N)) (N / (e_j + N)) / Y  on positives,  +e_j W / Y  on negatives,
//            W = sum_pos e_j / (e_j + N)^2
//   dl/dm = -(1/T) sum_pos q  (-m),  +(1/T) sum_neg q  (+m),  0 (none);  sum_pos q = -sum_neg q = -N W / Y  (Method2),
//            -(N/S)(P/S) / (P/S + eps)  (Method1)
//   learned margin m = (u - 1) a + v, u = (1/k) sum_neg s, v = (1/k) sum_pos s:  dm/ds_j = 1/k on positives, a/k on negatives
//   dl/ds_j = q_j / T + dl/dm * dm/ds_j
// ---------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void contrast_sim_unit_kernel(
    int m, int k, int nbr_stride, const float *__restrict__ unit, const int *__restrict__ nbr, const float *__restrict__ a,
    const int *__restrict__ sel, float *__restrict__ sim)
{
    // the gather of contrast_forward_unit_kernel (unit_gather_indices / unit_gather_rows): the cosines agree to the bit
    constexpr int R = 64 / LPR;
    const int lane = threadIdx.x & 63, q = lane & (LPR - 1), r = lane / LPR;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, blockIdx.x * 4 + (threadIdx.x >> 6), a, i, ai)) return;
    if (!contrast_selected(ai)) return;
    const float4 *h4 = reinterpret_cast<const float4 *>(unit);
    const float4 u = h4[(size_t)i * LPR + q];
    for (int j0 = 0; j0 < k; j0 += UNIT_U * R) {
        int nb[UNIT_U];
        unit_gather_indices<LPR>(nbr, i, nbr_stride, k, j0, r, nb);
        const int jq = j0 + q * R + r;  // the slot this lane writes
        const float s = unit_gather_rows<LPR>(h4, u, q, nb);
        if (q < UNIT_U && jq < k) sim[(size_t)i * k + jq] = s;
    }
}

// the gather of contrast_forward_kernel (any C, row_cosine): 32 lanes per anchor, lane j owns neighbour j
__global__ __launch_bounds__(256) void contrast_sim_kernel(
    int m, int C, int k, int nbr_stride, const float *__restrict__ f, const float *__restrict__ norm,
    const int *__restrict__ nbr, const float *__restrict__ a, const int *__restrict__ sel, float *__restrict__ sim)
{
    const int sub = threadIdx.x & 31;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) >> 5, a, i, ai)) return;
    if (!contrast_selected(ai)) return;
    const float ni = norm[i];
    const float *fi = f + (size_t)i * C;
    for (int j = sub; j < k; j += 32) {
        const int nb = nbr[(size_t)i * nbr_stride + j];
        const float nj = norm[nb];
        sim[(size_t)i * k + j] = row_cosine(fi, f + (size_t)nb * C, ni, nj, C);
    }
}

struct ContrastForm { int margin_mode, db, method, has_temperature; float mu, nu, temperature; };

// z_j: the exponent of slot j (MarginContrast.py:140-149)
__device__ __forceinline__ float variant_arg(const ContrastForm &F, float s, bool pos, float margin)
{
    float z = s;
    if (F.db == 1) z = pos ? __fsub_rn(s, margin) : s;
    else if (F.db == 2) z = pos ? s : __fadd_rn(s, margin);
    return F.has_temperature ? __fdiv_rn(z, F.temperature) : z;
}

// what both variant kernels need of one anchor; every lane of the group returns the same values
struct ContrastAnchorSums { float margin, psum, nsum, npos, ysum, wsum; };

__device__ __forceinline__ ContrastAnchorSums variant_anchor_sums(const ContrastForm &F, int k, int sub, float ai,
                                                                 const float *__restrict__ sim_i,
                                                                 const unsigned char *__restrict__ pm_i)
{
    ContrastAnchorSums r;
    r.margin = F.nu;
    if (F.margin_mode == 1) r.margin = contrast_margin(F.mu, ai, F.nu);
    if (F.margin_mode == 2) {  // u, v: means over all k slots of the masked cosines (:128-130)
        float su = 0.f, sv = 0.f;
        for (int j = sub; j < k; j += 32) {
            const bool pos = pm_i[j] != 0;
            const float s = sim_i[j];
            su += pos ? 0.f : s;
            sv += pos ? s : 0.f;
        }
        const float u = __fdiv_rn(group32_sum(su), (float)k), v = __fdiv_rn(group32_sum(sv), (float)k);
        r.margin = __fadd_rn(__fmul_rn(__fsub_rn(u, 1.f), ai), v);
    }
    float psum = 0.f, nsum = 0.f, npos = 0.f;
    for (int j = sub; j < k; j += 32) {
        const bool pos = pm_i[j] != 0;
        const float e = expf(variant_arg(F, sim_i[j], pos, r.margin));
        psum += pos ? e : 0.f;
        nsum += pos ? 0.f : e;
        npos += pos ? 1.f : 0.f;
    }
    r.psum = group32_sum(psum);
    r.nsum = group32_sum(nsum);
    r.npos = group32_sum(npos);
    r.ysum = r.wsum = 0.f;
    if (F.method == 2) {  // (:165-171, literally: a negative slot contributes 0 / (0 + N) + eps)
        float y = 0.f, wv = 0.f;
        for (int j = sub; j < k; j += 32) {
            const bool pos = pm_i[j] != 0;
            const float ep = pos ? expf(variant_arg(F, sim_i[j], pos, r.margin)) : 0.f;
            const float den = ep + r.nsum;
            y += __fadd_rn(__fdiv_rn(ep, den), 1e-12f);
            wv += pos ? __fdiv_rn(__fdiv_rn(ep, den), den) : 0.f;
        }
        r.ysum = group32_sum(y);
        r.wsum = group32_sum(wv);
    }
    return r;
}

__global__ __launch_bounds__(256) void contrast_variant_loss_kernel(
    int m, int k, const unsigned char *__restrict__ posmask, const float *__restrict__ a, const int *__restrict__ sel,
    ContrastForm F, const float *__restrict__ sim, float *__restrict__ loss_pt)
{
    const int sub = threadIdx.x & 31;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) >> 5, a, i, ai)) return;
    if (!contrast_selected(ai)) {
        if (sub == 0) loss_pt[i] = 0.f;
        return;
    }
    const ContrastAnchorSums r = variant_anchor_sums(F, k, sub, ai, sim + (size_t)i * k, posmask + (size_t)i * k);
    if (sub == 0) {
        const float ratio = F.method == 2 ? __fdiv_rn(r.ysum, __fadd_rn(r.npos, 1e-12f))
                                          : __fadd_rn(__fdiv_rn(r.psum, __fadd_rn(r.psum, r.nsum)), 1e-12f);
        loss_pt[i] = -logf(ratio);
    }
}

// gco[i,j] = (grad_out / count) * dl_i/ds_ij for the visited anchors (the header above); an anchor without a positive
// neighbour under Method1 gets exact zeros, as in contrast_coef_kernel
__global__ __launch_bounds__(256) void contrast_variant_coef_kernel(
    int m, int k, const unsigned char *__restrict__ posmask, const float *__restrict__ a, const int *__restrict__ sel,
    ContrastForm F, const float *__restrict__ sim, const float *__restrict__ mean_cnt,
    const float *__restrict__ grad_out, float *__restrict__ gco)
{
    const int sub = threadIdx.x & 31;
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) >> 5, a, i, ai)) return;
    if (!contrast_selected(ai)) return;
    const float *sim_i = sim + (size_t)i * k;
    const unsigned char *pm_i = posmask + (size_t)i * k;
    const ContrastAnchorSums r = variant_anchor_sums(F, k, sub, ai, sim_i, pm_i);
    const float scale = grad_out[0] / mean_cnt[1];
    const float inv_t = F.has_temperature ? 1.f / F.temperature : 1.f;
    // q_j = cp * e_j * (Method2: N / (e_j + N)^2) on positives, cn * e_j on negatives
    float cp, cn, qpos;  // qpos = sum_pos q = -sum_neg q
    bool dead = false;
    if (F.method == 2) {
        cp = -1.f / r.ysum;
        cn = r.wsum / r.ysum;
        qpos = -r.nsum * cn;
    } else {
        const float S = r.psum + r.nsum, rp = r.psum / S, rn = r.nsum / S;
        const float den = (rp + 1e-12f) * S;
        cp = -rn / den;
        cn = rp / den;
        qpos = -rn * rp / (rp + 1e-12f);
        dead = r.psum == 0.f;
    }
    const float dm = F.db != 0 ? -inv_t * qpos : 0.f;  // dl/dm; -m: -sum_pos q / T;  +m: sum_neg q / T, the same number
    const float dm_pos = F.margin_mode == 2 ? dm / (float)k : 0.f, dm_neg = dm_pos * ai;
    for (int j = sub; j < k; j += 32) {
        const bool pos = pm_i[j] != 0;
        const float e = expf(variant_arg(F, sim_i[j], pos, r.margin));
        float q;
        if (!pos) q = cn * e;
        else if (F.method == 2) {
            const float den = e + r.nsum;
            q = cp * (e / den) * (r.nsum / den);
        } else q = cp * e;
        const float g = scale * (q * inv_t + (pos ? dm_pos : dm_neg));
        gco[(size_t)i * k + j] = dead ? 0.f : g;
    }
}

// Gradient rows from g = gco by float atomics: the walk of contrast_backward_kernel (EdgeWalk) with the edge coefficient
// read instead of computed.  grad_f zero-initialised by the caller; C <= LPA * VPT.
template <int LPA, int VPT>
__global__ __launch_bounds__(256) void contrast_backward_edges_kernel(
    int m, int C, int k, int nbr_stride, const float *__restrict__ f, const float *__restrict__ norm,
    const int *__restrict__ nbr, const float *__restrict__ a, const int *__restrict__ sel, const float *__restrict__ sim,
    const float *__restrict__ gco, float *__restrict__ grad_f)
{
    const int sub = threadIdx.x & (LPA - 1);
    int i;
    float ai;
    if (!contrast_anchor(sel, m, (blockIdx.x * blockDim.x + threadIdx.x) / LPA, a, i, ai)) return;
    if (!contrast_selected(ai)) return;
    const float ni = norm[i];

    EdgeWalk<LPA, VPT> walk;
    walk.begin(C, sub, f, i, ni);
    for (int j0 = 0; j0 < k; j0 += LPA) {
        // lane `sub` holds neighbour j0 + sub of this chunk of LPA neighbours
        const int j = j0 + sub;
        int nb_l = -1;
        float sj_l = 0.f, nj_l = 1.f, g_l = 0.f;
        if (j < k) {
            nb_l = nbr[(size_t)i * nbr_stride + j];
            sj_l = sim[(size_t)i * k + j];
            g_l = gco[(size_t)i * k + j];
            nj_l = norm[nb_l];
        }
        walk.chunk(C, sub, f, ni, min(LPA, k - j0), nb_l, sj_l, nj_l, g_l, grad_f);
    }
    walk.finish(C, sub, i, grad_f);
}

// ---------------------------------------------------------------------------------------------
// The point losses: every criterion of openpoints.loss (loss/build.py:14-257, 328-340) over channel-major logits (B, C, N)
// with class targets (B, N), without the (B*N, C) transposed copy of the logits, as two form-generic families on one layout:
// one thread per point, class planes read coalesced along N, any C >= 1, per-point terms in fp32 combined and summed in fp64
// in a fixed order (wave shuffle tree, the block's waves in order, pl_finalize_kernel over the blocks' partials).  No atomics
// and nothing zero-filled.  A class is a handful of run-time numbers (PlSoftmax / PlSigmoid), filled in by the C entry points
// from the arguments include/amc3d.h documents.  nn.CrossEntropyLoss() with its defaults is the softmax form with only the
// ignore value set, F.cross_entropy with weight and label_smoothing the form weight_per_class 1, eps_rule 0, den_mode 1.
// ---------------------------------------------------------------------------------------------
constexpr int CE_THREADS = 256;
enum { PL_DEN_COUNT = 0, PL_DEN_WSUM = 1, PL_DEN_ONE = 2 };

// The one compile-time switch of the softmax kernels: the exponential and logarithm of the plain cross entropy are the
// native instructions' (__expf / __logf), those of every other form the library's.  The plain form is the one inside the
// captured AMContrast3D train step, whose bits are held fixed; in it every other factor of the generic arithmetic is 1 or 0.
template <bool NATIVE> __device__ __forceinline__ float pl_exp(float v) { return NATIVE ? __expf(v) : expf(v); }
template <bool NATIVE> __device__ __forceinline__ float pl_log(float v) { return NATIVE ? __logf(v) : logf(v); }

struct PlSoftmax {
    const long long *remap;  // label -> class table of remap_len entries, or null
    int remap_len;
    long long ignore;
    int has_ignore;
    const int *mask;         // (B,N): a point counts iff its entry == 1, or null
    const float *weight;     // (C) or null
    int weight_per_class;    // 1: w[c] inside the sum over the classes; 0: w[y] on the whole term
    float a_hot, a_off;      // the target distribution: q[y] = a_hot, q[c != y] = a_off
    float gamma;             // focal exponent of the detached (1 - p[y]); 0: none
    const float *alpha;      // (C) focal alpha table or null
    float poly;              // + poly * (1 - p[y]), attached
    int den_mode;
};

// the class of point (b, n) after the ignore test, the mask and the remap; -1: the point is left out
__device__ inline int pl_class(const PlSoftmax &f, int C, long long t, size_t at)
{
    if (f.has_ignore && t == f.ignore) return -1;
    if (f.mask && f.mask[at] != 1) return -1;
    if (f.remap) {
        if (t < 0 || t >= f.remap_len) return -1;
        t = f.remap[t];
    }
    return (t >= 0 && t < C) ? (int)t : -1;
}

// block sum of (num, den) in the fixed order -> partial[2 * block]
__device__ inline void pl_block_sum(double num, double den, double *__restrict__ partial)
{
    __shared__ double s_num[CE_THREADS / 64], s_den[CE_THREADS / 64];
    for (int s = 32; s >= 1; s >>= 1) {
        num += __shfl_xor(num, s, 64);
        den += __shfl_xor(den, s, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_num[threadIdx.x >> 6] = num; s_den[threadIdx.x >> 6] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, d = 0.0;
        for (int w = 0; w < CE_THREADS / 64; ++w) { t += s_num[w]; d += s_den[w]; }
        const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[slot * 2] = t;
        partial[slot * 2 + 1] = d;
    }
}

// out[0] = sum / den, out[1] = den; den = the summed denominators, or 1 for reduction 'sum' (0/0 = NaN, as torch's mean over nothing)
__global__ __launch_bounds__(1024) void pl_finalize_kernel(int nparts, const double *__restrict__ partial, int den_mode,
                                                           float *__restrict__ out)
{
    __shared__ double s_sum[16], s_den[16];
    double t = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 1024) { t += partial[(size_t)i * 2]; c += partial[(size_t)i * 2 + 1]; }
    for (int s = 32; s >= 1; s >>= 1) {
        t += __shfl_xor(t, s, 64);
        c += __shfl_xor(c, s, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = t; s_den[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tt = 0.0, cc = 0.0;
        for (int w = 0; w < 16; ++w) { tt += s_sum[w]; cc += s_den[w]; }
        if (den_mode == PL_DEN_ONE) cc = 1.0;
        out[0] = (float)(tt / cc);
        out[1] = (float)cc;
    }
}

// Softmax family.  With y the point's class (pl_class), Q[c] = q[c] * (weight_per_class ? w[c] : 1) and
// m = (weight_per_class ? 1 : w[y]) * alpha[y] * (1 - p[y])^gamma:   term = m * sum_c Q[c] (-lp[c]) + poly * (1 - p[y])
template <bool NATIVE>
__global__ __launch_bounds__(CE_THREADS) void pl_softmax_forward_kernel(int C, long N, const float *__restrict__ logits,
                                                                        const long long *__restrict__ target, PlSoftmax f,
                                                                        float *__restrict__ lse, double *__restrict__ partial)
{
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * CE_THREADS + threadIdx.x;
    double num = 0.0, den = 0.0;
    if (n < N) {
        const size_t at = (size_t)b * N + n;
        const float *x = logits + (size_t)b * C * N + n;
        float mx = -__builtin_inff();
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, x[(size_t)c * N]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += pl_exp<NATIVE>(x[(size_t)c * N] - mx);
        const float l = mx + pl_log<NATIVE>(se);
        lse[at] = l;
        const int y = pl_class(f, C, target[at], at);
        if (y >= 0) {
            const float wy = f.weight ? f.weight[y] : 1.f;
            const float lpy = x[(size_t)y * N] - l;
            float m = f.weight_per_class ? 1.f : wy;
            if (f.alpha) m *= f.alpha[y];
            if (f.gamma != 0.f) m *= powf(1.f - pl_exp<NATIVE>(lpy), f.gamma);
            double term = (double)(f.a_hot - f.a_off) * (double)((f.weight_per_class ? wy : 1.f) * -lpy);
            if (f.a_off != 0.f) {
                float sm = 0.f;  // sum_c w[c] * (-lp[c])
                for (int c = 0; c < C; ++c) {
                    const float nlp = l - x[(size_t)c * N];
                    sm += (f.weight && f.weight_per_class) ? f.weight[c] * nlp : nlp;
                }
                term += (double)f.a_off * (double)sm;
            }
            num = (double)m * term;
            if (f.poly != 0.f) num += (double)f.poly * (double)(1.f - pl_exp<NATIVE>(lpy));
            den = f.den_mode == PL_DEN_WSUM ? (double)wy : 1.0;
        }
    }
    pl_block_sum(num, den, partial);
}

// dlogits[c] = g / den * [ m (p[c] sum_c Q - Q[c]) + poly p[y] (p[c] - [c == y]) ] for counted points ((1 - p[y])^gamma is a
// constant: FocalLoss detaches pt), zero rows otherwise; den = loss_den[1]
template <bool NATIVE>
__global__ __launch_bounds__(CE_THREADS) void pl_softmax_backward_kernel(int C, long N, const float *__restrict__ logits,
                                                                         const long long *__restrict__ target, PlSoftmax f,
                                                                         const float *__restrict__ lse,
                                                                         const float *__restrict__ loss_den,
                                                                         const float *__restrict__ grad_out,
                                                                         float *__restrict__ dlogits)
{
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (n >= N) return;
    const size_t at = (size_t)b * N + n;
    const float *x = logits + (size_t)b * C * N + n;
    float *d = dlogits + (size_t)b * C * N + n;
    const int y = pl_class(f, C, target[at], at);
    if (y < 0) {
        for (int c = 0; c < C; ++c) d[(size_t)c * N] = 0.f;
        return;
    }
    const bool per_class = f.weight && f.weight_per_class;
    const float l = lse[at];
    const float wy = f.weight ? f.weight[y] : 1.f;
    const float py = pl_exp<NATIVE>(x[(size_t)y * N] - l);
    float m = f.weight_per_class ? 1.f : wy;
    if (f.alpha) m *= f.alpha[y];
    if (f.gamma != 0.f) m *= powf(1.f - py, f.gamma);
    const float hot = (f.a_hot - f.a_off) * (per_class ? wy : 1.f);  // Q[y] - a_off w[y]
    float sq = hot;
    if (f.a_off != 0.f) {
        float wsum = (float)C;
        if (per_class) {
            wsum = 0.f;
            for (int c = 0; c < C; ++c) wsum += f.weight[c];
        }
        sq += f.a_off * wsum;
    }
    const float scale = grad_out[0] / loss_den[1];
    const float pp = f.poly * py;
    for (int c = 0; c < C; ++c) {
        const float p = pl_exp<NATIVE>(x[(size_t)c * N] - l);
        const float is_y = c == y ? 1.f : 0.f;
        const float qc = f.a_off * (per_class ? f.weight[c] : 1.f) + is_y * hot;
        d[(size_t)c * N] = scale * (m * (p * sq - qc) + pp * (p - is_y));
    }
}

struct PlSigmoid {
    const float *weight, *pos_weight;  // (C) or null: BCEWithLogitsLoss's, per class
    float alpha;                       // >= 0: alpha_t = t ? alpha : 1 - alpha
    float gamma, poly;
    int den_mode;                      // PL_DEN_COUNT: the elements of the counted points; PL_DEN_ONE
};

// one element of the sigmoid family: logit x, one-hot target bit t.  z = t ? -x : x, u = sigmoid(z) = 1 - pt,
// ce = softplus(z) = max(x,0) - x t + log1p(exp(-|x|)) = -log(pt):   value = a ce u^gamma + poly u^(gamma+1),
// a = w[c] (t ? pos_weight[c] : 1) alpha_t;  *dx = d value / d x
__device__ inline float pl_sigmoid_element(const PlSigmoid &f, int c, float x, bool t, float *dx)
{
    const float z = t ? -x : x;
    const float e = expf(-fabsf(z));
    const float ce = fmaxf(z, 0.f) + log1pf(e);
    const float u = (z >= 0.f ? 1.f : e) / (1.f + e);
    float a = f.weight ? f.weight[c] : 1.f;
    if (t && f.pos_weight) a *= f.pos_weight[c];
    if (f.alpha >= 0.f) a *= t ? f.alpha : 1.f - f.alpha;
    const float ug = f.gamma != 0.f ? powf(u, f.gamma) : 1.f;
    if (dx) {
        const float dz = ug * (a * (u + ce * f.gamma * (1.f - u)) + f.poly * (f.gamma + 1.f) * u * (1.f - u));
        *dx = t ? -dz : dz;
    }
    return a * ce * ug + f.poly * ug * u;
}

__global__ __launch_bounds__(CE_THREADS) void pl_sigmoid_forward_kernel(int C, long N, const float *__restrict__ logits,
                                                                        const long long *__restrict__ target, PlSigmoid f,
                                                                        double *__restrict__ partial)
{
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * CE_THREADS + threadIdx.x;
    double num = 0.0, den = 0.0;
    if (n < N) {
        const long long t = target[(size_t)b * N + n];
        if (t >= 0 && t < C) {
            const float *x = logits + (size_t)b * C * N + n;
            for (int c = 0; c < C; ++c) num += (double)pl_sigmoid_element(f, c, x[(size_t)c * N], c == (int)t, nullptr);
            den = (double)C;
        }
    }
    pl_block_sum(num, den, partial);
}

__global__ __launch_bounds__(CE_THREADS) void pl_sigmoid_backward_kernel(int C, long N, const float *__restrict__ logits,
                                                                         const long long *__restrict__ target, PlSigmoid f,
                                                                         const float *__restrict__ loss_den,
                                                                         const float *__restrict__ grad_out,
                                                                         float *__restrict__ dlogits)
{
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (n >= N) return;
    const float *x = logits + (size_t)b * C * N + n;
    float *d = dlogits + (size_t)b * C * N + n;
    const long long t = target[(size_t)b * N + n];
    if (t < 0 || t >= C) {
        for (int c = 0; c < C; ++c) d[(size_t)c * N] = 0.f;
        return;
    }
    const float scale = grad_out[0] / loss_den[1];
    for (int c = 0; c < C; ++c) {
        float dx;
        pl_sigmoid_element(f, c, x[(size_t)c * N], c == (int)t, &dx);
        d[(size_t)c * N] = scale * dx;
    }
}

}  // namespace amc

using namespace amc;

AMC_API int amc3d_vote_labels(int m, int kr, int num_classes, const int *labels0, const int *nbr_idx, int *labels,
                              void *stream)
{
    if (m <= 0) return 0;
    if (kr <= 0 || kr > 128 || num_classes <= 0 || !labels0 || !nbr_idx || !labels)
        return bad_arg("amc3d_vote_labels: bad argument (kr must be in 1..128)");
    hipLaunchKernelGGL(vote_labels_kernel, dim3(div_up(m, 4)), dim3(256), 0, (hipStream_t)stream, m, kr, num_classes,
                       labels0, nbr_idx, labels);
    return launch_status("amc3d_vote_labels");
}

AMC_API int amc3d_posmask(int m, int k, int nbr_stride, const int *labels, const int *nbr, unsigned char *posmask,
                          void *stream)
{
    if (m <= 0) return 0;
    if (k <= 0 || nbr_stride < k || !labels || !nbr || !posmask) return bad_arg("amc3d_posmask: bad argument");
    hipLaunchKernelGGL(posmask_kernel, dim3(div_up((long)m * k, 256)), dim3(256), 0, (hipStream_t)stream, m, k,
                       nbr_stride, labels, nbr, posmask);
    return launch_status("amc3d_posmask");
}

AMC_API size_t amc3d_ambiguity_workspace_bytes(int m) { return (size_t)m * 12 + 64; }

AMC_API int amc3d_ambiguity(int m, int k, int nbr_stride, int mode, float beta, const float *p,
                            const unsigned char *posmask, const int *nbr, float *a, void *workspace,
                            size_t workspace_bytes, void *stream_)
{
    if (m <= 0) return 0;
    if (k <= 0 || nbr_stride < k || mode < 1 || mode > 3 || !p || !posmask || !nbr || !a || !workspace ||
        workspace_bytes < amc3d_ambiguity_workspace_bytes(m))
        return bad_arg("amc3d_ambiguity: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    int *max_npos = (int *)workspace;  // [0..63] header, then n_pos, d_pos, d_neg
    int *n_pos = (int *)((char *)workspace + 64);
    float *d_pos = (float *)(n_pos + m);
    float *d_neg = d_pos + m;
    if (int st = fill_i32(max_npos, 0, 1, stream)) return st;
    hipLaunchKernelGGL(ambiguity_stats_kernel, dim3(div_up(m, 256)), dim3(256), 0, stream, m, k, nbr_stride, mode, p,
                       posmask, nbr, n_pos, d_pos, d_neg, max_npos);
    hipLaunchKernelGGL(ambiguity_kernel, dim3(div_up(m, 256)), dim3(256), 0, stream, m, k, beta, n_pos, d_pos, d_neg,
                       max_npos, a);
    return launch_status("amc3d_ambiguity");
}

AMC_API int amc3d_loss_rows_supported(int k) { return (k >= 1 && k <= 64) ? 1 : 0; }

AMC_API int amc3d_loss_rows(int m, int k, int nbr_stride, int mode, float beta, const int *labels, const float *p,
                            const int *nbr, unsigned char *posmask, float *a, void *workspace, size_t workspace_bytes,
                            void *stream_)
{
    if (m <= 0) return 0;
    if (!amc3d_loss_rows_supported(k) || nbr_stride < k || mode < 1 || mode > 3 || !labels || !p || !nbr || !posmask ||
        !workspace || workspace_bytes < amc3d_ambiguity_workspace_bytes(m))
        return bad_arg("amc3d_loss_rows: bad argument (k must be in 1..64)");
    hipStream_t stream = (hipStream_t)stream_;
    int *max_npos = (int *)workspace;  // amc3d_ambiguity's layout
    int *n_pos = (int *)((char *)workspace + 64);
    float *d_pos = (float *)(n_pos + m);
    float *d_neg = d_pos + m;
    if (int st = fill_i32(max_npos, 0, 1, stream)) return st;
    const size_t lds = (size_t)LR_PTS * (5 * (size_t)k + 20);
    hipLaunchKernelGGL(loss_rows_kernel, dim3(div_up(m, LR_PTS)), dim3(256), lds, stream, m, k, nbr_stride, mode, labels, p,
                       nbr, posmask, n_pos, d_pos, d_neg, max_npos);
    if (a)
        hipLaunchKernelGGL(ambiguity_kernel, dim3(div_up(m, 256)), dim3(256), 0, stream, m, k, beta, n_pos, d_pos, d_neg,
                           max_npos, a);
    return launch_status("amc3d_loss_rows");
}

AMC_API size_t amc3d_select_anchors_ints(int m) { return (size_t)(m > 0 ? m : 0) + 1 + (size_t)div_up(m > 0 ? m : 1, 256); }

AMC_API int amc3d_select_anchors(int m, const float *a, int *sel, size_t sel_ints, void *stream_)
{
    if (m < 0 || !sel || sel_ints < amc3d_select_anchors_ints(m) || (m > 0 && !a))
        return bad_arg("amc3d_select_anchors: bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    if (m == 0) return fill_i32(sel, 0, 1, stream);
    const int nb = div_up(m, 256);
    hipLaunchKernelGGL(select_count_kernel, dim3(nb), dim3(256), 0, stream, m, a, sel);
    hipLaunchKernelGGL(select_write_kernel, dim3(nb), dim3(256), 0, stream, m, a, sel);
    return launch_status("amc3d_select_anchors");
}

// Width dispatch.  The unit-row and row-gather kernels are instantiated for C = 4 * LPR in {16, 32, 64, 128, 256}:
// fn(std::integral_constant<int, LPR>) is called with the constant; false for any other width.

template <class F>
static bool with_lpr(int C, F &&fn)
{
    switch (C) {
    case 16: fn(int_c<4>{}); return true;
    case 32: fn(int_c<8>{}); return true;
    case 64: fn(int_c<16>{}); return true;
    case 128: fn(int_c<32>{}); return true;
    case 256: fn(int_c<64>{}); return true;
    default: return false;
    }
}

// the wide rows kernel beside them: P float4 pieces per lane cover C = 4 * C4 <= 256 * P
template <class F>
static void with_wide_p(int C, F &&fn)
{
    if (C < 256) fn(int_c<1>{});
    else fn(int_c<2>{});
}

// the float-atomic walks: LPA lanes per anchor, VPT channels per lane, C <= LPA * VPT <= 512
template <class F>
static void with_lpa_vpt(int C, F &&fn)
{
    if (C <= 32) fn(int_c<32>{}, int_c<1>{});
    else if (C <= 64) fn(int_c<64>{}, int_c<1>{});
    else if (C <= 128) fn(int_c<64>{}, int_c<2>{});
    else if (C <= 256) fn(int_c<64>{}, int_c<4>{});
    else fn(int_c<64>{}, int_c<8>{});
}

// the forwards take the unit-row kernels (amc3d_contrast_forward and amc3d_contrast_variant_forward make the same choice:
// their cosines then agree to the bit); the row kernels index 16-byte pieces with 32 bits: m * C / 4 < 2^32
static bool contrast_rows_ok(const float *f, const float *unit, int m, int C)
{
    return unit && ((((uintptr_t)f) | ((uintptr_t)unit)) & 15) == 0 && amc3d_contrast_backward_csr_supported(C) &&
           (long)m * C < (1L << 34);
}

// cm_b > 0: f is channel-major (cm_b, C, m / cm_b) and only the unit-row kernels apply
static int contrast_forward_launch(int cm_b, int m, int C, int k, int nbr_stride, const float *f, const int *nbr,
                                   const unsigned char *posmask, const float *a, const int *sel, float mu, float nu,
                                   float temperature, float *norm, float *unit, float *sim, float *stats, float *loss_pt,
                                   float *mean_cnt, hipStream_t stream)
{
    const bool rows = contrast_rows_ok(f, unit, m, C);
    if (cm_b > 0 && !rows) return bad_arg("amc3d_contrast_forward_cm: C must be 16, 32, 64, 128 or 256; unit required, 16-byte aligned");
    if (!sim && !(rows && stats)) return bad_arg("amc3d_contrast_forward: sim may be NULL only with the unit-row kernels and stats");
    if (rows) {
        const bool launched = with_lpr(C, [&](auto lpr) {
            constexpr int LPR = decltype(lpr)::value;
            if (cm_b > 0) {
                constexpr int TP = LPR >= 32 ? 16 : 64;
                const size_t lds = (size_t)4 * LPR * (TP + 1) * sizeof(float);
                hipLaunchKernelGGL((row_unit_cm_kernel<LPR, TP>), dim3(div_up(m / cm_b, TP), cm_b), dim3(256), lds, stream,
                                   m / cm_b, f, norm, unit);
            } else
                hipLaunchKernelGGL((row_unit_kernel<LPR>), dim3(div_up((long)m * LPR, 256)), dim3(256), 0, stream, m, f, norm, unit);
            hipLaunchKernelGGL((contrast_forward_unit_kernel<LPR>), dim3(div_up(m, 4)), dim3(256), 0, stream, m, k, nbr_stride,
                               (const float *)unit, nbr, posmask, a, sel, mu, nu, temperature, sim, stats, loss_pt);
        });
        if (!launched) return bad_arg("amc3d_contrast_forward: no unit-row kernel for this width");
    } else {
        hipLaunchKernelGGL(row_norm_kernel, dim3(div_up(m, 4)), dim3(256), 0, stream, m, C, f, norm);
        hipLaunchKernelGGL(contrast_forward_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, C, k,
                           nbr_stride, f, norm, nbr, posmask, a, sel, mu, nu, temperature, sim, loss_pt);
    }
    // anchors the list skips never write loss_pt; masked_mean_kernel reads the selected ones only
    hipLaunchKernelGGL(masked_mean_kernel, dim3(1), dim3(1024), 0, stream, m, loss_pt, a, mean_cnt);
    return launch_status("amc3d_contrast_forward");
}

AMC_API int amc3d_contrast_forward(int m, int C, int k, int nbr_stride, const float *f, const int *nbr,
                                   const unsigned char *posmask, const float *a, const int *sel, float mu, float nu,
                                   float temperature, float *norm, float *unit, float *sim, float *stats, float *loss_pt,
                                   float *mean_cnt, void *stream_)
{
    if (m <= 0) return 0;
    if (C <= 0 || k <= 0 || nbr_stride < k || !f || !nbr || !posmask || !a || !norm || !loss_pt || !mean_cnt)
        return bad_arg("amc3d_contrast_forward: bad argument");
    return contrast_forward_launch(0, m, C, k, nbr_stride, f, nbr, posmask, a, sel, mu, nu, temperature, norm, unit, sim, stats,
                                   loss_pt, mean_cnt, (hipStream_t)stream_);
}

// the same on channel-major embeddings f_cm (b, C, n), m = b * n anchors in cloud-major order (the decoder's layout: no
// point-major copy of f is made; unit receives the point-major unit rows the backward reads)
AMC_API int amc3d_contrast_forward_cm(int b, int C, int n, int k, int nbr_stride, const float *f_cm, const int *nbr,
                                      const unsigned char *posmask, const float *a, const int *sel, float mu, float nu,
                                      float temperature, float *norm, float *unit, float *sim, float *stats, float *loss_pt,
                                      float *mean_cnt, void *stream_)
{
    if (b <= 0 || n <= 0) return 0;
    if ((long)b * n > 0x7fffffffL || C <= 0 || k <= 0 || nbr_stride < k || !f_cm || !nbr || !posmask || !a || !norm || !unit ||
        !loss_pt || !mean_cnt)
        return bad_arg("amc3d_contrast_forward_cm: bad argument");
    return contrast_forward_launch(b, b * n, C, k, nbr_stride, f_cm, nbr, posmask, a, sel, mu, nu, temperature, norm, unit, sim,
                                   stats, loss_pt, mean_cnt, (hipStream_t)stream_);
}

AMC_API int amc3d_contrast_backward(int m, int C, int k, int nbr_stride, const float *f, const float *norm,
                                    const int *nbr, const unsigned char *posmask, const float *a, const int *sel,
                                    float mu, float nu, float temperature, const float *sim, const float *mean_cnt,
                                    const float *grad_out, float *grad_f, void *stream_)
{
    if (m <= 0) return 0;
    if (C <= 0 || C > 512 || k <= 0 || !f || !norm || !nbr || !posmask || !a || !sim || !mean_cnt || !grad_out || !grad_f)
        return bad_arg("amc3d_contrast_backward: bad argument (C must be in 1..512)");
    hipStream_t stream = (hipStream_t)stream_;
    with_lpa_vpt(C, [&](auto lpa, auto vpt) {
        constexpr int LPA = decltype(lpa)::value, VPT = decltype(vpt)::value;
        hipLaunchKernelGGL((contrast_backward_kernel<LPA, VPT>), dim3(div_up((long)m * LPA, 256)), dim3(256), 0, stream, m, C, k,
                           nbr_stride, f, norm, nbr, posmask, a, sel, mu, nu, temperature, sim, mean_cnt, grad_out, grad_f);
    });
    return launch_status("amc3d_contrast_backward");
}

AMC_API int amc3d_contrast_backward_csr_supported(int C)
{
    return C == 16 || C == 32 || C == 64 || C == 128 || C == 256;
}

AMC_API int amc3d_contrast_backward_rows_supported(int C) { return C % 4 == 0 && C >= 4 && C <= 512; }

// gradient rows from gco over the reverse lists: the power-of-two widths on their kernels, every other width of
// amc3d_contrast_backward_rows_supported on the wide one
static void contrast_rows_launch(int m, int C, int k, int nbr_stride, const float *f, const float *norm, const int *nbr,
                                 const float *a, const int *rev, const float *sim, const float *gco, float *grad_f,
                                 hipStream_t stream)
{
    const bool narrow = with_lpr(C, [&](auto lpr) {
        hipLaunchKernelGGL((contrast_backward_rows_kernel<decltype(lpr)::value>), dim3(div_up(m, 4)), dim3(256), 0, stream, m, k,
                           nbr_stride, f, norm, nbr, a, rev, sim, gco, grad_f);
    });
    if (!narrow)
        with_wide_p(C, [&](auto p) {
            hipLaunchKernelGGL((contrast_backward_rows_wide_kernel<decltype(p)::value>), dim3(div_up(m, 4)), dim3(256), 0, stream,
                               m, C / 4, k, nbr_stride, f, norm, nbr, a, rev, sim, gco, grad_f);
        });
}

AMC_API int amc3d_contrast_backward_csr(int m, int C, int k, int nbr_stride, const float *f, const float *norm,
                                        const int *nbr, const unsigned char *posmask, const float *a, const int *sel,
                                        const int *rev, float mu, float nu, float temperature, const float *sim,
                                        const float *mean_cnt, const float *grad_out, float *gco, float *grad_f,
                                        void *stream_)
{
    if (m <= 0) return 0;
    if (!amc3d_contrast_backward_rows_supported(C) || k <= 0 || nbr_stride < k || !f || !norm || !nbr || !posmask || !a ||
        !sel || !rev || !sim || !mean_cnt || !grad_out || !gco || !grad_f || (((uintptr_t)f | (uintptr_t)grad_f) & 15))
        return bad_arg("amc3d_contrast_backward_csr: bad argument (C must be a multiple of 4 in 4..512; 16-byte aligned rows)");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(contrast_coef_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, k, posmask, a, sel, mu,
                       nu, temperature, sim, mean_cnt, grad_out, gco);
    contrast_rows_launch(m, C, k, nbr_stride, f, norm, nbr, a, rev, sim, gco, grad_f, stream);
    return launch_status("amc3d_contrast_backward_csr");
}

static bool contrast_form_ok(int margin_mode, int db, int method, int has_temperature, float temperature)
{
    return margin_mode >= 0 && margin_mode <= 2 && db >= 0 && db <= 2 && (method == 1 || method == 2) &&
           (has_temperature == 0 || (has_temperature == 1 && temperature != 0.f));
}

AMC_API int amc3d_contrast_variant_forward(int m, int C, int k, int nbr_stride, const float *f, const int *nbr,
                                           const unsigned char *posmask, const float *a, const int *sel, int margin_mode,
                                           int db, int method, int has_temperature, float mu, float nu, float temperature,
                                           float *norm, float *unit, float *sim, float *loss_pt, float *mean_cnt,
                                           void *stream_)
{
    if (m <= 0) return 0;
    if (C <= 0 || k <= 0 || nbr_stride < k || !f || !nbr || !posmask || !a || !norm || !sim || !loss_pt || !mean_cnt ||
        !contrast_form_ok(margin_mode, db, method, has_temperature, temperature))
        return bad_arg("amc3d_contrast_variant_forward: bad argument (margin_mode 0..2, db 0..2, method 1..2, has_temperature 0..1)");
    hipStream_t stream = (hipStream_t)stream_;
    const ContrastForm F{margin_mode, db, method, has_temperature, mu, nu, temperature};
    if (contrast_rows_ok(f, unit, m, C)) {
        const bool launched = with_lpr(C, [&](auto lpr) {
            constexpr int LPR = decltype(lpr)::value;
            hipLaunchKernelGGL((row_unit_kernel<LPR>), dim3(div_up((long)m * LPR, 256)), dim3(256), 0, stream, m, f, norm, unit);
            hipLaunchKernelGGL((contrast_sim_unit_kernel<LPR>), dim3(div_up(m, 4)), dim3(256), 0, stream, m, k, nbr_stride,
                               (const float *)unit, nbr, a, sel, sim);
        });
        if (!launched) return bad_arg("amc3d_contrast_variant_forward: no unit-row kernel for this width");
    } else {
        hipLaunchKernelGGL(row_norm_kernel, dim3(div_up(m, 4)), dim3(256), 0, stream, m, C, f, norm);
        hipLaunchKernelGGL(contrast_sim_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, C, k, nbr_stride, f,
                           (const float *)norm, nbr, a, sel, sim);
    }
    hipLaunchKernelGGL(contrast_variant_loss_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, k, posmask, a, sel,
                       F, (const float *)sim, loss_pt);
    hipLaunchKernelGGL(masked_mean_kernel, dim3(1), dim3(1024), 0, stream, m, loss_pt, a, mean_cnt);
    return launch_status("amc3d_contrast_variant_forward");
}

AMC_API int amc3d_contrast_variant_backward(int m, int C, int k, int nbr_stride, const float *f, const float *norm,
                                            const int *nbr, const unsigned char *posmask, const float *a, const int *sel,
                                            const int *rev, int margin_mode, int db, int method, int has_temperature,
                                            float mu, float nu, float temperature, const float *sim, const float *mean_cnt,
                                            const float *grad_out, float *gco, float *grad_f, void *stream_)
{
    if (m <= 0) return 0;
    if (C <= 0 || C > 512 || k <= 0 || nbr_stride < k || !f || !norm || !nbr || !posmask || !a || !sim || !mean_cnt ||
        !grad_out || !gco || !grad_f || !contrast_form_ok(margin_mode, db, method, has_temperature, temperature))
        return bad_arg("amc3d_contrast_variant_backward: bad argument (C in 1..512, margin_mode 0..2, db 0..2, method 1..2)");
    if (rev && (!sel || !amc3d_contrast_backward_rows_supported(C) || (((uintptr_t)f | (uintptr_t)grad_f) & 15) ||
                (long)m * k > 0x7fffffffL))
        return bad_arg("amc3d_contrast_variant_backward: rev needs sel, C a multiple of 4 in 4..512 and 16-byte aligned rows");
    hipStream_t stream = (hipStream_t)stream_;
    const ContrastForm F{margin_mode, db, method, has_temperature, mu, nu, temperature};
    hipLaunchKernelGGL(contrast_variant_coef_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, k, posmask, a, sel,
                       F, sim, mean_cnt, grad_out, gco);
    if (rev) {
        contrast_rows_launch(m, C, k, nbr_stride, f, norm, nbr, a, rev, sim, gco, grad_f, stream);
    } else {
        with_lpa_vpt(C, [&](auto lpa, auto vpt) {
            constexpr int LPA = decltype(lpa)::value, VPT = decltype(vpt)::value;
            hipLaunchKernelGGL((contrast_backward_edges_kernel<LPA, VPT>), dim3(div_up((long)m * LPA, 256)), dim3(256), 0, stream,
                               m, C, k, nbr_stride, f, norm, nbr, a, sel, sim, (const float *)gco, grad_f);
        });
    }
    return launch_status("amc3d_contrast_variant_backward");
}

AMC_API size_t amc3d_contrast_backward_mutual_workspace_bytes(int m) { return (size_t)(m > 0 ? m : 0) * sizeof(ContrastRecord) + 64; }

// grad_f (m,C): every row written once (no zero-initialisation, no atomics).  mutual / rev from amc3d_contrast_mutual on the
// same neighbour lists and ambiguities; unit (the rows f_i / norm_i), sim, norm, mean_cnt as amc3d_contrast_forward left them.
AMC_API int amc3d_contrast_backward_mutual(int m, int C, int k, int nbr_stride, const float *unit, const float *norm,
                                           const int *nbr, const unsigned char *posmask, const float *a,
                                           const unsigned char *mutual, const int *rev, float mu, float nu, float temperature,
                                           const float *sim, const float *stats, const float *mean_cnt, const float *grad_out,
                                           void *workspace, size_t workspace_bytes, float *grad_f, void *stream_)
{
    if (m <= 0) return 0;
    if (!amc3d_contrast_backward_csr_supported(C) || k <= 0 || nbr_stride < k || !unit || !norm || !nbr || !posmask || !a || !mutual ||
        !rev || (!sim && !stats) || !mean_cnt || !grad_out || !grad_f || !workspace ||
        workspace_bytes < amc3d_contrast_backward_mutual_workspace_bytes(m) || (long)m * C >= (1L << 34) ||
        (((uintptr_t)unit | (uintptr_t)grad_f | (uintptr_t)workspace) & 15))
        return bad_arg("amc3d_contrast_backward_mutual: bad argument (C must be 16, 32, 64, 128 or 256; 16-byte aligned rows)");
    hipStream_t stream = (hipStream_t)stream_;
    ContrastRecord *rec = (ContrastRecord *)workspace;
    if (stats)
        hipLaunchKernelGGL(contrast_record_stats_kernel, dim3(div_up(m, 256)), dim3(256), 0, stream, m, norm, a, mu, nu, temperature, stats,
                           mean_cnt, grad_out, rec);
    else
        hipLaunchKernelGGL(contrast_record_kernel, dim3(div_up((long)m * 32, 256)), dim3(256), 0, stream, m, k, norm, posmask, a, mu, nu,
                           temperature, sim, mean_cnt, grad_out, rec);
    const bool launched = with_lpr(C, [&](auto lpr) {
        hipLaunchKernelGGL((contrast_backward_mutual_kernel<decltype(lpr)::value>), dim3(div_up(m, 4)), dim3(256), 0, stream, m, k,
                           nbr_stride, unit, nbr, posmask, mutual, rev, (const ContrastRecord *)rec, temperature, grad_f);
    });
    if (!launched) return bad_arg("amc3d_contrast_backward_mutual: no row kernel for this width");
    return launch_status("amc3d_contrast_backward_mutual");
}

// what the single-stage entries require, of every stage, before anything is launched
static bool contrast_stages_ok(int nstages, const AmcContrastStage *stages, bool backward)
{
    if (nstages < 0 || nstages > AMC_CONTRAST_MAX_STAGES || !stages) return false;
    for (int s = 0; s < nstages; ++s) {
        const AmcContrastStage &t = stages[s];
        if (t.b <= 0 || t.n <= 0 || (long)t.b * t.n > 0x7fffffffL || !amc3d_contrast_backward_csr_supported(t.C) || t.k <= 0 ||
            t.nbr_stride < t.k || (long)t.b * t.n * t.C >= (1L << 34) || !t.nbr || !t.posmask || !t.a || !t.norm || !t.unit ||
            !t.stats || !t.mean_cnt || (((uintptr_t)t.unit) & 15))
            return false;
        if (backward ? (!t.mutual || !t.rev || !t.grad_cm) : (!t.f_cm || !t.sel || !t.loss_pt || (((uintptr_t)t.f_cm) & 15)))
            return false;
    }
    return true;
}

// The kernel argument of one launch: blocks(stage) blocks per stage, one after the other.  False where the grid leaves 31 bits.
// fewest_first: the stages with the fewest blocks lead the grid (the order of S.st is the kernel's own business) -- in the
// gather a short, wide stage is a few hundred workgroups whose waves each walk several rows one after the other; at the end
// of the grid that chain would run alone, at its head it runs beside the bulk of the fine stages.
template <class F>
static bool contrast_stages_grid(ContrastStages &S, F &&blocks, bool fewest_first = false)
{
    long count[AMC_CONTRAST_MAX_STAGES];
    for (int s = 0; s < S.nstages; ++s) count[s] = blocks(S.st[s]);
    if (fewest_first)
        for (int s = 1; s < S.nstages; ++s)  // (insertion sort, stable)
            for (int t = s; t > 0 && count[t] < count[t - 1]; --t) {
                std::swap(count[t], count[t - 1]);
                std::swap(S.st[t], S.st[t - 1]);
            }
    long total = 0;
    for (int s = 0; s < S.nstages; ++s) {
        S.first[s] = (int)total;
        total += count[s];
        if (total > 0x7fffffffL) return false;
    }
    for (int s = S.nstages; s <= AMC_CONTRAST_MAX_STAGES; ++s) S.first[s] = (int)total;
    return true;
}

// (tile points of the width C, as the kernels' switch chooses them) -> blocks and LDS bytes of a tiled stage
template <class TileOf>
static void contrast_stage_tiles(const AmcContrastStage &t, TileOf &&tile_of, long &blocks, size_t &lds)
{
    with_lpr(t.C, [&](auto lpr) {
        const int TP = tile_of(lpr);
        blocks = (long)t.b * div_up(t.n, TP);
        lds = (size_t)t.C * (TP + 1) * sizeof(float);
    });
}

static ContrastStages contrast_stages_arg(int nstages, const AmcContrastStage *stages)
{
    ContrastStages S{};
    S.nstages = nstages;
    for (int s = 0; s < nstages; ++s) S.st[s] = stages[s];
    return S;
}

AMC_API int amc3d_contrast_stages_forward_cm(int nstages, const AmcContrastStage *stages, float mu, float nu, float temperature,
                                             float scale, float *total, void *stream_)
{
    if (nstages == 0) return 0;
    if (!contrast_stages_ok(nstages, stages, false) || !total)
        return bad_arg("amc3d_contrast_stages_forward_cm: bad argument (1..8 stages; C must be 16, 32, 64, 128 or 256; f_cm and unit 16-byte aligned)");
    hipStream_t stream = (hipStream_t)stream_;
    ContrastStages tiles = contrast_stages_arg(nstages, stages), waves = tiles;
    size_t lds = 0;
    auto unit_blocks = [&](const AmcContrastStage &t) {
        long blocks = 0;
        size_t bytes = 0;
        contrast_stage_tiles(t, [](auto lpr) { return unit_tile_points<decltype(lpr)::value>(); }, blocks, bytes);
        lds = bytes > lds ? bytes : lds;
        return blocks;
    };
    if (!contrast_stages_grid(tiles, unit_blocks) ||
        !contrast_stages_grid(waves, [](const AmcContrastStage &t) { return (long)div_up((long)t.b * t.n, 4); }))
        return bad_arg("amc3d_contrast_stages_forward_cm: the stages' blocks do not fit one grid");
    hipLaunchKernelGGL(contrast_stages_unit_kernel, dim3(tiles.first[nstages]), dim3(256), lds, stream, tiles);
    hipLaunchKernelGGL(contrast_stages_forward_kernel, dim3(waves.first[nstages]), dim3(256), 0, stream, waves, mu, nu, temperature);
    hipLaunchKernelGGL(contrast_stages_mean_kernel, dim3(1), dim3(1024), 0, stream, waves, scale, total);
    return launch_status("amc3d_contrast_stages_forward_cm");
}

// the records of stage s start at rec_offset(s) bytes of the workspace (64-byte steps)
static size_t contrast_stages_rec_bytes(const AmcContrastStage &t) { return ((size_t)t.b * t.n * sizeof(ContrastRecord) + 63) / 64 * 64; }

AMC_API size_t amc3d_contrast_stages_backward_cm_workspace_bytes(int nstages, const AmcContrastStage *stages)
{
    size_t bytes = 64;
    if (nstages < 0 || nstages > AMC_CONTRAST_MAX_STAGES || !stages) return bytes;
    for (int s = 0; s < nstages; ++s)
        if (stages[s].b > 0 && stages[s].n > 0) bytes += contrast_stages_rec_bytes(stages[s]);
    return bytes;
}

AMC_API int amc3d_contrast_stages_backward_cm(int nstages, const AmcContrastStage *stages, float mu, float nu, float temperature,
                                              float scale, const float *grad_out, void *workspace, size_t workspace_bytes,
                                              void *stream_)
{
    if (nstages == 0) return 0;
    if (!contrast_stages_ok(nstages, stages, true) || !grad_out || !workspace || (((uintptr_t)workspace) & 15) ||
        workspace_bytes < amc3d_contrast_stages_backward_cm_workspace_bytes(nstages, stages))
        return bad_arg("amc3d_contrast_stages_backward_cm: bad argument (1..8 stages; C must be 16, 32, 64, 128 or 256; unit and workspace 16-byte aligned)");
    hipStream_t stream = (hipStream_t)stream_;
    ContrastStages anchors = contrast_stages_arg(nstages, stages);
    size_t at = 0;
    for (int s = 0; s < nstages; ++s) {
        anchors.st[s].rec = (char *)workspace + at;
        at += contrast_stages_rec_bytes(anchors.st[s]);
    }
    ContrastStages tiles = anchors;
    size_t lds = 0;
    auto grad_blocks = [&](const AmcContrastStage &t) {
        long blocks = 0;
        size_t bytes = 0;
        contrast_stage_tiles(t, [](auto lpr) { return grad_tile_points<decltype(lpr)::value>(); }, blocks, bytes);
        lds = bytes > lds ? bytes : lds;
        return blocks;
    };
    if (!contrast_stages_grid(anchors, [](const AmcContrastStage &t) { return (long)div_up((long)t.b * t.n, 256); }) ||
        !contrast_stages_grid(tiles, grad_blocks, true))
        return bad_arg("amc3d_contrast_stages_backward_cm: the stages' blocks do not fit one grid");
    hipLaunchKernelGGL(contrast_stages_record_kernel, dim3(anchors.first[nstages]), dim3(256), 0, stream, anchors, mu, nu, temperature,
                       scale, grad_out);
    hipLaunchKernelGGL(contrast_stages_backward_kernel, dim3(tiles.first[nstages]), dim3(256), lds, stream, tiles, temperature);
    return launch_status("amc3d_contrast_stages_backward_cm");
}

// ---------------------------------------------------------------------------------------------
// Confusion matrix of the training predictions (main_AA.py:414-415: cm.update(logits.argmax(dim=1), target), every
// iteration): arg-max over the class planes of channel-major logits (first maximum, as torch.argmax) and a v x v histogram,
// v = C (+1 when an ignore label exists: points with target == ignore count in the extra row/column, utils/metrics.py).  One
// launch: a histogram per workgroup in LDS, then one 64-bit atomic per non-empty bin -- the tensor form is an arg-max, ten
// elementwise launches and 192000 int64 atomics onto 169 addresses.  invalid += points whose target is outside [0, v).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void confusion_kernel(int C, long N, int v, long long ignore, int has_ignore,
                                                        const float *__restrict__ logits, const long long *__restrict__ target,
                                                        long long *__restrict__ cm, long long *__restrict__ invalid)
{
    extern __shared__ int s_bins[];  // v * v + 1
    for (int i = threadIdx.x; i <= v * v; i += 256) s_bins[i] = 0;
    __syncthreads();
    const int b = blockIdx.y;
    for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long)gridDim.x * 256) {
        const float *lp = logits + (size_t)b * C * N + n;
        float best = lp[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float x = lp[(size_t)c * N];
            if (x > best || (x != x && best == best)) { best = x; arg = c; }  // first maximum; a NaN wins, as in torch
        }
        long long t = target[(size_t)b * N + n];
        int p = arg;
        if (has_ignore && t == ignore) { t = v - 1; p = v - 1; }
        if (t >= 0 && t < v) atomicAdd(&s_bins[(int)t * v + p], 1);
        else atomicAdd(&s_bins[v * v], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < v * v; i += 256)
        if (s_bins[i]) atomicAdd((unsigned long long *)(cm + i), (unsigned long long)s_bins[i]);
    if (threadIdx.x == 0 && s_bins[v * v]) atomicAdd((unsigned long long *)invalid, (unsigned long long)s_bins[v * v]);
}

// cm (v*v) int64 += histogram of (target, argmax_c logits) over the B*N points; invalid (1) int64 += out-of-range targets.
// v = C + has_ignore <= 64.
AMC_API int amc3d_confusion_update(int B, int C, long N, const float *logits, const long long *target, long long ignore,
                                   int has_ignore, long long *cm, long long *invalid, void *stream_)
{
    if (B <= 0 || N <= 0) return 0;
    const int v = C + (has_ignore ? 1 : 0);
    if (C <= 0 || v > 64 || !logits || !target || !cm || !invalid) return bad_arg("amc3d_confusion_update: bad argument (at most 64 classes)");
    const int bx = (int)(div_up(N, 256) < 64 ? div_up(N, 256) : 64);
    hipLaunchKernelGGL(confusion_kernel, dim3(bx, B), dim3(256), (size_t)(v * v + 1) * sizeof(int), (hipStream_t)stream_, C, N, v, ignore,
                       has_ignore, logits, target, cm, invalid);
    return launch_status("amc3d_confusion_update");
}

AMC_API size_t amc3d_cross_entropy_workspace_bytes(int B, long N)
{
    return (size_t)(B > 0 ? B : 0) * (size_t)div_up(N > 0 ? N : 1, CE_THREADS) * 2 * sizeof(double);
}

// What the forward entries of both point-loss families share: the argument check, the grid (ceil(N / 256), B), the per-point
// kernel -- kernel(C, N, logits, target, args..., partials) -- and pl_finalize_kernel over the blocks' partials.  form_ok:
// the entry's own arguments are present and in range; hint: those ranges, for the error text.
template <typename Kernel, typename... Args>
static int pl_forward(const char *what, const char *hint, Kernel kernel, bool form_ok, int B, int C, long N, const float *logits,
                      const long long *target, int den_mode, float *loss_den, void *workspace, size_t workspace_bytes,
                      void *stream_, Args... args)
{
    if (B <= 0 || N <= 0) return 0;
    if (C <= 0 || !logits || !target || !loss_den || !workspace || !form_ok ||
        workspace_bytes < amc3d_cross_entropy_workspace_bytes(B, N)) {
        set_error("%s: bad argument%s", what, hint);
        return (int)hipErrorInvalidValue;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int gx = div_up(N, CE_THREADS);
    hipLaunchKernelGGL(kernel, dim3(gx, B), dim3(CE_THREADS), 0, stream, C, N, logits, target, args..., (double *)workspace);
    hipLaunchKernelGGL(pl_finalize_kernel, dim3(1), dim3(1024), 0, stream, gx * B, (const double *)workspace, den_mode, loss_den);
    return launch_status(what);
}

// the backward entries: kernel(C, N, logits, target, args..., loss_den, grad_out, dlogits) on the same grid
template <typename Kernel, typename... Args>
static int pl_backward(const char *what, const char *hint, Kernel kernel, bool form_ok, int B, int C, long N, const float *logits,
                       const long long *target, const float *loss_den, const float *grad_out, float *dlogits, void *stream,
                       Args... args)
{
    if (B <= 0 || N <= 0) return 0;
    if (C <= 0 || !logits || !target || !loss_den || !grad_out || !dlogits || !form_ok) {
        set_error("%s: bad argument%s", what, hint);
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(kernel, dim3(div_up(N, CE_THREADS), B), dim3(CE_THREADS), 0, (hipStream_t)stream, C, N, logits, target,
                       args..., loss_den, grad_out, dlogits);
    return launch_status(what);
}

// nn.CrossEntropyLoss() with its defaults: the softmax form with nothing but the ignore value set
static PlSoftmax pl_plain_form(long long ignore_index)
{
    return PlSoftmax{nullptr, 0, ignore_index, 1, nullptr, nullptr, 0, 1.f, 0.f, 0.f, nullptr, 0.f, PL_DEN_COUNT};
}

AMC_API int amc3d_cross_entropy_forward(int B, int C, long N, const float *logits, const long long *target,
                                        long long ignore_index, float *lse, float *mean_cnt, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    return pl_forward("amc3d_cross_entropy_forward", "", pl_softmax_forward_kernel<true>, lse != nullptr, B, C, N, logits, target,
                      PL_DEN_COUNT, mean_cnt, workspace, workspace_bytes, stream, pl_plain_form(ignore_index), lse);
}

AMC_API int amc3d_cross_entropy_backward(int B, int C, long N, const float *logits, const long long *target,
                                         long long ignore_index, const float *lse, const float *mean_cnt,
                                         const float *grad_out, float *dlogits, void *stream)
{
    return pl_backward("amc3d_cross_entropy_backward", "", pl_softmax_backward_kernel<true>, lse != nullptr, B, C, N, logits, target,
                       mean_cnt, grad_out, dlogits, stream, pl_plain_form(ignore_index), lse);
}

// the form of a softmax-family call from the C-ABI's arguments; false: an argument is out of range
static bool pl_softmax_form(int C, const long long *remap, int remap_len, long long ignore_index, int has_ignore, const int *mask,
                            const float *weight, int weight_per_class, float eps, int eps_rule, float gamma, const float *alpha,
                            float poly, int den_mode, PlSoftmax *f)
{
    if (!(eps >= 0.f && eps < 1.f) || eps_rule < 0 || eps_rule > 1 || den_mode < PL_DEN_COUNT || den_mode > PL_DEN_ONE ||
        !(gamma >= 0.f) || (remap && remap_len <= 0))
        return false;
    float a_hot = 1.f, a_off = 0.f;
    if (eps > 0.f && eps_rule == 0) {  // torch: eps / C on every class
        a_off = eps / (float)C;
        a_hot = 1.f - eps + a_off;
    } else if (eps > 0.f) {            // the reference: eps / (C - 1) on the others (C = 1: 0 * eps / 0 = NaN there, and here)
        a_off = eps / (float)(C - 1);
        a_hot = C > 1 ? 1.f - eps : __builtin_nanf("");
    }
    *f = PlSoftmax{remap, remap ? remap_len : 0, ignore_index, has_ignore, mask, weight, weight ? weight_per_class : 0, a_hot, a_off,
                   gamma, alpha, poly, den_mode};
    return true;
}

static const char *const PL_SOFTMAX_HINT = " (eps in [0, 1), gamma >= 0, den_mode in 0..2)";

AMC_API int amc3d_point_loss_softmax_forward(int B, int C, long N, const float *logits, const long long *target,
                                             const long long *remap, int remap_len, long long ignore_index, int has_ignore,
                                             const int *mask, const float *weight, int weight_per_class, float eps, int eps_rule,
                                             float gamma, const float *alpha, float poly, int den_mode, float *lse, float *loss_den,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    PlSoftmax f;
    const bool ok = pl_softmax_form(C, remap, remap_len, ignore_index, has_ignore, mask, weight, weight_per_class, eps, eps_rule,
                                    gamma, alpha, poly, den_mode, &f);
    return pl_forward("amc3d_point_loss_softmax_forward", PL_SOFTMAX_HINT, pl_softmax_forward_kernel<false>, ok && lse, B, C, N,
                      logits, target, den_mode, loss_den, workspace, workspace_bytes, stream, f, lse);
}

AMC_API int amc3d_point_loss_softmax_backward(int B, int C, long N, const float *logits, const long long *target,
                                              const long long *remap, int remap_len, long long ignore_index, int has_ignore,
                                              const int *mask, const float *weight, int weight_per_class, float eps, int eps_rule,
                                              float gamma, const float *alpha, float poly, int den_mode, const float *lse,
                                              const float *loss_den, const float *grad_out, float *dlogits, void *stream)
{
    PlSoftmax f;
    const bool ok = pl_softmax_form(C, remap, remap_len, ignore_index, has_ignore, mask, weight, weight_per_class, eps, eps_rule,
                                    gamma, alpha, poly, den_mode, &f);
    return pl_backward("amc3d_point_loss_softmax_backward", PL_SOFTMAX_HINT, pl_softmax_backward_kernel<false>, ok && lse, B, C, N,
                       logits, target, loss_den, grad_out, dlogits, stream, f, lse);
}

static const char *const PL_SIGMOID_HINT = " (gamma >= 0, alpha <= 1, den_mode 0 or 2)";

static bool pl_sigmoid_ok(float alpha, float gamma, int den_mode)
{
    return gamma >= 0.f && alpha <= 1.f && (den_mode == PL_DEN_COUNT || den_mode == PL_DEN_ONE);
}

AMC_API int amc3d_point_loss_sigmoid_forward(int B, int C, long N, const float *logits, const long long *target,
                                             const float *weight, const float *pos_weight, float alpha, float gamma, float poly,
                                             int den_mode, float *loss_den, void *workspace, size_t workspace_bytes, void *stream)
{
    return pl_forward("amc3d_point_loss_sigmoid_forward", PL_SIGMOID_HINT, pl_sigmoid_forward_kernel,
                      pl_sigmoid_ok(alpha, gamma, den_mode), B, C, N, logits, target, den_mode, loss_den, workspace, workspace_bytes,
                      stream, PlSigmoid{weight, pos_weight, alpha, gamma, poly, den_mode});
}

AMC_API int amc3d_point_loss_sigmoid_backward(int B, int C, long N, const float *logits, const long long *target,
                                              const float *weight, const float *pos_weight, float alpha, float gamma, float poly,
                                              int den_mode, const float *loss_den, const float *grad_out, float *dlogits, void *stream)
{
    return pl_backward("amc3d_point_loss_sigmoid_backward", PL_SIGMOID_HINT, pl_sigmoid_backward_kernel,
                       pl_sigmoid_ok(alpha, gamma, den_mode), B, C, N, logits, target, loss_den, grad_out, dlogits, stream,
                       PlSigmoid{weight, pos_weight, alpha, gamma, poly, den_mode});
}
