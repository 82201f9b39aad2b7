// fp32 MFMA GEMM for the deep pointwise convolutions (>= 64 channels on both sides) of gfx950.
//
// The three products of a 1x1 convolution on channel-major (B, C, P) tensors
//     forward        Y[b]  = W        . X[b]     M = Cout, N = P,   K = Cin
//     backward-data  dX[b] = W^T      . dY[b]    M = Cin,  N = P,   K = Cout
//     backward-weight dW   = sum_b dY[b] . X[b]^T  M = Cout, N = Cin, K = P (split over workgroups)
// are one kernel:  C[m][n] = sum_k A(m,k) B(k,n)  with strided operand views.  pwconv.hip streams these well when
// the layer is HBM-bound (few channels, many positions); with >= 64 channels the MFMA pipe is the limit and that
// kernel's single-buffered 32-position wave tiles leave it half idle.  Here:
//   * 128 x 128 output tile per workgroup, 2 x 2 waves of 64 x 64 (four 32x32 accumulators: every A and B
//     fragment feeds two v_mfma_f32_32x32x2_f32), or 64 x 128 / 64 x 64 with two / one accumulators per wave: the
//     launch's workgroup count chooses (gm_tile_for), and the K walk below is the same for all three;
//   * K in chunks of 16, double-buffered in LDS; the next chunk's global loads are issued before the current
//     chunk's MFMAs and written to the other buffer after them: one barrier per chunk.  A chunk that lies inside both
//     operands is loaded by straight-line code in a loop of its own (gm_load_whole), the chunks at an edge by guarded loads;
//   * an operand that is contiguous along k in global memory is kept [row][k] in LDS (row stride 20 floats:
//     8 consecutive rows x 16 bytes cover the 32 banks once) and a lane fetches its 8 k-values of a chunk with
//     two ds_read_b128; an operand contiguous along m / n is kept as it arrives, [k][row], and read with eight
//     conflict-free ds_read_b32 (a transposing store would hit 2 of the 32 banks).
// MFMA operand convention (v_mfma_f32_32x32x2_f32): lane l supplies A[i = l & 31][kk = l >> 5] and
// B[kk = l >> 5][j = l & 31]; step t of a chunk pairs k = t (lanes 0-31) with k = 8 + t (lanes 32-63) in both
// operands -- any pairing is a valid order of the K sum as long as A and B agree.

#include <type_traits>

#include "common.h"

namespace amc {

typedef float gm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int GM_T = 128;    // the largest tile edge (M and N): what the split-K rules count tiles in
constexpr int GM_KC = 16;    // K chunk
constexpr int GM_S = 20;     // LDS row stride in floats

int reduce_partials(int total, int nparts, const float *partial, float *out, hipStream_t stream);  // gcc.hip
int reduce_partials_rows(int rows, int cols, long ld, int nparts, const float *partial, float *out, hipStream_t stream);

struct GemmView {  // element (r, k) of an operand at base[r * sr + k * sk]; exactly one of sr, sk is 1
    const float *base;
    long sr, sk;
};

// registers of one chunk of one operand: ROWS rows x 16 k = ROWS * 4 float4, ROWS / 64 per thread
template <int ROWS>
struct GmRegs {
    float4 v[ROWS / 64];
};

// KCONT: the operand is contiguous along k in global memory (natural); otherwise along its row index
template <int ROWS, bool KCONT>
__device__ __forceinline__ void gm_load(GmRegs<ROWS> &r, const GemmView &g, int row0, int nrows, long k0, long kend, bool vec)
{
    constexpr int R4 = ROWS / 4;  // float4 per k-row of a row-contiguous operand
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < ROWS / 64; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (KCONT) {
            const int row = t / 4 + 64 * j, c4 = t % 4;
            const long k = k0 + c4 * 4;
            if (row < nrows && k < kend) {
                const float *p = g.base + (long)(row0 + row) * g.sr + k;
                if (vec && k + 3 < kend) v = *reinterpret_cast<const float4 *>(p);
                else { v.x = p[0]; if (k + 1 < kend) v.y = p[1]; if (k + 2 < kend) v.z = p[2]; if (k + 3 < kend) v.w = p[3]; }
            }
        } else {
            const int krow = t / R4 + (256 / R4) * j, r4 = t % R4;
            const long k = k0 + krow;
            const int row = r4 * 4;
            if (k < kend && row < nrows) {
                const float *p = g.base + k * g.sk + (row0 + row);
                if (vec && row + 3 < nrows) v = *reinterpret_cast<const float4 *>(p);
                else { v.x = p[0]; if (row + 1 < nrows) v.y = p[1]; if (row + 2 < nrows) v.z = p[2]; if (row + 3 < nrows) v.w = p[3]; }
            }
        }
        r.v[j] = v;
    }
}

// The same registers for a chunk that lies wholly inside the operand (all ROWS rows, all 16 k): no lane tests anything.  In
// gm_load a register's value depends on which guarded branch ran (zero, the float4, one to four scalars), and the compiler joins
// those branches by waiting for the loads: vmcnt(0) after the A operand, again after each float4 of B, so a chunk paid two or
// three memory latencies in a row before its first MFMA.  Here the loads are straight-line code, and the caller keeps them in a
// copy of the loop body of their own, so the registers meet no other definition before gm_store reads them.
template <int ROWS, bool KCONT>
__device__ __forceinline__ void gm_load_whole(GmRegs<ROWS> &r, const GemmView &g, int row0, long k0, bool vec)
{
    constexpr int R4 = ROWS / 4;
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < ROWS / 64; ++j) {
        const float *p = KCONT ? g.base + (long)(row0 + t / 4 + 64 * j) * g.sr + k0 + (t % 4) * 4
                               : g.base + (k0 + t / R4 + (256 / R4) * j) * g.sk + (row0 + (t % R4) * 4);
        if (vec) r.v[j] = *reinterpret_cast<const float4 *>(p);
        else r.v[j] = make_float4(p[0], p[1], p[2], p[3]);
    }
}

template <int ROWS, bool KCONT>
__device__ __forceinline__ void gm_store(const GmRegs<ROWS> &r, float *lds)
{
    constexpr int R4 = ROWS / 4;
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < ROWS / 64; ++j) {
        if (KCONT) {
            const int row = t / 4 + 64 * j, c4 = t % 4;
            *reinterpret_cast<float4 *>(lds + row * GM_S + c4 * 4) = r.v[j];
        } else {
            const int krow = t / R4 + (256 / R4) * j, row = (t % R4) * 4;
            *reinterpret_cast<float4 *>(lds + krow * ROWS + row) = r.v[j];
        }
    }
}

// this lane's 8 k-values (k = kh*8 + t) of operand row `row` of a stage image
template <int ROWS, bool KCONT>
__device__ __forceinline__ void gm_fragment(float (&f)[8], const float *img, int row, int kh)
{
    if (KCONT) {
        const float4 lo = *reinterpret_cast<const float4 *>(img + row * GM_S + kh * 8);
        const float4 hi = *reinterpret_cast<const float4 *>(img + row * GM_S + kh * 8 + 4);
        f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
        f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) f[t] = img[(kh * 8 + t) * ROWS + row];
    }
}

// One TM x TN output tile per workgroup (TM, TN in {64, 128}): 2 x 2 waves of (TM/2) x (TN/2), that is TM/64 x TN/64
// accumulators of 32 x 32 per wave.  The K walk -- chunks of 16 in sequence, step t pairing k = t with k = 8 + t -- is the same
// for every tile, so an output element has the same bits whichever tile computed it.  LDS: two stages of (TM + TN) * GM_S.
// grid: (N tiles, M tiles, batch * splits).  Per z: batch b = z / splits, split s = z % splits owns K range
// [s * kper, min(K, (s+1) * kper)).  Output C = cbase + z * czstride (forward/backward-data: splits = 1 and
// czstride = M * ldc; backward-weight: one partial (M, N) per z).  pm != 0: C is stored transposed, C[n][m] with row length M
// (backward-data as position-major rows): the four consecutive rows of an accumulator's (r >> 2) group are one 16-byte store
// when pm == 2 (M % 4 == 0, aligned base), four 4-byte stores otherwise.
template <int TM, int TN, bool A_KCONT, bool B_KCONT>
__global__ __launch_bounds__(256) void gm_gemm_kernel(int M, int N, long K, int splits, long kper, GemmView A, long a_bstride,
                                                      GemmView B, long b_bstride, float *__restrict__ cbase, long czstride,
                                                      long ldc, int vec_a, int vec_b, int pm)
{
    constexpr int WTM = TM / 2, WTN = TN / 2, IM = WTM / 32, JN = WTN / 32;
    constexpr int STAGE = (TM + TN) * GM_S;  // floats per stage (A then B)
    extern __shared__ __attribute__((aligned(16))) float gm_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pl = lane & 31, kh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int z = blockIdx.z, bz = z / splits, sp = z - bz * splits;
    const long kbeg = (long)sp * kper, kend = min(K, kbeg + kper);
    A.base += (long)bz * a_bstride;
    B.base += (long)bz * b_bstride;
    const int mrows = min(TM, M - m0), ncols = min(TN, N - n0);

    gm_f32x16 acc[IM][JN];
#pragma unroll
    for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[i][j] = gm_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    GmRegs<TM> ra;
    GmRegs<TN> rb;
    const long nchunks = (kend - kbeg + GM_KC - 1) / GM_KC;
    const bool inside = mrows == TM && ncols == TN;  // every row of both tiles exists
    if (inside && kbeg + GM_KC <= kend) {
        gm_load_whole<TM, A_KCONT>(ra, A, m0, kbeg, vec_a);
        gm_load_whole<TN, B_KCONT>(rb, B, n0, kbeg, vec_b);
        gm_store<TM, A_KCONT>(ra, gm_smem);
        gm_store<TN, B_KCONT>(rb, gm_smem + TM * GM_S);
    } else if (nchunks > 0) {
        gm_load<TM, A_KCONT>(ra, A, m0, mrows, kbeg, kend, vec_a);
        gm_load<TN, B_KCONT>(rb, B, n0, ncols, kbeg, kend, vec_b);
        gm_store<TM, A_KCONT>(ra, gm_smem);
        gm_store<TN, B_KCONT>(rb, gm_smem + TM * GM_S);
    }
    __syncthreads();
    // One chunk: the next chunk's global loads, this chunk's MFMAs, the next chunk's LDS image, a barrier.  WHOLE: the next chunk
    // exists and lies inside both operands.  The order of the sum is that of the chunks, whichever copy of the body runs them.
    auto chunk = [&](auto whole, long c) {
        constexpr bool WHOLE = decltype(whole)::value;
        const float *as = gm_smem + (c & 1) * STAGE, *bs = as + TM * GM_S;
        const bool more = WHOLE || c + 1 < nchunks;
        if (WHOLE) {  // in flight while this chunk is multiplied
            gm_load_whole<TM, A_KCONT>(ra, A, m0, kbeg + (c + 1) * GM_KC, vec_a);
            gm_load_whole<TN, B_KCONT>(rb, B, n0, kbeg + (c + 1) * GM_KC, vec_b);
            __builtin_amdgcn_sched_barrier(0);  // issued here: the scheduler would sink them to their first use, after the MFMAs
        } else if (more) {
            gm_load<TM, A_KCONT>(ra, A, m0, mrows, kbeg + (c + 1) * GM_KC, kend, vec_a);
            gm_load<TN, B_KCONT>(rb, B, n0, ncols, kbeg + (c + 1) * GM_KC, kend, vec_b);
        }
        // this lane's 8 k-values (k = kh*8 + t) of its IM A rows and JN B columns
        float av[IM][8], bv[JN][8];
#pragma unroll
        for (int i = 0; i < IM; ++i) gm_fragment<TM, A_KCONT>(av[i], as, wm * WTM + i * 32 + pl, kh);
#pragma unroll
        for (int j = 0; j < JN; ++j) gm_fragment<TN, B_KCONT>(bv[j], bs, wn * WTN + j * 32 + pl, kh);
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int i = 0; i < IM; ++i)
#pragma unroll
                for (int j = 0; j < JN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][t], bv[j][t], acc[i][j], 0, 0, 0);
        if (more) {
            float *nas = gm_smem + ((c + 1) & 1) * STAGE;
            gm_store<TM, A_KCONT>(ra, nas);
            gm_store<TN, B_KCONT>(rb, nas + TM * GM_S);
        }
        __syncthreads();
    };
    // two loops, not one loop with a branch: each keeps the accumulators in place over its iterations
    long c = 0;
    if (inside)
        for (; kbeg + (c + 2) * GM_KC <= kend; ++c) chunk(std::true_type{}, c);
    for (; c < nchunks; ++c) chunk(std::false_type{}, c);  // the chunks before an edge of K, or every chunk of an edge tile
    // accumulator layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float *C = cbase + (long)z * czstride;
#pragma unroll
    for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) {
            const int n = n0 + wn * WTN + j * 32 + pl;
            if (n < N && pm) {
                float *row = C + (long)n * M;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int m = m0 + wm * WTM + i * 32 + 8 * g + 4 * kh;
                    if (pm == 2) {
                        if (m < M)
                            *reinterpret_cast<float4 *>(row + m) =
                                make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (m + q < M) row[m + q] = acc[i][j][4 * g + q];
                    }
                }
            } else if (n < N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (m < M) C[(long)m * ldc + n] = acc[i][j][r];
                }
            }
        }
}


// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of the deep layers, streaming form:  dW[m][n] = sum over positions p of dY[m][p] X[n][p].
// Both operands are read along their contiguous axis and nothing else is read: the pass is HBM-bound (SA2 of PointNeXt-S:
// 295 MB for 6.4 GF), and gm_gemm_kernel<true, true> served it at 1.4 TB/s -- 64-byte row pieces per 16-position chunk, a
// 128 x 128 tile of which a 64-wide layer uses half, a thousand 32 KB partials.  Here
//   * a chunk is 32 positions: every row contributes one whole 128-byte line per chunk;
//   * the tile is 128 x TN with TN = 64 or 128 (template): a wave owns 32 rows of dY and all TN rows of X, TN/32
//     accumulators -- no MFMA issued for channels that do not exist;
//   * [row][k] LDS images with a 36-float stride (8 consecutive rows x 16 bytes cover the banks once: ds_read_b128 fragments),
//     double-buffered, the next chunk's six global loads per thread in flight during the MFMAs, one barrier per chunk;
//   * position ranges long enough for ~2 workgroups per CU (fewer, larger partials; same fixed-order reduction).
// k-pairing of v_mfma_f32_32x32x2_f32 as in gm_gemm_kernel: step t multiplies positions t (lanes 0-31) and 16 + t (32-63).
// Requires P % 4 == 0 and 16-byte aligned operands (float4 loads); anything else keeps the generic kernel.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GW_KC = 32, GW_S = 36, GW_TM = 128;

template <int TN>
__global__ __launch_bounds__(256) void gw_wgrad_kernel(int M, int N, long P, int splits, long kper, const float *__restrict__ dy,
                                                       const float *__restrict__ x, float *__restrict__ partial)
{
    constexpr int ROWS = GW_TM + TN;               // dY rows then X rows of the tile
    constexpr int LPT = ROWS * (GW_KC / 4) / 256;  // float4 loads per thread and chunk: 6 (TN = 64) or 8 (TN = 128)
    constexpr int NJ = TN / 32;
    extern __shared__ __attribute__((aligned(16))) float gw_smem[];  // 2 stages x ROWS x GW_S
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pl = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.y * GW_TM, n0 = blockIdx.x * TN;
    const int z = blockIdx.z, bz = z / splits, sp = z - bz * splits;
    const long kbeg = (long)sp * kper, kend = min(P, kbeg + kper);
    const float *A = dy + (size_t)bz * M * P, *B = x + (size_t)bz * N * P;

    gm_f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = gm_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    float4 r[LPT];
    auto load = [&](long k0) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int row = threadIdx.x / 8 + 32 * i, c4 = threadIdx.x % 8;
            const long k = k0 + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < kend) {  // kend - kbeg is a multiple of 4 except at the end of P, and P % 4 == 0: whole float4s
                if (row < GW_TM) { if (m0 + row < M) v = *reinterpret_cast<const float4 *>(A + (size_t)(m0 + row) * P + k); }
                else if (n0 + row - GW_TM < N) v = *reinterpret_cast<const float4 *>(B + (size_t)(n0 + row - GW_TM) * P + k);
            }
            r[i] = v;
        }
    };
    auto store = [&](float *stage) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int row = threadIdx.x / 8 + 32 * i, c4 = threadIdx.x % 8;
            *reinterpret_cast<float4 *>(stage + row * GW_S + c4 * 4) = r[i];
        }
    };
    const long nchunks = (kend - kbeg + GW_KC - 1) / GW_KC;
    if (nchunks > 0) { load(kbeg); store(gw_smem); }
    __syncthreads();
    for (long c = 0; c < nchunks; ++c) {
        const float *as = gw_smem + (c & 1) * ROWS * GW_S, *bs = as + GW_TM * GW_S;
        const bool more = c + 1 < nchunks;
        if (more) load(kbeg + (c + 1) * GW_KC);  // in flight while this chunk is multiplied
        // this lane's 16 positions (kh * 16 + t) of its dY row and of its X rows, in two halves of 8 to bound registers
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float av[8], bv[NJ][8];
            {
                const float *pa = as + (wave * 32 + pl) * GW_S + kh * 16 + h * 8;
                const float4 lo = *reinterpret_cast<const float4 *>(pa), hi = *reinterpret_cast<const float4 *>(pa + 4);
                av[0] = lo.x; av[1] = lo.y; av[2] = lo.z; av[3] = lo.w; av[4] = hi.x; av[5] = hi.y; av[6] = hi.z; av[7] = hi.w;
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float *pb = bs + (j * 32 + pl) * GW_S + kh * 16 + h * 8;
                const float4 lo = *reinterpret_cast<const float4 *>(pb), hi = *reinterpret_cast<const float4 *>(pb + 4);
                bv[j][0] = lo.x; bv[j][1] = lo.y; bv[j][2] = lo.z; bv[j][3] = lo.w;
                bv[j][4] = hi.x; bv[j][5] = hi.y; bv[j][6] = hi.z; bv[j][7] = hi.w;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[j][t], acc[j], 0, 0, 0);
        }
        if (more) store(gw_smem + ((c + 1) & 1) * ROWS * GW_S);
        __syncthreads();
    }
    // accumulator layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float *C = partial + (size_t)z * M * N;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + j * 32 + pl;
        if (n < N) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int m = m0 + wave * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * kh;
                if (m < M) C[(size_t)m * N + n] = acc[j][rr];
            }
        }
    }
}

static int aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The tiles of gm_gemm_kernel, largest first.
constexpr int GM_NTILES = 3;
static const int gm_tiles[GM_NTILES][2] = {{128, 128}, {64, 128}, {64, 64}};

static long gm_workgroups(int tile, int M, int N, int batch, int splits)
{
    return (long)div_up(M, gm_tiles[tile][0]) * div_up(N, gm_tiles[tile][1]) * batch * splits;
}

// THE dispatch rule, read from profiles/gemm_tiles_sweep.txt (channel counts 64-512, 1500-48000 positions, 8 clouds):
//   * 64 x 128 is the tile of a launch that fills the chip: it gives at least GM_FILL workgroups (two per CU of the 256), and a
//     CU holds five of them by registers and LDS (128 x 128: three);
//   * 128 x 128 only where all its workgroups are resident at once (GM_FILL .. GM_RESIDENT = 3 per CU) and M leaves no 64-row
//     half of its tiles empty: there it is 1-3 % ahead, one round of the larger tiles against a round and a tail; with more
//     rounds than that the 64 x 128 tile is level or up to 15 % ahead;
//   * 64 x 64 where 64 x 128 gives fewer than GM_FILL workgroups: the short layers and the weight gradients.
// With the interior chunks' loads in flight during the MFMAs (gm_load_whole) the sweep, alone on the chip, moved: 64 x 64 is then
// 3-10 % ahead up to 1504 workgroups of 128 x 128 and 128 x 128 from 6000 up (profiles/gemm_core_sweep.txt).  The thresholds
// stayed all the same: in the train step, where two other queues share the CUs, eight 64 x 64 workgroups per CU (all of its LDS)
// on the filled launches cost the neighbours more than the GEMMs gain -- the step is 0.02-0.03 ms slower with "64 x 64 up to
// 4096, 128 x 128 above" than with this rule (profiles/gemm_core_ab.json).
// A function of the launch's shape only -- the same choice eager and captured, on every rank -- and free to change: every tile
// walks K alike, so the choice never shows in a result.
constexpr long GM_FILL = 512, GM_RESIDENT = 768;
static int gm_tile_for(int M, int N, int batch, int splits)
{
    const long big = gm_workgroups(0, M, N, batch, splits);
    if (big >= GM_FILL && big <= GM_RESIDENT && div_up(M, 64) == 2 * div_up(M, 128)) return 0;
    return gm_workgroups(1, M, N, batch, splits) >= GM_FILL ? 1 : 2;
}

template <int TM, int TN, bool AK, bool BK>
static void gm_launch_tile(int M, int N, long K, int batch, int splits, long kper, GemmView A, long abs_, GemmView B, long bbs,
                           float *c, long czs, long ldc, int va, int vb, hipStream_t stream, int pm)
{
    const size_t lds = 2 * (TM + TN) * GM_S * sizeof(float);
    hipLaunchKernelGGL((gm_gemm_kernel<TM, TN, AK, BK>), dim3(div_up(N, TN), div_up(M, TM), batch * splits), dim3(256), lds, stream,
                       M, N, K, splits, kper, A, abs_, B, bbs, c, czs, ldc, va, vb, pm);
}

// tile < 0: the rule's choice (every product call); 0 .. GM_NTILES - 1: that tile (amc3d_gemm_probe)
template <bool AK, bool BK>
static void gm_launch(int M, int N, long K, int batch, int splits, long kper, GemmView A, long abs_, GemmView B, long bbs,
                      float *c, long czs, long ldc, int va, int vb, hipStream_t stream, int pm = 0, int tile = -1)
{
    if (pm) pm = (M % 4 == 0 && aligned16(c) && czs % 4 == 0) ? 2 : 1;
    if (tile < 0) tile = gm_tile_for(M, N, batch, splits);
    if (tile == 0) gm_launch_tile<128, 128, AK, BK>(M, N, K, batch, splits, kper, A, abs_, B, bbs, c, czs, ldc, va, vb, stream, pm);
    else if (tile == 1) gm_launch_tile<64, 128, AK, BK>(M, N, K, batch, splits, kper, A, abs_, B, bbs, c, czs, ldc, va, vb, stream, pm);
    else gm_launch_tile<64, 64, AK, BK>(M, N, K, batch, splits, kper, A, abs_, B, bbs, c, czs, ldc, va, vb, stream, pm);
}

bool gemm_conv_pays(int cin, int cout) { return cin >= 64 && cout >= 64; }

// y (b,cout,P) = W (cout,cin) . x (b,cin,P)
// ---- short layers (SetAbstraction 4, the coarse FeaturePropagation stages: a few hundred positions per cloud, 256-768
// channels): a handful of 128 x 128 tiles per cloud, each walking the whole K axis -- 48 workgroups for 50-70 us.  The K axis
// is split over several workgroups (the kernel's `splits`), the partial products land in the caller's workspace and are
// summed in a fixed order: deterministic, and the chip is filled.
static int gemm_short_splits(int b, int M, long N, long K)
{
    const long tiles = (long)div_up(M, GM_T) * div_up(N, GM_T) * b;
    if (tiles >= 192 || K < 128) return 1;
    long s = 512 / tiles;
    if (s > 8) s = 8;
    if (s > K / 64) s = K / 64;  // at least four chunks per split
    return s < 2 ? 1 : (int)s;
}

__global__ __launch_bounds__(256) void gm_split_reduce_kernel(long total, long P, int splits, const float *__restrict__ partial,
                                                              const float *__restrict__ bias, float *__restrict__ out)
{
    // out[b][i] = sum_s partial[b * splits + s][i] (+ bias[i / P]); grid (chunks of total, b); total % 4 == 0 is not assumed
    const long i = ((long)blockIdx.x * 256 + threadIdx.x);
    if (i >= total) return;
    const float *p = partial + (size_t)blockIdx.y * splits * total + i;
    float acc = p[0];
    for (int sidx = 1; sidx < splits; ++sidx) acc += p[(size_t)sidx * total];
    out[(size_t)blockIdx.y * total + i] = bias ? acc + bias[i / P] : acc;
}

__global__ __launch_bounds__(256) void gm_bias_kernel(long total, long P, const float *__restrict__ bias, float *__restrict__ y)
{
    const long i = ((long)blockIdx.x * 256 + threadIdx.x);
    if (i < total) y[(size_t)blockIdx.y * total + i] += bias[i / P];
}

bool gemm_conv_short(int b, int rows, long P) { return (long)div_up(rows, GM_T) * div_up(P, GM_T) * b < 192; }

size_t gemm_conv_forward_workspace_bytes(int b, int cin, int cout, long P)
{
    const int sp = gemm_short_splits(b, cout, P, cin);
    return sp > 1 ? (size_t)b * sp * cout * P * sizeof(float) : 0;
}

size_t gemm_conv_backward_data_workspace_bytes(int b, int cin, int cout, long P)
{
    const int sp = gemm_short_splits(b, cin, P, cout);
    return sp > 1 ? (size_t)b * sp * cin * P * sizeof(float) : 0;
}

// y_pm: y as (b,P,cout) rows (no bias); the split-K partials then have that layout too and their sum is elementwise -- the same
// accumulators and the same order of the partial sums as the channel-major form, so the rows equal its transpose bit for bit
// tile: see gm_launch
static int gm_conv_forward(int b, int cin, int cout, long P, const float *x, const float *w, long ldw, const float *bias, float *y,
                           int y_pm, float *partial, hipStream_t stream, int tile)
{
    if (y_pm && bias) return bad_arg("gemm_conv_forward: rows take no bias");
    GemmView A{w, ldw, 1}, B{x, 1, P};  // A(m=co,k=ci) k-contiguous; B(n=p,k=ci) at x[k*P + n]: n-contiguous
    const int va = cin % 4 == 0 && ldw % 4 == 0 && aligned16(w), vb = P % 4 == 0 && aligned16(x);
    const int sp = partial ? gemm_short_splits(b, cout, P, cin) : 1;
    if (sp > 1) {
        const long kper = (((long)cin + sp - 1) / sp + GM_KC - 1) / GM_KC * GM_KC;
        gm_launch<true, false>(cout, (int)P, cin, b, sp, kper, A, 0, B, (long)cin * P, partial, (long)cout * P, P, va, vb, stream,
                               y_pm, tile);
        const long total = (long)cout * P;
        hipLaunchKernelGGL(gm_split_reduce_kernel, dim3(div_up(total, 256), b), dim3(256), 0, stream, total, P, sp,
                           (const float *)partial, bias, y);
        return launch_status("gemm_conv_forward");
    }
    gm_launch<true, false>(cout, (int)P, cin, b, 1, cin, A, 0, B, (long)cin * P, y, (long)cout * P, P, va, vb, stream, y_pm,
                           tile);
    if (bias) {
        const long total = (long)cout * P;
        hipLaunchKernelGGL(gm_bias_kernel, dim3(div_up(total, 256), b), dim3(256), 0, stream, total, P, bias, y);
    }
    return launch_status("gemm_conv_forward");
}

int gemm_conv_forward(int b, int cin, int cout, long P, const float *x, const float *w, long ldw, const float *bias, float *y,
                      int y_pm, float *partial, hipStream_t stream)
{
    return gm_conv_forward(b, cin, cout, P, x, w, ldw, bias, y, y_pm, partial, stream, -1);
}

// dx (b,cin,P) = W^T . dy (b,cout,P)
// dx_pm: dx as (b,P,cin) rows; the split-K partials then have that layout too and their sum is elementwise
static int gm_conv_backward_data(int b, int cin, int cout, long P, const float *dy, const float *w, long ldw, float *dx, int dx_pm,
                                 float *partial, hipStream_t stream, int tile)
{
    GemmView A{w, 1, ldw}, B{dy, 1, P};  // A(m=ci,k=co) = w[k*ldw + m]: m-contiguous
    const int va = cin % 4 == 0 && ldw % 4 == 0 && aligned16(w), vb = P % 4 == 0 && aligned16(dy);
    const int sp = partial ? gemm_short_splits(b, cin, P, cout) : 1;
    if (sp > 1) {
        const long kper = (((long)cout + sp - 1) / sp + GM_KC - 1) / GM_KC * GM_KC;
        gm_launch<false, false>(cin, (int)P, cout, b, sp, kper, A, 0, B, (long)cout * P, partial, (long)cin * P, P, va, vb, stream,
                                dx_pm, tile);
        const long total = (long)cin * P;
        hipLaunchKernelGGL(gm_split_reduce_kernel, dim3(div_up(total, 256), b), dim3(256), 0, stream, total, P, sp,
                           (const float *)partial, (const float *)nullptr, dx);
        return launch_status("gemm_conv_backward_data");
    }
    gm_launch<false, false>(cin, (int)P, cout, b, 1, cout, A, 0, B, (long)cout * P, dx, (long)cin * P, P, va, vb, stream, dx_pm,
                            tile);
    return launch_status("gemm_conv_backward_data");
}

int gemm_conv_backward_data(int b, int cin, int cout, long P, const float *dy, const float *w, long ldw, float *dx, int dx_pm,
                            float *partial, hipStream_t stream)
{
    return gm_conv_backward_data(b, cin, cout, P, dy, w, ldw, dx, dx_pm, partial, stream, -1);
}

static bool gw_streaming(int b, int cin, int cout, long P) { return P % 4 == 0 && P >= 4 * GW_KC; }

static int gemm_wgrad_splits(int b, int cin, int cout, long P, long *kper)
{
    if (gw_streaming(b, cin, cout, P)) {
        // ~512 workgroups (two per CU), at least `minc` chunks each; a range is a whole number of chunks
        const long minc = 4;
        const int tn = cin <= 64 ? 64 : 128;
        const long tiles = (long)div_up(cout, GW_TM) * div_up(cin, tn);
        long s = 512 / (tiles * b);
        const long cap = P / (minc * GW_KC) > 1 ? P / (minc * GW_KC) : 1;
        if (s > cap) s = cap;
        if (s < 1) s = 1;
        const long per = ((P + s - 1) / s + GW_KC - 1) / GW_KC * GW_KC;
        *kper = per;
        return (int)((P + per - 1) / per);
    }
    // enough workgroups to fill the chip, at least 256 positions each
    const long tiles = (long)div_up(cout, GM_T) * div_up(cin, GM_T);
    long s = 1024 / (tiles * b);
    const long mink = 64;  // (short layers: 375 positions)
    const long cap = P / mink > 1 ? P / mink : 1;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    long per = ((P + s - 1) / s + GM_KC - 1) / GM_KC * GM_KC;
    *kper = per;
    return (int)((P + per - 1) / per);
}

size_t gemm_conv_wgrad_workspace_bytes(int b, int cin, int cout, long P)
{
    long kper;
    const int s = gemm_wgrad_splits(b, cin, cout, P, &kper);
    return (size_t)b * s * cout * cin * sizeof(float);
}

// dw (cout,cin) = sum_b dy[b] . x[b]^T, deterministic (partials summed in a fixed order)
// tile >= 0: the generic kernel with that tile, whatever the shape (amc3d_gemm_probe)
static int gm_conv_backward_weight(int b, int cin, int cout, long P, const float *x, const float *dy, float *dw, long lddw,
                                   float *partial, hipStream_t stream, int tile)
{
    long kper;
    const int s = gemm_wgrad_splits(b, cin, cout, P, &kper);
    if (tile < 0 && gw_streaming(b, cin, cout, P) && aligned16(dy) && aligned16(x)) {
        if (cin <= 64) {
            const size_t lds = 2 * (GW_TM + 64) * GW_S * sizeof(float);
            hipLaunchKernelGGL(gw_wgrad_kernel<64>, dim3(div_up(cin, 64), div_up(cout, GW_TM), b * s), dim3(256), lds, stream, cout,
                               cin, P, s, kper, dy, x, partial);
        } else {
            const size_t lds = 2 * (GW_TM + 128) * GW_S * sizeof(float);
            (void)hipFuncSetAttribute((const void *)gw_wgrad_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(gw_wgrad_kernel<128>, dim3(div_up(cin, 128), div_up(cout, GW_TM), b * s), dim3(256), lds, stream,
                               cout, cin, P, s, kper, dy, x, partial);
        }
        if (int st = launch_status("gemm_conv_backward_weight")) return st;
        return reduce_partials_rows(cout, cin, lddw, b * s, partial, dw, stream);
    }
    GemmView A{dy, P, 1}, B{x, P, 1};  // A(m=co,k=p), B(n=ci,k=p): both k-contiguous
    const int va = P % 4 == 0 && aligned16(dy), vb = P % 4 == 0 && aligned16(x);
    gm_launch<true, true>(cout, cin, P, b, s, kper, A, (long)cout * P, B, (long)cin * P, partial, (long)cout * cin, cin, va, vb,
                          stream, 0, tile);
    if (int st = launch_status("gemm_conv_backward_weight")) return st;
    return reduce_partials_rows(cout, cin, lddw, b * s, partial, dw, stream);
}

int gemm_conv_backward_weight(int b, int cin, int cout, long P, const float *x, const float *dy, float *dw, long lddw,
                              float *partial, hipStream_t stream)
{
    return gm_conv_backward_weight(b, cin, cout, P, x, dy, dw, lddw, partial, stream, -1);
}

}  // namespace amc

using namespace amc;

// ---- test and measurement entries: neither is called by the product path ----------------------------------------------------
AMC_API int amc3d_gemm_tile_for(int M, int N, int batch, int splits)
{
    if (M <= 0 || N <= 0 || batch <= 0 || splits <= 0) return -1;
    return gm_tile_for(M, N, batch, splits);
}

AMC_API int amc3d_gemm_probe(int tile_id, int product, int b, int cin, int cout, long P, long ldw, int pm, const float *x_or_dy,
                             const float *w, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (b <= 0 || P <= 0) return 0;
    if (tile_id < 0 || tile_id >= GM_NTILES || product < 0 || product > 2 || cin <= 0 || cout <= 0 || P >= (1L << 31) || ldw < cin ||
        !x_or_dy || !w || !out || (product == 2 && pm))
        return bad_arg("amc3d_gemm_probe: bad argument");
    if (product == 2) {
        if (!workspace || workspace_bytes < gemm_conv_wgrad_workspace_bytes(b, cin, cout, P))
            return bad_arg("amc3d_gemm_probe: workspace too small");
        return gm_conv_backward_weight(b, cin, cout, P, w, x_or_dy, out, ldw, (float *)workspace, (hipStream_t)stream, tile_id);
    }
    const size_t need = product == 0 ? gemm_conv_forward_workspace_bytes(b, cin, cout, P)
                                     : gemm_conv_backward_data_workspace_bytes(b, cin, cout, P);
    float *partial = (need && workspace && workspace_bytes >= need) ? (float *)workspace : nullptr;
    if (product == 0)
        return gm_conv_forward(b, cin, cout, P, x_or_dy, w, ldw, nullptr, out, pm, partial, (hipStream_t)stream, tile_id);
    return gm_conv_backward_data(b, cin, cout, P, x_or_dy, w, ldw, out, pm, partial, (hipStream_t)stream, tile_id);
}
