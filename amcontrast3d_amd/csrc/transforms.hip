// The training transforms of a config's `datatransforms.train` list as one compiled program (gfx950).
//
// amcontrast3d_amd/transforms.py turns any chain of the reference's transform classes (transforms/point_transform_cpu.py,
// point_transformer_gpu.py) into a table of micro-ops; one kernel interprets it for every point of a ragged batch, the ops
// of one point in registers and in chain order.  An op that needs a per-cloud reduction of the CURRENT state (the colour
// min / max of ChromaticAutoContrast, the colour maximum of the `> 1` test, the mean / gravity minimum of PointCloudXYZAlign,
// the mean and largest norm of PointCloudCenterAndNormalize, the coordinate extrema of RandomHorizontalFlip) names a
// reduction phase.  Launch k < n_phases replays, from the input, every op that needs only phases < k, stops each stream
// (positions, colours) at its first op of phase k and reduces the state there; launch n_phases runs the whole program and
// writes the outputs.  So 1 + n_phases launches, and no (total, .) intermediate in memory.
//
// Reductions: one partial record per workgroup (a tile of kTfTile points of one cloud), folded by every workgroup of the
// next launch in a fixed order (thread-strided, a fixed shuffle tree, then the waves in order).  No atomics: the same input
// gives the same bits.  Sums are double, rounded once where a mean is formed.
//
// Precision follows the reference per op: the numpy classes compute float32 (op) float64 in double and round when they
// assign into a float32 array, np.dot leaves the positions float64, the torch classes work in float32.  The positions are
// carried as double (a float32 value is exact in it); each op's record says whether its result is rounded to float32.
#include "room_common.h"

namespace amc {

constexpr int kTfMaxOps = 32;     // micro-ops a program holds
constexpr int kTfMaxPhases = 4;   // reduction phases
constexpr int kTfMaxNoise = 4;    // per-point draw tensors
constexpr int kTfThreads = 256;
constexpr int kTfPerThread = 4;
constexpr int kTfTile = kTfThreads * kTfPerThread;

enum TfCode {
    // positions
    TF_ROT_DOT = 0,        // np.dot(pos, M): c[9] row-major M, dgemm's order, result double; iarg bit 1: M is a transposed view
    TF_SCALE_NP,           // pos *= c[3] in double; iarg bit 0: the array is float64 (else rounded to float32)
    TF_SCALE_JITTER_NP,    // pos * c[3] + clip(d[0] * noise, -d[1], d[1]) -> double
    TF_FLIP_NP,            // c[0] / c[1]: negate x / y
    TF_JITTER_NP,          // pos += clip(d[0] * noise, ..) in double; iarg bit 0 as above
    TF_TO_F32,             // PointsToTensor
    TF_SCALE_T,            // float32: pos * c[3]
    TF_TRANSLATE_T,        // pos + c[3]
    TF_SCALE_TRANSLATE_T,  // pos * c[0..2] + c[3..5]
    TF_JITTER_T,           // pos + clamp(noise * f[0], -f[1], f[1])
    TF_SCALE_JITTER_T,     // pos * c[3] + clamp(..)
    TF_ROT_T,              // pos @ R^T, c[9] row-major R, float32
    TF_HEIGHTS_MIN,        // heights = pos[g] - min(pos[g])            (phase: plo)
    TF_CENTER,             // pos -= mean                               (phase: sum)
    TF_SUB_MIN_G,          // pos[g] -= min(pos[g]) of the centred cloud (phase: plo, sum; same phase as its TF_CENTER)
    TF_NORM_DIV,           // pos /= max norm                           (phase: nrm)
    TF_HFLIP,              // RandomHorizontalFlip, iarg = upright axis, c[2] flags (phase: plo, phi)
    // colours
    TF_FIRST_COLOUR,
    TF_AUTOCONTRAST = TF_FIRST_COLOUR,  // c = {taken, w_keep, w_contrast}    (phase: clo, chi)
    TF_TRANSLATE_C,        // c = {taken, tr[3]}: clip(tr + x, 0, 255) in double
    TF_JITTER_C,           // c = {taken}: clip(noise * d[0] + x, 0, 255) in double
    TF_HUESAT,             // c = {hue_val, sat_ratio}
    TF_DROP,               // c = {taken}; iarg: channel mask
    TF_PERDROP,            // x *= (u > f[0])
    TF_NORMALIZE,          // [/ 255 when the colour maximum > 1], iarg bit 0: (x - f[0..2]) / f[3..5]  (phase: cmax)
};

struct TfOp { int code, phase, slot, iarg; float f[8]; double d[2]; };                                 // 64 bytes
struct TfProgram { int n_ops, n_phases, stride, gravity; int phase_mask[kTfMaxPhases]; TfOp op[kTfMaxOps]; };
struct TfNoise { const void *ptr[kTfMaxNoise]; };
struct TfAcc { double sum[3]; float plo[3], phi[3], nrm, clo[3], chi[3], cmax, pad; };                 // 88 bytes

__device__ __forceinline__ float tf_nan() { return __int_as_float(0x7fc00000); }
// numpy's / torch's min and max: NaN as soon as one operand is NaN
__device__ __forceinline__ float tf_nanmax(float a, float b) { return (a != a || b != b) ? tf_nan() : fmaxf(a, b); }
__device__ __forceinline__ float tf_nanmin(float a, float b) { return (a != a || b != b) ? tf_nan() : fminf(a, b); }
// np.clip / clamp_: a NaN stays a NaN
__device__ __forceinline__ double tf_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float tf_clip(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ double tf_sel(const double p[3], int g) { return g == 0 ? p[0] : (g == 1 ? p[1] : p[2]); }
__device__ __forceinline__ float tf_sel(const float p[3], int g) { return g == 0 ? p[0] : (g == 1 ? p[1] : p[2]); }
// numpy's float `%` for a divisor of 1 (npy_divmod): fmod, moved into [0, 1]
__device__ __forceinline__ double tf_mod1(double a)
{
    double m = fmod(a, 1.0);
    if (m != 0.0) { if (m < 0.0) m = __dadd_rn(m, 1.0); } else m = 0.0;
    return m;
}
// ndarray.astype('uint8') of a double in 0..255 (truncation); out of range and NaN as x86's conversion leaves the low byte
__device__ __forceinline__ int tf_u8(double v) { return (v != v || v >= 2147483648.0 || v <= -2147483649.0) ? 0 : ((int)v & 255); }

__device__ __forceinline__ void tf_acc_init(TfAcc &a)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.sum[c] = 0.0; a.plo[c] = 3.4e38f; a.phi[c] = -3.4e38f; a.clo[c] = 3.4e38f; a.chi[c] = -3.4e38f; }
    a.nrm = -3.4e38f; a.cmax = -3.4e38f; a.pad = 0.f;
}

__device__ __forceinline__ void tf_acc_merge(TfAcc &a, const TfAcc &b)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.sum[c] += b.sum[c];
        a.plo[c] = fminf(a.plo[c], b.plo[c]);
        a.phi[c] = fmaxf(a.phi[c], b.phi[c]);
        a.clo[c] = tf_nanmin(a.clo[c], b.clo[c]);
        a.chi[c] = tf_nanmax(a.chi[c], b.chi[c]);
    }
    a.nrm = fmaxf(a.nrm, b.nrm);
    a.cmax = tf_nanmax(a.cmax, b.cmax);
}

__device__ __forceinline__ TfAcc tf_acc_shfl(const TfAcc &a, int d)
{
    TfAcc o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.sum[c] = __shfl_xor(a.sum[c], d, 64);
        o.plo[c] = __shfl_xor(a.plo[c], d, 64);
        o.phi[c] = __shfl_xor(a.phi[c], d, 64);
        o.clo[c] = __shfl_xor(a.clo[c], d, 64);
        o.chi[c] = __shfl_xor(a.chi[c], d, 64);
    }
    o.nrm = __shfl_xor(a.nrm, d, 64);
    o.cmax = __shfl_xor(a.cmax, d, 64);
    o.pad = 0.f;
    return o;
}

// the workgroup's records folded in a fixed order; the result is in s[0] after the call's last barrier
__device__ __forceinline__ void tf_block_fold(TfAcc &a, TfAcc *s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) {
        const TfAcc o = tf_acc_shfl(a, d);  // a + b == b + a: both partners hold the same sum afterwards
        tf_acc_merge(a, o);
    }
    __syncthreads();  // s may still be read from an earlier fold
    if (lane == 0 && wave > 0) s[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kTfThreads / 64; ++w) tf_acc_merge(a, s[w]);
        s[0] = a;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kTfThreads) void transform_chain_kernel(int launch, int nb, int groups, const long long *__restrict__ off,
                                                                    const TfProgram *__restrict__ prog,
                                                                    const double *__restrict__ table, TfNoise nz, int flags,
                                                                    const void *__restrict__ pos_in, const float *__restrict__ x_in,
                                                                    TfAcc *__restrict__ partials, TfAcc *__restrict__ stats,
                                                                    void *__restrict__ pos_out, float *__restrict__ x_out,
                                                                    float *__restrict__ heights)
{
    __shared__ TfAcc s_st[kTfMaxPhases];
    __shared__ TfAcc s_red[kTfThreads / 64];
    // (cloud, tile) of this workgroup: clouds in order, ceil(n / kTfTile) tiles each
    int b = 0;
    long long tbase = 0, start = 0, n = 0, nt = 0;
    for (; b < nb; ++b) {
        start = off[b];
        n = off[b + 1] - start;
        nt = (n + kTfTile - 1) / kTfTile;
        if ((long long)blockIdx.x < tbase + nt) break;
        tbase += nt;
    }
    if (b == nb) return;  // the grid is an upper bound (total / kTfTile + clouds)
    const long long tile = (long long)blockIdx.x - tbase;
    const int n_ops = prog->n_ops, n_phases = prog->n_phases, stride = prog->stride, g = prog->gravity;
    const bool final = launch >= n_phases;

    if (launch > 0) {
        // phases < launch - 1 were folded by an earlier launch; phase launch - 1 is folded here, by every workgroup alike
        if (threadIdx.x < launch - 1) s_st[threadIdx.x] = stats[(size_t)threadIdx.x * nb + b];
        TfAcc a;
        tf_acc_init(a);
        const TfAcc *P = partials + (size_t)(launch - 1) * groups + tbase;
        for (long long j = threadIdx.x; j < nt; j += kTfThreads) tf_acc_merge(a, P[j]);
        tf_block_fold(a, s_red);
        if (threadIdx.x == 0) {
            s_st[launch - 1] = s_red[0];
            if (tile == 0) stats[(size_t)(launch - 1) * nb + b] = s_red[0];
        }
        __syncthreads();
    }

    const double *crec = table + (size_t)b * stride;
    const double dn = (double)n;
    TfAcc acc;
    tf_acc_init(acc);
    const int mask = final ? 0 : prog->phase_mask[launch];

    for (int j = 0; j < kTfPerThread; ++j) {
        const long long li = tile * kTfTile + (long long)j * kTfThreads + threadIdx.x;
        if (li >= n) break;
        const long long i = start + li;
        double p[3];
        float x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[c] = (flags & 1) ? ((const double *)pos_in)[i * 3 + c] : (double)((const float *)pos_in)[i * 3 + c];
            x[c] = x_in[i * 3 + c];
            if (flags & 2) x[c] = __fmul_rn(__fadd_rn(x[c], 1.f), 127.5f);  // scannet.py:140: [-1, 1] -> 0..255 in float32
        }
        float h = (float)tf_sel(p, g);  // the gravity coordinate before the chain (s3dis.py:142-143)
        bool stop_p = false, stop_x = false;
        for (int k = 0; k < n_ops; ++k) {
            const TfOp &o = prog->op[k];
            const bool is_x = o.code >= TF_FIRST_COLOUR;
            if (is_x ? stop_x : stop_p) continue;
            if (o.phase == launch) { if (is_x) stop_x = true; else stop_p = true; continue; }
            const double *c = crec + o.slot;
            const TfAcc &s = s_st[o.phase > 0 ? o.phase : 0];
            const bool keep64 = (o.iarg & 1) != 0;
            switch (o.code) {
            case TF_ROT_DOT: {
                double q[3];
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    q[r] = ((o.iarg & 2) && n == 1)  // one row times a transposed view: numpy calls dgemv, which starts at column 1
                               ? __fma_rn(p[2], c[6 + r], __fma_rn(p[0], c[r], __dmul_rn(p[1], c[3 + r])))
                               : __fma_rn(p[2], c[6 + r], __fma_rn(p[1], c[3 + r], __dmul_rn(p[0], c[r])));
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            } break;
            case TF_SCALE_NP:
#pragma unroll
                for (int r = 0; r < 3; ++r) { const double v = __dmul_rn(p[r], c[r]); p[r] = keep64 ? v : (double)(float)v; }
                break;
            case TF_SCALE_JITTER_NP: {
                const double *N = (const double *)nz.ptr[o.iarg >> 8];
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    p[r] = __dadd_rn(__dmul_rn(p[r], c[r]), tf_clip(__dmul_rn(o.d[0], N[i * 3 + r]), -o.d[1], o.d[1]));
            } break;
            case TF_FLIP_NP:
                if (c[0] != 0.0) p[0] = -p[0];
                if (c[1] != 0.0) p[1] = -p[1];
                break;
            case TF_JITTER_NP: {
                const double *N = (const double *)nz.ptr[o.iarg >> 8];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double v = __dadd_rn(p[r], tf_clip(__dmul_rn(o.d[0], N[i * 3 + r]), -o.d[1], o.d[1]));
                    p[r] = keep64 ? v : (double)(float)v;
                }
            } break;
            case TF_TO_F32:
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = (double)(float)p[r];
                break;
            case TF_SCALE_T:
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = (double)__fmul_rn((float)p[r], (float)c[r]);
                break;
            case TF_TRANSLATE_T:
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = (double)__fadd_rn((float)p[r], (float)c[r]);
                break;
            case TF_SCALE_TRANSLATE_T:
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = (double)__fadd_rn(__fmul_rn((float)p[r], (float)c[r]), (float)c[3 + r]);
                break;
            case TF_JITTER_T: {
                const float *N = (const float *)nz.ptr[o.iarg >> 8];
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    p[r] = (double)__fadd_rn((float)p[r], tf_clip(__fmul_rn(N[i * 3 + r], o.f[0]), -o.f[1], o.f[1]));
            } break;
            case TF_SCALE_JITTER_T: {
                const float *N = (const float *)nz.ptr[o.iarg >> 8];
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    p[r] = (double)__fadd_rn(__fmul_rn((float)p[r], (float)c[r]), tf_clip(__fmul_rn(N[i * 3 + r], o.f[0]), -o.f[1], o.f[1]));
            } break;
            case TF_ROT_T: {  // pos @ R^T, accumulated in the order of a length-3 dot product
                const float q0 = (float)p[0], q1 = (float)p[1], q2 = (float)p[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    float v = __fmul_rn(q0, (float)c[r * 3]);
                    v = fmaf(q1, (float)c[r * 3 + 1], v);
                    v = fmaf(q2, (float)c[r * 3 + 2], v);
                    p[r] = (double)v;
                }
            } break;
            case TF_HEIGHTS_MIN:
                h = __fsub_rn((float)tf_sel(p, o.iarg >> 8), tf_sel(s.plo, o.iarg >> 8));
                break;
            case TF_CENTER:
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = (double)__fsub_rn((float)p[r], (float)(s.sum[r] / dn));
                break;
            case TF_SUB_MIN_G: {
                // min over the points of fl(z - mean): monotone in z, so it sits at the minimum of z
                const int gg = o.iarg >> 8;
                const float zmin = __fsub_rn(tf_sel(s.plo, gg), (float)(tf_sel(s.sum, gg) / dn));
#pragma unroll
                for (int r = 0; r < 3; ++r) if (r == gg) p[r] = (double)__fsub_rn((float)p[r], zmin);
            } break;
            case TF_NORM_DIV:
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = (double)__fdiv_rn((float)p[r], s.nrm);
                break;
            case TF_HFLIP: {
                // coord_max = torch.max(pos) of the state at each flip: after a flip of axis a by m the axis spans
                // [fl(m - hi), fl(m - lo)] (monotone), so the later maximum follows from the per-axis extrema
                float lo[3] = {s.plo[0], s.plo[1], s.plo[2]}, hi[3] = {s.phi[0], s.phi[1], s.phi[2]};
                const int up = o.iarg >> 8;
                int slot = 0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    if (r == up) continue;
                    if (c[slot] != 0.0) {
                        const float m = fmaxf(fmaxf(hi[0], hi[1]), hi[2]);
                        const float nl = __fsub_rn(m, hi[r]), nh = __fsub_rn(m, lo[r]);
                        lo[r] = nl; hi[r] = nh;
                        p[r] = (double)__fsub_rn(m, (float)p[r]);
                    }
                    ++slot;
                }
            } break;
            case TF_AUTOCONTRAST:
                if (c[0] != 0.0) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const float sc = __fdiv_rn(255.f, __fsub_rn(s.chi[r], s.clo[r]));  // inf when hi == lo
                        x[r] = __fadd_rn(__fmul_rn((float)c[1], x[r]), __fmul_rn((float)c[2], __fmul_rn(__fsub_rn(x[r], s.clo[r]), sc)));
                    }
                }
                break;
            case TF_TRANSLATE_C:
                if (c[0] != 0.0) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) x[r] = (float)tf_clip(__dadd_rn(c[1 + r], (double)x[r]), 0.0, 255.0);
                }
                break;
            case TF_JITTER_C:
                if (c[0] != 0.0) {
                    const double *N = (const double *)nz.ptr[o.iarg >> 8];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        x[r] = (float)tf_clip(__dadd_rn(__dmul_rn(N[i * 3 + r], o.d[0]), (double)x[r]), 0.0, 255.0);
                }
                break;
            case TF_HUESAT: {  // HueSaturationTranslation: rgb_to_hsv, the two shifts, hsv_to_rgb, all in double
                const double r = (double)x[0], gch = (double)x[1], bch = (double)x[2];
                const double maxc = fmax(fmax(r, gch), bch), minc = fmin(fmin(r, gch), bch);
                const bool m = maxc != minc;
                const double span = __dsub_rn(maxc, minc);
                double sat = m ? __ddiv_rn(span, maxc) : 0.0;
                const double rc = m ? __ddiv_rn(__dsub_rn(maxc, r), span) : 0.0;
                const double gc = m ? __ddiv_rn(__dsub_rn(maxc, gch), span) : 0.0;
                const double bc = m ? __ddiv_rn(__dsub_rn(maxc, bch), span) : 0.0;
                double hue = r == maxc ? __dsub_rn(bc, gc)
                                       : (gch == maxc ? __dsub_rn(__dadd_rn(2.0, rc), bc) : __dsub_rn(__dadd_rn(4.0, gc), rc));
                hue = tf_mod1(__ddiv_rn(hue, 6.0));
                hue = tf_mod1(__dadd_rn(__dadd_rn(c[0], hue), 1.0));
                sat = tf_clip(__dmul_rn(c[1], sat), 0.0, 1.0);
                const double h6 = __dmul_rn(hue, 6.0);
                const int iu = tf_u8(h6);
                const double f = __dsub_rn(h6, (double)iu);
                const double pp = __dmul_rn(maxc, __dsub_rn(1.0, sat));
                const double qq = __dmul_rn(maxc, __dsub_rn(1.0, __dmul_rn(sat, f)));
                const double tt = __dmul_rn(maxc, __dsub_rn(1.0, __dmul_rn(sat, __dsub_rn(1.0, f))));
                const int i6 = iu % 6;
                double o0, o1, o2;
                if (sat == 0.0) { o0 = maxc; o1 = maxc; o2 = maxc; }
                else if (i6 == 1) { o0 = qq; o1 = maxc; o2 = pp; }
                else if (i6 == 2) { o0 = pp; o1 = maxc; o2 = tt; }
                else if (i6 == 3) { o0 = pp; o1 = qq; o2 = maxc; }
                else if (i6 == 4) { o0 = tt; o1 = pp; o2 = maxc; }
                else if (i6 == 5) { o0 = maxc; o1 = pp; o2 = qq; }
                else { o0 = maxc; o1 = tt; o2 = pp; }
                x[0] = (float)tf_u8(o0); x[1] = (float)tf_u8(o1); x[2] = (float)tf_u8(o2);
            } break;
            case TF_DROP:
                if (c[0] != 0.0) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) if ((o.iarg >> (8 + r)) & 1) x[r] = 0.f;
                }
                break;
            case TF_PERDROP: {
                const float keep = ((const float *)nz.ptr[o.iarg >> 8])[i] > o.f[0] ? 1.f : 0.f;
#pragma unroll
                for (int r = 0; r < 3; ++r) x[r] = __fmul_rn(x[r], keep);
            } break;
            case TF_NORMALIZE:
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    if (s.cmax > 1.f) x[r] = __fdiv_rn(x[r], 255.f);  // false for a NaN maximum
                    if (keep64) x[r] = __fdiv_rn(__fsub_rn(x[r], o.f[r]), o.f[3 + r]);
                }
                break;
            default: break;
            }
        }
        if (final) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (flags & 4) ((double *)pos_out)[i * 3 + c] = p[c]; else ((float *)pos_out)[i * 3 + c] = (float)p[c];
                x_out[i * 3 + c] = x[c];
            }
            if (heights) heights[i] = h;
        } else {
            if (mask & 1) {
                const float q[3] = {(float)p[0], (float)p[1], (float)p[2]};
#pragma unroll
                for (int c = 0; c < 3; ++c) { acc.sum[c] += p[c]; acc.plo[c] = fminf(acc.plo[c], q[c]); acc.phi[c] = fmaxf(acc.phi[c], q[c]); }
                const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[1], q[1])), __fmul_rn(q[2], q[2]));
                acc.nrm = fmaxf(acc.nrm, __fsqrt_rn(n2));
            }
            if (mask & 2) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    acc.clo[c] = tf_nanmin(acc.clo[c], x[c]);
                    acc.chi[c] = tf_nanmax(acc.chi[c], x[c]);
                    acc.cmax = tf_nanmax(acc.cmax, x[c]);
                }
            }
        }
    }
    if (!final) {
        tf_block_fold(acc, s_red);
        if (threadIdx.x == 0) partials[(size_t)launch * groups + blockIdx.x] = s_red[0];
    }
}

static inline long long tf_groups(int b, long long total) { return (total + kTfTile - 1) / kTfTile + b; }

}  // namespace amc

using namespace amc;

AMC_API int amc3d_transform_max_ops(void) { return kTfMaxOps; }
AMC_API int amc3d_transform_max_phases(void) { return kTfMaxPhases; }
AMC_API int amc3d_transform_program_bytes(void) { return (int)sizeof(TfProgram); }

AMC_API size_t amc3d_transform_workspace_bytes(int b, long long total, int n_phases)
{
    if (b <= 0 || total <= 0 || n_phases <= 0) return 256;
    return align256((size_t)n_phases * (size_t)tf_groups(b, total) * sizeof(TfAcc)) + align256((size_t)n_phases * b * sizeof(TfAcc));
}

AMC_API int amc3d_transform_chain(int b, long long total, int n_phases, const long long *offsets, const void *program,
                                  const double *table, const void *const *noise, int flags, const void *pos, const float *x,
                                  void *pos_out, float *x_out, float *heights, void *workspace, size_t workspace_bytes,
                                  void *stream_)
{
    if (b <= 0 || total <= 0) return 0;
    if (n_phases < 0 || n_phases > kTfMaxPhases || !offsets || !program || !table || !noise || !pos || !x || !pos_out || !x_out ||
        !workspace || workspace_bytes < amc3d_transform_workspace_bytes(b, total, n_phases))
        return bad_arg("amc3d_transform_chain: bad argument");
    const long long groups = tf_groups(b, total);
    if (groups > 0x7fffffffLL) return bad_arg("amc3d_transform_chain: too many points");
    hipStream_t stream = (hipStream_t)stream_;
    TfNoise nz;
    for (int k = 0; k < kTfMaxNoise; ++k) nz.ptr[k] = noise[k];
    TfAcc *partials = (TfAcc *)workspace;
    TfAcc *stats = (TfAcc *)((char *)workspace + align256((size_t)n_phases * (size_t)groups * sizeof(TfAcc)));
    for (int launch = 0; launch <= n_phases; ++launch)
        hipLaunchKernelGGL(transform_chain_kernel, dim3((unsigned)groups), dim3(kTfThreads), 0, stream, launch, b, (int)groups, offsets,
                           (const TfProgram *)program, table, nz, flags, pos, x, partials, stats, pos_out, x_out, heights);
    return launch_status("amc3d_transform_chain");
}
