"""NumPy restatement of the separable aggregation of ASSA (include/amc3d.h, amc3d_assa_aggregate_*), in the arithmetic and
the ORDER the kernels promise, so that the fp32 results can be compared bit for bit:

    out[b, d*C + c, m] = red_k ( dp[b,d,m,k] * f[b,c,idx[b,m,k]] )        d in 0..2, red in {mean, sum, max}

  * every product is rounded once; `sum` adds in ascending k from +0; `mean` divides that sum by K once; `max` keeps the
    first maximum in k (the first NaN, once there is one: torch.max's rule) and reports its k;
  * the backward reaches f only: df[b,c,n] is the sequential sum, in ascending (m, k), of the terms of the edges with
    idx[b,m,k] == n; a term is s * ((dp0*g0 + dp1*g1) + dp2*g2) with s = 1/K for mean and 1 for sum, and for max the same
    sum with the product of d replaced by +0 unless that (d, c, m)'s stored k is this edge's.

`dtype=np.float32` is the statement of the kernels, `dtype=np.float64` the twin the default (atomic) backward is judged by.
NumPy's elementwise float32 multiply, add and divide are single IEEE operations: nothing here is fused or reassociated.
"""
import numpy as np


def forward(f, idx, dp, reduction, dtype=np.float32):
    """f (B,C,N), idx (B,M,K) int, dp (B,3,M,K) -> out (B,3C,M), arg (B,3C,M) int64 (max) or None"""
    f, dp = np.asarray(f, dtype), np.asarray(dp, dtype)
    B, C, N = f.shape
    _, M, K = idx.shape
    acc = np.zeros((B, 3, C, M), dtype)
    arg = np.zeros((B, 3, C, M), np.int64) if reduction == "max" else None
    for k in range(K):
        j = np.broadcast_to(idx[:, None, :, k].astype(np.int64), (B, C, M))
        fj = np.take_along_axis(f, j, axis=2)                       # (B,C,M)
        prod = dp[:, :, None, :, k] * fj[:, None, :, :]             # (B,3,C,M), one rounding each
        if reduction == "max":
            if k == 0:
                acc = prod.copy()
            else:
                later = (prod > acc) | (np.isnan(prod) & ~np.isnan(acc))  # strictly greater, or the first NaN: it stays
                acc = np.where(later, prod, acc)
                arg = np.where(later, k, arg)
        else:
            acc = acc + prod
    if reduction == "mean":
        acc = acc / dtype(K)
    return acc.reshape(B, 3 * C, M), (arg.reshape(B, 3 * C, M) if arg is not None else None)


def magnitude(f, idx, dp):
    """sum over k of |dp * f| per output element, in fp64: the scale of the forward's rounding bound"""
    f, dp = np.asarray(f, np.float64), np.asarray(dp, np.float64)
    B, C, N = f.shape
    _, M, K = idx.shape
    tot = np.zeros((B, 3, C, M))
    for k in range(K):
        j = np.broadcast_to(idx[:, None, :, k].astype(np.int64), (B, C, M))
        tot += np.abs(dp[:, :, None, :, k] * np.take_along_axis(f, j, axis=2)[:, None])
    return tot.reshape(B, 3 * C, M)


def backward(g, idx, dp, arg, reduction, n_support, dtype=np.float32, magnitudes=False):
    """g (B,3C,M), arg from forward (max) -> df (B,C,N): sequential sums in ascending (m, k) from +0.
    magnitudes=True: also (sum of |products| of the incoming terms in fp64, in-degree) per element / per support point."""
    g, dp = np.asarray(g, dtype), np.asarray(dp, dtype)
    B, C3, M = g.shape
    C, K = C3 // 3, idx.shape[-1]
    g = g.reshape(B, 3, C, M)
    s = dtype(1) / dtype(K) if reduction == "mean" else dtype(1)
    df = np.zeros((B, n_support, C), dtype)
    mag = np.zeros((B, n_support, C), np.float64)
    cnt = np.zeros((B, n_support), np.int64)
    rows = np.arange(B)
    if arg is not None:
        arg = arg.reshape(B, 3, C, M)
    for m in range(M):
        gm = g[:, :, :, m]                                           # (B,3,C)
        for k in range(K):
            j = idx[:, m, k].astype(np.int64)
            p = dp[:, :, m, k][:, :, None] * gm                      # (B,3,C), one rounding each
            if reduction == "max":
                p = np.where(arg[:, :, :, m] == k, p, dtype(0))
                t = (p[:, 0] + p[:, 1]) + p[:, 2]
            else:
                t = s * ((p[:, 0] + p[:, 1]) + p[:, 2])
            df[rows, j] = df[rows, j] + t
            if magnitudes:
                mag[rows, j] += float(s) * np.abs(p.astype(np.float64)).sum(axis=1)
                cnt[rows, j] += 1
    df = np.ascontiguousarray(df.transpose(0, 2, 1))
    if magnitudes:
        return df, np.ascontiguousarray(mag.transpose(0, 2, 1)), cnt
    return df


def ball_like_idx(rng, B, M, K, N, zero_rows=3):
    """ball-query-like rows: a prefix of distinct hits padded with the first hit, and a few rows of all zeros (what an
    empty ball gives)"""
    idx = np.zeros((B, M, K), np.int32)
    for b in range(B):
        for m in range(M):
            hits = rng.permutation(N)[:min(int(rng.integers(1, K + 1)), N)]
            idx[b, m, :len(hits)] = hits
            idx[b, m, len(hits):] = hits[0]
    idx[:, :min(zero_rows, M)] = 0
    return idx
