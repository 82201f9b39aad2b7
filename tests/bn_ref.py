"""Host-side reference for the BatchNorm kernels of csrc/bn.hip (numpy and torch on the CPU only; no fixtures).

The kernels are judged in three separate steps, so that each has the tightest honest bound:

1.  Statistics.  The kernel adds the n = B*L float32 values of a channel, and their squares, in fp64.  A float32
    value and the square of one are exact in fp64, so the only errors are those of the additions.  Summing n terms in
    any order has forward error at most (n-1) u |terms| summed, u = 2^-53 (Higham, Accuracy and Stability, 4.2).  With
    S1 = sum|x| and S2 = sum x^2:
        mean = s1/n            |error| <= u S1 (the sum: n u S1 / n) + u |mean| (the division), then one rounding to float32
        tol_mean  = 2^-24 |mean| + 2 * 2^-53 * S1
        var  = s2/n - mean^2   |error| <= u S2 (first term) + 2 |mean| u S1 (second) + three roundings of values <= S2/n;
                               |mean| S1 <= S1^2 / n <= S2 (Cauchy-Schwarz), so the total is below 4 u S2; the factor
                               n/(n-1) <= 2 of the unbiased form doubles it, and the result is rounded to float32
        tol_var_u = 2^-23 var_u + 8 * 2^-53 * S2          (tol_var_b, for the biased value kept in fp64: 8 * 2^-53 * S2)
        invstd = 1/sqrt(var + eps), d invstd / d var = -invstd / (2 (var + eps)), two fp64 roundings and one to float32
        tol_invstd = 2^-23 invstd + 0.5 invstd tol_var_b / (var + eps)
    The bounds scale with S2, so a channel with a large mean and a small spread (the E[x^2] - mean^2 cancellation) gets
    the allowance its arithmetic really needs and no more.

2.  Normalisation.  With the library built without floating-point contraction, bn_val is four float32 operations rounded to
    nearest: ((x - mean) * invstd) * gamma + beta, then + res, then max(., 0).  `normalise` repeats them in numpy float32 from
    the mean and invstd THE KERNEL published, and the output must be equal bit for bit (np.array_equal; it treats -0 and +0
    alike, as the comparisons in the kernels do).  Not for the sigmoid, whose expf is not predictable to the bit.

3.  Backward.  `backward64` takes the published float32 mean and invstd and the gradient dq that reaches the BatchNorm output
    (already masked by y > 0, routed through the recorded arg-max, or multiplied by y (1 - y): all float32 operations the
    caller repeats exactly from the kernel's own forward output), so only the element arithmetic remains:
        xh = fl(fl(x - mean) * invstd)                       2 roundings
        Sa = sum dq, Sb = sum dq * xh                        fp64; the products of two float32 are exact in fp64
        ma = (float)(Sa/n), mb = (float)(Sb/n)               1 rounding each (+ the fp64 sums: u sum|terms| each)
        dx = gi * (dq - ma - xh * mb), gi = fl(gamma*invstd) 1 + 1 + 1 + 1 + 1 roundings
    seven rounded operations in the expression, one more in each of ma and mb: nine relative errors of 2^-24, each on a
    partial result no larger than |gi| (|dq| + |ma| + |xh mb|) to first order.  16 covers the nine with a factor below two
    to spare for the second-order terms:
        tol_dx = 16 * 2^-24 * |gi| (|dq| + |ma| + |xh mb|)  +  2^-53 |gi| (sum|dq| + |xh| sum|dq xh|)
    (the second term is the fp64 summation error that ma and mb inherit: n u sum|terms| / n; it is 2^-29 of the first at most
    for the sizes tested and is there because the derivation has it, not to make room).
        dbeta = (float)Sa, dgamma = (float)Sb:   tol = 2^-24 |sum| + n * 2^-53 * sum|terms|, terms with the float32 xh.

The ReLU mask is never taken from a reference forward: an element within rounding of zero would flip it.  It is the kernel's
own y > 0, and y itself is pinned by step 2.
"""
import collections

import numpy as np
import torch

U24 = 2.0 ** -24
U53 = 2.0 ** -53
F32 = np.float32


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def per_channel(a):
    """(B, C, *) -> (C, n): the n = B*L values of each channel"""
    a = _np(a)
    B, C = a.shape[:2]
    return np.moveaxis(a.reshape(B, C, -1), 1, 0).reshape(C, -1)


def _bc(v, ndim):
    """(C,) -> (1, C, 1, ...) against a (B, C, *) array"""
    return np.asarray(v).reshape((1, -1) + (1,) * (ndim - 2))


Stats = collections.namedtuple("Stats", "n mean var_b var_u S1 S2")


def stats64(x):
    """per channel in float64: mean, biased variance (two-pass), unbiased variance (the biased one where n == 1, as the
    kernel publishes it), S1 = sum|x|, S2 = sum x^2"""
    v = per_channel(x).astype(np.float64)
    n = v.shape[1]
    mean = v.sum(1) / n
    var_b = ((v - mean[:, None]) ** 2).sum(1) / n
    var_u = var_b * n / (n - 1) if n > 1 else var_b.copy()
    return Stats(n, mean, var_b, var_u, np.abs(v).sum(1), (v * v).sum(1))


def tol_mean(st):
    return U24 * np.abs(st.mean) + 2 * U53 * st.S1


def tol_var_b(st):
    return 8 * U53 * st.S2


def tol_var_u(st):
    return 2 * U24 * st.var_u + 8 * U53 * st.S2


def invstd64(st, eps):
    return 1.0 / np.sqrt(st.var_b + float(F32(eps)))


def tol_invstd(st, eps):
    i = invstd64(st, eps)
    return 2 * U24 * i + 0.5 * i * tol_var_b(st) / (st.var_b + float(F32(eps)))


def check_stats(x, mean, invstd, var_u, eps, what=""):
    """assert the published float32 statistics against stats64(x) within the derived bounds; returns the Stats"""
    st = stats64(x)
    for name, got, want, tol in (("mean", mean, st.mean, tol_mean(st)), ("invstd", invstd, invstd64(st, eps), tol_invstd(st, eps)),
                                 ("var_unbiased", var_u, st.var_u, tol_var_u(st))):
        got = _np(got).astype(np.float64)
        assert got.dtype == np.float64 and np.isfinite(got).all(), (what, name)
        err = np.abs(got - want)
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, f"{what} {name}: channel {bad[0]} off by {err[bad[0]]:.3e}, bound {tol[bad[0]]:.3e} (n = {st.n})"
    return st


def normalise(x, mean, invstd, gamma, beta, act, res=None):
    """bn_val in numpy float32, one rounded operation per statement, in the kernel's order; then + res, then ReLU"""
    x = _np(x)
    assert x.dtype == F32
    m, i, g, b = (_bc(_np(v).astype(F32, copy=False), x.ndim) for v in (mean, invstd, gamma, beta))
    for v in (mean, invstd, gamma, beta):
        assert _np(v).dtype == F32
    t = x - m
    t = t * i
    t = t * g
    t = t + b
    if res is not None:
        r = _np(res)
        assert r.dtype == F32
        t = t + r
    if act:
        t = np.maximum(t, F32(0))
    assert t.dtype == F32
    return t


def pool(v):
    """row maximum over the last axis and the FIRST index attaining it (torch.max's rule)"""
    return v.max(-1), v.argmax(-1).astype(np.uint8)


def route(dy, arg, K, mask=None):
    """the gradient of a max-pool as a dense (B, C, M, K) float32 array: dy (times the mask) at the recorded arg, 0 elsewhere"""
    dy, arg = _np(dy), _np(arg)
    d = dy if mask is None else np.where(mask, dy, F32(0))
    dq = np.zeros(dy.shape + (K,), F32)
    np.put_along_axis(dq, arg[..., None].astype(np.int64), d[..., None].astype(F32), -1)
    return dq


def sigmoid_dq(dy, y):
    """dy * (y * (1 - y)) in float32, the three operations in the kernel's order"""
    dy, y = _np(dy), _np(y)
    assert dy.dtype == F32 and y.dtype == F32
    t = F32(1) - y
    t = y * t
    return dy * t


Backward = collections.namedtuple("Backward", "dx tol_dx dgamma tol_dgamma dbeta tol_dbeta")


def backward64(x, dq, mean, invstd, gamma):
    """BatchNorm backward of the gradient dq (float32, same shape as x) in float64 from the published float32 mean and
    invstd, with the bounds of the module docstring"""
    x, dq = _np(x), _np(dq)
    assert x.dtype == F32 and dq.dtype == F32 and x.shape == dq.shape
    nd = x.ndim
    m32, i32, g32 = (_bc(_np(v).astype(F32, copy=False), nd) for v in (mean, invstd, gamma))
    xh32 = (x - m32) * i32  # as the kernel forms it: two float32 roundings
    assert xh32.dtype == F32
    red = (0,) + tuple(range(2, nd))
    n = x.size // x.shape[1]
    d = dq.astype(np.float64)
    t = d * xh32.astype(np.float64)
    Sa, Sb = d.sum(red), t.sum(red)
    A1, B1 = np.abs(d).sum(red), np.abs(t).sum(red)
    m, i, g = (v.astype(np.float64) for v in (m32, i32, g32))
    xh = (x.astype(np.float64) - m) * i
    gi = g * i
    ma, mb = _bc(Sa / n, nd), _bc(Sb / n, nd)
    dx = gi * (d - ma - xh * mb)
    tol_dx = (16 * U24 * np.abs(gi) * (np.abs(d) + np.abs(ma) + np.abs(xh * mb))
              + U53 * np.abs(gi) * (_bc(A1, nd) + np.abs(xh) * _bc(B1, nd)))
    return Backward(dx, tol_dx, Sb, U24 * np.abs(Sb) + n * U53 * B1, Sa, U24 * np.abs(Sa) + n * U53 * A1)


def check_backward(ref, dx, dgamma, dbeta, what=""):
    got = _np(dx).astype(np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref.dx)
    if not (err <= ref.tol_dx).all():
        k = np.unravel_index(np.argmax(err - ref.tol_dx), err.shape)
        raise AssertionError(f"{what} dx{list(k)} off by {err[k]:.3e}, bound {ref.tol_dx[k]:.3e} (value {ref.dx[k]:.3e})")
    for name, g, want, tol in (("dgamma", dgamma, ref.dgamma, ref.tol_dgamma), ("dbeta", dbeta, ref.dbeta, ref.tol_dbeta)):
        g = _np(g).astype(np.float64)
        assert np.isfinite(g).all(), (what, name)
        e = np.abs(g - want)
        bad = np.flatnonzero(~(e <= tol))
        assert bad.size == 0, f"{what} {name}: channel {bad[0]} off by {e[bad[0]]:.3e}, bound {tol[bad[0]]:.3e}"


def running_update(running, batch, momentum, step):
    """nn.BatchNorm's training-mode buffer rule in float32 (torch/nn/modules/batchnorm.py, aten batch_norm_update_stats):
    running = running * (1 - f) + f * batch with f = momentum, or 1 / step (the count after the increment) for momentum
    None.  Returns (new value, allowance): 2 ulp of the larger operand, because the fused and the two-rounding form of
    a * (1 - f) + f * b, and the running += (batch - running) * f form of the cumulative average, differ by that much."""
    r, b = _np(running).astype(F32), _np(batch).astype(F32)
    f = F32(1.0 / step) if momentum is None else F32(momentum)
    new = r * (F32(1) - f) + f * b
    big = np.maximum(np.maximum(np.abs(r), np.abs(b)), np.abs(new))
    return new.astype(F32), 2 * np.spacing(big.astype(F32)).astype(np.float64)


def sigmoid_yardstick(x, gamma, beta, eps):
    """(y64, allowance): sigmoid(batch_norm(x)) in float64 on the host and what an fp32 implementation may miss it by:
    4 x the error of torch's own float32 sigmoid(batch_norm(.)) of the same input against float64 (the device expf and
    torch's may each be off by a couple of ulp in opposite directions), at least 4 * 2^-24.  Also returns the measured
    torch error, so that tests can report it."""
    xs, gs, bs = (torch.as_tensor(_np(v)) for v in (x, gamma, beta))

    def run(dt):
        return torch.sigmoid(torch.nn.functional.batch_norm(xs.to(dt), None, None, gs.to(dt), bs.to(dt), True, 0.1, eps))

    y64 = run(torch.float64)
    err_torch = float((run(torch.float32).double() - y64).abs().max())
    return y64.numpy(), max(4 * err_torch, 4 * U24), err_torch
