"""Every route of csrc/bn.hip against tests/bn_ref.py: statistics within the bounds derived there, the normalised output
bit for bit, pooling with its arg byte, gradients within the element-arithmetic bounds.  The C entry points are called
directly (as ops.py does) so that mean, invstd, var_unbiased and arg are all visible; the autograd Functions run next to
them and must return the same bits.

Route -> case that reaches it (bn_split / bn_channel_form of csrc/bn.hip; tests/test_bn_ref_host.py restates them and checks this table):
    channel form, float4 loops                  act (2,64,8192) [B*L = 16384, the bound], (2,65,100) [L < one pass], (1,64,4)
    channel form, scalar loops                  act (3,64,333)
    two launches, one segment, one unit/chunk   act (2,5,1), (1,3,1) [count 1], residual (8,128,100) [C >= 64 but no channel form]
    two launches, several segments, float4      act / residual / sigmoid (2,3,8200) [2 segments of 4100]
    two launches, several segments, scalar      act (2,3,8197) [last segment 4097], act (1,64,16385) [one past the channel bound, 4 segments]
    strided unit loop (units > 64 chunks)       act / residual / sigmoid (70,5,37) [70 units], (130,3,8) [130: three units for chunks 0, 1]
                                                forward (bn_stats_kernel) and backward (bn_bwd_stats_kernel, all three dq forms);
                                                pooled layout: test_max_more_units_than_chunks (70,3,5,8), (130,3,5,5);
                                                13107 units: test_grid_bound's case at the bound
    bn_act_kernel float4 / scalar               (2,3,8200) / (2,3,8197), (3,7,65); with res: residual cases; sigmoid: sigmoid cases
    bn_max_coop_kernel<2,4,8,16>                max K = 8, 16, 32, 64 with M = 37 (last wave partly live) and M = 3 (< one wave)
    bn_max_kernel float4 branch                 max K = 12, 20, 24, 40 with M = 300 (two workgroups)
    bn_max_kernel scalar branch                 max K = 1, 3, 5, 31, 255; K = 8 at an odd storage offset
    K = 256                                     test_max_k256_is_refused (argument check, no launch)
    bn_bwd_apply float4, mode 1 ((ak-k0) < 4u)  max K % 4 == 0;   scalar mode 1: K % 4 != 0
    bn_bwd_apply / bn_bwd_stats ymask loops     residual and sigmoid cases, float4 ((2,3,8200), (8,128,100)) and scalar ((3,7,65), (70,5,37))
    bn_bwd_channel_kernel                       the channel-form cases above
    running update (bn_running_update of csrc/bn_math.h, called from)
      bn_fwd_channel_kernel                     test_running_statistics[act_channel]
      bn_channel_stats                          test_running_statistics[act_two, max, residual, sigmoid]
    bn_running_kernel (momentum None)           the same with momentum None; c += 1024 loop: test_cumulative_average_beyond_1024_channels
    momentum None bypasses the channel form     test_running_statistics[act_channel-None] (the channel kernel has no cumulative rule:
                                                the buffers move only if the two-launch form ran)
    scalar loops for misaligned pointers        test_offset_view
    B * C > 65535                               test_grid_bound
    amc3d_bn_act / amc3d_bn_max (evaluation)    test_eval_bit_exact
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# direct calls
# ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offset_view(t):
    """the same numbers as a contiguous view whose storage offset is one element: data_ptr() % 16 == 4"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class Out:
    pass


def _lib_ops():
    from amcontrast3d_amd import _lib, ops
    return _lib.load(), ops


def _bufs_ptrs(bufs, ops):
    if bufs is None:
        return None, None, None
    return tuple(ops._ptr(b) for b in bufs)


def c_forward(kind, x, gamma, beta, relu=False, K=0, res=None, mom=0.0, bufs=None, y=None, expect_error=False):
    """kind 'act' / 'max': amc3d_bn_forward; 'residual' / 'sigmoid': their own entry points.  x (B, C, *) on the device."""
    lib, ops = _lib_ops()
    B, C = x.shape[:2]
    L = x.numel() // (B * C)
    o = Out()
    o.mean, o.invstd, o.var_u = (torch.full((C,), -777.0, device=DEV) for _ in range(3))
    o.arg = None
    if K:
        o.y = torch.full((B, C, L // K), -777.0, device=DEV)
        o.arg = torch.full((B, C, L // K), 255, dtype=torch.uint8, device=DEV)
    else:
        o.y = torch.full(x.shape, -777.0, device=DEV) if y is None else y
    work, wb = ops._bn_ws(C, DEV)
    rm, rv, nbt = _bufs_ptrs(bufs, ops)
    p, s = ops._ptr, ops._stream(x)
    with torch.cuda.device(DEV):
        if kind in ("act", "max"):
            st = lib.amc3d_bn_forward(B, C, L, K, int(relu), EPS, mom, p(x), p(gamma), p(beta), p(o.y),
                                      None if o.arg is None else p(o.arg), p(o.mean), p(o.invstd), p(o.var_u), rm, rv, nbt,
                                      p(work), wb, s)
        elif kind == "residual":
            st = lib.amc3d_bn_residual_forward(B, C, L, EPS, mom, p(x), p(res), p(gamma), p(beta), p(o.y), p(o.mean), p(o.invstd),
                                               p(o.var_u), rm, rv, nbt, p(work), wb, s)
        else:
            st = lib.amc3d_bn_sigmoid_forward(B, C, L, EPS, mom, p(x), p(gamma), p(beta), p(o.y), p(o.mean), p(o.invstd),
                                              p(o.var_u), rm, rv, nbt, p(work), wb, s)
    torch.cuda.synchronize()
    o.status = st
    if not expect_error:
        assert st == 0, lib.amc3d_last_error().decode()
    return o


def c_backward(kind, x, dy, o, gamma, beta, relu=False, K=1, dx=None):
    lib, ops = _lib_ops()
    B, C = x.shape[:2]
    L = x.numel() // (B * C)
    g = Out()
    g.dx = torch.full(x.shape, -777.0, device=DEV) if dx is None else dx
    g.dres = torch.full(x.shape, -777.0, device=DEV) if kind == "residual" else None
    g.dgamma, g.dbeta = torch.full((C,), -777.0, device=DEV), torch.full((C,), -777.0, device=DEV)
    work, wb = ops._bn_ws(C, DEV, extra=C * 8)
    p, s = ops._ptr, ops._stream(x)
    with torch.cuda.device(DEV):
        if kind in ("act", "max"):
            st = lib.amc3d_bn_backward(B, C, L, K if kind == "max" else 1, int(relu), p(x), p(dy), p(o.arg) if kind == "max" else None,
                                       p(o.mean), p(o.invstd), p(gamma), p(beta), p(g.dx), p(g.dgamma), p(g.dbeta), p(work), wb, s)
        elif kind == "residual":
            st = lib.amc3d_bn_residual_backward(B, C, L, p(x), p(o.y), p(dy), p(o.mean), p(o.invstd), p(gamma), p(beta), p(g.dx),
                                                p(g.dres), p(g.dgamma), p(g.dbeta), p(work), wb, s)
        else:
            st = lib.amc3d_bn_sigmoid_backward(B, C, L, p(x), p(o.y), p(dy), p(o.mean), p(o.invstd), p(gamma), p(beta), p(g.dx),
                                               p(g.dgamma), p(g.dbeta), p(work), wb, s)
    torch.cuda.synchronize()
    assert st == 0, lib.amc3d_last_error().decode()
    return g


def function_run(kind, x, gamma, beta, dy, relu=False, res=None, bn=None):
    """the autograd Function of the same route: (y, mean, var_u, dx, dgamma, dbeta[, dres])"""
    from amcontrast3d_amd import ops
    xg = x.detach().requires_grad_(True)
    gg, bg = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    rg = None
    if kind == "act":
        y, m, v = ops.BatchNormAct.apply(xg, gg, bg, EPS, relu, bn)
    elif kind == "max":
        y, m, v = ops.BatchNormMax.apply(xg, gg, bg, EPS, relu, bn)
    elif kind == "residual":
        rg = res.detach().requires_grad_(True)
        y, m, v = ops.BatchNormResidualAct.apply(xg, rg, gg, bg, EPS, bn)
    else:
        y, m, v = ops.BatchNormSigmoid.apply(xg, gg, bg, EPS, bn)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), m, v, xg.grad, gg.grad, bg.grad, None if rg is None else rg.grad


# ---------------------------------------------------------------------------------------------------------------------
# the assertions every route shares
# ---------------------------------------------------------------------------------------------------------------------
def check_forward(kind, x, o, gamma, beta, relu, K=0, res=None, what=""):
    """statistics within the derived bounds; y (and arg) bit for bit from the kernel's own mean and invstd"""
    st = R.check_stats(x, o.mean, o.invstd, o.var_u, EPS, what)
    if kind == "sigmoid":
        return st
    v = R.normalise(x, o.mean, o.invstd, gamma, beta, relu or kind == "residual", res)
    y = o.y.cpu().numpy()
    if K:
        ymax, amax = R.pool(v.reshape(x.shape[0], x.shape[1], -1, K))
        assert np.array_equal(y, ymax), (what, "pooled value")
        assert np.array_equal(o.arg.cpu().numpy(), amax), (what, "arg is not the first index of the maximum")
    else:
        assert np.array_equal(y, v), (what, int((y != v).sum()), float(np.abs(y - v).max()))
    return st


def dq_of(kind, dy, o, relu, K=0):
    """the gradient reaching the BatchNorm output, from the kernel's OWN forward output (never a reference forward)"""
    y, d = o.y.cpu().numpy(), dy.cpu().numpy()
    if kind == "max":
        return R.route(d, o.arg.cpu().numpy(), K, (y > 0) if relu else None)
    if kind == "sigmoid":
        return R.sigmoid_dq(d, y)
    if relu or kind == "residual":
        return np.where(y > 0, d, F32(0))
    return d


def check_backward(kind, x, dy, o, g, gamma, relu, K=0, what=""):
    dq = dq_of(kind, dy, o, relu, K)
    xs = x.cpu().numpy()
    ref = R.backward64(xs.reshape(dq.shape), dq, o.mean, o.invstd, gamma)
    R.check_backward(ref, g.dx.cpu().numpy().reshape(dq.shape), g.dgamma, g.dbeta, what)
    if kind == "residual":
        assert np.array_equal(g.dres.cpu().numpy(), dq), (what, "dres != dy * (y > 0)")
    return dq


def run_case(kind, x, gamma, beta, dy, relu=False, K=0, res=None, what=""):
    """direct forward and backward with every assertion, then the autograd Function: the same bits"""
    o = c_forward(kind, x, gamma, beta, relu, K, res)
    check_forward(kind, x, o, gamma, beta, relu, K, res, what)
    g = c_backward(kind, x, dy, o, gamma, beta, relu, K)
    check_backward(kind, x, dy, o, g, gamma, relu, K, what)
    y, m, v, dx, dgamma, dbeta, dres = function_run(kind, x, gamma, beta, dy, relu, res)
    for name, a, b in (("y", y, o.y), ("mean", m, o.mean), ("var_u", v, o.var_u), ("dx", dx, g.dx), ("dgamma", dgamma, g.dgamma),
                       ("dbeta", dbeta, g.dbeta)) + ((("dres", dres, g.dres),) if kind == "residual" else ()):
        assert torch.equal(a, b), (what, name, "autograd Function and direct call differ")
    return o, g


def make(shape, seed, gamma_kind="mixed"):
    rng = np.random.default_rng(seed)
    C = shape[1]
    x = (rng.standard_normal(shape) * 3 + 1.5).astype(F32)
    gamma = (rng.random(C) - 0.3).astype(F32)
    if gamma_kind == "mixed" and C >= 3:
        gamma[0], gamma[1], gamma[2] = -abs(gamma[0]) - 0.1, 0.0, abs(gamma[2]) + 0.1
    if gamma_kind == "positive":
        gamma = np.abs(gamma) + F32(0.3)
    beta = rng.standard_normal(C).astype(F32)
    return rng, x, gamma, beta


# ---------------------------------------------------------------------------------------------------------------------
# BatchNormAct
# ---------------------------------------------------------------------------------------------------------------------
ACT_SHAPES = [(2, 64, 8192), (1, 64, 16385), (3, 64, 333), (2, 65, 100), (1, 64, 4), (2, 5, 1), (1, 3, 1), (2, 3, 8200),
              (2, 3, 8197), (70, 5, 37), (130, 3, 8), (3, 7, 65)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_act(shape, relu):
    rng, x, gamma, beta = make(shape, 11)
    dy = rng.standard_normal(shape).astype(F32)
    run_case("act", dev(x), dev(gamma), dev(beta), dev(dy), relu, what=f"act {shape} relu={relu}")


# ---------------------------------------------------------------------------------------------------------------------
# BatchNormMax
# ---------------------------------------------------------------------------------------------------------------------
def pool_data(B, C, M, K, seed):
    """random rows, then: ties between columns k and k ^ 1, k ^ 2, ... (every distance the cooperative combine steps over,
    the first two inside one float4) made the row's maximum, in different rows; rows that are negative throughout after the
    normalisation (all tie at 0 under ReLU); gamma negative, zero and positive"""
    rng, x, gamma, beta = make((B, C, M, K), seed)
    gamma[0], gamma[2] = gamma[0] - F32(0.4), gamma[2] + F32(0.4)  # clear of zero: a tied pair stays the maximum under ReLU
    rows = x.reshape(B * C * M, K)
    sign = np.where(gamma < 0, -1.0, 1.0).astype(F32)
    chan = (np.arange(B * C * M) // M) % C
    t, j = 1, 1
    ties = []
    while j < K and t < len(rows):
        lo = ((K - 1) >> 1) & ~j
        if (lo | j) >= K:
            lo = 0
        rows[t, :] = np.where(sign[chan[t]] > 0, np.minimum(rows[t], 4.0), np.maximum(rows[t], -1.0))
        rows[t, lo] = rows[t, lo | j] = sign[chan[t]] * 20.0  # the row's extreme in the direction gamma maximises
        ties.append((t, lo))
        t, j = t + 2, j * 2
    dead = [r for r in (0, 4, 8) if r < len(rows)]
    for r in dead:
        rows[r, :] = -sign[chan[r]] * (30.0 + np.abs(rows[r]))  # far on the side that normalises to a negative value
    beta = -np.abs(beta) * F32(0.1)  # ... and stays negative with the shift
    return rng, x, gamma, beta.astype(F32), ties, dead, chan


MAX_CASES = ([(K, M) for K in (8, 16, 32, 64) for M in (37, 3)] + [(K, 300) for K in (12, 20, 24, 40)]
             + [(K, 37) for K in (1, 3, 5, 31, 255)])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,M", MAX_CASES)
def test_max(K, M, relu):
    B, C = 2, 3
    rng, x, gamma, beta, ties, dead, chan = pool_data(B, C, M, K, 100 + K)
    dy = rng.standard_normal((B, C, M)).astype(F32)
    o, g = run_case("max", dev(x), dev(gamma), dev(beta), dev(dy), relu, K, what=f"max K={K} M={M} relu={relu}")
    arg, y = o.arg.cpu().numpy().reshape(-1), o.y.cpu().numpy().reshape(-1)
    for t, lo in ties:  # the lower of the two tied columns, every time (gamma == 0: the whole row ties, index 0)
        assert arg[t] == (0 if gamma[chan[t]] == 0 else lo), (t, lo, arg[t])
    assert (arg[chan == 1] == 0).all()  # gamma == 0: every neighbour gives beta
    if relu:
        # what passes through a row that is non-positive throughout: nothing.  All its K positions then carry the dense part
        # of dx alone, gi * (0 - ma - xh * mb), which the routed reference above has already pinned; here, that the row's
        # own dy has no influence: run again with other dy values in those rows
        for r in dead:
            assert arg[r] == 0 and y[r] == 0
        dy2 = dy.copy().reshape(-1)
        dy2[dead] += 1000.0
        g2 = c_backward("max", dev(x), dev(dy2.reshape(B, C, M)), o, dev(gamma), dev(beta), relu, K)
        assert torch.equal(g2.dx, g.dx) and torch.equal(g2.dgamma, g.dgamma) and torch.equal(g2.dbeta, g.dbeta)
    # dx is nonzero only through the recorded arg: away from it the routed reference allows 16 * 2^-24 |gi| (|ma| + |xh mb|),
    # a millionth of what a dy that leaked to another neighbour would add


@pytest.mark.parametrize("B,K", [(70, 8), (130, 5)])
def test_max_more_units_than_chunks(B, K):
    """the strided unit loops with the pooled layout: forward statistics over L = M*K, backward sums over the Lq = M pooled
    positions (mode 1 of bn_bwd_stats_kernel), 70 resp. 130 units for 64 chunks; cooperative (K = 8) and scalar (K = 5) kernels"""
    C, M = 3, 5
    rng, x, gamma, beta, ties, dead, chan = pool_data(B, C, M, K, 200 + K)
    dy = rng.standard_normal((B, C, M)).astype(F32)
    run_case("max", dev(x), dev(gamma), dev(beta), dev(dy), True, K, what=f"max B={B} K={K}")


def test_max_k256_is_refused():
    from amcontrast3d_amd import ops
    lib, _ = _lib_ops()
    x = torch.randn(1, 2, 3, 256, device=DEV)
    w, b = torch.ones(2, device=DEV), torch.zeros(2, device=DEV)
    with pytest.raises(RuntimeError):
        ops.BatchNormMax.apply(x, w, b, EPS, True)
    o = c_forward("max", x, w, b, True, 256, expect_error=True)
    assert o.status != 0 and b"bad argument" in lib.amc3d_last_error()
    for t in (o.y, o.mean, o.invstd, o.var_u):  # nothing was launched: every output still holds its fill
        assert bool((t == -777.0).all())
    assert bool((o.arg == 255).all())


# ---------------------------------------------------------------------------------------------------------------------
# BatchNormResidualAct, BatchNormSigmoid
# ---------------------------------------------------------------------------------------------------------------------
RES_SHAPES = [(8, 128, 100), (3, 7, 65), (2, 3, 8200), (70, 5, 37), (130, 3, 8)]


@pytest.mark.parametrize("shape", RES_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_residual(shape):
    rng, x, gamma, beta = make(shape, 21)
    res = rng.standard_normal(shape).astype(F32)
    dy = rng.standard_normal(shape).astype(F32)
    run_case("residual", dev(x), dev(gamma), dev(beta), dev(dy), True, res=dev(res), what=f"residual {shape}")


def sigmoid_case(shape, seed, gamma30=False):
    rng, x, gamma, beta = make(shape, seed, "positive")
    if gamma30:
        gamma[:] = 30.0
        x.reshape(-1)[::97] += 25.0   # normalised values beyond +-3, so that 30 * xhat passes +-88.8 where expf leaves
        x.reshape(-1)[5::89] -= 25.0  # float32's range: the output is exactly 1 resp. 0 there
    dy = rng.standard_normal(shape).astype(F32)
    return x, gamma, beta, dy


SIG_CASES = [((8, 128, 100), False), ((3, 7, 65), False), ((2, 3, 8200), False), ((70, 5, 37), False), ((130, 3, 8), False),
             ((3, 7, 65), True)]


@pytest.mark.parametrize("shape,gamma30", SIG_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"g30={s}")
def test_sigmoid(shape, gamma30):
    """allowance for y: 4 x the error of torch's float32 sigmoid(batch_norm(.)) against float64 on the same input (host),
    floor 4 * 2^-24 = 2.4e-7.  Torch's error and the allowance for these inputs: (8,128,100) 9.45e-8 -> 3.78e-7; (3,7,65)
    8.07e-8 -> 3.23e-7; (2,3,8200) 9.45e-8 -> 3.78e-7; (70,5,37) 8.17e-8 -> 3.27e-7; (130,3,8) 8.36e-8 -> 3.35e-7; (3,7,65) with
    gamma 30: 1.70e-7 -> 6.78e-7.  The test prints the kernel's own error next to them."""
    x, gamma, beta, dy = sigmoid_case(shape, 31, gamma30)
    what = f"sigmoid {shape} gamma30={gamma30}"
    o, g = run_case("sigmoid", dev(x), dev(gamma), dev(beta), dev(dy), what=what)
    y = o.y.cpu().numpy()
    y64, allow, err_torch = R.sigmoid_yardstick(x, gamma, beta, EPS)
    err = float(np.abs(y.astype(np.float64) - y64).max())
    print(f"{what}: kernel error {err:.3e}, torch fp32 error {err_torch:.3e}, allowance {allow:.3e}")
    assert err <= allow, (what, err, err_torch, allow)
    assert np.isfinite(y).all() and (y >= 0).all() and (y <= 1).all()
    if gamma30:
        sat = (y == 0) | (y == 1)
        assert (y == 0).any() and (y == 1).any()
        dq = R.sigmoid_dq(dy, y)
        assert (dq[sat] == 0).all() and np.isfinite(dq).all()  # what passes a saturated sigmoid is exactly zero
        # so a saturated position's own dy has no influence on any gradient: change it there and nothing moves, bit for bit
        dy2 = dy.copy()
        dy2[sat] = 1e30
        g2 = c_backward("sigmoid", dev(x), dev(dy2), o, dev(gamma), dev(beta))
        assert torch.equal(g2.dx, g.dx) and torch.equal(g2.dgamma, g.dgamma) and torch.equal(g2.dbeta, g.dbeta)
        assert bool(torch.isfinite(g.dx).all())


# ---------------------------------------------------------------------------------------------------------------------
# data edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 6, 500), (2, 64, 500)], ids=["two_launch", "channel_form"])
def test_data_edges(shape):
    rng, x, gamma, beta = make(shape, 41, "positive")
    x[:, 0] = F32(3.7)                                                  # constant: variance 0
    x[:, 1] = (100.0 + 0.05 * rng.standard_normal(x[:, 1].shape)).astype(F32)  # E[x^2] - mean^2 cancels 6 digits
    x[0, 2, 123] = 1e4                                                  # one outlier
    dy = rng.standard_normal(shape).astype(F32)
    o, g = run_case("act", dev(x), dev(gamma), dev(beta), dev(dy), False, what=f"edges {shape}")
    st = R.stats64(x)
    assert st.var_b[0] == 0.0
    assert float(o.var_u[0]) <= R.tol_var_u(st)[0] and float(o.var_u[0]) >= 0.0
    assert float(o.mean[0]) == F32(3.7)
    assert bool((o.y[:, 0] == float(beta[0])).all())  # x - mean is exactly 0
    for t in (g.dx, g.dgamma, g.dbeta, o.invstd):
        assert bool(torch.isfinite(t).all())
    run_case("act", dev(x), dev(gamma), dev(beta), dev(dy), True, what=f"edges {shape} relu")


# ---------------------------------------------------------------------------------------------------------------------
# running statistics
# ---------------------------------------------------------------------------------------------------------------------
RUNNING = {"act_channel": ("act", (2, 64, 100)), "act_two": ("act", (2, 5, 333)), "max": ("max", (2, 3, 37, 8)),
           "residual": ("residual", (3, 7, 65)), "sigmoid": ("sigmoid", (3, 7, 65))}


def _module(shape, momentum, seed):
    C = shape[1]
    bn = (nn.BatchNorm2d if len(shape) == 4 else nn.BatchNorm1d)(C, momentum=momentum).to(DEV).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn


def running_steps(kind, shape, momentum, steps=3):
    bn = _module(shape, momentum, 5)
    for step in range(1, steps + 1):
        rng, x, gamma, beta = make(shape, 50 + step)
        res = dev(rng.standard_normal(shape).astype(F32)) if kind == "residual" else None
        dy = dev(rng.standard_normal(shape[:3] if kind == "max" else shape).astype(F32))
        before = (bn.running_mean.clone(), bn.running_var.clone())
        y, mean, var_u = function_run(kind, dev(x), dev(gamma), dev(beta), dy, True, res, bn)[:3]
        st = R.stats64(x)
        assert (np.abs(mean.cpu().numpy() - st.mean) <= R.tol_mean(st)).all()
        assert (np.abs(var_u.cpu().numpy() - st.var_u) <= R.tol_var_u(st)).all()
        for name, buf, prev, batch in (("running_mean", bn.running_mean, before[0], mean), ("running_var", bn.running_var, before[1], var_u)):
            want, tol = R.running_update(prev, batch, momentum, step)
            err = np.abs(buf.cpu().numpy().astype(np.float64) - want)
            assert (err <= tol).all(), (kind, momentum, step, name, float(err.max()), float(tol.min()))
            assert not torch.equal(buf, prev)
        assert int(bn.num_batches_tracked) == step
    return bn


@pytest.mark.parametrize("momentum", [0.1, 0.37, None])
@pytest.mark.parametrize("name", list(RUNNING))
def test_running_statistics(name, momentum):
    """momentum None on the channel-form shape (C >= 64, small): bn_fwd_channel_kernel has no cumulative rule and leaves the
    buffers alone when momentum < 0, so buffers that follow the cumulative average show that the two-launch form ran (the
    timing spans do not distinguish the two forms)"""
    kind, shape = RUNNING[name]
    bn = running_steps(kind, shape, momentum)
    assert int(bn.num_batches_tracked) == 3


def test_momentum_none_gives_the_two_launch_numbers():
    """the bypass computes what the channel form computes: y bit for bit from its own statistics, statistics within the bounds of
    the same fp64 values (they need not be the same bits: the summation order differs)"""
    shape = (2, 64, 100)
    rng, x, gamma, beta = make(shape, 61)
    outs = []
    for mom in (0.1, -1.0):
        bn = _module(shape, None if mom < 0 else mom, 6)
        o = c_forward("act", dev(x), dev(gamma), dev(beta), True, mom=mom, bufs=(bn.running_mean, bn.running_var, bn.num_batches_tracked))
        check_forward("act", dev(x), o, gamma, beta, True, what=f"momentum {mom}")
        assert int(bn.num_batches_tracked) == 1
        outs.append(o)
    st = R.stats64(x)
    assert (np.abs(outs[0].mean.cpu().numpy().astype(np.float64) - outs[1].mean.cpu().numpy()) <= 2 * R.tol_mean(st)).all()


def test_cumulative_average_beyond_1024_channels():
    bn = running_steps("act", (2, 1030, 5), None)
    assert bn.running_mean.shape == (1030,)


def test_no_module_no_buffer_touched():
    shape = (2, 64, 100)
    rng, x, gamma, beta = make(shape, 71)
    for kind, shp in (("act", shape), ("act", (2, 5, 333)), ("max", (2, 3, 37, 8)), ("residual", (3, 7, 65)), ("sigmoid", (3, 7, 65))):
        bn = _module(shp, 0.1, 7)
        keep = copy.deepcopy(bn.state_dict())
        rng, x, gamma, beta = make(shp, 72)
        res = dev(rng.standard_normal(shp).astype(F32)) if kind == "residual" else None
        dy = dev(rng.standard_normal(shp[:3] if kind == "max" else shp).astype(F32))
        function_run(kind, dev(x), dev(gamma), dev(beta), dy, True, res, None)
        for k, v in bn.state_dict().items():
            assert torch.equal(v, keep[k]), (kind, k)


# ---------------------------------------------------------------------------------------------------------------------
# contiguous views at an odd storage offset: scalar loops, same assertions
# ---------------------------------------------------------------------------------------------------------------------
OFFSET = {"act_two": ("act", (2, 3, 8200), 0), "act_channel": ("act", (2, 64, 100), 0), "max_coop": ("max", (2, 3, 37, 8), 8),
          "max_f4": ("max", (2, 3, 300, 12), 12), "residual": ("residual", (3, 7, 64), 0), "sigmoid": ("sigmoid", (3, 7, 64), 0)}


@pytest.mark.parametrize("name", list(OFFSET))
def test_offset_view(name):
    """L % 4 == 0 and data_ptr() % 16 == 4 for every tensor the caller hands over (x, res, dy): no 16-byte access may be made
    to them, and the results obey the same bounds as those of an aligned copy"""
    kind, shape, K = OFFSET[name]
    rng, x, gamma, beta = make(shape, 81, "positive" if kind == "sigmoid" else "mixed")
    res = rng.standard_normal(shape).astype(F32) if kind == "residual" else None
    dy = rng.standard_normal(shape[:3] if kind == "max" else shape).astype(F32)
    relu = kind != "sigmoid"
    ys = []
    for shift in (offset_view, lambda t: t):
        xs, dys = shift(dev(x)), shift(dev(dy))
        rs = None if res is None else shift(dev(res))
        o, g = run_case(kind, xs, dev(gamma), dev(beta), dys, relu, K, rs, what=f"offset {name}")
        ys.append(o)
    if kind == "sigmoid":
        y64, allow, _ = R.sigmoid_yardstick(x, gamma, beta, EPS)
        for o in ys:
            assert float(np.abs(o.y.cpu().numpy() - y64).max()) <= allow
    # outputs at an odd offset as well (direct calls: the Functions allocate their own)
    if kind in ("act", "residual"):
        xs = offset_view(dev(x))
        yo = offset_view(torch.full(shape, -777.0, device=DEV))
        o = c_forward(kind, xs, dev(gamma), dev(beta), True, res=None if res is None else dev(res), y=yo)
        check_forward(kind, xs, o, gamma, beta, True, res=res, what=f"offset y {name}")
        dxo = offset_view(torch.full(shape, -777.0, device=DEV))
        g = c_backward(kind, xs, dev(dy), o, dev(gamma), dev(beta), True, dx=dxo)
        check_backward(kind, xs, dev(dy), o, g, gamma, True, what=f"offset dx {name}")


# ---------------------------------------------------------------------------------------------------------------------
# B * C beyond the grid's y axis
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_bound():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import timing
    from openpoints.models.layers.blocks import batchnorm_act
    lib, ops = _lib_ops()
    torch.manual_seed(0)
    bn = nn.BatchNorm1d(4).to(DEV).train()
    ref = copy.deepcopy(bn)
    x = torch.randn(70000, 4, device=DEV) * 2 + 1
    with timing.count_calls() as launched:
        got = batchnorm_act(bn, x, None)
    assert not launched, dict(launched)  # the torch module
    assert torch.equal(got, ref(x))
    for (k, a), (_, b) in zip(bn.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k
    bn.eval(); ref.eval()
    with torch.no_grad(), timing.count_calls() as launched:
        assert torch.equal(batchnorm_act(bn, x, nn.ReLU()), torch.relu(ref(x)))
    assert not launched, dict(launched)
    # the C entry points report it and launch nothing
    B, C = 70000, 4
    w, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    x3 = x.view(B, C, 1)
    for kind in ("act", "residual", "sigmoid"):
        o = c_forward(kind, x3, w, b, True, res=x3, expect_error=True)
        assert o.status != 0 and b"65535" in lib.amc3d_last_error(), kind
        for t in (o.y, o.mean, o.invstd, o.var_u):
            assert bool((t == -777.0).all()), kind
    fill = lambda *s: torch.full(s, -777.0, device=DEV)
    y, dx, dres, dg, db = fill(B, C, 1), fill(B, C, 1), fill(B, C, 1), fill(C), fill(C)
    arg = torch.zeros(B, C, 1, dtype=torch.uint8, device=DEV)
    work, wb = ops._bn_ws(C, DEV, extra=C * 8)
    p, s = ops._ptr, ops._stream(x)
    with torch.cuda.device(DEV):
        calls = {
            "bn_act": lib.amc3d_bn_act(B, C, 1, 1, p(x3), p(b), p(w), p(w), p(b), p(y), s),
            "bn_max": lib.amc3d_bn_max(B, C, 1, 1, 1, p(x3), p(b), p(w), p(w), p(b), p(y), p(arg), s),
            "bn_forward max": lib.amc3d_bn_forward(B, C, 1, 1, 1, EPS, 0.0, p(x3), p(w), p(b), p(y), p(arg), p(dg), p(db), p(dg), None,
                                                   None, None, p(work), wb, s),
            "bn_backward": lib.amc3d_bn_backward(B, C, 1, 1, 1, p(x3), p(x3), None, p(b), p(w), p(w), p(b), p(dx), p(dg), p(db),
                                                 p(work), wb, s),
            "bn_backward max": lib.amc3d_bn_backward(B, C, 1, 1, 1, p(x3), p(x3), p(arg), p(b), p(w), p(w), p(b), p(dx), p(dg), p(db),
                                                     p(work), wb, s),
            "bn_residual_backward": lib.amc3d_bn_residual_backward(B, C, 1, p(x3), p(x3), p(x3), p(b), p(w), p(w), p(b), p(dx),
                                                                   p(dres), p(dg), p(db), p(work), wb, s),
            "bn_sigmoid_backward": lib.amc3d_bn_sigmoid_backward(B, C, 1, p(x3), p(x3), p(x3), p(b), p(w), p(w), p(b), p(dx), p(dg),
                                                                 p(db), p(work), wb, s),
        }
    torch.cuda.synchronize()
    assert all(v != 0 for v in calls.values()), calls
    for t in (y, dx, dres, dg, db):
        assert bool((t == -777.0).all())
    # exactly at the bound the kernels run
    xb = torch.randn(13107, 5, 1, device=DEV)
    w5, b5 = torch.rand(5, device=DEV) + 0.5, torch.randn(5, device=DEV)
    o = c_forward("act", xb, w5, b5, True)
    check_forward("act", xb, o, w5.cpu().numpy(), b5.cpu().numpy(), True, what="B * C == 65535")


# ---------------------------------------------------------------------------------------------------------------------
# evaluation mode
# ---------------------------------------------------------------------------------------------------------------------
EVAL_CASES = [((2, 3, M, K), True) for K, M in MAX_CASES] + [((2, 5, 333), False), ((2, 24, 1000), False), ((70, 5, 36), False)]


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,pooled", EVAL_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None)
def test_eval_bit_exact(shape, pooled, relu, offset):
    from amcontrast3d_amd import ops
    rng, x, gamma, beta = make(shape, 91)
    C = shape[1]
    bn = (nn.BatchNorm2d if len(shape) == 4 else nn.BatchNorm1d)(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(dev(gamma)); bn.bias.copy_(dev(beta))
        bn.running_mean.copy_(dev(rng.standard_normal(C).astype(F32)))
        bn.running_var.copy_(dev((rng.random(C) + 0.2).astype(F32)))
    bn.eval()
    xs = offset_view(dev(x)) if offset else dev(x)
    got = ops.bn_eval(xs, bn, relu, pooled).cpu().numpy()
    invstd = torch.rsqrt(bn.running_var + bn.eps)  # the call ops.bn_eval makes
    v = R.normalise(x, bn.running_mean, invstd, gamma, beta, relu)
    want = R.pool(v)[0] if pooled else v
    assert got.shape == want.shape and np.array_equal(got, want)
