"""tests/bn_ref.py on the host: its float64 backward against torch's autograd, and its bounds against a numpy model of the
kernels' arithmetic (fp64 sums in another order than numpy's own, float32 element operations in the kernels' order).  An honest
float32 implementation must fit every bound on the very inputs the GPU tests use; the four one-line mistakes the GPU tests are
there to catch must not.  Also checks the route table of tests/test_gpu_bn_routes.py against bn_split / bn_channel_form."""
import numpy as np
import pytest
import torch

import bn_ref as R
import test_gpu_bn_routes as T

F32 = np.float32
EPS = 1e-5


def split(B, C, Lq):
    """bn_split of csrc/bn.hip: (segments per cloud, units, chunks, segment length)"""
    want = (2048 + C - 1) // C
    cps = min(max((want + B - 1) // B, 1), max(Lq // 4096, 1))
    seg = ((Lq + cps - 1) // cps + 3) & ~3
    cps = (Lq + seg - 1) // seg
    return cps, B * cps, min(B * cps, 64), seg


def channel_form(B, C, L):
    return C >= 64 and B * L <= 16384


def test_routes_named_in_the_gpu_tests():
    assert channel_form(2, 64, 8192) and not channel_form(1, 64, 16385) and channel_form(3, 64, 333)
    assert channel_form(2, 65, 100) and channel_form(1, 64, 4) and channel_form(8, 128, 100) and channel_form(2, 64, 500)
    assert channel_form(2, 64, 100) and channel_form(2, 1030, 5) and not channel_form(2, 6, 500)
    assert split(2, 5, 1)[:3] == (1, 2, 2) and split(1, 3, 1)[:3] == (1, 1, 1)
    assert split(2, 3, 8200) == (2, 4, 4, 4100) and split(2, 3, 8197) == (2, 4, 4, 4100)
    assert split(1, 64, 16385)[0] == 4
    assert split(70, 5, 37)[1:3] == (70, 64) and split(130, 3, 8)[1:3] == (130, 64)
    assert split(70, 5, 36)[1:3] == (70, 64) and split(13107, 5, 1)[1:3] == (13107, 64)
    assert split(70, 3, 40)[1:3] == (70, 64) and split(70, 3, 5)[1:3] == (70, 64)  # pooled: forward over M*K, backward over M
    assert split(130, 3, 25)[1:3] == (130, 64) and split(130, 3, 5)[1:3] == (130, 64)
    for K, M in T.MAX_CASES:
        lpr = K // 4
        coop = K % 4 == 0 and lpr in (2, 4, 8, 16)
        assert coop == (K in (8, 16, 32, 64))
        if not coop and K % 4 == 0:
            assert M > 256  # the float4 branch of the generic kernel with two workgroups
    assert sorted({K for K, _ in T.MAX_CASES}) == [1, 3, 5, 8, 12, 16, 20, 24, 31, 32, 40, 64, 255]


# ---------------------------------------------------------------------------------------------------------------------
# a numpy model of the kernels
# ---------------------------------------------------------------------------------------------------------------------
def model_stats(x, biased=False):
    v = R.per_channel(x).astype(np.float64)
    n = v.shape[1]
    s1 = v[:, ::-1].cumsum(1)[:, -1]  # plain recursive sums, from the far end: an order of its own
    s2 = (v * v)[:, ::-1].cumsum(1)[:, -1]
    m = s1 / n
    var = np.maximum(s2 / n - m * m, 0.0)
    invstd = (1.0 / np.sqrt(var + float(F32(EPS)))).astype(F32)
    vu = var if (biased or n == 1) else var * n / (n - 1.0)
    return m.astype(F32), invstd, vu.astype(F32)


def model_backward(x, dq, mean, invstd, gamma, drop_ma=False):
    nd = x.ndim
    m, i, g = (R._bc(v, nd) for v in (mean, invstd, gamma))
    xh = (x - m) * i
    red = (0,) + tuple(range(2, nd))
    n = x.size // x.shape[1]
    sa = dq.astype(np.float64).sum(red)
    sb = (dq.astype(np.float64) * xh.astype(np.float64)).sum(red)
    ma, mb = R._bc((sa / n).astype(F32), nd), R._bc((sb / n).astype(F32), nd)
    gi = g * i
    t = dq if drop_ma else dq - ma
    dx = gi * (t - xh * mb)
    assert dx.dtype == F32
    return dx, sb.astype(F32), sa.astype(F32)


SHAPES = sorted(set(T.ACT_SHAPES + T.RES_SHAPES + [(2, 6, 500), (2, 64, 500), (2, 1030, 5), (13107, 5, 1)]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bounds_admit_an_honest_float32_kernel_and_refuse_the_mutations(shape):
    rng, x, gamma, beta = T.make(shape, 11)
    dy = rng.standard_normal(shape).astype(F32)
    mean, invstd, var_u = model_stats(x)
    st = R.check_stats(x, mean, invstd, var_u, EPS)
    y = R.normalise(x, mean, invstd, gamma, beta, True)
    dq = np.where(y > 0, dy, F32(0))
    ref = R.backward64(x, dq, mean, invstd, gamma)
    dx, dgamma, dbeta = model_backward(x, dq, mean, invstd, gamma)
    R.check_backward(ref, dx, dgamma, dbeta)
    if st.n > 1:
        with pytest.raises(AssertionError, match="var_unbiased"):  # mutation 1: the biased variance published
            R.check_stats(x, mean, invstd, model_stats(x, biased=True)[2], EPS)
    if st.n > 2 and np.abs(ref.dbeta * gamma).max() > 0:
        with pytest.raises(AssertionError, match="dx"):  # mutation 4: `- ma` dropped
            R.check_backward(ref, model_backward(x, dq, mean, invstd, gamma, drop_ma=True)[0], dgamma, dbeta)


def test_data_edges_on_the_model():
    for shape in ((2, 6, 500), (2, 64, 500)):
        rng, x, gamma, beta = T.make(shape, 41, "positive")
        x[:, 0] = F32(3.7)
        x[:, 1] = (100.0 + 0.05 * rng.standard_normal(x[:, 1].shape)).astype(F32)
        x[0, 2, 123] = 1e4
        mean, invstd, var_u = model_stats(x)
        st = R.check_stats(x, mean, invstd, var_u, EPS)
        assert st.var_b[0] == 0 and mean[0] == F32(3.7) and var_u[0] <= R.tol_var_u(st)[0]
        assert (R.normalise(x, mean, invstd, gamma, beta, False)[:, 0] == beta[0]).all()
        # the cancellation channel: the allowance is far below the variance itself, so the check still means something
        assert R.tol_var_u(st)[1] < 1e-3 * st.var_u[1]


@pytest.mark.parametrize("K,M", T.MAX_CASES)
def test_pool_data_and_routing(K, M):
    B, C = 2, 3
    rng, x, gamma, beta, ties, dead, chan = T.pool_data(B, C, M, K, 100 + K)
    assert gamma[0] < 0 and gamma[1] == 0 and gamma[2] > 0
    mean, invstd, var_u = model_stats(x)
    R.check_stats(x, mean, invstd, var_u, EPS)
    for relu in (False, True):
        v = R.normalise(x, mean, invstd, gamma, beta, relu)
        y, arg = R.pool(v)
        a = arg.reshape(-1)
        assert len(ties) == (K - 1).bit_length()
        for t, lo in ties:
            want = 0 if gamma[chan[t]] == 0 else lo
            assert a[t] == want and (gamma[chan[t]] == 0 or v.reshape(-1, K)[t, lo] > 0)
            if gamma[chan[t]] != 0:  # a second column holds the same value: only the first-index rule decides
                assert (v.reshape(-1, K)[t] == v.reshape(-1, K)[t, lo]).sum() == 2
        if relu:
            for r in dead:
                assert y.reshape(-1)[r] == 0 and a[r] == 0 and (v.reshape(-1, K)[r] == 0).all()
        dy = rng.standard_normal((B, C, M)).astype(F32)
        dq = R.route(dy, arg, K, (y > 0) if relu else None)
        assert (np.count_nonzero(dq, -1) <= 1).all()
        ref = R.backward64(x, dq, mean, invstd, gamma)
        R.check_backward(ref, *model_backward(x, dq, mean, invstd, gamma))
        # a gradient routed to the LAST instead of the first of two tied neighbours is outside the bound
        if ties and gamma[chan[ties[0][0]]] != 0 and (not relu):
            wrong = arg.copy().reshape(-1)
            t, lo = ties[0]
            wrong[t] = lo | 1
            bad = R.route(dy, wrong.reshape(arg.shape), K, None)
            with pytest.raises(AssertionError, match="dx"):
                R.check_backward(ref, *model_backward(x, bad, mean, invstd, gamma))


def test_backward64_is_torch_autograd_in_float64():
    rng, x, gamma, beta = T.make((3, 7, 65), 3)
    dy = rng.standard_normal(x.shape).astype(F32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    y = torch.relu(torch.nn.functional.batch_norm(xt, None, None, gt, bt, True, 0.1, EPS))
    y.backward(torch.from_numpy(dy).double())
    mean, invstd, _ = model_stats(x)
    dq = np.where(y.detach().numpy() > 0, dy, F32(0))
    ref = R.backward64(x, dq, mean, invstd, gamma)
    # the float32 statistics are the only difference: 2^-23 relative on xhat and invstd
    assert np.abs(ref.dx - xt.grad.numpy()).max() <= 1e-5 * np.abs(ref.dx).max()
    assert np.allclose(ref.dgamma, gt.grad.numpy(), rtol=1e-5, atol=1e-6) and np.allclose(ref.dbeta, bt.grad.numpy(), rtol=1e-6, atol=1e-9)


def test_sigmoid_helpers():
    x, gamma, beta, dy = T.sigmoid_case((3, 7, 65), 31, True)
    y64, allow, err_torch = R.sigmoid_yardstick(x, gamma, beta, EPS)
    assert allow == max(4 * err_torch, 4 * R.U24) and y64.dtype == np.float64
    assert (y64 < 1e-38).any() and (y64 == 1).any()  # the saturating case does saturate
    y = y64.astype(F32)
    dq = R.sigmoid_dq(dy, y)
    assert (dq[(y == 0) | (y == 1)] == 0).all() and np.isfinite(dq).all()


def test_running_update_rule():
    """against nn.BatchNorm1d itself on the host, three steps, for each momentum"""
    for momentum in (0.1, 0.37, None):
        bn = torch.nn.BatchNorm1d(5, momentum=momentum).train()
        g = torch.Generator().manual_seed(0)
        for step in (1, 2, 3):
            x = torch.randn(4, 5, 9, generator=g) * 2 + 1
            before = (bn.running_mean.clone(), bn.running_var.clone())
            bn(x)
            for prev, now, batch in ((before[0], bn.running_mean, x.mean((0, 2))), (before[1], bn.running_var, x.var((0, 2), unbiased=True))):
                want, tol = R.running_update(prev, batch, momentum, step)
                assert (np.abs(now.numpy().astype(np.float64) - want) <= tol + 4 * np.spacing(np.abs(batch.numpy()))).all()
            assert int(bn.num_batches_tracked) == step
