"""ops.pointwise_conv_cloud_term -- y = W x + c[b] with one Cout-vector per cloud -- against the fp64 restatement of
tests/cloud_term_ref.py, and the fused first feature-propagation block built on it.

Bounds (u = 2^-24, the unit roundoff of fp32; derived, not tuned):
  y    Cin products and Cin - 1 adds in fp32 in some order, then one add of c: each of the at most Cin + 1 operations rounds a
       partial sum that is at most S = sum |w||x| + |c| in magnitude                  |y - y64|   <= (Cin + 2) u S  per element
  dc   P - 1 adds of a row of dy in some order                                       |dc - dc64| <= P u sum_p |dy|
  dx, dw   the rule of tests/test_gpu_pwconv.py: no further from fp64 than 4 x torch's own fp32 convolution is, or 2e-6 of
       max(1, the tensor's range)
With c == 0 the output is ops.pointwise_conv's, bit for bit, at every shape.  Forward and backward repeat their bits, in default
and in deterministic mode.  The fused block's peak memory stays below the size of the (B, E + C1, N) tensor it avoids."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cloud_term_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
CINS, COUTS = (1, 3, 35, 64), (1, 32, 50, 130)


def _case(B, P, Cin, Cout, zero_c=False):
    g = torch.Generator().manual_seed(((B * 4099 + P) * 131 + Cin) * 257 + Cout)
    x = torch.randn(B, Cin, P, generator=g)
    w = torch.randn(Cout, Cin, 1, generator=g) * 0.3
    # clearly different rows: cloud b's term is offset by 10 b, far more than any rounding, so a wrong cloud index shows
    c = torch.zeros(B, Cout) if zero_c else torch.randn(B, Cout, generator=g) + 10.0 * torch.arange(B).reshape(B, 1)
    dy = torch.randn(B, Cout, P, generator=g)
    return x.to(DEV), w.to(DEV), c.to(DEV), dy.to(DEV)


def _run(x, w, c, dy):
    from amcontrast3d_amd import ops
    xg, wg, cg = (t.clone().requires_grad_(True) for t in (x, w, c))
    y = ops.pointwise_conv_cloud_term(xg, wg, cg)
    y.backward(dy)
    return y.detach(), cg.grad, xg.grad, wg.grad


@pytest.mark.parametrize("P", [1, 63, 100, 257, 2053])
@pytest.mark.parametrize("B", [1, 3])
def test_against_the_fp64_restatement(B, P):
    worst = {"y": 0.0, "dc": 0.0}
    for Cin in CINS:
        for Cout in COUTS:
            x, w, c, dy = _case(B, P, Cin, Cout)
            y, dc, dx, dw = _run(x, w, c, dy)
            xn, wn, cn, dyn = (t.cpu().numpy() for t in (x, w[:, :, 0], c, dy))
            what = f"B {B} P {P} Cin {Cin} Cout {Cout}"
            assert y.shape == (B, Cout, P) and dc.shape == (B, Cout) and dx.shape == x.shape and dw.shape == w.shape, what
            y64 = R.forward(xn, wn, cn)
            bound = (Cin + 2) * U * R.forward_magnitude(xn, wn, cn)
            err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
            worst["y"] = max(worst["y"], float((err / bound).max()))
            assert (err <= bound).all(), what
            dc64, dx64, dw64 = R.backward(xn, wn, dyn)
            bound_dc = P * U * np.abs(dyn.astype(np.float64)).sum(-1)
            err_dc = np.abs(dc.cpu().numpy().astype(np.float64) - dc64)
            worst["dc"] = max(worst["dc"], float((err_dc / bound_dc).max()))
            assert (err_dc <= bound_dc).all(), what
            # dx, dw: torch's fp32 convolution as the yardstick of what fp32 costs
            xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            F.conv1d(xr, wr).backward(dy)
            for got, ref64, ref32, name in ((dx, dx64, xr.grad, "dx"), (dw[:, :, 0], dw64, wr.grad[:, :, 0], "dw")):
                e = float(np.abs(got.cpu().numpy().astype(np.float64) - ref64).max())
                e_torch = float(np.abs(ref32.cpu().numpy().astype(np.float64) - ref64).max())
                scale = max(1.0, float(np.abs(ref64).max()))
                assert e <= max(4 * e_torch, 2e-6 * scale), (what, name, e, e_torch, scale)
    print(f"B {B} P {P}: worst error / bound: y {worst['y']:.3f}, dc {worst['dc']:.3f}")


@pytest.mark.parametrize("B,P", [(3, 257), (2, 2053), (3, 100)])
def test_zero_term_is_pointwise_conv_bit_for_bit(B, P):
    """every channel pair, the deep ones (64 -> 130: the tiled GEMM, which adds the term in a pass of its own) included; and a
    column block of a wider weight, used where it lies"""
    from amcontrast3d_amd import ops
    for Cin in CINS:
        for Cout in COUTS:
            x, w, c, _ = _case(B, P, Cin, Cout, zero_c=True)
            a = ops.pointwise_conv_cloud_term(x, w, c)
            b = ops.pointwise_conv(x, w)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (Cin, Cout)
            wide = torch.randn(Cout, Cin + 5, generator=torch.Generator().manual_seed(Cin + Cout)).to(DEV)
            assert torch.equal(ops.pointwise_conv_cloud_term(x, wide[:, 5:], c), ops.pointwise_conv(x, wide[:, 5:].contiguous().unsqueeze(-1)))


def test_each_cloud_gets_its_own_row():
    """x == 0: the output is the term alone, exactly, at every position of every cloud (P = 2053: 17 tiles per cloud)"""
    from amcontrast3d_amd import ops
    for Cin, Cout in ((3, 50), (64, 130)):
        x, w, c, _ = _case(3, 2053, Cin, Cout)
        y = ops.pointwise_conv_cloud_term(torch.zeros_like(x), w, c)
        assert torch.equal(y, c.unsqueeze(-1).expand_as(y))


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_two_runs_give_equal_bits(det):
    from amcontrast3d_amd import ops
    for Cin, Cout, P in ((35, 50, 2053), (64, 130, 257), (3, 32, 100)):
        x, w, c, dy = _case(3, P, Cin, Cout)
        with ops.deterministic_mode(det):
            first, second = _run(x, w, c, dy), _run(x, w, c, dy)
        assert all(torch.equal(a, b) for a, b in zip(first, second)), (Cin, Cout, P)


def test_more_clouds_than_a_grid_axis_holds():
    """B = 65537: the cloud is a grid axis of at most 65535, so forward and backward go in runs; the last two clouds lie in
    the second run and must get their own rows of the term, their own dx, and their share of dw and dc"""
    B, P, Cin, Cout = 65537, 2, 3, 2
    g = torch.Generator().manual_seed(9)
    x, w, dy = torch.randn(B, Cin, P, generator=g).to(DEV), torch.randn(Cout, Cin, 1, generator=g).to(DEV), torch.randn(B, Cout, P, generator=g).to(DEV)
    c = (torch.arange(B, dtype=torch.float32).reshape(B, 1) * 0.001 + torch.tensor([[0.0, 100.0]])).to(DEV)
    y, dc, dx, dw = _run(x, w, c, dy)
    xn, wn, cn, dyn = (t.cpu().numpy() for t in (x, w[:, :, 0], c, dy))
    err = np.abs(y.cpu().numpy().astype(np.float64) - R.forward(xn, wn, cn))
    assert (err <= (Cin + 2) * U * R.forward_magnitude(xn, wn, cn)).all()
    dc64, dx64, dw64 = R.backward(xn, wn, dyn)
    assert (np.abs(dc.cpu().numpy() - dc64) <= P * U * np.abs(dyn.astype(np.float64)).sum(-1)).all()
    _, dx_mag, dw_mag = R.backward_magnitudes(xn, wn, dyn)
    assert (np.abs(dx.cpu().numpy() - dx64) <= (Cout + 1) * U * dx_mag).all()
    # dw sums B P products in the kernels' order, then the runs: the plain bound n u sum |dy||x| of any summation order
    assert (np.abs(dw[:, :, 0].cpu().numpy() - dw64) <= B * P * U * dw_mag).all()


def test_cpu_tensors_are_refused():
    from amcontrast3d_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pointwise_conv_cloud_term(torch.rand(1, 2, 3), torch.rand(4, 2), torch.rand(1, 4))


def _fp_module(E, C1, C2, Cout, seed=0):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.backbone import FeaturePropogation
    torch.manual_seed(seed)
    return FeaturePropogation([E + C1 + C2, Cout, Cout]).to(DEV).train()


def test_fused_block_never_holds_the_concatenated_tensor():
    """B = 2, E = 242, C1 = 32, N = 4096 (coarse cloud: 64 channels on 2048 points): the peak above the inputs of a training
    forward of the first block stays below the (B, E + C1, N) tensor the composition builds first"""
    B, E, C1, C2, Cout, N, M = 2, 242, 32, 64, 32, 4096, 2048
    fp = _fp_module(E, C1, C2, Cout)
    from openpoints.models.layers import cloud_term_route, feature_propagation_first_block
    g = torch.Generator().manual_seed(5)
    p1 = torch.rand(B, N, 3, generator=g).to(DEV)
    p2 = p1[:, :M].contiguous()
    f1 = torch.randn(B, C1, N, generator=g).to(DEV).requires_grad_(True)
    f2 = torch.randn(B, C2, M, generator=g).to(DEV).requires_grad_(True)
    e = torch.randn(B, E, generator=g).to(DEV).requires_grad_(True)
    geom = fp.plan(p1, p2)
    assert cloud_term_route(fp.convs[0], f1, f2, e) == "cloud_term"
    out = feature_propagation_first_block(fp.convs[0], f1, f2, geom, (e, E))  # warm: library handles, scratch
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = feature_propagation_first_block(fp.convs[0], f1, f2, geom, (e, E))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    avoided = B * (E + C1) * N * 4
    print(f"fused first FP block: peak {peak} bytes above the inputs; the (B, E + C1, N) tensor alone is {avoided} bytes")
    assert out.shape == (B, Cout, N) and peak < avoided
