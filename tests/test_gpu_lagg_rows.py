"""The neighbourhood layers with G = W_f . f stored as rows by the conv itself (csrc/pwconv.hip, gemm.hip: the position-major
epilogue on the forward; csrc/lagg.hip: lagg_stats_rows_kernel, the two finalize kernels over partial[channel][part][5],
lagg_bwd_apply_kernel with several points per wave row).

 * the row-storing conv equals the channel-major conv transposed, bit for bit, on every route and store form;
 * LocalAggregationFused / GroupedConvBN against the fp64 torch evaluation of tests/test_gpu_lagg.py, with its tolerances, on
   its shapes and on the sizes at which the new kernels take another path (every channel width that selects another instance,
   a cloud below one tile, odd clouds, one and three clouds, in-degree 0, the point count at which a statistics workgroup takes
   a second pass, more partial records than one pass of the finalize's unrolled loop), atomic and reverse-list backward;
 * eval mode bit-equal to the entries that take G channel-major; the same bits on every run in deterministic mode;
   SyncBatchNorm's two phases on one rank; the entries that take G channel-major still within tolerance."""
import contextlib
import ctypes

import pytest
import torch

from test_gpu_lagg import _case, _reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from amcontrast3d_amd import _lib, ops
    return ops, _lib, _lib.load()


# ---- the conv ------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [
    (2, 8, 8, 257),        # pw_gemm<1>, P odd
    (2, 32, 32, 1000),     # pw_gemm<1>
    (1, 16, 40, 130),      # pw_gemm<2>
    (2, 24, 70, 333),      # Cout % 4 != 0: the 4-byte stores
    (1, 32, 96, 512),      # pw_gemm<3>
    (1, 48, 128, 300),     # pw_gemm<4>
    (2, 64, 64, 6000),     # gm_gemm, P not a multiple of 128
    (3, 128, 128, 1500),   # split-K
    (2, 256, 256, 375),    # split-K
]


def _conv_both(B, Cin, Cout, P, strided, misaligned=False, seed=0):
    ops, _lib, lib = _ops()
    g = torch.Generator().manual_seed(seed + Cin + Cout + P)
    x = torch.randn(B, Cin, P, generator=g).to(DEV)
    if strided:  # the feature columns of a neighbourhood layer's [W_dp | W_f]
        w = (torch.randn(Cout, Cin + 3, generator=g) * 0.3).to(DEV)[:, 3:]
    else:
        w = (torch.randn(Cout, Cin, generator=g) * 0.3).to(DEV)
    y_cm = torch.full((B, Cout, P), float("nan"), device=DEV)
    buf = torch.full((B * P * Cout + 4,), float("nan"), device=DEV)
    off = 1 if misaligned else 0
    y_pm = buf[off:off + B * P * Cout].view(B, P, Cout)
    assert (y_pm.data_ptr() % 16 != 0) == misaligned
    with torch.cuda.device(DEV):
        wsf = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(B, Cin, Cout, P, 0))
        work = torch.empty(max(wsf, 4), dtype=torch.uint8, device=DEV)
        _lib.check(lib.amc3d_pointwise_conv_forward_strided(B, Cin, Cout, P, ops._ptr(x), ops._ptr(w), ops._ld(w), None,
                                                            ops._ptr(y_cm), ops._ptr(work), wsf, ops._stream(x)), "conv cm")
        ops._pw_forward_rows(lib, B, Cin, Cout, P, x, w, y_pm)
    torch.cuda.synchronize()
    return y_cm, y_pm, buf, off


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,Cin,Cout,P", CONV_SHAPES)
def test_conv_rows_are_the_channel_major_output_transposed(B, Cin, Cout, P, strided):
    y_cm, y_pm, buf, off = _conv_both(B, Cin, Cout, P, strided)
    assert not torch.isnan(y_cm).any()
    assert torch.equal(y_pm, y_cm.transpose(1, 2))
    assert torch.isnan(buf[B * P * Cout:]).all()  # nothing behind the last row


@pytest.mark.parametrize("B,Cin,Cout,P", [(2, 32, 32, 1000), (2, 64, 64, 6000), (3, 128, 128, 1500)])
def test_conv_rows_at_a_base_that_is_not_16_byte_aligned(B, Cin, Cout, P):
    y_cm, y_pm, buf, off = _conv_both(B, Cin, Cout, P, True, misaligned=True)
    assert torch.equal(y_pm, y_cm.transpose(1, 2))
    assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + B * P * Cout:]).all()


# ---- the layers, forward and backward -------------------------------------------------------------------------------------
def _counts(B, C, N, M, K):
    ops, _lib, lib = _ops()
    c = (ctypes.c_int * 4)()
    _lib.check(lib.amc3d_local_aggregation_partial_counts(B, C, N, M, K, c), "partial counts")
    return {"forward": c[0], "scatter": c[1], "collapse": c[2], "lists": c[3]}


FINALIZE_PASS = 1024  # records one pass of lagg_sum_records' unrolled loop consumes (640 threads x 8 loads / 5)

LA_CASES = [
    # tests/test_gpu_lagg.py's list
    (2, 8, 8, 700, 700, 32, True),
    (2, 16, 32, 900, 225, 32, True),
    (3, 32, 64, 1500, 375, 32, False),
    (2, 64, 64, 1200, 1200, 32, True),
    (1, 128, 128, 800, 800, 32, True),
    (2, 64, 256, 640, 160, 32, True),
    (1, 24, 512, 300, 75, 16, True),
    # 16 channels; a cloud below one tile of any kernel; odd clouds, one and three of them; M = N / 4 (in-degree 0)
    (3, 8, 16, 1111, 277, 32, True),
    (1, 8, 16, 63, 63, 32, True),
    (1, 16, 32, 1501, 375, 32, False),
    (3, 8, 8, 63, 15, 32, True),
    # 2 x 140001 points: above 1024 passes of 256 points, a statistics workgroup takes two (512 points, the last one fewer)
    (2, 8, 8, 140001, 300, 32, True),
]


@pytest.mark.parametrize("B,Cin,C,N,M,K,relu", LA_CASES)
def test_local_aggregation_on_rows(B, Cin, C, N, M, K, relu):
    ops, _lib, lib = _ops()
    p, idx, dp, f, w, gamma, beta, go = _case(B, Cin, C, N, M, K, 11 + C, relu)
    if M * 4 <= N and N >= 500:  # (a ball holds far more than K points: those late in the cloud are nobody's neighbour)
        indeg = torch.zeros(B, N, device=DEV).scatter_add_(1, idx.reshape(B, -1).long(), torch.ones(B, M * K, device=DEV))
        assert float((indeg == 0).float().mean()) > 0.05
    cnt = _counts(B, C, N, M, K)
    print("partial records per channel:", cnt)
    # which side of the threshold: one 256-point pass per statistics workgroup while that keeps them at ~1024 per launch
    passes, most = (B * N + 255) // 256, max(1, 1024 // max(1, C // 64))
    assert (cnt["forward"] == passes) == (passes <= most)
    assert (N == 140001) == (passes > most)
    mom = ops.group_moments(idx, dp, N)
    ref = None
    for det in (False, True):  # the atomic and the reverse-list backward
        bn = torch.nn.BatchNorm2d(C).to(f.device)
        fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
        log = {}
        ops.pool_log(log)
        try:
            with (ops.deterministic_mode() if det else contextlib.nullcontext()):
                pooled = ops.LocalAggregationFused.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, relu, bn)
        finally:
            ops.pool_log(None)
        pooled.backward(go)
        arg = log[0]
        if ref is None:
            ref = _reference(idx, dp, f, w, gamma, beta, go, relu, arg)
            arg0 = arg
        assert torch.equal(arg, arg0)
        tol = lambda r: 2e-5 * max(1.0, float(r.abs().max()))  # noqa: E731
        assert float((pooled.double() - ref["pooled"]).abs().max()) <= tol(ref["pooled"])
        assert float((ref["pooled"] - ref["own_max"]).abs().max()) <= tol(ref["own_max"])
        assert float((bn.running_mean.double() - 0.1 * ref["mean"]).abs().max()) <= 1e-5
        assert float((bn.running_var.double() - (0.9 + 0.1 * ref["var_u"])).abs().max()) <= 1e-5 * max(1.0, float(ref["var_u"].max()))
        assert int(bn.num_batches_tracked) == 1
        for name, got, want in (("df", fr.grad, ref["df"]), ("dw", wr.grad, ref["dw"]), ("dgamma", gr.grad, ref["dgamma"]),
                                ("dbeta", br.grad, ref["dbeta"])):
            err = float((got.double() - want).abs().max())
            assert err <= 5e-5 * max(1.0, float(want.abs().max())), (det, name, err, float(want.abs().max()))


def _reference_x1(idx, dp, f, w, gamma, beta, go):
    """GroupedConvBN as the reference writes it, fp64 torch (tests/test_gpu_lagg.py::test_grouped_conv_bn_first_block)"""
    B, Cin, N = f.shape
    _, M, K = idx.shape
    C = w.shape[0]
    f64 = f.double().requires_grad_(True)
    w64, g64, b64 = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    fj = f64.gather(2, idx.reshape(B, 1, -1).expand(-1, Cin, -1).long()).reshape(B, Cin, M, K)
    y = torch.nn.functional.conv2d(torch.cat([dp.double(), fj], 1), w64)
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    x1 = torch.relu((y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-5) * g64[None, :, None, None]
                    + b64[None, :, None, None])
    x1.backward(go.double())
    cnt = y.numel() / C
    return {"x1": x1.detach(), "mean": mean.detach(), "var": var.detach(), "var_u": (var * cnt / (cnt - 1)).detach(),
            "df": f64.grad, "dw": w64.grad, "dgamma": g64.grad, "dbeta": b64.grad}


GC_CASES = [
    # tests/test_gpu_lagg.py's list
    (2, 8, 8, 900, 225),
    (2, 32, 32, 2000, 500),
    (3, 64, 64, 1200, 300),
    (2, 128, 128, 640, 160),
    (1, 256, 256, 372, 93),
    # 16 channels; below one tile; odd clouds, one and three of them (M = N / 4 throughout)
    (2, 16, 16, 2000, 500),
    (1, 8, 16, 63, 15),
    (3, 8, 8, 1111, 277),
    (1, 32, 32, 1501, 375),
    # more partial records than one pass of the finalize's unrolled loop, plus a remainder: the atomic collapse's ...
    (3, 8, 8, 3000, 3000),
    # ... and the reverse-list collapse's
    (3, 16, 64, 3000, 750),
]


@pytest.mark.parametrize("B,Cin,C,N,M", GC_CASES)
def test_grouped_conv_bn_on_rows(B, Cin, C, N, M):
    ops, _lib, lib = _ops()
    K = 32
    p, idx, dp, f, w, gamma, beta, _ = _case(B, Cin, C, N, M, K, 31 + C, True)
    go = torch.randn(B, C, M, K, generator=torch.Generator().manual_seed(3)).to(f.device)
    cnt = _counts(B, C, N, M, K)
    print("partial records per channel:", cnt)
    if (B, N, M) == (3, 3000, 3000):
        assert cnt["collapse"] > FINALIZE_PASS and cnt["collapse"] % FINALIZE_PASS != 0
    if (B, N, M) == (3, 3000, 750):
        assert cnt["lists"] > FINALIZE_PASS and cnt["lists"] % FINALIZE_PASS != 0
    mom = ops.group_moments(idx, dp, N)
    ref = _reference_x1(idx, dp, f, w, gamma, beta, go)
    csr = ops.group_csr(idx, N)
    # the atomic backward, the reverse-list backward, and the latter on a gradient that arrives as position-major rows
    go_pm = go.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not go_pm.is_contiguous() and torch.equal(go_pm, go)
    for lists, grad in ((None, go), (csr, go), (csr, go_pm)):
        bn = torch.nn.BatchNorm2d(C).to(f.device)
        fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
        x1 = ops.GroupedConvBN.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, bn, lists)
        x1.backward(grad)
        assert float((x1.double() - ref["x1"]).abs().max()) <= 2e-5 * max(1.0, float(ref["x1"].abs().max()))
        assert float((bn.running_mean.double() - 0.1 * ref["mean"]).abs().max()) <= 1e-5
        assert float((bn.running_var.double() - (0.9 + 0.1 * ref["var_u"])).abs().max()) <= 1e-5 * max(1.0, float(ref["var"].max()))
        for name, got, want in (("df", fr.grad, ref["df"]), ("dw", wr.grad, ref["dw"]), ("dgamma", gr.grad, ref["dgamma"]),
                                ("dbeta", br.grad, ref["dbeta"])):
            err = float((got.double() - want).abs().max())
            assert err <= 1e-4 * max(1.0, float(want.abs().max())), (lists is not None, name, err, float(want.abs().max()))


# ---- eval mode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,C,N,M", [(2, 16, 32, 900, 225), (1, 8, 8, 63, 15), (3, 64, 64, 1201, 300), (1, 128, 256, 640, 160)])
def test_eval_mode_equals_the_channel_major_entries(B, Cin, C, N, M):
    ops, _lib, lib = _ops()
    K = 32
    p, idx, dp, f, w, gamma, beta, _ = _case(B, Cin, C, N, M, K, 5, True)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5); bn.weight.copy_(gamma); bn.bias.copy_(beta)
    bn.eval()
    w2 = w.reshape(C, Cin + 3).contiguous()
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    P_, S_ = ops._ptr, ops._stream
    g_cm = torch.empty(B, C, N, device=DEV)
    g_pm = torch.empty(B, N, C, device=DEV)
    with torch.cuda.device(DEV), torch.no_grad():
        ops._pw_forward(lib, False, B, Cin, C, N, f, w2[:, 3:], None, g_cm)
        pooled, ystar = torch.empty(B, C, M, device=DEV), torch.empty(B, C, M, device=DEV)
        arg = torch.empty(B, C, M, dtype=torch.uint8, device=DEV)
        _lib.check(lib.amc3d_local_aggregation_forward(
            B, C, N, M, K, 0, 1, float(bn.eps), 0.0, P_(g_cm), P_(idx), P_(dp), P_(w2), Cin + 3, None, P_(bn.weight), P_(bn.bias),
            P_(g_pm), P_(pooled), P_(arg), P_(ystar), P_(bn.running_mean), P_(invstd), None, None, None, None, None, 0, None,
            None, 0, S_(f)), "old pooled entry")
        x1 = torch.empty(B, C, M, K, device=DEV)
        _lib.check(lib.amc3d_grouped_conv_bn_forward(
            B, C, N, M, K, 0, 1, float(bn.eps), 0.0, P_(g_cm), P_(idx), P_(dp), P_(w2), Cin + 3, None, P_(bn.weight), P_(bn.bias),
            P_(g_pm), P_(x1), P_(bn.running_mean), P_(invstd), None, None, None, None, None, 0, None, None, 0, S_(f)),
            "old expand entry")
    assert torch.equal(ops.local_aggregation_eval(f, dp, idx, w, bn, True), pooled)
    assert torch.equal(ops.grouped_conv_bn_eval(f, dp, idx, w, bn, True), x1)
    fj = ops.grouping_operation(f, idx)
    want = torch.relu(bn(torch.nn.functional.conv2d(torch.cat([dp, fj], 1), w)))
    assert float((x1 - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))


# ---- the same bits on every run ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,C,N,M", [(3, 8, 8, 1111, 277), (2, 32, 32, 2000, 500), (2, 64, 128, 1201, 300)])
def test_deterministic_mode_gives_equal_bits_twice(B, Cin, C, N, M):
    from test_gpu_deterministic import _lagg_backward
    ops, _lib, lib = _ops()
    K = 32
    p, idx, dp, f, w, gamma, beta, go = _case(B, Cin, C, N, M, K, 7 + C, True)
    go4 = torch.randn(B, C, M, K, generator=torch.Generator().manual_seed(3)).to(DEV)
    mom = ops.group_moments(idx, dp, N)
    csr = ops.group_csr(idx, N)
    runs = []
    for _ in range(2):
        out = []
        for layer, grad in ((ops.LocalAggregationFused, go), (ops.GroupedConvBN, go4)):
            fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
            with ops.deterministic_mode():
                y = layer.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, None)
            saved = y.grad_fn.saved_tensors
            mean, invstd, gd = saved[9], saved[10], saved[11]
            y.backward(grad)
            out += [mean.clone(), invstd.clone(), gd.clone(), y.detach().clone(), fr.grad, wr.grad, gr.grad, br.grad]
            if layer is ops.LocalAggregationFused:  # dg itself, from the entry the layer calls
                out += list(_lagg_backward(saved, go, True, csr))
        runs.append(out)
    assert len(runs[0]) == 8 + 5 + 8
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- SyncBatchNorm: phase 1 then phase 2 on one rank = phase 0 -----------------------------------------------------------
TOL = 2e-5  # tests/test_gpu_syncbn.py


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B,Cin,C,N,M", [(2, 16, 32, 900, 225), (3, 64, 64, 1111, 277)])
def test_two_phases_on_one_rank_equal_phase_zero(B, Cin, C, N, M, det, monkeypatch):
    ops, _lib, lib = _ops()
    K = 32
    p, idx, dp, f, w, gamma, beta, go = _case(B, Cin, C, N, M, K, 3 + C, True)
    go4 = torch.randn(B, C, M, K, generator=torch.Generator().manual_seed(3)).to(DEV)
    mom = ops.group_moments(idx, dp, N)
    synced = []
    monkeypatch.setattr(ops, "_sync", lambda group, buf: synced.append(buf.numel()))  # one rank: the sums stay as written
    group = object()
    for layer, grad, extra in ((ops.LocalAggregationFused, go, lambda g: (g, None)), (ops.GroupedConvBN, go4, lambda g: (None, g))):
        res = []
        for grp in (None, group):
            bn = torch.nn.BatchNorm2d(C).to(DEV)
            fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
            del synced[:]
            with (ops.deterministic_mode() if det else contextlib.nullcontext()):
                y = layer.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, bn, *extra(grp))
            y.backward(grad)
            assert synced == ([] if grp is None else [2 * C + 1, 2 * C])
            res.append((y.detach(), fr.grad, wr.grad, gr.grad, br.grad, bn.running_mean.clone(), bn.running_var.clone()))
        (y0, df0, dw0, dg0, db0, rm0, rv0), (y1, df1, dw1, dg1, db1, rm1, rv1) = res
        assert float((y1 - y0).abs().max()) <= TOL and float((df1 - df0).abs().max()) <= TOL
        for a, b in ((dw1, dw0), (dg1, dg0), (db1, db0)):
            assert float((a - b).abs().max() / b.abs().max()) <= TOL
        assert float((rm1 - rm0).abs().max()) <= TOL and float((rv1 - rv0).abs().max()) <= TOL


# ---- the entries that take G channel-major -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,C,N,M", [(2, 16, 32, 900, 225), (3, 8, 8, 1111, 277), (1, 64, 128, 640, 160)])
def test_channel_major_entries_still_match_the_reference(B, Cin, C, N, M):
    ops, _lib, lib = _ops()
    K = 32
    p, idx, dp, f, w, gamma, beta, go = _case(B, Cin, C, N, M, K, 9 + C, True)
    go4 = torch.randn(B, C, M, K, generator=torch.Generator().manual_seed(3)).to(DEV)
    mom = ops.group_moments(idx, dp, N)
    w2 = w.reshape(C, Cin + 3).contiguous()
    P_, S_ = ops._ptr, ops._stream
    g_cm, g_pm = torch.empty(B, C, N, device=DEV), torch.full((B, N, C), float("nan"), device=DEV)
    mean, invstd, var_u = (torch.empty(C, device=DEV) for _ in range(3))
    gd = torch.empty(C, 3, dtype=torch.float64, device=DEV)
    wb = int(lib.amc3d_local_aggregation_workspace_bytes(B, C, N, M))
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        ops._pw_forward(lib, False, B, Cin, C, N, f, w2[:, 3:], None, g_cm)
        x1 = torch.empty(B, C, M, K, device=DEV)
        _lib.check(lib.amc3d_grouped_conv_bn_forward(
            B, C, N, M, K, 1, 1, 1e-5, 0.1, P_(g_cm), P_(idx), P_(dp), P_(w2), Cin + 3, P_(mom), P_(gamma), P_(beta), P_(g_pm),
            P_(x1), P_(mean), P_(invstd), P_(var_u), P_(gd), None, None, None, 0, None, P_(work), wb, S_(f)), "old expand entry")
    ref = _reference_x1(idx, dp, f, w, gamma, beta, go4)
    assert torch.equal(g_pm, g_cm.transpose(1, 2))
    assert float((x1.double() - ref["x1"]).abs().max()) <= 2e-5 * max(1.0, float(ref["x1"].abs().max()))
    assert float((mean.double() - ref["mean"]).abs().max()) <= 1e-5
    assert float((var_u.double() - ref["var_u"]).abs().max()) <= 1e-5 * max(1.0, float(ref["var"].max()))
    assert float((invstd.double() - torch.rsqrt(ref["var"] + 1e-5)).abs().max()) <= 2e-5 * float(torch.rsqrt(ref["var"] + 1e-5).max())
    # the pooled layer: the same statistics (the same sums in the same order), the maximum of x1 over the neighbours
    mean2, invstd2, var_u2 = (torch.empty(C, device=DEV) for _ in range(3))
    pooled, ystar = torch.empty(B, C, M, device=DEV), torch.empty(B, C, M, device=DEV)
    arg = torch.empty(B, C, M, dtype=torch.uint8, device=DEV)
    g_pm.fill_(float("nan"))
    with torch.cuda.device(DEV):
        _lib.check(lib.amc3d_local_aggregation_forward(
            B, C, N, M, K, 1, 1, 1e-5, 0.1, P_(g_cm), P_(idx), P_(dp), P_(w2), Cin + 3, P_(mom), P_(gamma), P_(beta), P_(g_pm),
            P_(pooled), P_(arg), P_(ystar), P_(mean2), P_(invstd2), P_(var_u2), P_(gd), None, None, None, 0, None, P_(work), wb,
            S_(f)), "old pooled entry")
    assert torch.equal(mean2, mean) and torch.equal(invstd2, invstd) and torch.equal(var_u2, var_u)
    want = ref["x1"].max(-1).values
    assert float((pooled.double() - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
