"""Mixed precision (torch.autocast('cuda', torch.bfloat16), the reference's use_amp) against an exact model of its
arithmetic: conv operands rounded to bf16 (round-to-nearest-even), products accumulated in fp32, every tensor --
outputs and gradients included -- fp32 (include/amc3d.h, csrc/gemm_bf16.hip).

The arbiter is torch in fp64 ON THE SAME bf16-ROUNDED OPERANDS (t.to(torch.bfloat16).double()): then only the fp32
summation order differs and the bound stays at 2e-5 of the result's range, some hundred times below what a skipped
rounding, a rounded output or a lost K tail costs.  Covered:
  * csrc/gemm_bf16.hip at its edges: K tails of each loader, M / N tile tails, batch strides with odd P, every shape
    class of the weight-gradient split (gb_wgrad_splits), unvectorised loads, one gradient only, exact bf16 ties and
    carries, an fp32 bias under small products, the APM tower widths;
  * every bf16 route of a layer: the conv before the gather (LocalAggregationFused, GroupedConvBN) with its routing
    edges, the library GEMMs (LibraryGemmConv), and the eval-mode routes, which must stay fp32."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5


def _bf(t):
    return t.detach().to(torch.bfloat16).double()


def _close(name, got, ref, tol=TOL):
    assert got.dtype == torch.float32, (name, got.dtype)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    err = float((got.double() - ref).abs().max())
    bound = tol * max(1.0, float(ref.abs().max()))
    print(f"  {name}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (name, err, bound)


def _pw_reference(x, w, bias, go):
    """fp64 on bf16-rounded operands; the bias and the bias gradient stay fp32 / exact"""
    xr, wr = _bf(x), _bf(w)
    y = torch.einsum("oc,bcp->bop", wr, xr)
    if bias is not None:
        y = y + bias.detach().double()[None, :, None]
    return {"y": y, "dx": torch.einsum("oc,bop->bcp", wr, _bf(go)), "dw": torch.einsum("bop,bcp->oc", _bf(go), xr),
            "db": go.double().sum((0, 2))}


def _run_pw(B, ci, co, P, bias=False, need_x=True, need_w=True, seed=0, wscale=0.1):
    """ops.pointwise_conv(bf16=True) forward and backward against _pw_reference -> the weight gradient"""
    from amcontrast3d_amd import ops
    g = torch.Generator().manual_seed(seed * 7919 + B * 1000003 + ci * 1009 + co * 31 + P)
    x = torch.randn(B, ci, P, generator=g).to(DEV).requires_grad_(need_x)
    w = (torch.randn(co, ci, 1, generator=g) * wscale).to(DEV).requires_grad_(need_w)
    b = torch.randn(co, generator=g).to(DEV).requires_grad_(True) if bias else None
    go = torch.randn(B, co, P, generator=g).to(DEV)
    y = ops.pointwise_conv(x, w, b, True)
    y.backward(go)
    ref = _pw_reference(x, w[..., 0], b, go)
    print(f"B={B} Cin={ci} Cout={co} P={P}")
    _close("y", y, ref["y"])
    if need_x:
        _close("dx", x.grad, ref["dx"])
    if need_w:
        _close("dw", w.grad[..., 0], ref["dw"])
    else:
        assert w.grad is None
    if not need_x:
        assert x.grad is None
    if bias:
        _close("db", b.grad, ref["db"])
    return w.grad


# forward K = Cin on the k-contiguous weight loader: scalar tails of 1..3 and a partial last chunk of 32
@pytest.mark.parametrize("ci", [1, 3, 17, 33, 63, 65])
def test_bf16_forward_k_tails(ci):
    _run_pw(2, ci, 40, 1000, bias=True)


# backward-data K = Cout on the row-contiguous loader: odd K takes the `k + 1 < kend` branch
@pytest.mark.parametrize("co", [1, 13, 33])
def test_bf16_backward_data_k_tails(co):
    _run_pw(2, 48, co, 1000)


# weight gradient K = P (both operands k-contiguous)
@pytest.mark.parametrize("B,P", [(1, 1), (1, 31), (1, 33), (1, 4097), (2, 33), (3, 4097)])
def test_bf16_weight_gradient_k_tails(B, P):
    _run_pw(B, 40, 24, P)


# M / N tails of the 128 x 128 tile: Cout (forward M, weight-gradient M), Cin (backward-data M, weight-gradient N), P
# (forward / backward-data N), with batch strides at odd P
@pytest.mark.parametrize("B,ci,co,P", [(2, 64, 1, 300), (2, 64, 129, 300), (2, 64, 255, 300), (2, 129, 64, 257),
                                      (2, 255, 96, 130), (3, 64, 64, 1), (3, 64, 64, 127), (3, 64, 64, 129),
                                      (2, 96, 200, 4099)])
def test_bf16_tile_tails(B, ci, co, P):
    _run_pw(B, ci, co, P, bias=True)


def _wgrad_splits(b, cin, cout, P):
    """gb_wgrad_splits (csrc/gemm_bf16.hip) restated: (splits asked for, K per split, splits launched)"""
    tiles = -(-cout // 128) * -(-cin // 128)
    s = max(1, min(1024 // (tiles * b), max(P // 512, 1)))
    per = -(-(-(-P // s)) // 32) * 32
    return s, per, -(-P // per)


@pytest.mark.parametrize("B,ci,co,P,kind", [
    (1, 64, 64, 1535, "short"),     # just below 512 * 3: two splits of 768, the last one short
    (1, 64, 64, 1536, "even"),      # at 512 * 3: three splits of 512
    (1, 64, 64, 1537, "short"),     # just above: K per split rounded up to 544, the last split is short
    (1, 64, 64, 10241, "fewer"),    # 20 asked, 544 per split -> 19 launched
    (2, 256, 256, 8191, "short"),   # 4 tiles x 2 clouds (at most 128 splits), P / 512 = 15 splits of 576, the last short
    (2, 200, 130, 16385, "fewer"),  # 32 asked, 544 per split -> 31
])
def test_bf16_weight_gradient_splits(B, ci, co, P, kind):
    """every class of the weight-gradient split; the result is bit-identical run to run (fixed-order reduction)"""
    from amcontrast3d_amd import _lib
    s, per, n = _wgrad_splits(B, ci, co, P)
    # the restatement is the kernel's: the workspace holds one (Cout, Cin) partial per cloud and launched split
    assert int(_lib.load().amc3d_pointwise_conv_workspace_bytes_bf16(B, ci, co, P)) == 4 * B * n * co * ci
    last = P - (n - 1) * per
    assert n > 1
    assert {"even": last == per, "short": last < per and n == s, "fewer": n < s}[kind], (s, per, n, last)
    dws = [_run_pw(B, ci, co, P, seed=1).clone() for _ in range(3)]
    assert torch.equal(dws[0], dws[1]) and torch.equal(dws[0], dws[2])


def test_bf16_unvectorised_loads():
    """P % 4 == 0 and Cin % 4 == 0 but every operand 4 bytes off 16-byte alignment (a view at storage offset 1): the
    loaders take their scalar paths (vec_a = vec_b = 0).  Through the C-ABI, which keeps the pointers as given."""
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    B, ci, co, P = 2, 64, 96, 1024
    g = torch.Generator().manual_seed(17)

    def off(*shape, scale=1.0):
        n = 1
        for s in shape:
            n *= s
        t = (torch.randn(n + 1, generator=g) * scale).to(DEV)[1:].view(*shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t

    x, w, dy = off(B, ci, P), off(co, ci, scale=0.1), off(B, co, P)
    bias = torch.randn(co, generator=g).to(DEV)
    y, dx, dw = (torch.empty(B, co, P, device=DEV), torch.empty(B, ci, P, device=DEV), torch.empty(co, ci, device=DEV))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.amc3d_pointwise_conv_forward_bf16(B, ci, co, P, p(x), p(w), p(bias), p(y), st), "forward_bf16")
    wb = int(lib.amc3d_pointwise_conv_workspace_bytes_bf16(B, ci, co, P))
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.amc3d_pointwise_conv_backward_bf16(B, ci, co, P, p(x), p(w), p(dy), p(dx), p(dw), p(work), wb, st),
               "backward_bf16")
    ref = _pw_reference(x, w, bias, dy)
    for name, got in (("y", y), ("dx", dx), ("dw", dw)):
        _close(name, got, ref[name])


@pytest.mark.parametrize("need_x,need_w", [(True, False), (False, True)])
def test_bf16_one_gradient_only(need_x, need_w):
    _run_pw(2, 96, 72, 2001, bias=True, need_x=need_x, need_w=need_w)


def _special_values(n, seed):
    """fp32 values at and around the bf16 rounding boundaries: exact ties below odd and even bf16 mantissas (RNE: odd
    rounds up, even down), one bit either side of a tie, ties whose rounding up carries into the exponent (mantissa all
    ones), both signs"""
    g = torch.Generator().manual_seed(seed)
    hi = torch.randint(0x3D80, 0x4180, (n,), generator=g, dtype=torch.int32)  # |v| in [1/16, 16)
    hi[: n // 4] = (hi[: n // 4] | 0x7F)  # mantissa all ones: a tie or more carries into the next binade
    lo = torch.tensor([0x8000, 0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF, 0x4000, 0xC000], dtype=torch.int32)
    lo = lo[torch.randint(0, len(lo), (n,), generator=g)]
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 31
    v = ((hi << 16) | lo | sign).view(torch.float32)
    assert torch.isfinite(v).all()
    return v


def test_bf16_operands_round_to_nearest_even():
    """A product with one operand exactly 1.0 is the other operand's bf16 rounding, exact in fp32: every operand of every
    product (forward weight and x, backward-data dy, weight-gradient dy and x) must come out as torch.to(bfloat16)
    rounds it -- ties to even, carries into the exponent included -- bit for bit."""
    from amcontrast3d_amd import ops
    n = 4099
    v = _special_values(n, 5)
    want = v.to(torch.bfloat16).float().to(DEV)
    vd = v.to(DEV)
    assert ((v.view(torch.int32) & 0xFFFF) == 0x8000).sum() > n // 8  # plenty of exact ties
    one = lambda *s: torch.ones(*s, device=DEV)
    # forward, values in x (the n-contiguous loader), weight 1
    y = ops.pointwise_conv(vd.view(1, 1, n), one(1, 1, 1), None, True)
    assert torch.equal(y.view(-1), want)
    # forward, values in the weight (the k-contiguous loader), x = 1
    y = ops.pointwise_conv(one(1, 1, 1), vd.view(n, 1, 1), None, True)
    assert torch.equal(y.view(-1), want)
    # weight gradient dW = dy x^T with x = 1, the values in dy; then backward-data dx = W^T dy with W = 1
    x = one(1, 1, 1).requires_grad_(True)
    w = one(n, 1, 1).requires_grad_(True)
    ops.pointwise_conv(x, w, None, True).backward(vd.view(1, n, 1))
    assert torch.equal(w.grad.view(-1), want)
    x = one(1, 1, n).requires_grad_(True)
    w = one(1, 1, 1).requires_grad_(True)
    ops.pointwise_conv(x, w, None, True).backward(vd.view(1, 1, n))
    assert torch.equal(x.grad.view(-1), want)
    # weight gradient with the values in x, dy = 1
    x = vd.view(1, n, 1).clone().requires_grad_(True)
    w = one(1, n, 1).requires_grad_(True)
    ops.pointwise_conv(x, w, None, True).backward(one(1, 1, 1))
    assert torch.equal(w.grad.view(-1), want)


def test_bf16_bias_is_added_in_fp32():
    """bias ~ 1000 (bf16's ulp there is 4) plus products of ~0.01: a bias rounded to bf16 is off by up to 2, the bound is
    2e-5 x 1000"""
    from amcontrast3d_amd import ops
    g = torch.Generator().manual_seed(23)
    B, ci, co, P = 2, 64, 130, 777
    x = (torch.randn(B, ci, P, generator=g) * 0.1).to(DEV)
    w = (torch.randn(co, ci, 1, generator=g) * 0.01).to(DEV)
    bias = (1000 + 4 * torch.rand(co, generator=g)).to(DEV)
    assert float((bias.to(torch.bfloat16).float() - bias).abs().max()) > 0.5
    y = ops.pointwise_conv(x, w, bias, True)
    _close("y", y, _pw_reference(x, w[..., 0], bias, torch.zeros_like(y))["y"])


# the APM towers of AMContrast3D++ (APM/concatenation.py: [p ; f] -> 32 -> 16 -> 8 -> 4 -> 2 -> 1, pointwise_conv with the
# autocast flag) at the positions of a 1 x 120000 cloud's first two encoder stages and of a batch of 8 x 24000
@pytest.mark.parametrize("B,ci,co,P", [(1, 35, 32, 30000), (1, 32, 16, 30000), (1, 16, 8, 7500), (1, 8, 4, 7500),
                                      (1, 4, 2, 120000), (1, 2, 1, 120000), (8, 35, 32, 6000)])
def test_bf16_apm_tower_widths(B, ci, co, P):
    _run_pw(B, ci, co, P, bias=True, wscale=0.3)


# ------------------------------------------------------------------------------------------------------------ layer routes

def _lagg_case(B, Cin, C, N, M, K, seed, radius=0.35):
    from amcontrast3d_amd import ops
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, N, 3, generator=g).to(DEV)
    q = p[:, :M].contiguous()
    idx = ops.ball_query(radius, K, p, q)
    dp = (ops.grouping_operation(p.transpose(1, 2).contiguous(), idx) - q.transpose(1, 2).unsqueeze(-1)) / radius
    f = torch.randn(B, Cin, N, generator=g).to(DEV)
    w = (torch.randn(C, Cin + 3, 1, 1, generator=g) * 0.3).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    gamma[::5] *= -1
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    return idx, dp.contiguous(), f, w, gamma, beta


def _grouped_reference(idx, dp, f, w, gamma, beta, go, relu, arg, rounded, eps=1e-5):
    """The layer in fp64 in the product's factorisation W.[dp ; f[idx]] = (W_f.f)[idx] + W_dp.dp.  `rounded`: the
    contract of the bf16 route -- W_f and f rounded for the forward product, W_f and the gradient dg of W_f.f rounded for
    the two backward products; W_dp and dp stay fp32.  arg: the kernel's max-pool picks (LocalAggregation) or None (the
    activation itself, GroupedConvBN)."""
    B, Cin, N = f.shape
    C = w.shape[0]
    _, M, K = idx.shape
    rnd = _bf if rounded else (lambda t: t.detach().double())
    w2 = w.detach().reshape(C, Cin + 3).double()
    wf, fr = rnd(w2[:, 3:]), rnd(f)
    wdp = w2[:, :3].clone().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    gcm = torch.einsum("oc,bcn->bon", wf, fr).requires_grad_(True)
    y = (gcm.gather(2, idx.reshape(B, 1, -1).expand(-1, C, -1).long()).reshape(B, C, M, K)
         + torch.einsum("oc,bcmk->bomk", wdp, dp.double()))
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    z = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps) * g64[None, :, None, None] + b64[None, :, None, None]
    if relu:
        z = torch.relu(z)
    out = z if arg is None else z.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)
    out.backward(go.double())
    dg = rnd(gcm.grad)
    dwf = torch.einsum("bon,bcn->oc", dg, fr)
    return {"out": out.detach(), "df": torch.einsum("oc,bon->bcn", wf, dg),
            "dw": torch.cat((wdp.grad, dwf), 1).view(w.shape), "dgamma": g64.grad, "dbeta": b64.grad}


def _spy_bf16(monkeypatch):
    """count the bf16 entries of the pointwise conv (ops._pw with the bf16 flag) a layer asks for"""
    from amcontrast3d_amd import ops
    calls = []
    orig = ops._pw

    def spy(lib, bf16):
        calls.append(bool(bf16))
        return orig(lib, bf16)
    monkeypatch.setattr(ops, "_pw", spy)
    return calls


def _check_grouped(name, got, want, unrounded, bf16, tol):
    """forward values and the fp32 gradients (dgamma, dbeta, W_dp's columns) at the fp32 bound; df and W_f's gradient
    depend on dg, which the product computes in fp32 before rounding it, so a rare element rounds the other way than the
    fp64 dg does.  Those are held to 2 % of the rounding signal (L2) -- what an unrounded or a wrongly rounded
    operand costs -- and to the fp32 bound where no rounding happens"""
    err = float((got.double() - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    if bf16 and name in ("df", "dw"):
        dist = float((got.double() - want).norm())
        signal = float((unrounded - want).norm())
        print(f"  {name}: L2 err {dist:.3e}, rounding signal {signal:.3e}, max err {err:.3e} (range {scale:.3e})")
        assert dist <= 0.02 * signal, (name, dist, signal)
    else:
        print(f"  {name}: max err {err:.3e} (bound {tol * scale:.3e})")
        assert err <= tol * scale, (name, err, tol * scale)


@pytest.mark.parametrize("layer", ["lagg", "gcbn"])
@pytest.mark.parametrize("B,Cin,C,N,M,bf16", [
    (1, 64, 64, 4096, 1024, True),    # B * N = 4096, min(Cin, C) = 64: the bf16 MFMA
    (1, 64, 64, 4095, 1024, False),   # B * N one short
    (1, 63, 64, 4096, 1024, False),   # min(Cin, C) one short
    (2, 128, 64, 2048, 512, True),    # two clouds, Cin > C
])
def test_conv_before_gather_under_autocast(layer, B, Cin, C, N, M, bf16, monkeypatch):
    """LocalAggregationFused / GroupedConvBN under autocast against the fp64 layer under the contract: which route ran is
    asserted by the product's own bf16 entries (two: the forward product and the backward pair)"""
    from amcontrast3d_amd import ops
    K = 32
    idx, dp, f, w, gamma, beta = _lagg_case(B, Cin, C, N, M, K, 3 + Cin + N)
    calls = _spy_bf16(monkeypatch)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    mom = ops.group_moments(idx, dp, N)
    fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
    log = {}
    ops.pool_log(log)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if layer == "lagg":
                out = ops.LocalAggregationFused.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, bn)
            else:
                out = ops.GroupedConvBN.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, bn)
    finally:
        ops.pool_log(None)
    assert out.dtype == torch.float32
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    out.backward(go)
    assert calls.count(True) == (2 if bf16 else 0), calls
    arg = log[0] if layer == "lagg" else None
    want = _grouped_reference(idx, dp, f, w, gamma, beta, go, True, arg, rounded=bf16)
    plain = _grouped_reference(idx, dp, f, w, gamma, beta, go, True, arg, rounded=False) if bf16 else want
    print(f"{layer} B={B} Cin={Cin} C={C} N={N} bf16={bf16}")
    gt = 5e-5 if layer == "lagg" else 1e-4  # the gradient bounds of test_gpu_lagg.py for the two layers
    for name, got, tol in (("out", out, 2e-5), ("df", fr.grad, gt), ("dw", wr.grad, gt), ("dgamma", gr.grad, gt),
                           ("dbeta", br.grad, gt)):
        _check_grouped(name, got, want[name], plain[name], bf16, tol)
    if bf16:  # the column block of W_dp is plain fp32 arithmetic: fp32 bound
        _check_grouped("dw_dp", wr.grad.reshape(C, -1)[:, :3], want["dw"].reshape(C, -1)[:, :3], None, False, gt)
        # the forward sees the rounding: the unrounded layer is far outside the bound
        assert float((plain["out"] - want["out"]).abs().max()) > 10 * 2e-5 * max(1.0, float(want["out"].abs().max()))


def test_eval_routes_stay_fp32_under_autocast():
    """local_aggregation_eval, grouped_conv_bn_eval and bn_eval have no bf16 route: bit-identical with and without
    autocast at a shape where the training routes would take the bf16 MFMA"""
    from amcontrast3d_amd import ops
    idx, dp, f, w, gamma, beta = _lagg_case(1, 64, 64, 4096, 1024, 32, 41)
    bn = torch.nn.BatchNorm2d(64).to(DEV)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5); bn.weight.copy_(gamma); bn.bias.copy_(beta)
    bn.eval()
    x = torch.randn(1, 64, 1024, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    runs = (lambda: ops.local_aggregation_eval(f, dp, idx, w, bn, True),
            lambda: ops.grouped_conv_bn_eval(f, dp, idx, w, bn, True),
            lambda: ops.bn_eval(x, bn, True, False), lambda: ops.bn_eval(x, bn, True, True))
    for run in runs:
        plain = run()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = run()
        assert amp.dtype == torch.float32 and torch.equal(plain, amp)


@pytest.mark.parametrize("shape", [(8, 256, 256, (375,)), (4, 768, 256, (94,)), (2, 128, 192, (50, 32)),
                                   (8, 768, 256, (94,)), (8, 128, 192, (50, 32))])
def test_library_gemm_conv_bf16_contract(shape):
    """ops.LibraryGemmConv under autocast (the deep, short layers: SA4 and the coarse FeaturePropagation stages): bf16
    operands, fp32 accumulation, and fp32 results -- y, dx and each cloud's share of dW are not rounded to bf16"""
    from amcontrast3d_amd import ops
    B, ci, co, sp = shape
    g = torch.Generator().manual_seed(5 + B)
    x = torch.randn(B, ci, *sp, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(co, ci, *([1] * len(sp)), generator=g) * 0.05).to(DEV).requires_grad_(True)
    go = torch.randn(B, co, *sp, generator=g).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = ops.library_gemm_conv(x, w)
    y.backward(go)
    ref = _pw_reference(x.reshape(B, ci, -1), w.reshape(co, ci), None, go.reshape(B, co, -1))
    print(f"B={B} Cin={ci} Cout={co} spatial={sp}")
    _close("y", y.reshape(B, co, -1), ref["y"])
    _close("dx", x.grad.reshape(B, ci, -1), ref["dx"])
    _close("dw", w.grad.reshape(co, ci), ref["dw"])
