"""Deterministic mode (ops.deterministic / set_deterministic / deterministic_mode, cfg.deterministic): no kernel that adds
floats with atomics runs, and a train step has the same bits on every run.

Per kernel -- the three reverse-list gathers that stand in for the float-atomic scatters (amc3d_three_interpolate_grad_csr,
amc3d_local_aggregation_backward with lists, amc3d_masked_refine_backward_csr) -- the summation order of include/amc3d.h is restated
on the CPU: stable argsort of the targets, numpy float32 sequential adds from +0.0, the product rounded first; the kernel must
give those bits, and the same bits from a second call.  Against the atomic entry the bound is that of two orderings of one
fp32 sum of k terms, |a - b| <= 2 (k + 1) 2^-24 sum|terms| (each ordering is within (k - 1) 2^-24 sum|terms| of the exact sum
to first order; the product's own rounding, 2^-24 |term| per term, is common to both; the factor 2 (k + 1) covers the
second-order terms for every k used here), with sum|terms| in fp64 by index_add.

Whole step: three forward + backward runs from one state give torch.equal loss, logits and gradients, and the call counts show
the atomic entries at 0.  Captured: train_one_epoch with cfg.deterministic twice from one state gives equal state_dicts."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _ops():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import _lib, ops
    return ops, _lib, _lib.load()


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- interpolation ------------------------------------------------------------------------------------------------------
def _interp_reference(go, idx, w, m):
    """contract order on the CPU: per cloud, positions p = u*3 + j in stable order of their target, float32 adds from +0.0"""
    go, idx, w = go.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy()
    b, c, n = go.shape
    out = np.zeros((b, c, m), dtype=np.float32)
    for bs in range(b):
        tgt = idx[bs].reshape(-1)
        for p in np.argsort(tgt, kind="stable"):
            u = p // 3
            out[bs, :, tgt[p]] = out[bs, :, tgt[p]] + go[bs, :, u] * w[bs].reshape(-1)[p]  # float32 product, then float32 add
    return torch.from_numpy(out)


def _interp_case(b, c, m, n, seed, idx=None):
    g = torch.Generator().manual_seed(seed)
    if idx is None:
        idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32)
    w = torch.rand(b, n, 3, generator=g) + 0.05
    w = w / w.sum(2, keepdim=True)
    go = torch.randn(b, c, n, generator=g)
    return go.to(DEV), idx.to(DEV).contiguous(), w.to(DEV).contiguous()


def _interp_csr(go, idx, w, m, prefill=None):
    ops, _lib, lib = _ops()
    b, c, n = go.shape
    rs, re = ops.group_csr(idx, m)
    out = torch.full((b, c, m), float("nan") if prefill is None else prefill, device=DEV)
    _lib.check(lib.amc3d_three_interpolate_grad_csr(b, c, n, m, _p(go), _p(idx), _p(w), _p(rs), _p(re), _p(out), _stream()), "csr")
    return out


def _hand_made_idx():
    # the same index twice in a row of one point, and the same point in consecutive rows
    idx = torch.tensor([[[2, 2, 0], [2, 1, 2], [0, 0, 0], [3, 2, 2]]], dtype=torch.int32)
    return idx


@pytest.mark.parametrize("b,c,m,n,hand", [(2, 5, 7, 300, False), (1, 64, 3, 1, False), (2, 33, 200, 50, False), (1, 9, 5, 4, True)])
def test_interpolate_grad_csr_has_the_contract_bits(b, c, m, n, hand):
    ops, _lib, lib = _ops()
    ops.set_deterministic(False)
    go, idx, w = _interp_case(b, c, m, n, 3 + c, _hand_made_idx() if hand else None)
    got = _interp_csr(go, idx, w, m)  # output pre-filled with NaN: every element must be written
    want = _interp_reference(go, idx, w, m)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, _interp_csr(go, idx, w, m, prefill=7.0))
    # targets without an incoming position: exactly +0.0
    empty = torch.ones(b, m, dtype=torch.bool)
    for bs in range(b):
        empty[bs, idx[bs].reshape(-1).long().cpu()] = False
    z = got.cpu().permute(0, 2, 1)[empty]
    assert torch.equal(z, torch.zeros_like(z)) and not torch.signbit(z).any()
    if (b, c, m, n) == (2, 33, 200, 50):
        assert int(empty.sum()) > b * m // 3
    # the same function as the atomic entry
    atom = torch.zeros(b, c, m, device=DEV)
    _lib.check(lib.amc3d_three_interpolate_grad(b, c, n, m, _p(go), _p(idx), _p(w), _p(atom), None, 0, _stream()), "atomic")
    terms = (go.double().unsqueeze(-1) * w.double().unsqueeze(1)).abs().reshape(b, c, -1)  # (b, c, n*3)
    flat = idx.reshape(b, -1).long()
    sabs = torch.zeros(b, c, m, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(b, m, dtype=torch.float64, device=DEV)
    for bs in range(b):
        sabs[bs].index_add_(1, flat[bs], terms[bs])
        cnt[bs].index_add_(0, flat[bs], torch.ones_like(flat[bs], dtype=torch.float64))
    bound = 2 * (cnt.unsqueeze(1) + 1) * U * sabs
    assert bool(((got.double() - atom.double()).abs() <= bound).all())


def test_interpolate_backward_takes_the_list_route_only_in_the_mode():
    ops, _lib, lib = _ops()
    from amcontrast3d_amd import timing
    ops.set_deterministic(False)
    go, idx, w = _interp_case(2, 12, 40, 160, 1)
    f = torch.randn(2, 12, 40, device=DEV, requires_grad=True)
    base = torch.randn(2, 12, 160, device=DEV, requires_grad=True)
    want = _interp_reference(go, idx, w, 40)
    with ops.deterministic_mode():
        y1 = ops.three_interpolate(f, idx, w)
        y2 = ops.three_interpolate_add(f, idx, w, base)
        y3 = ops.three_interpolate(f, idx, w, ops.group_csr(idx, 40))  # lists from a plan
    with timing.count_calls() as c:  # backward OUTSIDE the block: the Functions honour the mode they were built under
        g1, = torch.autograd.grad(y1, f, go)
        g2, gb = torch.autograd.grad(y2, (f, base), go)
        g3, = torch.autograd.grad(y3, f, go)
    assert c["three_interpolate_grad"] == 0 and c["three_interpolate_grad_csr"] == 3 and c["group_csr"] == 2
    assert torch.equal(g1.cpu(), want) and torch.equal(g2.cpu(), want) and torch.equal(g3.cpu(), want) and torch.equal(gb, go)
    y = ops.three_interpolate(f, idx, w)  # default mode after leaving the context: the old entry again
    with ops.deterministic_mode(), timing.count_calls() as c:
        torch.autograd.grad(y, f, go)
    assert c["three_interpolate_grad"] == 1 and c["three_interpolate_grad_csr"] == 0


# ---- local aggregation --------------------------------------------------------------------------------------------------
def _lagg_case(C, K, M, relu, N=40, B=2, Cin=8, seed=0):
    """ball query with a radius small enough that most rows are padding repeats of their first hit; source point N-1 lies
    outside every ball"""
    ops, _lib, lib = _ops()
    g = torch.Generator().manual_seed(seed + C + K + M)
    p = torch.rand(B, N, 3, generator=g)
    p[:, N - 1] = 10.0
    p = p.to(DEV)
    q = p[:, :M].contiguous()
    radius = 0.3
    idx = ops.ball_query(radius, K, p, q)
    dp = ((ops.grouping_operation(p.transpose(1, 2).contiguous(), idx) - q.transpose(1, 2).unsqueeze(-1)) / radius).contiguous()
    f = torch.randn(B, Cin, N, generator=g).to(DEV)
    w = (torch.randn(C, Cin + 3, 1, 1, generator=g) * 0.3).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    gamma[::5] *= -1
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    go = torch.randn(B, C, M, generator=g).to(DEV)
    mom = ops.group_moments(idx, dp, N)
    pooled = ops.LocalAggregationFused.apply(f.requires_grad_(True), dp, idx, mom, w, gamma, beta, 1e-5, relu, None)
    return idx, go, pooled.grad_fn.saved_tensors


def _lagg_backward(saved, go, relu, csr):
    """the C entry the layer calls, atomic (csr None) or list form -> dg_cm, dw_dp (C,3), dgamma, dbeta, Q (B,N,C)"""
    ops, _lib, lib = _ops()
    f, w_f, w_dp, g_pm, idx, dp, moments, gamma, beta, mean, invstd, gd, ystar, arg, sums = saved
    B, Cin, N = f.shape
    _, M, K = idx.shape
    C = w_f.shape[0]
    ldw = w_dp.shape[1]
    dg = torch.full((B, C, N), float("nan"), device=DEV)
    dw = torch.zeros(C, ldw, device=DEV)
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    wb = int((lib.amc3d_local_aggregation_csr_workspace_bytes if csr else lib.amc3d_local_aggregation_workspace_bytes)(B, C, N, M))
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=DEV)  # (a NaN pattern where the kernels leave Q unwritten)
    head = (B, C, N, M, K, int(relu), _p(go), _p(ystar), _p(arg), _p(g_pm), _p(idx), _p(dp), _p(w_dp), ldw, _p(moments), _p(gd),
            _p(mean), _p(invstd), _p(gamma), _p(beta))
    tail = (_p(dg), _p(dw), ldw, _p(dgamma), _p(dbeta), 0, None, None, _p(work), wb, _stream())
    lists = (_p(csr[0]), _p(csr[1])) if csr else (None, None)
    _lib.check(lib.amc3d_local_aggregation_backward(*head, *lists, *tail), "lagg csr" if csr else "lagg atomic")
    off = int(lib.amc3d_local_aggregation_workspace_q_offset(B, C, N, M))
    Q = work[off:off + 4 * B * N * C].view(torch.float32).view(B, N, C).clone()
    return dg, dw[:, :3].clone(), dgamma, dbeta, Q


def _lagg_dq(saved, go, relu):
    """the ReLU-masked pooled gradient exactly as lagg_bwd_scatter_kernel forms it (fp32, unfused)"""
    f, w_f, w_dp, g_pm, idx, dp, moments, gamma, beta, mean, invstd, gd, ystar, arg, sums = saved
    y, d = ystar.cpu(), go.cpu().clone()
    if relu:
        xh = (y - mean.cpu()[None, :, None]) * invstd.cpu()[None, :, None]
        d[~((xh * gamma.cpu()[None, :, None] + beta.cpu()[None, :, None]) > 0)] = 0.0
    return d


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M", [1, 24, 37])       # 37: not a multiple of the kernel's 32-centroid tile, two tiles
@pytest.mark.parametrize("C,K", [(8, 32), (8, 20), (128, 32), (128, 20), (256, 32), (256, 20)])
def test_local_aggregation_backward_csr_has_the_contract_bits(C, K, M, relu):
    ops, _lib, lib = _ops()
    ops.set_deterministic(False)
    idx, go, saved = _lagg_case(C, K, M, relu)
    B, N = idx.shape[0], 40
    flat = idx.reshape(B, -1).cpu().numpy()
    assert not (flat == N - 1).any()                                 # a source point outside every ball
    if M > 1:
        assert float((idx[:, :, 1:] == idx[:, :, :1]).float().mean()) > 0.5  # most of a row: padding repeats of the first hit
    csr = ops.group_csr(idx, N)
    dg, dw, dgam, dbet, Q = _lagg_backward(saved, go, relu, csr)
    # Q in the contract order: positions ascending per target, only the position that equals arg carries the gradient
    dq, arg = _lagg_dq(saved, go, relu).numpy(), saved[13].cpu().numpy()
    want = np.zeros((B, N, C), dtype=np.float32)
    for b in range(B):
        for p in np.argsort(flat[b], kind="stable"):
            m, k = divmod(int(p), K)
            hit = arg[b, :, m] == k
            want[b, flat[b, p], hit] = want[b, flat[b, p], hit] + dq[b, hit, m]
    assert torch.equal(Q.cpu(), torch.from_numpy(want))
    assert not torch.signbit(Q[:, N - 1]).any() and not Q[:, N - 1].any()  # no incoming position: exactly +0.0
    again = _lagg_backward(saved, go, relu, csr)
    for a, b_ in zip((dg, dw, dgam, dbet, Q), again):
        assert torch.equal(a, b_)
    assert not torch.isnan(dg).any()
    # the same function as the atomic entry: the partial sums do not involve Q at all -> equal bits
    dg0, dw0, dgam0, dbet0, Q0 = _lagg_backward(saved, go, relu, None)
    assert torch.equal(dw, dw0) and torch.equal(dgam, dgam0) and torch.equal(dbet, dbet0)
    d64 = torch.from_numpy(dq).double()
    sabs = torch.zeros(B, N, C, dtype=torch.float64)
    cnt = torch.zeros(B, N, C, dtype=torch.float64)
    a_t, f_t = torch.from_numpy(arg.astype(np.int64)), torch.from_numpy(flat.astype(np.int64))
    for b in range(B):
        m_of, k_of = torch.arange(M * K) // K, torch.arange(M * K) % K
        hit = (a_t[b][:, m_of] == k_of[None, :]).double()            # (C, M*K)
        sabs[b].index_add_(0, f_t[b], (hit * d64[b][:, m_of].abs()).t())
        cnt[b].index_add_(0, f_t[b], hit.t())
    bound = 2 * (cnt + 1) * U * sabs
    assert bool(((Q.cpu().double() - Q0.cpu().double()).abs() <= bound).all())
    # dg_cm comes from Q through the unchanged apply kernel, element by element: wherever Q has the same bits, so has dg_cm
    same = (Q == Q0).permute(0, 2, 1)
    assert torch.equal(dg[same], dg0[same])


def test_local_aggregation_layer_takes_the_list_route_in_the_mode():
    ops, _lib, lib = _ops()
    from amcontrast3d_amd import timing
    ops.set_deterministic(False)
    idx, go, saved = _lagg_case(128, 32, 24, True)
    f, w_f, w_dp, g_pm, idx, dp, moments, gamma, beta = saved[:9]
    w = w_dp.reshape(128, -1, 1, 1)
    res = []
    for csr in (None, ops.group_csr(idx, 40)):
        for _ in range(2):
            fr, wr, gr, br = (t.detach().clone().requires_grad_(True) for t in (f, w, gamma, beta))
            with ops.deterministic_mode():
                y = ops.LocalAggregationFused.apply(fr, dp, idx, moments, wr, gr, br, 1e-5, True, None, None, csr)
            with timing.count_calls() as c:
                y.backward(go)
            assert c["local_aggregation_backward"] == 0 and c["local_aggregation_backward_csr"] == 1
            assert c["group_csr"] == (1 if csr is None else 0)
            res.append([t.grad.clone() for t in (fr, wr, gr, br)])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


# ---- refinement ---------------------------------------------------------------------------------------------------------
def _refine_reference(dout, best, mask, gamma):
    B, D, n = dout.shape
    d = dout.cpu().numpy().reshape(-1)
    best, mask = best.cpu().numpy(), mask.cpu().numpy()
    g32 = np.float32(gamma)
    omg = np.float32(1.0 - float(g32))  # (float)(1.0 - (double)gamma) of the C entry
    t = np.arange(B * D * n)
    bn = (t // n // D) * n + t % n
    msk = mask[bn] != 0
    direct = (g32 * d) * np.where(msk, np.float32(0), np.float32(1)) + omg * d
    s = np.zeros(B * n * D, dtype=np.float32)
    for r in np.argsort(best, kind="stable"):  # rows in stable order of their target
        src = r * D + np.arange(D)
        hit = msk[src]
        dst = best[r] * D + np.arange(D)
        s[dst[hit]] = s[dst[hit]] + g32 * d[src[hit]]
    return torch.from_numpy((direct + s).astype(np.float32).reshape(B, D, n))


@pytest.mark.parametrize("case", ["same_all_true", "same_all_false", "random"])
def test_masked_refine_backward_csr_has_the_contract_bits(case):
    ops, _lib, lib = _ops()
    from amcontrast3d_amd import timing
    ops.set_deterministic(False)
    B, D, n, k = 2, 6, 50, 11
    g = torch.Generator().manual_seed(5)
    f = torch.randn(B, D, n, generator=g).to(DEV)
    dout = torch.randn(B, D, n, generator=g).to(DEV)
    nbr = torch.randint(0, B * n, (B * n, k), generator=g, dtype=torch.int32)
    a = torch.rand(B * n, generator=g) * 0.5 + 0.25
    gamma = 0.7
    if case.startswith("same"):
        nbr[:, 4] = 13      # every row lists row 13, whose ambiguity is the smallest: every row picks it
        a[13] = 0.01
    thr, thr_max = {"same_all_true": (0.0, 1.0), "same_all_false": (2.0, 3.0), "random": (0.5, 1.0)}[case]
    nbr, a = nbr.to(DEV), a.to(DEV)
    fr = f.clone().requires_grad_(True)
    with ops.deterministic_mode():
        out, _ = ops.MaskedRefineDual.apply(fr, a, nbr, thr, thr_max, gamma)
    best, mask = out.grad_fn.saved_tensors
    if case.startswith("same"):
        assert bool((best == 13).all()) and bool((mask == (1 if case == "same_all_true" else 0)).all())
    with timing.count_calls() as c:
        got, = torch.autograd.grad(out, fr, dout, retain_graph=True)
    assert c["masked_refine_backward"] == 0 and c["masked_refine_backward_csr"] == 1
    assert torch.equal(got.cpu(), _refine_reference(dout, best, mask, gamma))
    again, = torch.autograd.grad(out, fr, dout)
    assert torch.equal(got, again)
    # the same function as the atomic entry (default mode)
    fr0 = f.clone().requires_grad_(True)
    out0, _ = ops.MaskedRefineDual.apply(fr0, a, nbr, thr, thr_max, gamma)
    with timing.count_calls() as c:
        atom, = torch.autograd.grad(out0, fr0, dout)
    assert c["masked_refine_backward"] == 1 and c["masked_refine_backward_csr"] == 0
    t = torch.arange(B * D * n, device=DEV)
    msk = mask[(t // n // D) * n + t % n].bool()
    d = dout.reshape(-1).double()
    terms = ((gamma * d).abs() * msk).view(B * n, D)
    sabs = torch.zeros(B * n, D, dtype=torch.float64, device=DEV).index_add_(0, best.long(), terms)
    cnt = torch.zeros(B * n, D, dtype=torch.float64, device=DEV).index_add_(0, best.long(), msk.view(B * n, D).double())
    sabs = sabs + d.abs().view(B * n, D)  # the element's direct term
    bound = (2 * (cnt + 2) * U * sabs).view(B, D, n)
    assert bool(((got.double() - atom.double()).abs() <= bound).all())


# ---- whole step ---------------------------------------------------------------------------------------------------------
def _build(kind):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import configs
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(0)
    c = EasyConfig()
    if kind == "S":
        c.update(configs.model_cfg("S", dropout=0, width=16))
    elif kind == "L":  # L-shaped: single-layer SetAbstraction and one InvResMLP block in every stage
        c.update(configs.model_cfg("L", dropout=0, width=16, blocks=[1, 2, 2, 2, 2]))
    else:              # AMContrast3D++ as shipped (XL: blocks [1,4,7,4,4], sa_layers 1) with prediction and refinement
        c.update(configs.model_cfg_mm(dropout=0, width=16, threshold=0.5))
    model = build_model_from_cfg(c).to(DEV).train()
    cc = EasyConfig()
    cc.update(configs.criterion_cfg_mm() if kind == "MM" else configs.criterion_cfg())
    crit = build_criterion_from_cfg(cc).to(DEV)
    aa = EasyConfig()
    aa.update(configs.ambiguity_args_mm("s3dis") if kind == "MM" else configs.ambiguity_args("s3dis"))
    return model, crit, aa


def _batch(b, n, first_id):
    from amcontrast3d_amd import synthetic
    nb = synthetic.make_batch(b, n, first_id=first_id)
    return {k: torch.from_numpy(v).to(DEV) for k, v in nb.items()}


def _step(model, crit, aa, data, mm):
    model.zero_grad(set_to_none=True)
    if mm:
        logits, stage, rate = model(data)
        seg, ce, am, reg = crit(logits, data["y"], stage, 13, None, aa)
        loss = seg + reg
    else:
        logits, stage = model(data)
        loss = crit(logits, data["y"], stage, 13, None, aa)
    loss.backward()
    return loss.detach().clone(), logits.detach().clone(), [None if p.grad is None else p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("kind", ["S", "L", "MM"])
def test_a_train_step_has_the_same_bits_on_every_run(kind):
    ops, _lib, lib = _ops()
    from amcontrast3d_amd import timing
    ops.set_deterministic(False)
    model, crit, aa = _build(kind)
    state = copy.deepcopy(model.state_dict())
    data = _batch(2, 2048, 60)
    runs, counts = [], []
    with ops.deterministic_mode():
        for _ in range(3):
            model.load_state_dict(state)
            with timing.count_calls() as c:
                runs.append(_step(model, crit, aa, dict(data), kind == "MM"))
            counts.append(dict(c))
    for loss, logits, grads in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(logits, runs[0][1])
        for a, b in zip(grads, runs[0][2]):
            assert (a is None and b is None) or torch.equal(a, b)
    assert sum(g is not None for g in runs[0][2]) > 10 and bool(torch.isfinite(runs[0][0]))
    c = counts[0]
    assert counts[1] == c and counts[2] == c
    for old in ("three_interpolate_grad", "local_aggregation_backward", "masked_refine_backward", "grouped_conv_backward",
                "group_points_grad", "library_gemm_conv"):
        assert c.get(old, 0) == 0, (old, c)
    assert c["three_interpolate_grad_csr"] == 4                                    # the four decoder levels
    # every LocalAggregation and single-layer SetAbstraction: none in S (two-layer SetAbstractions, no InvResMLP block), one of
    # each per stage in the L shape, 4 + (3 + 6 + 3 + 3) in the XL shape of the MM model
    n_lagg = c.get("local_aggregation_forward", 0)
    assert c.get("local_aggregation_backward_csr", 0) == n_lagg == {"S": 0, "L": 8, "MM": 19}[kind]
    assert c.get("grouped_conv_bn_backward", 0) == c.get("grouped_conv_bn_forward", 0) == {"S": 4, "L": 0, "MM": 0}[kind]
    if kind == "MM":
        assert c["masked_refine_backward_csr"] == c["masked_refine_forward"] > 0
    # default mode after leaving the context calls the old entries again
    with timing.count_calls() as c0:
        _step(model, crit, aa, dict(data), kind == "MM")
    assert c0["three_interpolate_grad"] == 4 and c0["three_interpolate_grad_csr"] == 0
    assert c0.get("local_aggregation_backward", 0) == n_lagg and c0.get("local_aggregation_backward_csr", 0) == 0
    if kind == "MM":
        assert c0["masked_refine_backward"] > 0 and c0.get("masked_refine_backward_csr", 0) == 0


# ---- captured -----------------------------------------------------------------------------------------------------------
def test_captured_epochs_with_cfg_deterministic_end_in_the_same_state():
    ops, _lib, lib = _ops()
    from amcontrast3d_amd import configs, train
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    ops.set_deterministic(False)
    model, crit, aa = _build("S")
    cfg = EasyConfig()
    cfg.update({"num_classes": 13, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
                "ambiguity_args": aa, "grad_norm_clip": 10, "sched_on_epoch": False, "fps_lanes": 2, "deterministic": True})

    class Sched:
        def step(self, epoch):
            pass

    def loader():
        out = []
        for k in range(4):
            d = _batch(2, 2048, 80 + 2 * k)  # resident batches
            out.append({"pos": d["pos"].clone(), "y": d["y"].clone(), "x": d["x"][:, :3].transpose(1, 2).contiguous(),
                        "heights": d["x"][:, 3:4].transpose(1, 2).contiguous()})
        return out

    m0 = copy.deepcopy(model.state_dict())
    ends = []
    try:
        for _ in range(2):
            model.load_state_dict(m0)
            opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=1e-4)  # a fresh optimizer state
            torch.manual_seed(1)
            train.train_one_epoch(model, loader(), crit, opt, Sched(), None, 1, cfg)
            first = copy.deepcopy(model.state_dict())
            train.train_one_epoch(model, loader(), crit, opt, Sched(), None, 2, cfg)  # second epoch on the cached pipeline
            torch.cuda.synchronize()
            ends.append((first, copy.deepcopy(model.state_dict())))
            assert not ops.deterministic()  # the mode lasts for the epoch only
            assert len(train._PIPELINES) == 1 and all(k[-1] is True for k in train._PIPELINES)  # one pipeline, keyed by the mode
            train.release_pipelines()
        for a, b in zip(ends[0], ends[1]):
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]), k
        moved = max(float((ends[0][1][k].float() - m0[k].float()).abs().max()) for k in m0)
        assert moved > 0
    finally:
        train.release_pipelines()


# ---- contract -----------------------------------------------------------------------------------------------------------
def test_an_operator_without_a_deterministic_route_raises():
    ops, _lib, lib = _ops()
    ops.set_deterministic(False)
    f = torch.randn(2, 4, 30, device=DEV, requires_grad=True)
    idx = torch.randint(0, 30, (2, 10, 8), dtype=torch.int32, device=DEV)
    with ops.deterministic_mode():
        y = ops.grouping_operation(f, idx)
    with pytest.raises(RuntimeError, match=r"group_points_grad: no deterministic route"):
        y.sum().backward()
    y = ops.grouping_operation(f, idx)  # default mode: the scatter runs
    y.sum().backward()
    assert f.grad is not None
    # gather_points_grad: one atomic per address is deterministic -> allowed with unique picks, refused with repeats
    for picks, ok in ((torch.tensor([[3, 1, 7], [0, 2, 9]]), True), (torch.tensor([[3, 3, 7], [0, 2, 9]]), False)):
        f2 = torch.randn(2, 4, 30, device=DEV, requires_grad=True)
        with ops.deterministic_mode():
            y = ops.gather_operation(f2, picks.to(torch.int32).to(DEV))
        if ok:
            y.sum().backward()
        else:
            with pytest.raises(RuntimeError, match=r"gather_points_grad: no deterministic route"):
                y.sum().backward()
