"""The reverse-list collapse of GroupedConvBN's backward (csrc/csr.hip, csr_collapse) where a lane group owns SEVERAL source
points: per = 3 .. 17 instead of the 1 of every other test that looks at this pass on its own.  `per` depends on B * n alone, so
the clouds of csr_group_cases.py have very many source points and a few thousand hand-placed edges (what they hold is asserted
on the CPU by test_csr_group_cases_host.py): lane groups that walk from list to list and over empty ones, that hold the
boundary between two clouds, a last workgroup with fewer points than its lane groups could take and no edge, and the sizes that reach
csr_collapse_shfl_kernel<8|16|32> (per > 16) and fill the stream kernel's s_gv (per == 16).

Per case: the route (the library's own count of partial records), the reverse lists at key widths up to 22 bits, the three
backward forms against each other (atomics; lists: the plain gather loop; lists with records: the pipelined stream / shuffle
kernels -- the same bits as the gather loop), and all of it against grouping + cat + Conv2d + BatchNorm2d (batch statistics)
[+ ReLU] evaluated by torch in fp64, whole tensors and, row by row, the points of the lane groups named above.
Bounds: those of test_gpu_lagg.py (its lists have 30-200 edges, these at most 256)."""
import ctypes

import numpy as np
import pytest
import torch

import csr_group_cases as CG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, CIN, EPS = CG.K, 8, 1e-5
RUNS = [(c, True) for c in CG.CASES] + [(c, False) for c in CG.CASES if c.relu_off]


def _lists_partials(B, C, n, M):
    from amcontrast3d_amd import _lib
    c = (ctypes.c_int * 4)()
    _lib.check(_lib.load().amc3d_local_aggregation_partial_counts(B, C, n, M, K, c), "partial counts")
    return c[3]


def _inputs(case):
    B, n, C, M = case.B, case.n, case.C, case.M
    idx, dp = CG.build(B, n, C, M, seed=0)
    g = torch.Generator().manual_seed(1000 * case.per + C)
    f = torch.randn(B, CIN, n, generator=g).to(DEV)
    w = (torch.randn(C, CIN + 3, 1, 1, generator=g) * 0.3).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    gamma[::5] *= -1  # negative scale factors too
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    go = torch.randn(B, C, M, K, generator=g).to(DEV)
    return idx, torch.from_numpy(idx).to(DEV), torch.from_numpy(dp).to(DEV), f, w, gamma, beta, go


def _reference(idx, dp, f, w, gamma, beta, go, relu, x1):
    """the layer in fp64; behind a ReLU the backward routes by the kernel's own x1 > 0 (one pre-activation within rounding of
    zero must not decide the test: what that mask may differ in is asserted apart)"""
    B, _, n = f.shape
    _, M, _ = idx.shape
    f64, w64, g64, b64 = (t.double().requires_grad_(True) for t in (f, w, gamma, beta))
    fj = f64.gather(2, idx.reshape(B, 1, -1).expand(-1, CIN, -1).long()).reshape(B, CIN, M, K)
    y = torch.nn.functional.conv2d(torch.cat([dp.double(), fj], 1), w64)
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    z = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS) * g64[None, :, None, None] + b64[None, :, None, None]
    out = z * (x1 > 0) if relu else z
    out.backward(go.double())
    z = z.detach()
    return {"x1": torch.relu(z) if relu else z, "z": z, "grads": [f64.grad, w64.grad, g64.grad, b64.grad]}


@pytest.mark.parametrize("case,relu", RUNS, ids=[f"{c.tag}-{'relu' if r else 'linear'}" for c, r in RUNS])
def test_collapse_with_several_points_per_group(case, relu):
    from amcontrast3d_amd import ops, timing
    B, n, C, M = case.B, case.n, case.C, case.M
    G, P = B * n, M * K
    groups, per, parts = CG.plan(B, n, C)
    assert per == case.per > 1
    # the route: the library's own csr_partials() -- other constants there and this file no longer tests what it says
    assert _lists_partials(B, C, n, M) == parts == case.parts
    idx_np, idx, dp, f, w, gamma, beta, go = _inputs(case)
    d = CG.describe(idx_np, B, n, C)

    # ---- the reverse lists at this size (radix sort over csr_bits(G) bits of the key)
    start, edge = ops.group_csr(idx, n)
    s, e = start.cpu().numpy().astype(np.int64), edge.cpu().numpy().astype(np.int64)
    assert s.shape == (G + 1,) and s[0] == 0 and s[-1] == B * P and np.all(np.diff(s) >= 0)
    deg = np.diff(s)
    assert np.array_equal(deg, d["deg"])
    owner = np.repeat(np.arange(G), deg)  # the source point of every edge
    cloud = owner // n
    assert np.array_equal(cloud, np.arange(B * P) // P)
    for b in range(B):
        assert np.array_equal(np.sort(e[b * P:(b + 1) * P]), np.arange(P))  # every position of the cloud exactly once
    assert np.array_equal(idx_np.reshape(-1)[cloud * P + e], owner - cloud * n)  # under its target
    assert np.all(np.diff(e)[owner[1:] == owner[:-1]] > 0)  # every list ascending
    m_csr = ops.group_moments_csr(idx, dp, n, (start, edge)).cpu().numpy()
    assert np.array_equal(m_csr[128:128 + 4 * G].view(np.int32), d["deg"])
    edge_dp = ops.group_csr_dp(idx, dp, edge)

    # ---- the three backward forms
    mom = ops.group_moments(idx, dp, n)

    def run(csr, grad):
        leaves = [t.clone().requires_grad_(True) for t in (f, w, gamma, beta)]
        x1 = ops.GroupedConvBN.apply(leaves[0], dp, idx, mom, *leaves[1:], EPS, relu, None, csr)
        with timing.count_calls() as calls:
            x1.backward(grad)
        return x1.detach(), [t.grad for t in leaves], dict(calls)

    x1, g_atomic, _ = run(None, go)
    x1_l, g_lists, _ = run((start, edge), go)
    x1_r, g_records, _ = run((start, edge, edge_dp), go)
    _, g_again, _ = run((start, edge, edge_dp), go)
    names = ("df", "dw", "dgamma", "dbeta")
    figures = []  # (what, error, bound)
    assert torch.equal(x1, x1_l) and torch.equal(x1, x1_r)
    for name, a, b_, c in zip(names, g_lists, g_records, g_again):
        figures.append((f"{name}: gather loop vs {CG.kernel(B, n, C, True)}, differing elements", int((a != b_).sum()), 0))
        figures.append((f"{name}: second run of the record form, differing elements", int((b_ != c).sum()), 0))
    for name, a, b_ in zip(names, g_atomic, g_records):
        figures.append((f"{name}: atomics vs lists", float((a - b_).abs().max()), 2e-5 * max(1.0, float(a.abs().max()))))
    if case.position_major and relu:  # a gradient that arrives as position-major rows is read in place: the same bits
        go_pm = go.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not go_pm.is_contiguous() and torch.equal(go_pm, go)
        for form, csr in (("lists", (start, edge)), ("records", (start, edge, edge_dp))):
            _, g_pm, calls = run(csr, go_pm)
            assert calls == {"grouped_conv_bn_backward": 1, "pointwise_conv_backward": 1}, calls  # lists given, none built
            for name, a, b_ in zip(names, g_lists, g_pm):
                figures.append((f"{name}: position-major gradient, {form}, differing elements", int((a != b_).sum()), 0))

    # ---- fp64
    ref = _reference(idx, dp, f, w, gamma, beta, go, relu, x1)
    fwd_bound = 2e-5 * max(1.0, float(ref["x1"].abs().max()))
    figures.append(("x1", float((x1.double() - ref["x1"]).abs().max()), fwd_bound))
    if relu:
        differ = (x1 > 0) != (ref["z"] > 0)
        figures.append((f"|fp64 pre-activation| where the kernel's ReLU mask differs ({int(differ.sum())} places)",
                        float(ref["z"][differ].abs().max()) if bool(differ.any()) else 0.0, fwd_bound))
    for name, got, want in zip(names, g_records, ref["grads"]):
        figures.append((f"{name} vs fp64 (|want| max {float(want.abs().max()):.3g})", float((got.double() - want).abs().max()),
                        1e-4 * max(1.0, float(want.abs().max()))))
    # df row by row: a wrong row in a group is nothing in a maximum over 10^5 .. 10^6 rows
    want_rows = ref["grads"][0].transpose(1, 2).reshape(G, CIN)
    empty = torch.from_numpy(d["deg"] == 0).to(DEV)
    for form, grads in (("atomics", g_atomic), ("lists", g_lists), ("records", g_records)):
        rows = grads[0].transpose(1, 2).reshape(G, CIN)
        figures.append((f"df rows of points with an empty list, {form}", float(rows[empty].abs().max()), 0.0))
        for what in ("pts_straddle", "pts_interior", "pts_last2"):
            pts = torch.from_numpy(d[what]).to(DEV)
            assert len(pts) and int((~empty[pts]).sum()) > 0, what
            top = float(want_rows[pts].abs().max())
            figures.append((f"df rows, {what[4:]} ({len(pts)} points, |want| max {top:.3g}), {form}",
                            float((rows[pts].double() - want_rows[pts]).abs().max()), 1e-4 * max(1.0, top)))
    print(f"\n{case.tag} relu={relu}: per {per}, {parts} workgroups, {CG.kernel(B, n, C, True)}")
    for what, err, bound in figures:
        print(f"    {what}: {err:.3g} (bound {bound:.3g})")
    missed = [(what, err, bound) for what, err, bound in figures if not err <= bound]
    assert not missed, missed
