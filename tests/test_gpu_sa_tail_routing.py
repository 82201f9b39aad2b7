"""Where the SetAbstraction tail (csrc/sa_tail.hip) sends the pooled gradient: negative and zero BatchNorm scales, exact ties among
the 32 neighbours, the algebraic and the recomputing backward held against each other, and one case per row of the shape dispatch.

The arbiter is the layer-by-layer torch composition of tests/test_gpu_sa_tail.py (`reference`) in fp64; `_layerwise` below is that
composition with the intermediate tensors handed out (and is held bit-equal to `reference` where both apply).  Parts A-C feed
inputs on a grid on which z = W2 . x1 is exact in fp32 in any summation order, so the winning neighbour is the same in the kernel,
in torch fp32 and in torch fp64 and gradients can be compared element by element."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from test_gpu_sa_tail import reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
NAN = float("nan")


# ---- the dispatch of csrc/sa_tail.hip, restated.  The library exports only sat_supported (held against it below); the rest of the
# table is documentation, kept in step with sa_tail.hip by hand: whoever changes the dispatch there moves the row here ------------
def sat_supported(C1, C2, K=32):
    return K == 32 and 2 <= C1 <= 64 and C1 % 2 == 0 and 1 <= C2 <= 128


def sat_alg_supported(C1, C2):
    return (C1 % 4 == 0 and C2 % 4 == 0 and 256 % C2 == 0 and C2 <= 128 and (C1 * C2) % 256 == 0 and C1 % (256 // C2) == 0
            and (C1 * C2) // 256 <= 32)


def dispatch(C1, C2):
    """(backward form with zext given, NCT, NIT, WR, FULL, position-major dx1 from ops.SATailActivated)"""
    alg = sat_alg_supported(C1, C2)
    nit = 2 if C1 > 32 else 1
    return ("algebraic" if alg else "recompute", (C2 + 31) // 32, nit, C1 * C2 // 256 if alg else None,
            alg and C1 == 32 * nit and C2 % 16 == 0, C1 % 4 == 0)


# C1, C2, B, M   form         NCT NIT WR    FULL   PM      what the row is there for
DISPATCH = [
    (2, 1, 1, 1, "recompute", 1, 1, None, False, False),   # smallest supported; odd C2; less than one 4-centroid tile
    (6, 33, 2, 3, "recompute", 2, 1, None, False, False),  # ragged second channel tile, odd C2, C1 % 8 != 0 (two-step z loop)
    (20, 32, 1, 33, "recompute", 1, 1, None, False, True),  # C1 * C2 % 256 != 0 with position-major dx1; one past 8 tiles
    (16, 16, 3, 3, "algebraic", 1, 1, 1, False, True),     # WR = 1: C2 / 4 = 4 channels x 16 chunks per wave
    (32, 8, 2, 65, "algebraic", 1, 1, 1, False, True),     # WR = 1: 2 x 32; one past sat_pool_grad_kernel's 64 centroids
    (64, 4, 1, 33, "algebraic", 1, 2, 1, False, True),     # WR = 1: 1 x 64; NIT = 2
    (12, 64, 2, 3, "algebraic", 2, 1, 3, False, True),     # WR = 3: not a power of two, NIT = 1
    (32, 64, 2, 130, "algebraic", 2, 1, 8, True, True),    # the benchmarked SA1 layer
    (48, 64, 1, 65, "algebraic", 2, 2, 12, False, True),   # NIT = 2 with C1 ragged in the second tile; WR = 12
    (64, 128, 2, 33, "algebraic", 4, 2, 32, True, True),   # WR at its cap
    (64, 96, 1, 65, "recompute", 3, 2, None, False, True),  # 256 % 96 != 0
    (34, 128, 3, 1, "recompute", 4, 2, None, False, False),  # NCT = 4; C1 ragged in its second 32-channel tile
]
SHAPES = [row[:4] for row in DISPATCH]


def test_dispatch_table_and_supported_shapes():
    from amcontrast3d_amd import ops
    for C1, C2, B, M, *want in DISPATCH:
        assert tuple(want) == dispatch(C1, C2), (C1, C2, dispatch(C1, C2))
        assert sat_supported(C1, C2) and ops.sa_tail_supported(C1, C2, 32), (C1, C2)
        assert 1 <= B <= 3 and M <= 130
    assert {m for _, _, _, m in SHAPES} == {1, 3, 33, 65, 130}
    assert not ops.sa_tail_supported(3, 8, 32)
    assert not ops.sa_tail_supported(66, 8, 32)
    assert not ops.sa_tail_supported(32, 129, 32)
    assert not ops.sa_tail_supported(32, 64, 16)
    for c1 in range(0, 70):  # the restated predicate is the library's
        for c2 in (0, 1, 33, 128, 129):
            assert sat_supported(c1, c2) == ops.sa_tail_supported(c1, c2, 32), (c1, c2)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _add_ties(t):
    """exact ties among the 32 neighbours of (B, C, M, 32), the way ball query produces them and where the kernel's three
    copies of the first-index rule meet.  A lane's 16 registers hold neighbours (r & 3) + 8 (r >> 2) + 4 kh: 0-3, 8-11, 16-19,
    24-27 sit in half kh = 0, the others in half kh = 1"""
    M = t.shape[2]
    even = torch.arange(M) % 2 == 0
    t[:, :, even, 4] = t[:, :, even, 3]      # adjacent indices, different halves
    t[:, :, even, 12] = t[:, :, even, 11]
    t[:, :, even, 17] = t[:, :, even, 10]    # both in half 0 (in-lane comparison, not at register 0)
    t[:, :, even, 13] = t[:, :, even, 5]     # both in half 1
    t[..., 7] = t[..., 3]                    # everywhere
    pad = torch.arange(M) % 3 == 0           # a short neighbourhood: ball query repeats the first hit
    t[:, :, pad, 20:32] = t[:, :, pad, 0:1]
    return t


def _scales(C2, variant, g):
    """|gamma2| in [0.5, 1.5], every third channel negative, and zero scales: +0.0 with beta2 > 0, -0.0, +0.0 with beta2 < 0
    (as many of the three as C2 has room for; `variant` rotates which come first)"""
    g2 = torch.rand(C2, generator=g) + 0.5
    g2[2::3] *= -1
    b2 = torch.randn(C2, generator=g) * 0.2
    special = [(0.0, 0.3), (-0.0, None), (0.0, -0.3)]
    special = special[variant % 3:] + special[:variant % 3]
    slots = (1, 4, 6) if C2 >= 7 else (1, 3) if C2 >= 4 else ()
    for s, (gv, bv) in zip(slots, special):
        g2[s] = gv
        if bv is not None:
            b2[s] = bv
    if C2 == 1:
        if variant % 2:
            g2[0], b2[0] = 0.0, 0.3
        else:
            g2[0] = -g2[0].abs()
    return g2, b2


def _layerwise(x, bn1, w2, g2, b2, relu2, gout, dtype):
    """test_gpu_sa_tail.reference, from x1 when bn1 is None, keeping the raw and the normalised values"""
    leaf = lambda t: t.detach().to(dtype, copy=True).requires_grad_(True)  # (never the caller's tensor: .to(float32) would be)
    xin, ps = leaf(x), [leaf(t) for t in (w2, g2, b2)]
    h, p1 = xin, []
    if bn1 is not None:
        p1 = [leaf(t) for t in bn1]
        h = F.relu(F.batch_norm(h, None, None, p1[0], p1[1], True, 0.1, EPS))
    zraw = F.conv2d(h, ps[0])
    zn = F.batch_norm(zraw, None, None, ps[1], ps[2], True, 0.1, EPS)
    post = F.relu(zn) if relu2 else zn
    out, idx = post.max(-1)
    out.backward(gout.to(dtype))
    assert torch.equal(idx, post.argmax(-1))  # the gradient went to the first maximal index
    return SimpleNamespace(out=out.detach(), dx=xin.grad, dw2=ps[0].grad, dg2=ps[1].grad, db2=ps[2].grad,
                           d1=[p.grad for p in p1], zraw=zraw.detach(), zn=zn.detach(), arg=idx, carry=(out.detach() > 0) if relu2 else
                           torch.ones_like(out, dtype=torch.bool))


def _next_distinct_gap(zn):
    """per (b, c2, centroid): the winning normalised value minus the next distinct one (inf when all 32 are equal)"""
    top = zn.max(-1, keepdim=True)[0]
    return top.squeeze(-1) - zn.masked_fill(zn >= top, -math.inf).max(-1)[0]


@functools.lru_cache(maxsize=None)
def _grid_case(C1, C2, B, M, relu2):
    """x1: multiples of 1/4 in [0, 2], about half of them zero; w2: multiples of 1/8 in [-1, 1].  Products are multiples of 1/32
    and |z| <= 128: 17 significant bits at most, exact in fp32 however the sum is ordered"""
    g = torch.Generator().manual_seed(1000 * C1 + 10 * C2 + M)
    x1 = torch.randint(0, 9, (B, C1, M, 32), generator=g).float() / 4
    x1 = _add_ties(x1 * (torch.rand(B, C1, M, 32, generator=g) < 0.5))
    w2 = torch.randint(-8, 9, (C2, C1, 1, 1), generator=g).float() / 8
    g2, b2 = _scales(C2, int(relu2), g)
    gout = torch.randn(B, C2, M, generator=g)
    r64 = _layerwise(x1, None, w2, g2, b2, relu2, gout, torch.float64)
    r32 = _layerwise(x1, None, w2, g2, b2, relu2, gout, torch.float32)
    c = SimpleNamespace(x1=x1, w2=w2, g2=g2, b2=b2, gout=gout, r64=r64, r32=r32, zero=(g2 == 0).nonzero().flatten().tolist())
    # -- the routing is decided on the reference alone: two raw values are bit-equal or >= 1/32 apart and every nonzero
    #    |gamma2| >= 0.5, so distinct normalised values of a triple are >= (1/32) * invstd * 0.5 apart, no triple left out
    assert torch.equal(r32.zraw.double(), r64.zraw) and torch.equal(r32.arg, r64.arg)
    nz = g2 != 0
    assert bool((g2[nz].abs() >= 0.5).all())
    invstd = (r64.zraw.var((0, 2, 3), unbiased=False) + EPS).rsqrt()
    floor = invstd / 64
    gap = _next_distinct_gap(r64.zn)
    assert bool((gap >= floor[None, :, None] * (1 - 1e-9))[:, nz].all()), float(gap[:, nz].min())
    # ... and that is far above fp32 rounding of the normalised value: |z - mean| <= 256, |gamma2| <= 1.5, |beta2| invstd^-1 < 128
    # give floor / max|value| >= (1/64) / 512 = 512 * 2^-24; asked for here: 64 roundings' worth
    assert bool((floor >= 64 * 2.0 ** -24 * r64.zn.abs().amax((0, 2, 3)))[nz].all())
    assert bool(r64.carry.any())
    return c


# ---- the library, called as ops.SATail / ops.SATailActivated call it -----------------------------------------------------------------
def _forward(x1, w2f, g2, b2, relu2, bn1=None):
    from amcontrast3d_amd import _lib, ops
    lib = _lib.load()
    B, C1, M, K = x1.shape
    C2 = w2f.shape[0]
    if bn1 is None:  # identity BatchNorm: relu(bn(x1)) == x1 for x1 >= 0
        bn1 = (torch.zeros(C1, device=DEV), torch.ones(C1, device=DEV), torch.ones(C1, device=DEV), torch.zeros(C1, device=DEV))
    f = SimpleNamespace(bn1=bn1, pooled=torch.full((B, C2, M), NAN, device=DEV), mean2=torch.empty(C2, device=DEV),
                        invstd2=torch.empty(C2, device=DEV), var2=torch.empty(C2, device=DEV),
                        zext=torch.full((B, C2, M), NAN, device=DEV), arg=torch.full((B, C2, M), 255, dtype=torch.uint8, device=DEV))
    wb = int(lib.amc3d_sa_tail_workspace_bytes(B, C1, C2, M))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=DEV)
    p = ops._ptr
    _lib.check(lib.amc3d_sa_tail_forward(B, C1, C2, M, K, p(x1), p(bn1[0]), p(bn1[1]), p(bn1[2]), p(bn1[3]), p(w2f), p(g2), p(b2),
                                         EPS, 0.0, int(relu2), p(f.pooled), p(f.mean2), p(f.invstd2), p(f.var2), None, None, None,
                                         p(f.zext), p(f.arg), p(work), wb, ops._stream(x1)), "sa_tail_forward")
    torch.cuda.synchronize()
    return f


def _backward(x1, w2f, g2, b2, relu2, gout, f, algebraic, pm):
    """algebraic: hand the forward's zext / arg over (the algebraic form where sat_alg_supported); otherwise null pointers for
    both, which always takes the recomputing form (modes 2 and 3)"""
    from amcontrast3d_amd import _lib, ops
    lib = _lib.load()
    B, C1, M, K = x1.shape
    C2 = w2f.shape[0]
    buf = torch.full((B, M, K, C1) if pm else (B, C1, M, K), NAN, device=DEV)
    r = SimpleNamespace(dx=buf.permute(0, 3, 1, 2) if pm else buf, dw2=torch.full((C2, C1), NAN, device=DEV),
                        dg2=torch.full((C2,), NAN, device=DEV), db2=torch.full((C2,), NAN, device=DEV),
                        arg=torch.full((B, C2, M), 255, dtype=torch.uint8, device=DEV))
    wb = int(lib.amc3d_sa_tail_workspace_bytes(B, C1, C2, M))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=DEV)
    p = ops._ptr
    _lib.check(lib.amc3d_sa_tail_backward(B, C1, C2, M, K, p(x1), p(f.bn1[0]), p(f.bn1[1]), p(f.bn1[2]), p(f.bn1[3]), p(w2f),
                                          p(f.mean2), p(f.invstd2), p(g2), p(b2), int(relu2), p(gout),
                                          p(f.zext) if algebraic else None, p(f.arg) if algebraic else None, p(buf), int(pm),
                                          p(r.dw2), p(r.dg2), p(r.db2), p(r.arg), p(work), wb, ops._stream(x1)), "sa_tail_backward")
    torch.cuda.synchronize()
    return r


def _bound(r64, r32, floor):
    err_torch = float((r32.double() - r64).abs().max())
    return max(4 * err_torch, floor * max(1.0, float(r64.abs().max()))), err_torch


def _check(what, got, r64, r32, floor):
    """the file's bound, element by element: err <= max(4 * err_torch32, floor * scale)"""
    got = got.detach().cpu().reshape(r64.shape)
    bound, err_torch = _bound(r64, r32, floor)
    err = float((got.double() - r64).abs().max())
    print(f"{what}: err {err:.3e} torch32 {err_torch:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, err_torch, bound)  # (a NaN left in an output fails here too)


def _check_args(what, got, r64):
    got, want = got.cpu().long(), r64.arg
    bad = (got != want) & r64.carry
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:8].tolist(), want[bad][:8].tolist())


GRADS = (("dx1", "dx", 1e-5), ("dw2", "dw2", 1e-5), ("dgamma2", "dg2", 1e-5), ("dbeta2", "db2", 1e-5))


# ---- A: routing decided exactly, through ops.SATailActivated ----------------------------------------------------------------------
@pytest.mark.parametrize("relu2", [False, True])
@pytest.mark.parametrize("C1,C2,B,M", SHAPES)
def test_activated_tail_routes_ties_and_signed_scales_like_torch(C1, C2, B, M, relu2, monkeypatch):
    from amcontrast3d_amd import ops
    c = _grid_case(C1, C2, B, M, relu2)
    x1, w2, g2, b2, gout = (t.to(DEV) for t in (c.x1, c.w2, c.g2, c.b2, c.gout))
    f = _forward(x1, w2.reshape(C2, C1).contiguous(), g2, b2, relu2)
    _check("pooled", f.pooled, c.r64.out, c.r32.out, 2e-6)
    # the routed neighbour, bit-exact wherever the triple carries gradient; z is exact, so is the raw value kept for the backward
    _check_args("forward arg", f.arg, c.r64)
    want_z = c.r64.zraw.gather(-1, c.r64.arg.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(f.zext.cpu().double()[c.r64.carry], want_z[c.r64.carry])
    for ch in c.zero:  # a zero scale: every neighbour gives beta2, the first one is routed to
        assert bool((f.arg[:, ch].cpu()[c.r64.carry[:, ch]] == 0).all()), ch
    for cm in (False, True):  # the position-major hand-over of dx1 (C1 % 4 == 0) and the channel-major store
        if cm:
            monkeypatch.setenv("AMC3D_SAT_DX1_CM", "1")
        else:
            monkeypatch.delenv("AMC3D_SAT_DX1_CM", raising=False)
        leaves = [t.clone().requires_grad_(True) for t in (x1, w2, g2, b2)]
        out = ops.SATailActivated.apply(leaves[0], leaves[1], leaves[2], leaves[3], EPS, relu2, None)
        out.backward(gout)
        got = SimpleNamespace(dx=leaves[0].grad, dw2=leaves[1].grad, dg2=leaves[2].grad, db2=leaves[3].grad)
        _check(f"pooled cm={cm}", out, c.r64.out, c.r32.out, 2e-6)
        for what, name, floor in GRADS:  # element by element: a gradient sent to a tied neighbour (7 for 3) is an error of its size
            _check(f"{what} cm={cm}", getattr(got, name), getattr(c.r64, name), getattr(c.r32, name), floor)


# ---- B: the algebraic and the recomputing backward on the same input ---------------------------------------------------------------
@pytest.mark.parametrize("relu2", [False, True])
@pytest.mark.parametrize("C1,C2,B,M", SHAPES)
def test_both_backward_forms_meet_fp64_and_each_other(C1, C2, B, M, relu2):
    c = _grid_case(C1, C2, B, M, relu2)
    x1, w2, g2, b2, gout = (t.to(DEV) for t in (c.x1, c.w2, c.g2, c.b2, c.gout))
    w2f = w2.reshape(C2, C1).contiguous()
    f = _forward(x1, w2f, g2, b2, relu2)
    for pm in ((0, 1) if C1 % 4 == 0 else (0,)):
        alg = _backward(x1, w2f, g2, b2, relu2, gout, f, True, pm)
        rec = _backward(x1, w2f, g2, b2, relu2, gout, f, False, pm)
        _check_args(f"arg handed through pm={pm}", alg.arg, c.r64)
        _check_args(f"arg of mode 2 pm={pm}", rec.arg, c.r64)
        for what, name, floor in GRADS:
            r64, r32 = getattr(c.r64, name), getattr(c.r32, name)
            _check(f"{what} given zext pm={pm}", getattr(alg, name), r64, r32, floor)
            _check(f"{what} recomputed pm={pm}", getattr(rec, name), r64, r32, floor)
            bound, _ = _bound(r64, r32, floor)
            d = float((getattr(alg, name).double() - getattr(rec, name).double()).abs().max())
            print(f"{what} pm={pm}: forms differ by {d:.3e}, allowed {2 * bound:.3e}")
            assert d <= 2 * bound, (what, pm, d, bound)
        for ch in c.zero:
            # a zero scale: both forms sum q * xhat of neighbour 0, the same fp32 xhat (z is exact).  They differ in the summation
            # alone: one rounds each product and adds 64 of them in an fp32 tree (1 + 6 roundings), the other adds in fp64, both
            # round the result once -- 8 half-ulps of sum |q xhat|, asked for with a factor two to spare
            zr = c.r64.zraw[:, ch]
            xh0 = (zr[..., 0] - zr.mean()) * (zr.var(unbiased=False) + EPS).rsqrt()
            allowed = 16 * 2.0 ** -24 * float((c.gout[:, ch].double().abs() * xh0.abs() * c.r64.carry[:, ch]).sum())
            d = abs(float(alg.dg2[ch]) - float(rec.dg2[ch]))
            print(f"dgamma2[{ch}] (zero scale) pm={pm}: forms differ by {d:.3e}, allowed {allowed:.3e}")
            assert d <= allowed, (ch, pm, d, allowed)


# ---- D: ops.SATail, BN1 + ReLU staged in the kernel: x1 is off the grid, near-ties exist ---------------------------------------------
@pytest.mark.parametrize("relu2", [False, True])
@pytest.mark.parametrize("C1,C2,B,M", [(32, 64, 2, 33), (6, 33, 2, 3)])
def test_tail_from_raw_y1_with_ties_and_signed_scales(C1, C2, B, M, relu2):
    from amcontrast3d_amd import _lib, ops
    g = torch.Generator().manual_seed(C1 * 7 + C2)
    y1 = _add_ties(torch.randn(B, C1, M, 32, generator=g) * 2 + 0.3)
    g1, b1 = torch.rand(C1, generator=g) + 0.5, torch.randn(C1, generator=g) * 0.2
    w2 = torch.randn(C2, C1, 1, 1, generator=g) * 0.2
    g2, b2 = _scales(C2, int(relu2), g)
    gout = torch.randn(B, C2, M, generator=g)
    r64 = reference(y1, g1, b1, w2, g2, b2, relu2, gout, torch.float64)
    r32 = reference(*(t.clone() for t in (y1, g1, b1, w2, g2, b2)), relu2, gout, torch.float32)  # (it marks fp32 inputs as leaves)
    lw = _layerwise(y1, (g1, b1), w2, g2, b2, relu2, gout, torch.float64)
    assert torch.equal(lw.out, r64[0]) and torch.equal(lw.dx, r64[1]) and torch.equal(lw.dg2, r64[5])  # one and the same composition

    dev = [t.to(DEV) for t in (y1, g1, b1, w2, g2, b2)]
    leaves = [t.clone().requires_grad_(True) for t in dev]
    log = {}
    ops.pool_log(log)
    try:
        out = ops.SATail.apply(leaves[0], leaves[1], leaves[2], EPS, leaves[3], leaves[4], leaves[5], EPS, relu2)
        out.backward(gout.to(DEV))
    finally:
        ops.pool_log(None)
    got = [out.detach().cpu()] + [t.grad.cpu() for t in leaves]
    for a, b64, b32, what in zip(got, r64, r32, ("pooled", "dy1", "dgamma1", "dbeta1", "dw2", "dgamma2", "dbeta2")):
        assert a.shape == b64.shape, what
        if what == "pooled":
            _check(what, a, b64, b32, 2e-6)
        else:  # arg-max flips between near-equal neighbours move single gradient entries: norm-wise, as in test_gpu_sa_tail.py
            rel = float((a.double() - b64).norm() / (b64.norm() + 1e-30))
            rel_torch = float((b32.double() - b64).norm() / (b64.norm() + 1e-30))
            print(f"{what}: rel {rel:.3e} torch32 {rel_torch:.3e}")
            assert rel <= max(4 * rel_torch, 1e-5), (what, rel, rel_torch)

    # the routed neighbour wherever the reference decides it: winner and next distinct value >= 1e-4 * max|z_norm| apart
    # (at (6, 33, M = 3) 1 % of at most 198 triples is ONE triple, and this seed has one: the case is deterministic, but a change
    # to the construction or the seed can move it to two -- then choose another seed, the limit stays)
    decided = _next_distinct_gap(lw.zn) >= 1e-4 * float(lw.zn.abs().max())
    assert int((lw.carry & ~decided).sum()) <= 0.01 * int(lw.carry.sum()), (int((lw.carry & ~decided).sum()), int(lw.carry.sum()))
    lw.carry = lw.carry & decided
    lib = _lib.load()
    mean1, invstd1, var1 = (torch.empty(C1, device=DEV) for _ in range(3))
    work1, wb1 = ops._bn_ws(C1, torch.device(DEV))
    _lib.check(lib.amc3d_bn_stats(B, C1, M * 32, EPS, ops._ptr(dev[0]), ops._ptr(mean1), ops._ptr(invstd1), ops._ptr(var1),
                                  ops._ptr(work1), wb1, ops._stream(dev[0])), "bn_stats")
    f = _forward(dev[0], dev[3].reshape(C2, C1).contiguous(), dev[4], dev[5], relu2, bn1=(mean1, invstd1, dev[1], dev[2]))
    _check("pooled, direct call", f.pooled, r64[0], r32[0], 2e-6)
    _check_args("forward arg", f.arg, lw)
    _check_args("arg the backward routed to", log[0], lw)
    for ch in (g2 == 0).nonzero().flatten().tolist():
        assert bool((f.arg[:, ch].cpu()[lw.carry[:, ch]] == 0).all()), ch
