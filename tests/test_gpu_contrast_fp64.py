"""The adaptive-margin contrast loss, row by row against an fp64 restatement, on every route.

Reference (plain torch, below): ref_stage restates MarginContrast.py:250-257 + 117-174 with the cosine written as
x / clamp_min(||x||, 1e-8) per row, evaluated at float64 (the arbiter) and float32 (the yardstick).  ref_conditioning gives,
from the closed form in csrc/loss.hip's header, the per-row scale A_n = sum over the edges touching n of
|g| / max(||f_n||, eps) * max_c |fhat_x - s fhat_n|.  A kernel passes when, for EVERY row,
max_c |got - df64| <= 4 * rho32 * A_n with rho32 = max_n max_c |df32 - df64| / A_n: four times torch's own fp32 error (the
project's margin, test_gpu_gcc.py / test_gpu_pwconv.py), measured per row so that rows with small gradients (unselected
anchors that only receive edges, anchors without a positive neighbour) count as much as the large ones.  Rows with A_n == 0
must be exactly zero.  Nothing in a tolerance comes from the code under test.

The inputs are built to contain the branches the kernels have (and assert so from the reference alone): mutual edges,
repeated neighbours (multiplicity 2 and 23), self edges, anchors without a positive neighbour at the far end of a mutual edge,
anchors whose neighbours are all positive, a in {0, 1, nextafter(1), 1e-30, -0.25}, near-parallel / anti-parallel rows, zero
rows and rows below the norm clamp, widths that are no multiple of 4, k on both sides of 32 and 64, m on both sides of the
4-anchor workgroup and the 256-row list block, channel-major tiles that end inside a cloud.

The empty selection (no anchor with 0 < a <= 1): the fp64 reference gives a NaN loss (mean of nothing) and an all-zero
gradient; every route gives the same (test_row_counts_and_selections).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-8
PARAMS = [(-1.0, 0.5, 0.3), (-1.0, 0.6, 0.5), (-1.0, 0.5, 0.07)]
GRAD_OUT = 0.9
ROW_C = (16, 32, 64, 128, 256)           # widths of the row kernels (16-byte pieces, C/4 lanes per row)
GENERAL_C = (3, 5, 33, 130, 260, 512)    # the general kernels: scalar channel loop, every <LPA, VPT> with c < C guards
ROW_ROUTES = ("atomic", "atomic_list", "csr", "mutual", "cm")
A_ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))
A_SPECIAL = (0.0, 1.0, A_ABOVE_ONE, 1e-30, -0.25)


# ------------------------------------------------------------------------------------------------------------ the reference
def ref_stage(f, nidx, posmask, a, mu, nu, T, dtype, grad_out=GRAD_OUT):
    """loss and d(grad_out * loss)/df of one stage at `dtype`; the anchors are chosen on the fp32 ambiguities as they are"""
    x = f.detach().to(dtype).requires_grad_(True)
    rows = torch.nonzero((a > 0) & (a <= 1)).flatten()
    h = x / torch.linalg.vector_norm(x, dim=1).clamp_min(EPS)[:, None]
    sim = (h[rows][:, None, :] * h[nidx[rows].long()]).sum(-1)
    pm = posmask[rows]
    margin = (mu * a[rows].to(dtype) + nu)[:, None]
    e = torch.exp(torch.where(pm, sim - margin, sim) / T)
    loss = (-torch.log((e * pm).sum(-1) / e.sum(-1) + 1e-12)).mean()
    (loss * grad_out).backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return loss.detach(), grad.detach()


def ref_conditioning(f, nidx, posmask, a, mu, nu, T, grad_out=GRAD_OUT):
    """fp64, from the closed form (csrc/loss.hip): l = -log(P/S + eps), g_ij = dL/ds_ij = coef_i e_ij ([pos] S_i - P_i),
    coef_i = -(grad_out / count) / ((P/S + eps) S^2 T); dL/df_n = sum over the edges (n, x) touching n, own and incoming, of
    g / max(||f_n||, eps) * (fhat_x - s fhat_n) -- without the projection s fhat_n where the clamp is active (fhat_n = f_n / eps
    is then linear in f_n).  [pos] S - P is written as the sum of the negatives' exponentials (pos) or -P: the same number
    without a cancellation.  Returns (A (m): the sum of the terms' magnitudes, max over the channels; df (m, C): their sum)."""
    x = f.detach().double()
    m, C = x.shape
    A = torch.zeros(m, dtype=torch.float64, device=x.device)
    df = torch.zeros(m, C, dtype=torch.float64, device=x.device)
    rows = torch.nonzero((a > 0) & (a <= 1)).flatten()
    if rows.numel() == 0:
        return A, df
    raw = torch.linalg.vector_norm(x, dim=1)
    n = raw.clamp_min(EPS)
    h = x / n[:, None]
    live = (raw >= EPS).double()
    nb = nidx[rows].long()
    hi, hx = h[rows][:, None, :], h[nb]
    s = (hi * hx).sum(-1)
    pm = posmask[rows]
    margin = (mu * a[rows].double() + nu)[:, None]
    e = torch.exp(torch.where(pm, s - margin, s) / T)
    P, N = (e * pm).sum(-1, keepdim=True), (e * ~pm).sum(-1, keepdim=True)
    S = P + N
    coef = -(grad_out / rows.numel()) / ((P / S + 1e-12) * S * S * T)
    g = coef * e * torch.where(pm, N.expand_as(e), -P.expand_as(e))
    own = (g / n[rows][:, None])[..., None] * (hx - (live[rows][:, None] * s)[..., None] * hi)
    inc = (g / n[nb])[..., None] * (hi - (live[nb] * s)[..., None] * hx)
    df.index_add_(0, rows, own.sum(1))
    df.index_add_(0, nb.flatten(), inc.reshape(-1, C))
    A.index_add_(0, rows, own.abs().amax(-1).sum(1))
    A.index_add_(0, nb.flatten(), inc.abs().amax(-1).flatten())
    return A, df


def ref_mutual(nidx, keep):
    """count (m,k): how often i stands in the list of its s-th neighbour, kept at the first slot of i's list that names that
    neighbour (what mutual & 0x7f encodes, capped at 127); listed (m,k): edges of selected anchors whose far end does not
    list them back; rev_start (m+1), rev_edge: the listed positions i*k + s grouped by far end, ascending"""
    nid = nidx.long()
    m, k = nid.shape
    me = torch.arange(m, device=nid.device)
    raw = (nid[nid] == me[:, None, None]).sum(-1)
    earlier = (nid[:, :, None] == nid[:, None, :]) & torch.ones(k, k, dtype=torch.bool, device=nid.device).tril(-1)
    first = ~earlier.any(-1)
    count = torch.where(first, raw.clamp_max(127), torch.zeros_like(raw))
    listed = (raw == 0) & keep[:, None]
    return count, listed, raw, *_reverse_lists(nid, listed)


def _reverse_lists(nid, take):
    m, k = nid.shape
    pos = torch.nonzero(take.flatten()).flatten()
    tgt = nid.flatten()[pos]
    order = torch.argsort(tgt * (m * k) + pos)
    start = torch.searchsorted(tgt[order].contiguous(), torch.arange(m + 1, device=nid.device))
    return start, pos[order]


def _keep(a):
    return (a > 0) & (a <= 1)


# ---------------------------------------------------------------------------------------- CPU checks of the reference itself
def _small_case(seed, degenerate):
    g = torch.Generator().manual_seed(seed)
    m, k, C = 40, 5, 8
    f = torch.randn(m, C, generator=g, dtype=torch.float64)
    nidx = torch.randint(0, m, (m, k), generator=g, dtype=torch.int32)
    nidx[3, 0] = 3          # a self edge
    nidx[4, 2] = nidx[4, 1]  # a repeated neighbour
    lab = torch.randint(0, 3, (m,), generator=g)
    a = torch.rand(m, generator=g)
    a[::7] = 0.0
    a[1], a[2], a[5], a[6] = 1.0, A_ABOVE_ONE, 1e-30, -0.25
    if degenerate:
        f[8] = 0.0
        f[9] *= 1e-9 / float(f[9].norm())
        f[10] = -3.0 * f[int(nidx[10, 0])] + 1e-4 * torch.randn(C, generator=g, dtype=torch.float64)
        a[8] = a[9] = a[10] = 0.5
        nidx[11, 0], nidx[11, 1], nidx[12, 3] = 8, 9, 9
        a[11] = a[12] = 0.7
    return f, nidx, lab[:, None] == lab[nidx.long()], a


@pytest.mark.parametrize("seed,degenerate,prm", [(0, False, PARAMS[0]), (1, True, PARAMS[2])])
def test_closed_form_reproduces_autograd(seed, degenerate, prm):
    """validates the closed form before it is used as a scale: its signed sum is autograd's fp64 gradient to 1e-12"""
    f, nidx, posmask, a = _small_case(seed, degenerate)
    _, df = ref_stage(f, nidx, posmask, a, *prm, torch.float64)
    A, closed = ref_conditioning(f, nidx, posmask, a, *prm)
    assert float(df.abs().max()) > 0
    if degenerate:
        assert float(df[8].abs().max()) > 0 and float(df[9].abs().max()) > 0
    assert float((closed - df).abs().max()) <= 1e-12 * float(df.abs().max())
    assert bool((closed.abs().amax(1) <= A * (1 + 1e-12) + 1e-300).all())


def test_ref_mutual_against_a_plain_enumeration():
    _, nidx, _, a = _small_case(2, False)
    keep = _keep(a)
    count, listed, raw, start, edge = ref_mutual(nidx, keep)
    m, k = nidx.shape
    want, nonmut = torch.zeros(m, k, dtype=torch.long), []
    for i in range(m):
        for s in range(k):
            x = int(nidx[i, s])
            c = int((nidx[x] == i).sum())
            if not bool((nidx[i, :s] == x).any()):
                want[i, s] = c
            if c == 0 and bool(keep[i]):
                nonmut.append((x, i * k + s))
    nonmut.sort()
    assert torch.equal(count, want) and int(count.max()) >= 1
    assert edge.tolist() == [p for _, p in nonmut]
    assert torch.equal(start, torch.searchsorted(torch.tensor([x for x, _ in nonmut]), torch.arange(m + 1)))
    assert torch.equal(listed.flatten().nonzero().flatten(), torch.tensor(sorted(p for _, p in nonmut)))


# ------------------------------------------------------------------------------------------------------------------ inputs
def _knn(p, k):
    """the k nearest OTHER points (the self-search without its first column), as views, with the distances of the same view"""
    from amcontrast3d_amd import ops
    o = torch.tensor([p.shape[0]], dtype=torch.int32, device=DEV)
    idx, d = ops.knnquery(k + 1, p, p, o, o)
    return idx[:, 1:], d[:, 1:]


def _labels_and_a(p, nidx, seed, base=None):
    """4 classes (spatially coherent where `base` is given), one block of a single class, six classes that occur once at far
    ends of mutual edges of selected rows; a uniform with fixed shares of the special values"""
    m = p.shape[0]
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 4, (m,), generator=g)
    if base is not None:
        lab = torch.where(torch.rand(m, generator=g) < 0.25, lab, base.cpu() % 4)
    pc = p.cpu()
    lab[pc[:, 0] < torch.quantile(pc[:, 0], 0.2)] = 0
    a = torch.rand(m, generator=g)
    u = torch.rand(m, generator=g)
    for lo, v in zip((0.0, 0.25, 0.30, 0.35, 0.40), A_SPECIAL):
        a[(u >= lo) & (u < (0.25 if lo == 0.0 else lo + 0.05))] = v
    count, _, raw, _, _ = ref_mutual(nidx.cpu(), _keep(a))
    far = nidx.cpu().long()[(raw > 0) & _keep(a)[:, None]].unique()   # far ends of mutual edges of selected rows
    single = far[torch.linspace(0, far.numel() - 1, 6).long()] if far.numel() >= 6 else far
    lab[single] = 4 + torch.arange(single.numel())
    a[single] = 0.5
    return lab.to(DEV), a.to(DEV), single.to(DEV)


class Graph:
    def __init__(self, name, p, nidx, dist, lab, a, single, B=1):
        from amcontrast3d_amd import ops
        self.name, self.p, self.nidx, self.dist, self.lab, self.a, self.single, self.B = name, p, nidx, dist, lab, a, single, B
        self.m, self.k = nidx.shape
        self.posmask = (lab[:, None] == lab[nidx.long()]).contiguous()
        assert torch.equal(ops.posmask_from_labels(lab.int(), nidx), self.posmask)
        self.plans = {}

    def plan(self, a=None, dist=False):
        """anchor list, reverse lists of all edges (csr), mutual bytes + reverse lists of the non-mutual edges (dist: built
        from the search's distances, as the model builds them; otherwise by scanning the lists).  Kept for the graph's own
        ambiguities only, one per form; a plan for other ambiguities is built for the caller and not kept."""
        from amcontrast3d_amd import ops
        own = a is None or a is self.a
        if own and dist in self.plans:
            return self.plans[dist]
        a = self.a if own else a
        anchors = ops.select_anchors(a)
        rev_csr = ops.contrast_csr(self.nidx, anchors)
        mutual, rev_m = ops.contrast_mutual(self.nidx, a, self.dist if dist else None) if self.k <= 64 else (None, None)
        if own:
            self.plans[dist] = (anchors, rev_csr, mutual, rev_m)
        return anchors, rev_csr, mutual, rev_m

    @functools.cached_property
    def structure(self):
        return ref_mutual(self.nidx, _keep(self.a))


@functools.lru_cache(None)
def graph(name, k=23):
    from amcontrast3d_amd import synthetic
    rng = np.random.default_rng(7)
    base, B = None, 1
    if name in ("room", "crafted"):
        nb = synthetic.make_batch(2, 1200)
        p = torch.from_numpy(nb["pos"]).reshape(-1, 3).contiguous().to(DEV)
        base, B = torch.from_numpy(nb["y"]).reshape(-1), 2
    elif name == "lattice":
        p = torch.from_numpy((rng.integers(0, 12, (2500, 3)) * 0.25).astype(np.float32)).to(DEV)
    elif name == "dup":
        pts = rng.uniform(0, 1, size=(500, 3)).astype(np.float32)
        p = torch.from_numpy(np.ascontiguousarray(pts[rng.integers(0, 500, size=1500)])).to(DEV)
    elif name.startswith("tiny"):
        p = torch.from_numpy(rng.uniform(0, 1, size=(int(name[4:]), 3)).astype(np.float32)).to(DEV)
    nidx, dist = _knn(p, k)
    if name == "crafted":  # repeated neighbours (multiplicity 2), self edges, one row that lists one neighbour 23 times
        nid = nidx.cpu().clone()
        m = nid.shape[0]
        third, tenth = torch.from_numpy(rng.uniform(size=m) < 1 / 3), torch.from_numpy(rng.uniform(size=m) < 0.1)
        nid[third, 5] = nid[third, 2]
        nid[tenth, 0] = torch.arange(m, dtype=torch.int32)[tenth]
        r0 = int(torch.nonzero(~tenth)[m // 2])
        nid[int(nid[r0, 0]), :] = r0  # r0 lists that row once, in slot 0: multiplicity 23 at (r0, 0)
        nidx, dist = nid.contiguous().to(DEV), None
    lab, a, single = _labels_and_a(p, nidx, 11, base)
    return Graph(name, p, nidx, dist, lab, a, single, B)


def _assert_branches(G):
    """the branches a graph is there for, from the reference alone; printed for the record"""
    count, listed, raw, start, edge = G.structure
    keep, nid, pm = _keep(G.a), G.nidx.long(), G.posmask
    share = float((raw > 0).float().mean())
    multi = int((count >= 2).sum())
    selfe = int((nid == torch.arange(G.m, device=DEV)[:, None]).sum())
    nopos = keep & ~pm.any(1)
    mut_sel = (raw > 0) & keep[:, None]                       # mutual edges of selected rows
    nopos_reached = int((nopos[nid] & mut_sel).sum())         # ... whose far end is an anchor with psum == 0
    allpos = int((keep & pm.all(1)).sum())
    has_mut_in = torch.zeros(G.m, dtype=torch.bool, device=DEV)
    has_mut_in[nid[mut_sel]] = True                           # rows that are the far end of a mutual edge of a selected row
    special = {v: int((has_mut_in & (G.a == v)).sum()) for v in A_SPECIAL}
    print(f"CONTRAST-FP64 branches graph={G.name} m={G.m} k={G.k} mutual_share={share:.3f} multiplicity>=2_edges={multi} "
          f"max_multiplicity={int(count.max())} self_edges={selfe} psum0_anchors={int(nopos.sum())} "
          f"psum0_reached_by_mutual={nopos_reached} all_positive_anchors={allpos} special_a_rows={special} "
          f"listed_nonmutual={int(listed.sum())}")
    assert nopos_reached >= 1 and allpos >= 1 and all(c >= 1 for c in special.values()), (nopos_reached, allpos, special)
    if G.name == "room":
        assert share > 0.5 and int(count.max()) == 1 and selfe == 0
    if G.name == "crafted":
        assert multi >= 1 and int(count.max()) == 23 and selfe >= 1 and int((count == 2).sum()) >= 1
    return share


def features(G, kind, C):
    """(i) 'gauss'; (ii) 'parallel': a tenth of the rows are +-10^[-3,3] multiples of one of their neighbours plus 1e-4 noise;
    (iii) 'degenerate': five zero rows and five of norm ~1e-9, each selected and a neighbour of selected rows (returns the
    ambiguities changed to make them so)"""
    g = torch.Generator().manual_seed(1000 + C)
    m = G.m
    f = torch.randn(m, C, generator=g)
    a = G.a
    if kind == "parallel":
        rows = torch.nonzero(torch.rand(m, generator=g) < 0.1).flatten()
        slot = torch.randint(0, G.k, (rows.numel(),), generator=g)
        src = G.nidx.cpu().long()[rows, slot]
        scale = 10 ** (torch.rand(rows.numel(), generator=g) * 6 - 3) * (torch.randint(0, 2, (rows.numel(),), generator=g) * 2 - 1)
        base = f.clone()
        f[rows] = scale[:, None] * base[src] + 1e-4 * torch.randn(rows.numel(), C, generator=g)
    if kind == "degenerate":
        keep = _keep(a)
        cand = G.nidx.long()[keep].unique()
        cand = cand[~torch.isin(cand, G.single)].cpu()
        pick = cand[torch.linspace(0, cand.numel() - 1, 10).long()]
        f[pick[:5]] = 0.0
        f[pick[5:]] *= (1e-9 / f[pick[5:]].norm(dim=1))[:, None]
        a = a.clone()
        a[pick.to(DEV)] = 0.5
        keep2 = _keep(a)
        listed_by_selected = torch.zeros(m, dtype=torch.bool, device=DEV)
        listed_by_selected[G.nidx.long()[keep2]] = True
        assert bool(keep2[pick.to(DEV)].all()) and bool(listed_by_selected[pick.to(DEV)].all())
        assert bool((f[pick[:5]] == 0).all()) and float(f[pick[5:]].norm(dim=1).max()) < 2e-9
    return f.to(DEV), a


# ------------------------------------------------------------------------------------------------------------------ routes
def run_route(route, f, G, a, posmask, prm, grad_out=GRAD_OUT, B=None, plan=None):
    from amcontrast3d_amd import ops
    anchors, rev_csr, mutual, rev_m = G.plan(a) if plan is None else plan
    m, C = f.shape
    if route == "cm":
        B = G.B if B is None else B
        f_cm = f.view(B, m // B, C).transpose(1, 2).contiguous().requires_grad_(True)
        assert ops.contrast_stage_supported_cm(f_cm, anchors, rev_m, mutual)
        loss = ops.contrast_stage_cm(f_cm, G.nidx, posmask, a, *prm, anchors, rev_m, mutual)
        (loss * grad_out).backward()
        return loss.detach(), f_cm.grad.transpose(1, 2).reshape(m, C)
    extra = {"atomic": (), "atomic_list": (anchors,), "csr": (anchors, rev_csr), "mutual": (anchors, rev_m, mutual)}[route]
    fg = f.clone().requires_grad_(True)
    loss = ops.contrast_stage(fg, G.nidx, posmask, a, *prm, *extra)
    (loss * grad_out).backward()
    return loss.detach(), fg.grad


class Ref:
    def __init__(self, f, G, a, posmask, prm, grad_out=GRAD_OUT):
        self.loss64, self.df64 = ref_stage(f, G.nidx, posmask, a, *prm, torch.float64, grad_out)
        self.loss32, df32 = ref_stage(f, G.nidx, posmask, a, *prm, torch.float32, grad_out)
        self.A, closed = ref_conditioning(f, G.nidx, posmask, a, *prm, grad_out)
        # (autograd's own fp64 rounding is relative to the terms it cancels, at most grad_out / (T |f|_min) each, not to the sum:
        #  where the closed form is exactly zero -- k = 1, a single class -- autograd leaves ~1e-20)
        nmin = float(torch.linalg.vector_norm(f.double(), dim=1).clamp_min(EPS).min())
        bound = 1e-10 * float(self.A.max()) + 1e-13 * abs(grad_out) / (prm[2] * nmin)
        assert float((closed - self.df64).abs().max()) <= bound, "closed form and autograd disagree at fp64"
        self.live = self.A > 0
        d32 = (df32.double() - self.df64).abs().amax(1)
        self.rho32 = float((d32[self.live] / self.A[self.live]).max()) if bool(self.live.any()) else 0.0

    def check(self, what, loss, grad, factor=4):
        assert bool(torch.isfinite(grad).all()), what
        assert bool((grad[~self.live] == 0).all()), (what, "rows no edge with a gradient touches must be exactly zero")
        err = (grad.double() - self.df64).abs().amax(1)
        unit = self.rho32 * self.A
        ratio = float((err[self.live] / unit[self.live]).max()) if self.rho32 > 0 and bool(self.live.any()) else 0.0
        worst = int(torch.argmax(torch.where(self.live, err / unit.clamp_min(1e-300), torch.zeros_like(err))))
        l32 = abs(float(self.loss32) - float(self.loss64))
        lerr = abs(float(loss) - float(self.loss64))
        ltol = max(4 * l32, 1e-6 * max(1.0, abs(float(self.loss64))))
        print(f"CONTRAST-FP64 {what} rho32={self.rho32:.3e} ratio={ratio:.3f} worst_row={worst} "
              f"loss64={float(self.loss64):.9f} loss_err={lerr:.2e} loss_tol={ltol:.2e}")
        assert lerr <= ltol, (what, float(loss), float(self.loss64), lerr, ltol)
        assert bool((err[self.live] <= factor * unit[self.live]).all()), (what, ratio, worst, float(err[worst]), float(unit[worst]))
        return ratio


def _routes_against_fp64(G, kind, C, routes, params=PARAMS, posmask=None, dist=False):
    f, a = features(G, kind, C)
    posmask = G.posmask if posmask is None else posmask
    plan = G.plan(a, dist)
    for prm in params:
        ref = Ref(f, G, a, posmask, prm)
        for route in routes:
            loss, grad = run_route(route, f, G, a, posmask, prm, plan=plan)
            ref.check(f"graph={G.name} k={G.k} feat={kind} C={C} prm={prm} route={route}", loss, grad)
    return f, a


# ---------------------------------------------------------------------------------------------- A. every route against fp64
@gpu
@pytest.mark.parametrize("C", ROW_C)
@pytest.mark.parametrize("kind", ["gauss", "parallel"])
@pytest.mark.parametrize("name", ["room", "crafted"])
def test_row_routes_against_fp64(name, kind, C):
    G = graph(name)
    _assert_branches(G)
    f, a = _routes_against_fp64(G, kind, C, ROW_ROUTES)
    if kind == "parallel":  # the case is there for cosines next to +-1 on selected edges
        h = F.normalize(f.double(), dim=1)
        s = (h[:, None, :] * h[G.nidx.long()]).sum(-1)[_keep(a)]
        assert int((s > 0.999).sum()) >= 10 and int((s < -0.999).sum()) >= 10


@gpu
@pytest.mark.parametrize("C", GENERAL_C)
@pytest.mark.parametrize("kind", ["gauss", "parallel"])
@pytest.mark.parametrize("name", ["room", "crafted"])
def test_general_kernels_against_fp64(name, kind, C):
    """widths without row kernels: the atomic form, also when the mutual-edge plan is passed (ContrastStage falls back)"""
    _routes_against_fp64(graph(name), kind, C, ("atomic", "atomic_list") + (("mutual", "csr") if C in (3, 5, 33) else ()))


@gpu
def test_zero_upstream_gradient_gives_exact_zeros():
    G = graph("crafted")
    f, a = features(G, "gauss", 32)
    for route in ROW_ROUTES:
        _, grad = run_route(route, f, G, a, G.posmask, PARAMS[0], grad_out=0.0)
        assert bool(torch.isfinite(grad).all()) and bool((grad == 0).all()), route


@functools.lru_cache(None)
def _small_graph(m, k, seed, B=1):
    """random lists (any m, also below k): repeated neighbours and self edges come by themselves"""
    g = torch.Generator().manual_seed(seed)
    nidx = torch.randint(0, m, (m, k), generator=g, dtype=torch.int32).to(DEV)
    lab = torch.randint(0, 3, (m,), generator=g).to(DEV)
    a = torch.rand(m, generator=g)
    a[torch.rand(m, generator=g) < 0.3] = 0.0
    return Graph(f"random{m}", None, nidx, None, lab, a.to(DEV), None, B)


@gpu
@pytest.mark.parametrize("n", [1, 15, 17, 63, 65, 600])
@pytest.mark.parametrize("B", [2, 3])
def test_channel_major_tiles_against_fp64(B, n):
    """clouds that end inside a tile, on both sides of both tile widths (64 points below 128 channels, 16 from there)"""
    G = _small_graph(B * n, 23, 100 * B + n, B)
    for ci, C in enumerate(ROW_C):
        f, a = features(G, "gauss", C)
        prm = PARAMS[(ci + n) % 3]
        ref = Ref(f, G, a, G.posmask, prm)
        loss_cm, grad = run_route("cm", f, G, a, G.posmask, prm)
        ref.check(f"graph=cm B={B} n={n} C={C} prm={prm} route=cm", loss_cm, grad)
        loss_row, grad = run_route("mutual", f, G, a, G.posmask, prm)
        ref.check(f"graph=cm B={B} n={n} C={C} prm={prm} route=mutual", loss_row, grad)
        assert torch.equal(loss_cm, loss_row) or (bool(torch.isnan(loss_cm)) and bool(torch.isnan(loss_row)))


# ------------------------------------------------------------------------------------------------- B. degenerate features
@gpu
@pytest.mark.parametrize("C", ROW_C)
@pytest.mark.parametrize("name", ["room", "crafted"])
def test_zero_and_clamped_rows_against_fp64(name, C):
    """rows of norm 0 and ~1e-9 (below the 1e-8 clamp: fhat = f / 1e-8 is linear there, its gradient has no projection term)"""
    G = graph(name)
    f, a = features(G, "degenerate", C)
    ref = Ref(f, G, a, G.posmask, PARAMS[0])
    small = torch.linalg.vector_norm(f, dim=1) < 1e-8
    assert int(small.sum()) == 10 and bool(ref.live[small].all())
    plan = G.plan(a)
    for route in ROW_ROUTES:
        loss, grad = run_route(route, f, G, a, G.posmask, PARAMS[0], plan=plan)
        ref.check(f"graph={name} feat=degenerate C={C} prm={PARAMS[0]} route={route}", loss, grad)
    if C == 32:  # for the record only: does the installed F.cosine_similarity clamp as the kernels document?
        rows = torch.nonzero(small).flatten()
        x, y = f[rows].double()[:, None, :], f[G.nidx[rows].long()].double()
        mine = ((x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)) * (y / y.norm(dim=-1, keepdim=True).clamp_min(EPS))).sum(-1)
        theirs = F.cosine_similarity(x, y, dim=2)
        print(f"CONTRAST-FP64 F.cosine_similarity vs explicit clamp on the degenerate rows: max |diff| = "
              f"{float((mine - theirs).abs().max()):.3e} (cosines up to {float(mine.abs().max()):.3e})")


# ------------------------------------------------------------------------------------------------- C. neighbourhood sizes
@gpu
@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 64, 65])
def test_neighbourhood_sizes(k):
    """one and two slots, both sides of a 32-slot round and of the 64-lane list; 65: beyond the mutual-edge plan"""
    from amcontrast3d_amd import ops
    G = graph("room", k)
    assert G.nidx.shape[1] == k
    if k == 65:
        with pytest.raises(RuntimeError, match=r"k must be in 1\.\.64"):
            ops.contrast_mutual(G.nidx, G.a)
    routes = ROW_ROUTES if k <= 64 else ("atomic", "atomic_list", "csr")
    for C in (32, 128):
        _routes_against_fp64(G, "gauss", C, routes, params=[PARAMS[k % 3]])
    _routes_against_fp64(G, "gauss", 20, ("atomic", "atomic_list"), params=[PARAMS[(k + 1) % 3]])


# ------------------------------------------------------------------------------------------------------- D. row counts
@gpu
@pytest.mark.parametrize("selection", ["none", "one", "all"])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 255, 257])
def test_row_counts_and_selections(m, selection):
    """four anchors per workgroup, anchor lists in 256-row blocks.  No anchor selected: the fp64 reference's loss is NaN (the
    mean of nothing) and its gradient all zeros; every route must give the NaN and the same gradient as the others."""
    G = _small_graph(m, 23, 500 + m)
    a = {"none": torch.zeros(m), "one": torch.zeros(m), "all": torch.full((m,), 0.4)}[selection]
    if selection == "none":
        a[::2] = -0.25
        a[1::3] = A_ABOVE_ONE
    if selection == "one":
        a[m - 1] = 1.0
    a = a.to(DEV)
    assert int(_keep(a).sum()) == {"none": 0, "one": 1, "all": m}[selection]
    plan = G.plan(a)
    for C, routes in ((32, ROW_ROUTES), (256, ROW_ROUTES), (20, ("atomic", "atomic_list"))):
        f, _ = features(G, "gauss", C)
        ref = Ref(f, G, a, G.posmask, PARAMS[0])
        grads = []
        for route in routes:
            loss, grad = run_route(route, f, G, a, G.posmask, PARAMS[0], B=1, plan=plan)
            if selection == "none":
                assert bool(torch.isnan(ref.loss64)) and bool(torch.isnan(loss)), route
                assert bool((ref.df64 == 0).all())
                grads.append(grad)
            else:
                ref.check(f"graph=random m={m} sel={selection} C={C} route={route}", loss, grad)
        for g2 in grads[1:]:
            assert torch.equal(g2, grads[0])
        if grads:
            assert bool((grads[0] == 0).all()), "the empty selection's gradient is zero, as torch's"


# ---------------------------------------------------------------------------------------------------- E. mutual structure
def _check_lists(what, got, start_w, edge_w, m):
    """rev = [rev_start (m+1) | rev_edge]: starts equal, every row's list ascending at every length (lists of more than 96
    entries -- hubs of duplicate points, the padded slots of a tiny cloud -- go through another sort than the short ones).
    Returns the longest list's length."""
    start, edge = got[:m + 1].long(), got[m + 1:].long()
    assert torch.equal(start, start_w), what
    E = int(start_w[m])
    assert E == edge_w.numel()
    assert torch.equal(edge[:E], edge_w), what
    return int((start_w[1:] - start_w[:-1]).max()) if m else 0


def _check_structure(G, with_dist):
    from amcontrast3d_amd import ops
    count, listed, raw, start, edge = G.structure
    want = (count + listed.long() * 0x80).to(torch.uint8)
    forms = [("scan", None)] + ([("dist", G.dist)] if with_dist else [])
    longest_m = 0
    for form, d in forms:
        mutual, rev = ops.contrast_mutual(G.nidx, G.a, d)
        assert torch.equal(mutual & 0x7f, want & 0x7f), (G.name, form, "multiplicity")
        assert torch.equal(mutual & 0x80, want & 0x80), (G.name, form, "listed flag")
        longest_m = _check_lists((G.name, form), rev, start, edge, G.m)
    keep = _keep(G.a)
    s_all, e_all = _reverse_lists(G.nidx.long(), keep[:, None].expand(G.m, G.k))
    longest = _check_lists((G.name, "csr"), ops.contrast_csr(G.nidx, ops.select_anchors(G.a)), s_all, e_all, G.m)
    return longest, longest_m


@gpu
@pytest.mark.parametrize("name", ["room", "lattice", "dup", "tiny7", "tiny23", "tiny24", "crafted"])
def test_mutual_structure_against_enumeration(name):
    """contrast_mutual by scan and by distance comparison (ties with the neighbour's k-th distance, zero distances and
    placeholder slots fall back to the scan) and contrast_csr against the vectorised enumeration"""
    G = graph(name)
    count, listed, raw, _, _ = G.structure
    note = ""
    if G.dist is not None:
        rk = G.dist[:, -1]
        tie = G.dist == rk[G.nidx.long()]
        zero = G.dist == 0
        placeholder = G.dist > 9e4
        note = (f"tie_decided={int(tie.sum())} (mutual {int((tie & (raw > 0)).sum())}, not {int((tie & (raw == 0)).sum())}) "
                f"zero_distance={int(zero.sum())} placeholder_slots={int(placeholder.sum())}")
        if name == "lattice":
            assert int(tie.sum()) > 0 and int(zero.sum()) > 0 and int((tie & (raw == 0)).sum()) > 0
        if name == "dup":
            assert int(zero.sum()) > 0
        if name in ("tiny7", "tiny23"):  # the search pads short segments with (index 0, 1e10): valid rows, so the loss can run
            assert int(placeholder.sum()) == G.m * (G.k + 1 - G.m) and bool((G.nidx[placeholder] == 0).all())
        if name == "tiny24":
            assert int(placeholder.sum()) == 0
    if name == "crafted":
        assert int(count.max()) == 23
    longest, longest_m = _check_structure(G, G.dist is not None)
    print(f"CONTRAST-FP64 structure graph={name} m={G.m} mutual_share={float((raw > 0).float().mean()):.3f} "
          f"max_multiplicity={int(count.max())} listed={int(listed.sum())} longest_csr_list={longest} "
          f"longest_nonmutual_list={longest_m} lists_over_96={'yes' if max(longest, longest_m) > 96 else 'no'} {note}")


@gpu
def test_hub_lists_beyond_the_short_sort_are_ascending_and_repeat():
    """every row names row 0 first: its reverse lists (all edges; the non-mutual ones) hold hundreds of entries, beyond the
    96 that the ordering pass sorts by insertion.  Ascending all the same, so the gathering routes repeat bit for bit."""
    m, k = 400, 23
    g = torch.Generator().manual_seed(77)
    nidx = torch.randint(0, m, (m, k), generator=g, dtype=torch.int32)
    nidx[:, 0] = 0
    lab = torch.randint(0, 3, (m,), generator=g).to(DEV)
    a = torch.rand(m, generator=g)
    a[torch.rand(m, generator=g) < 0.3] = 0.0
    G = Graph("hub", None, nidx.to(DEV), None, lab, a.to(DEV), None, 1)
    longest, longest_m = _check_structure(G, False)
    print(f"CONTRAST-FP64 structure graph=hub m={m} longest_csr_list={longest} longest_nonmutual_list={longest_m}")
    assert longest > 96 and longest_m > 96
    f, _ = _routes_against_fp64(G, "gauss", 32, ROW_ROUTES, params=[PARAMS[0]])
    for r in ("csr", "mutual", "cm"):
        (l1, g1), (l2, g2) = (run_route(r, f, G, G.a, G.posmask, PARAMS[0]) for _ in range(2))
        assert torch.equal(g1, g2) and torch.equal(l1, l2), r


@gpu
@pytest.mark.parametrize("name", ["tiny7", "tiny23", "lattice", "dup"])
def test_loss_on_tied_duplicate_and_padded_graphs(name):
    """the lists the distance form has to scan for -- with the plan built FROM the distances, as the model builds it"""
    _routes_against_fp64(graph(name), "gauss", 64, ROW_ROUTES, params=[PARAMS[1]], dist=True)


# ------------------------------------------------------------------------- F. routes against each other and run to run
@gpu
@pytest.mark.parametrize("name", ["room", "lattice", "crafted"])
def test_gather_routes_repeat_bit_for_bit_and_cm_loss_equals_row_loss(name):
    G = graph(name)
    for C in ROW_C:
        f, a = features(G, "gauss", C)
        out = {r: [run_route(r, f, G, a, G.posmask, PARAMS[1]) for _ in range(2)] for r in ("csr", "mutual", "cm")}
        for r, ((l1, g1), (l2, g2)) in out.items():
            assert torch.equal(g1, g2) and torch.equal(l1, l2), (name, C, r)
        assert torch.equal(out["cm"][0][0], out["mutual"][0][0]), (name, C, float(out["cm"][0][0]), float(out["mutual"][0][0]))
        assert torch.equal(out["csr"][0][0], out["mutual"][0][0])


# --------------------------------------------------------------------------------------------------- G. mask precondition
@gpu
def test_asymmetric_mask_on_the_routes_that_do_not_assume_symmetry():
    """the mutual-edge backward reads the mask of an incoming mutual edge from the receiving row: right for label-derived
    masks only.  The atomic and reverse-list forms read the anchor's own mask: any mask"""
    G = graph("room")
    posmask = (torch.rand(G.m, G.k, generator=torch.Generator().manual_seed(5)) < 0.4).to(DEV)
    count, _, raw, _, _ = G.structure
    nid = G.nidx.long()
    back = (nid[nid] == torch.arange(G.m, device=DEV)[:, None, None])
    asym = (back & (posmask[nid] != posmask[:, :, None])).any(-1)
    assert int(asym.sum()) > 100
    _routes_against_fp64(G, "gauss", 64, ("atomic", "atomic_list", "csr"), posmask=posmask)
    _routes_against_fp64(G, "gauss", 33, ("atomic", "atomic_list"), posmask=posmask, params=[PARAMS[0]])


@gpu
@pytest.mark.parametrize("name", ["room", "lattice"])
def test_label_masks_are_symmetric_on_mutual_edges(name):
    from amcontrast3d_amd import ops
    G = graph(name)
    posmask = ops.posmask_from_labels(G.lab.int(), G.nidx)
    nid = G.nidx.long()
    back = (nid[nid] == torch.arange(G.m, device=DEV)[:, None, None])  # [i, s, j]: slot j of i's s-th neighbour names i
    assert int(back.sum()) > G.m
    assert not bool((back & (posmask[nid] != posmask[:, :, None])).any())
