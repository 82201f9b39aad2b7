"""ops.contrast_stage_variant -- every form of the contrast loss on the form-generic kernels -- row by row against fp64.

Method of tests/test_gpu_contrast_fp64.py with a reference of its own (tests/contrast_variants_ref.py, pinned to the head's
code by tests/test_contrast_variants_host.py): the stage is restated in plain torch with the cosine written as
x / clamp_min(||x||, 1e-8) per row and evaluated at float64 (the arbiter) and float32 (the yardstick).  The edge weights
g = dL/dsim come from autograd on the retained cosines, so no closed form per variant enters the reference; the per-row scale
is A_n = sum over the edges touching n of |g| / max(||f_n||, eps) * max_c |fhat_x - s fhat_n| (projection dropped where the clamp
is active), and every Ref asserts that the signed sum over the same edges reproduces autograd's fp64 gradient to 1e-12
relative.  The kernels pass when, for EVERY row, max_c |got - df64| <= 4 * rho32 * A_n with rho32 = max_n max_c |df32 - df64| / A_n
of torch's own fp32 evaluation of that form on that input (four times torch's fp32 error: the project's margin), rows with
A_n == 0 are exactly zero, and every selected anchor's loss is within 4 * max_i |l32_i - l64_i| of l64_i.  Nothing in a
tolerance comes from the code under test.

The crafted inputs contain (asserted from the reference alone): a selected anchor without a positive neighbour (six classes
that occur once), one whose neighbours are all positive (a block of one class), a repeated neighbour, a self edge,
a in {0, 1, nextafter(1), 1e-30, -0.25}, a zero row and a row below the norm clamp, both listed by selected anchors.  Inputs of
fewer than 64 rows (m = 3) cannot hold all of that and are plain random lists.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from contrast_variants_ref import DEFAULT_FORM, EPS, FORMS, MU, NU, StageRef, edge_decomposition, form_id, keep_rows
from test_gpu_train_edges import (GRAD_BOUND, _Probe, _fresh_pipelines, _grad_error, _grads, _loader, _make,  # noqa: F401
                                  _same_results, _same_state, _the_pipeline)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_OUT = 0.9
A_ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))
A_SPECIAL = (0.0, 1.0, A_ABOVE_ONE, 1e-30, -0.25)
SIX_FORMS = (("constant", "-m", "Method1", 0.3), ("adaptive", "+m", "Method2", 0.07), ("learned", "-m", "Method1", None),
             ("learned", "+m", "Method2", 0.3), ("adaptive", "NONE", "Method1", None), ("constant", "-m", "Method2", 0.07))
NON_DEFAULT = tuple(f for f in FORMS if f != DEFAULT_FORM)
R_SELF, R_REPEAT, R_ALLPOS = 10, 11, 12   # crafted rows (the special ambiguities sit in rows 0..4)


# ------------------------------------------------------------------------------------------------------------------ inputs
class Input:
    """points in the unit cube, their k nearest other points as the idx[:, 1:] view of the (m, k + 1) search result (row
    stride k + 1), labels, ambiguities, features of width C"""

    def __init__(self, m, k, C, seed=5):
        from amcontrast3d_amd import ops
        g = torch.Generator().manual_seed(seed + 1000 * m + k)
        self.m, self.k, self.C = m, k, C
        self.crafted = m >= 64
        p = torch.rand(m, 3, generator=g)
        if m > k + 1:
            o = torch.tensor([m], dtype=torch.int32, device=DEV)
            full = ops.knnquery(k + 1, p.to(DEV), p.to(DEV), o, o)[0].cpu().clone()
        else:
            full = torch.randint(0, m, (m, k + 1), generator=g, dtype=torch.int32)
        lab = torch.randint(0, 4, (m,), generator=g)
        if k >= 23:
            lab[p[:, 0] < 0.25] = 0                               # a block of one class
        a = torch.rand(m, generator=g)
        a[torch.rand(m, generator=g) < 0.2] = 0.0
        singles = torch.empty(0, dtype=torch.long)
        if self.crafted:
            full[R_SELF, 1] = R_SELF                              # a self edge
            full[R_REPEAT, 6 if k >= 6 else 2] = full[R_REPEAT, 1]  # a repeated neighbour
            lab[full[R_ALLPOS, 1:].long()] = 0                    # all neighbours positive
            lab[R_ALLPOS] = 0
            taken = set(full[R_ALLPOS, 1:].tolist()) | {R_SELF, R_REPEAT, R_ALLPOS}
            singles = torch.tensor([r for r in range(20, m) if r not in taken][:6])
            lab[singles] = 4 + torch.arange(6)                    # six classes that occur once: no positive neighbour
            a[singles] = 0.5
            a[torch.tensor([R_SELF, R_REPEAT, R_ALLPOS])] = 0.6
            # (short lists: without the block, and with the all-positive anchor's neighbours selected themselves, so that no row is
            #  touched only by edges whose fp64 weight is autograd's cancellation residue of an exact zero -- see Ref.rho32)
            if k < 23:
                a[full[R_ALLPOS, 1:].long()] = 0.6
            a[:5] = torch.tensor(A_SPECIAL)
        nid = full[:, 1:]
        f = torch.randn(m, C, generator=g)
        self.zero_row = self.clamped_row = None
        if self.crafted:
            keep = (a > 0) & (a <= 1)
            cand = nid[keep].long().unique()
            cand = [int(r) for r in cand if r >= 20 and int(r) not in set(singles.tolist())]
            self.zero_row, self.clamped_row = cand[0], cand[len(cand) // 2]
            f[self.zero_row] = 0.0
            f[self.clamped_row] *= 1e-9 / float(f[self.clamped_row].norm())
            a[self.zero_row] = a[self.clamped_row] = 0.5          # selected themselves as well: own edges of a clamped row
        self.full = full.to(DEV)
        self.nidx = self.full[:, 1:]                              # a strided view: no copy
        assert self.nidx.stride(0) == k + 1 and self.nidx.shape == (m, k)
        self.lab, self.a, self.f = lab.to(DEV), a.to(DEV).contiguous(), f.to(DEV).contiguous()
        self.posmask = (self.lab[:, None] == self.lab[self.nidx.long()]).contiguous()
        self.singles = singles.to(DEV)
        self._plan = None
        if self.crafted:
            self.assert_branches()

    def assert_branches(self):
        keep, nid, pm = (self.a > 0) & (self.a <= 1), self.nidx.long(), self.posmask
        nopos, allpos = int((keep & ~pm.any(1)).sum()), int((keep & pm.all(1)).sum())
        srt = nid.sort(1).values
        repeated = int((keep[:, None] & (srt[:, 1:] == srt[:, :-1])).sum())
        selfe = int((keep[:, None] & (nid == torch.arange(self.m, device=DEV)[:, None])).sum())
        special = {v: int((self.a == v).sum()) for v in A_SPECIAL}
        norms = torch.linalg.vector_norm(self.f.double(), dim=1)
        listed = torch.zeros(self.m, dtype=torch.bool, device=DEV)
        listed[nid[keep]] = True
        zero_rows, clamped = int(((norms == 0) & listed).sum()), int(((norms > 0) & (norms < EPS) & listed).sum())
        print(f"CONTRAST-VARIANT input m={self.m} k={self.k} C={self.C} selected={int(keep.sum())} no_positive={nopos} "
              f"all_positive={allpos} repeated={repeated} self_edges={selfe} special_a={special} zero_rows={zero_rows} "
              f"clamped_rows={clamped}")
        assert nopos >= 1 and allpos >= 1 and repeated >= 1 and selfe >= 1 and all(c >= 1 for c in special.values())
        assert zero_rows >= 1 and clamped >= 1

    def plan(self):
        from amcontrast3d_amd import ops
        if self._plan is None:
            anchors = ops.select_anchors(self.a)
            self._plan = (anchors, ops.contrast_csr(self.nidx, anchors))
        return self._plan


@functools.lru_cache(None)
def make_input(m, k, C):
    return Input(m, k, C)


# --------------------------------------------------------------------------------------------------------------- reference
class Ref:
    def __init__(self, f, nidx, posmask, a, form, grad_out=GRAD_OUT, mu=MU, nu=NU):
        r64 = StageRef(f, nidx, posmask, a, form, torch.float64, grad_out, mu, nu)
        r32 = StageRef(f, nidx, posmask, a, form, torch.float32, grad_out, mu, nu)
        self.rows, self.loss_pt64, self.loss64, self.df64 = r64.rows, r64.loss_pt, r64.loss, r64.grad
        self.A, closed = edge_decomposition(f, nidx, r64.rows, r64.sim, r64.g)
        gmax = float(self.df64.abs().max())
        assert float((closed - self.df64).abs().max()) <= 1e-12 * gmax, "the edge decomposition and autograd disagree at fp64"
        assert bool(torch.isfinite(self.df64).all()) and bool(torch.isfinite(self.loss_pt64).all())
        self.live = self.A > 0
        d32 = (r32.grad.double() - self.df64).abs().amax(1)
        self.rho32 = float((d32[self.live] / self.A[self.live]).max()) if bool(self.live.any()) else 0.0
        # The yardstick must not be vacuous.  Autograd leaves, for an anchor whose neighbours are all positive, edge weights of
        # ~1e-17 at fp64 (1/S - P/S^2 with P == S) and of ~1e-8 at fp32 where the derivative is exactly zero; a row touched by
        # such edges ONLY has A_n ~ 1e-17 and would put rho32 at ~1e9.  The inputs are built so that no such row exists; torch's
        # fp32 error on them is 8e-8 .. 3e-4 of A_n (the largest: learned / Method1 / T = 0.07, its S - P cancellation).
        assert self.rho32 <= 1e-3, ("the input has a row touched only by cancellation residues", self.rho32)
        self.l32 = float((r32.loss_pt.double() - self.loss_pt64).abs().max()) if self.rows.numel() else 0.0

    def check(self, what, loss_pt, grad, factor=4):
        assert bool(torch.isfinite(grad).all()), what
        assert bool((grad[~self.live] == 0).all()), (what, "rows no edge with a gradient touches must be exactly zero")
        err = (grad.double() - self.df64).abs().amax(1)
        unit = self.rho32 * self.A
        ratio = float((err[self.live] / unit[self.live]).max()) if self.rho32 > 0 and bool(self.live.any()) else 0.0
        worst = int(torch.argmax(torch.where(self.live, err / unit.clamp_min(1e-300), torch.zeros_like(err))))
        lerr = float((loss_pt[self.rows].double() - self.loss_pt64).abs().max()) if self.rows.numel() else 0.0
        print(f"CONTRAST-VARIANT {what} rho32={self.rho32:.3e} ratio={ratio:.3f} worst_row={worst} "
              f"loss_err={lerr:.3e} l32={self.l32:.3e} loss_ratio={lerr / self.l32 if self.l32 > 0 else 0.0:.3f}")
        assert lerr <= factor * self.l32, (what, "per-anchor loss", lerr, self.l32)
        assert bool((err[self.live] <= factor * unit[self.live]).all()), (what, ratio, worst, float(err[worst]), float(unit[worst]))
        return ratio


def run_variant(X, form, route, f=None, a=None, grad_out=GRAD_OUT):
    """route 'rows': anchors + rev (the gather where the width has row kernels); 'list': anchors, no rev (atomics);
    'none': neither (atomics, every anchor visited and tested) -> (stage loss, per-anchor loss buffer, gradient)"""
    from amcontrast3d_amd import ops
    f = X.f if f is None else f
    a = X.a if a is None else a
    if a is X.a:
        anchors, rev = X.plan()
    else:
        anchors = ops.select_anchors(a)
        rev = ops.contrast_csr(X.nidx, anchors)
    extra = {"rows": (anchors, rev), "list": (anchors, None), "none": (None, None)}[route]
    fg = f.clone().requires_grad_(True)
    loss = ops.contrast_stage_variant(fg, X.nidx, X.posmask, a, *form[:3], MU, NU, form[3], *extra)
    (loss * grad_out).backward()
    b = ops.contrast_variant_forward(f, X.nidx, X.posmask, a, ops.contrast_form(*form), MU, NU, extra[0])
    assert torch.equal(b["mean_cnt"][0], loss.detach()) or (bool(torch.isnan(loss)) and bool(torch.isnan(b["mean_cnt"][0])))
    rows = keep_rows(a)
    if rows.numel():  # the stage loss is masked_mean_kernel's: the fp64 mean of the selected anchors' losses, rounded once
        assert float(loss.detach()) == float(b["loss_pt"][rows].double().mean().float())
    return loss.detach(), b["loss_pt"], fg.grad


def _check_forms(X, forms, route):
    with_timing_counts = {}
    from amcontrast3d_amd import timing
    for form in forms:
        ref = Ref(X.f, X.nidx, X.posmask, X.a, form)
        with timing.count_calls() as c:
            loss, loss_pt, grad = run_variant(X, form, route)
        with_timing_counts = dict(c)
        gather = route == "rows" and X.C in (16, 32, 64, 128, 256)
        assert c["contrast_variant_backward_csr" if gather else "contrast_variant_backward"] == 1, with_timing_counts
        ref.check(f"form={form_id(form)} m={X.m} k={X.k} C={X.C} route={route}", loss_pt, grad)


# ------------------------------------------------------------------------------- 1. all 53 non-default forms, rows route
@pytest.mark.parametrize("form", NON_DEFAULT, ids=form_id)
def test_every_non_default_form_against_fp64(form):
    """m = 331: no multiple of the 4-anchor workgroup or of 8; k = 23 as the idx[:, 1:] view of a 24-column search"""
    assert len(NON_DEFAULT) == 53
    _check_forms(make_input(331, 23, 32), [form], "rows")


# ------------------------------------------------------------------------------------------------ 2. the route families
@pytest.mark.parametrize("k", [5, 33, 64])
@pytest.mark.parametrize("C", [16, 64, 128, 256])
def test_rows_route_widths_and_neighbourhood_sizes(C, k):
    _check_forms(make_input(331, k, C), SIX_FORMS, "rows")


@pytest.mark.parametrize("C", [3, 5, 33, 130, 512])
def test_atomic_route_with_an_anchor_list(C):
    _check_forms(make_input(331, 23, C), SIX_FORMS, "list")


@pytest.mark.parametrize("m", [3, 257])
def test_atomic_route_without_an_anchor_list(m):
    _check_forms(make_input(m, 23, 32), SIX_FORMS, "none")


def test_a_reverse_list_with_a_width_without_row_kernels_takes_the_atomic_route():
    _check_forms(make_input(331, 23, 33), SIX_FORMS[:2], "rows")


# ------------------------------------------------------------------------------------- 3. the cosines, bit for bit
@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("C", [32, 33])
def test_cosines_equal_the_default_forwards_bit_for_bit(C, listed):
    from amcontrast3d_amd import _lib, ops
    X = make_input(331, 23, C)
    lib = _lib.load()
    anchors = X.plan()[0] if listed else None
    got = ops.contrast_variant_forward(X.f, X.nidx, X.posmask, X.a, ops.contrast_form("learned", "+m", "Method2", None), MU, NU,
                                       anchors)
    # (unvisited rows are not written: compare the visited ones)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    m, k = X.m, X.k
    norm = torch.empty(m, device=DEV)
    unit = torch.empty_like(X.f) if lib.amc3d_contrast_backward_csr_supported(C) else None
    sim = torch.zeros(m, k, device=DEV)
    loss_pt, mean_cnt = torch.empty(m, device=DEV), torch.empty(2, device=DEV)
    _lib.check(lib.amc3d_contrast_forward(m, C, k, X.nidx.stride(0), ptr(X.f), ptr(X.nidx), ptr(X.posmask), ptr(X.a), ptr(anchors),
                                          MU, NU, 0.3, ptr(norm), ptr(unit), ptr(sim), None, ptr(loss_pt), ptr(mean_cnt),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "contrast_forward")
    torch.cuda.synchronize()
    rows = keep_rows(X.a)
    assert rows.numel() > 100 and bool((sim[rows] != 0).any())
    assert torch.equal(got["sim"][rows], sim[rows])
    assert torch.equal(got["norm"], norm)


# ------------------------------------------------------------------------------------ 4. the default form, a 54th call
def test_the_default_form_on_the_variant_kernels():
    _check_forms(make_input(331, 23, 32), [DEFAULT_FORM], "rows")
    _check_forms(make_input(331, 23, 33), [DEFAULT_FORM], "list")


# --------------------------------------------------------------------------------------------------- 5. empty selection
@pytest.mark.parametrize("form", SIX_FORMS[:4], ids=form_id)
def test_empty_selection_gives_nan_and_a_zero_gradient(form):
    X = make_input(331, 23, 32)
    a = torch.zeros(X.m)
    a[::2], a[1::3] = -0.25, A_ABOVE_ONE
    a = a.to(DEV)
    assert keep_rows(a).numel() == 0
    ref = StageRef(X.f, X.nidx, X.posmask, a, form, torch.float64, GRAD_OUT)
    assert bool(torch.isnan(ref.loss)) and bool((ref.grad == 0).all())
    for route in ("rows", "list", "none"):
        loss, _, grad = run_variant(X, form, route, a=a)
        assert bool(torch.isnan(loss)), route
        assert bool((grad == 0).all()), route


# ------------------------------------------------------------------------------------------------------------ 6. capture
def test_forward_and_backward_replay_under_a_captured_graph():
    """learned / +m / Method2 / no temperature with a plan (anchors, rev): captured once, replayed with new feature values in
    the static input; each replay equals the eager call bit for bit (the rows route has a fixed summation order)"""
    from amcontrast3d_amd import ops
    X = make_input(331, 23, 32)
    form = ("learned", "+m", "Method2", None)
    anchors, rev = X.plan()
    static = X.f.clone().requires_grad_(True)

    def step(x):
        loss = ops.contrast_stage_variant(x, X.nidx, X.posmask, X.a, *form[:3], MU, NU, form[3], anchors, rev)
        return loss, torch.autograd.grad(loss * GRAD_OUT, x)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            loss_s, grad_s = step(static)
    torch.cuda.synchronize()
    for it in range(2):
        new = torch.randn(X.m, X.C, generator=torch.Generator().manual_seed(40 + it)).to(DEV)
        with torch.no_grad():
            static.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        want_loss, want_grad = step(new.clone().requires_grad_(True))
        assert bool(torch.isfinite(want_loss)) and float(want_grad.abs().max()) > 0
        assert torch.equal(loss_s, want_loss.detach()), it
        assert torch.equal(grad_s, want_grad), it


# --------------------------------------------------------------------------------------------------------- 7. head level
def _head_case(margin="constant"):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import configs
    from openpoints.AMContrast3D.MarginContrast import ContrastHead
    from openpoints.utils import EasyConfig
    g = torch.Generator().manual_seed(21)
    n0, n1 = 1024, 256
    p0 = torch.rand(n0, 3, generator=g)
    target = (p0[:, 0] * 3).long() + 3 * (p0[:, 1] > 0.5).long()   # six spatially coherent classes
    stages = []
    for n, C in ((n0, 32), (n1, 33)):                               # a width with row kernels and one without
        stages.append({"p_out": p0[:n].contiguous().to(DEV), "f_out": torch.randn(n, C, generator=g).to(DEV),
                       "offset": torch.tensor([n], dtype=torch.int32, device=DEV)})
    args = EasyConfig()
    args.update(dict(configs.ambiguity_args("s3dis"), margin=margin, stages_num=2))
    return ContrastHead(), target.to(DEV), {"up": stages, "down": stages}, args


@pytest.mark.parametrize("planned", [False, True], ids=["plan-inside", "plan-precomputed"])
def test_the_head_takes_the_variant_op_and_matches_the_cpu_composition(planned):
    from amcontrast3d_amd import timing
    head, target, stage_list, args = _head_case()
    plan = head.plan(target, stage_list, 13, None, args)
    assert all(g["mutual"] is None and g["rev"] is not None for g in plan), "non-default form: reverse lists of all edges"
    if planned:
        stage_list = dict(stage_list, geometry={"loss": plan})
    with timing.count_calls() as c:
        loss, _, ai = head(None, target, stage_list, 13, None, args)
    assert c["contrast_variant_forward"] == 2 and c["contrast_forward"] == 0, dict(c)
    assert c["contrast_csr"] == (0 if planned else 2)
    # the torch composition on CPU copies of the same tensors (the plan's lists, masks and ambiguities; the head's CPU branch)
    cpu_plan = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in g.items()} for g in plan]
    cpu_list = {"up": [{k: v.cpu() for k, v in s.items()} for s in stage_list["up"]], "geometry": {"loss": cpu_plan}}
    cpu_list["down"] = cpu_list["up"]
    with timing.count_calls() as c2:
        want, _, _ = head(None, target.cpu(), cpu_list, 13, None, args)
    assert not c2, "the CPU branch launches nothing"
    bound = 0.0
    form = (args.margin, args.db, args.supervisedCL, args.temperature)
    for g, s in zip(plan, stage_list["up"]):
        ref = Ref(s["f_out"], g["neighbor_idx"], g["posmask"], g["ambiguity"], form, 1.0, float(args.mu), float(args.nu))
        assert ref.rows.numel() > 10
        bound += 4 * ref.l32
    print(f"CONTRAST-VARIANT head planned={planned} loss={float(loss):.7f} cpu={float(want):.7f} "
          f"diff={abs(float(loss) - float(want)):.3e} bound={bound:.3e}")
    assert abs(float(loss) - float(want)) <= bound


# ------------------------------------------------------------------------------------------------- 8. the captured train step
def test_train_one_epoch_runs_a_variant_on_the_captured_pipeline():
    """db '+m', supervisedCL Method2 through train_one_epoch: the captured pipeline against the product's eager loop
    (graph_pipeline: False) on a twin model.  Tolerances of tests/test_gpu_train_edges.py's pipeline-versus-eager comparison
    (_ragged_case, :288-306): lr = 0, so that the loss averages agree to rtol 1e-6 (_same_results, :188), every parameter
    and BatchNorm statistic after the epoch is bit-identical (_same_state, :194-196), and the gradient the optimizer read
    agrees within GRAD_BOUND = 2e-3 of each tensor's range (:39, :303)."""
    from amcontrast3d_amd import configs, timing, train
    aa = dict(configs.ambiguity_args("s3dis"), db="+m", supervisedCL="Method2")
    shapes = [(2, 1024)] * 2
    model, crit, cfg, opt = _make("sgd", 0.0, width=8, ambiguity_args=aa)
    model2, crit2, cfg2, opt2 = _make("sgd", 0.0, width=8, ambiguity_args=aa, graph_pipeline=False)
    assert cfg.ambiguity_args.db == "+m" and cfg.ambiguity_args.supervisedCL == "Method2"
    seen, seen2 = [], []
    hook = opt.register_step_pre_hook(lambda o, args, kwargs: seen.append(_grads(model)))
    with timing.count_calls() as c:
        got = train.train_one_epoch(model, _loader(shapes), crit, opt, _Probe(), None, 1, cfg)
    hook.remove()
    torch.cuda.synchronize()
    assert c["contrast_variant_forward"] >= 4 and c["contrast_forward"] == 0, dict(c)
    pipe = _the_pipeline()
    assert pipe is not None
    hook2 = opt2.register_step_pre_hook(lambda o, args, kwargs: seen2.append(_grads(model2)))
    want = train.train_one_epoch(model2, _loader(shapes), crit2, opt2, _Probe(), None, 1, cfg2)
    hook2.remove()
    torch.cuda.synchronize()
    assert len(train._PIPELINES) == 1, "graph_pipeline: False builds no pipeline"
    assert len(seen) >= 2 and len(seen2) == 2   # (building the pipeline steps the optimizer on the first batch while it warms up)
    _same_results(got, want)
    _same_state(model, model2)
    assert _grad_error(seen[-1], seen2[-1], "variant epoch, last update") <= GRAD_BOUND
