"""Deterministic mode at the widths without a power-of-two row kernel: contrast_backward_rows_wide_kernel (csrc/loss.hip),
any C % 4 == 0 up to 512 -- the 512-wide loss stage of PointNeXt-XL at its shipped width 64 among them.

The references, inputs and bounds are those of tests/test_gpu_contrast_fp64.py (default form) and
tests/test_gpu_contrast_variants.py (every other form), imported: per row, max_c |got - df64| <= 4 * rho32 * A_n, rows no edge
touches exactly zero.  The float-atomic kernels meet the same bound at these widths in those files.

WIDE: 20 = one float4 piece per lane with 5 live lanes; 260 = a second piece with one live lane; 384 = a half-full second
piece; 512 = both pieces full.  Default mode must not change: at 512 it still launches the atomic kernels."""
import copy

import pytest
import torch

import test_gpu_contrast_fp64 as tf
import test_gpu_contrast_variants as tv
import test_gpu_deterministic as td
from amcontrast3d_amd.timing import count_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE = (20, 260, 384, 512)


def _ops():
    return td._ops()


def _stage(f, G, a, posmask, prm, extra):
    """forward + backward of ops.contrast_stage -> (loss, gradient, call counts)"""
    ops, _, _ = _ops()
    fg = f.clone().requires_grad_(True)
    with count_calls() as c:
        loss = ops.contrast_stage(fg, G.nidx, posmask, a, *prm, *extra)
        (loss * tf.GRAD_OUT).backward()
    return loss.detach(), fg.grad, dict(c)


def _inputs(plan):
    """lists from the plan; anchors only (the lists are built in backward); the mutual-edge plan, whose lists hold the
    non-mutual edges only and must not reach the gather: ContrastStage drops them and builds the lists of all edges"""
    anchors, rev_csr, mutual, rev_m = plan
    out = {"plan": (anchors, rev_csr), "anchors": (anchors,)}
    if mutual is not None:
        out["mutual"] = (anchors, rev_m, mutual)
    return out


def _against_fp64(G, kind, C, params):
    ops, _, _ = _ops()
    f, a = tf.features(G, kind, C)
    plan = G.plan(a)
    with ops.deterministic_mode():
        for prm in params:
            ref = tf.Ref(f, G, a, G.posmask, prm)
            for name, extra in _inputs(plan).items():
                loss, grad, c = _stage(f, G, a, G.posmask, prm, extra)
                assert c.get("contrast_backward_csr", 0) == 1 and c.get("contrast_backward", 0) == 0, (name, c)
                assert c.get("contrast_csr", 0) == (0 if name == "plan" else 1), (name, c)
                ref.check(f"wide graph={G.name} k={G.k} feat={kind} C={C} prm={prm} input={name}", loss, grad, factor=4)
    return f, a


# ------------------------------------------------------------------------------------------------------------ A. predicates
def test_predicates():
    _, _, lib = _ops()
    for C in range(0, 1030):
        assert bool(lib.amc3d_contrast_backward_csr_supported(C)) == (C in (16, 32, 64, 128, 256)), C
    for C in (20, 512):
        assert not lib.amc3d_contrast_backward_csr_supported(C)
    for C in (4, 16, 20, 260, 384, 512):
        assert lib.amc3d_contrast_backward_rows_supported(C), C
    for C in (0, 2, 33, 514, 516, 1024, -4):
        assert not lib.amc3d_contrast_backward_rows_supported(C), C


# ------------------------------------------------------------------------------------------ B. the default form against fp64
@pytest.mark.parametrize("C", WIDE)
@pytest.mark.parametrize("kind", ["gauss", "parallel"])
@pytest.mark.parametrize("name", ["room", "crafted"])
def test_wide_rows_against_fp64(name, kind, C):
    G = tf.graph(name)
    tf._assert_branches(G)
    assert G.k == 23 and G.nidx.stride(0) in (23, 24)
    _against_fp64(G, kind, C, tf.PARAMS)


@pytest.mark.parametrize("C", [260, 512])
@pytest.mark.parametrize("name", ["room", "crafted"])
def test_wide_rows_zero_and_clamped_rows(name, C):
    G = tf.graph(name)
    f, a = _against_fp64(G, "degenerate", C, [tf.PARAMS[0]])
    assert int((torch.linalg.vector_norm(f, dim=1) < 1e-8).sum()) == 10


@pytest.mark.parametrize("k", [1, 23, 64])
def test_wide_rows_neighbourhood_sizes(k):
    G = tf.graph("room", k)
    assert G.nidx.shape[1] == k
    _against_fp64(G, "gauss", 512, [tf.PARAMS[k % 3]])


@pytest.mark.parametrize("selection", ["none", "all"])
@pytest.mark.parametrize("C", [260, 512])
def test_wide_rows_selections(C, selection):
    """m = 257: no multiple of the 4-row workgroup.  No anchor selected: a NaN loss (the mean of nothing) and a gradient of
    exact zeros, as the fp64 reference's"""
    ops, _, _ = _ops()
    m = 257
    G = tf._small_graph(m, 23, 500 + m)
    a = torch.full((m,), 0.4)
    if selection == "none":
        a[:] = 0.0
        a[::2] = -0.25
        a[1::3] = tf.A_ABOVE_ONE
    a = a.to(DEV)
    assert int(tf._keep(a).sum()) == (0 if selection == "none" else m)
    f, _ = tf.features(G, "gauss", C)
    ref = tf.Ref(f, G, a, G.posmask, tf.PARAMS[0])
    plan = G.plan(a)
    with ops.deterministic_mode():
        for name, extra in _inputs(plan).items():
            loss, grad, c = _stage(f, G, a, G.posmask, tf.PARAMS[0], extra)
            assert c.get("contrast_backward_csr", 0) == 1 and c.get("contrast_backward", 0) == 0, (name, c)
            if selection == "none":
                assert bool(torch.isnan(ref.loss64)) and bool((ref.df64 == 0).all())
                assert bool(torch.isnan(loss)), name
                assert bool((grad == 0).all()) and not bool(torch.signbit(grad).any()), name
            else:
                ref.check(f"wide graph=random m={m} sel=all C={C} input={name}", loss, grad, factor=4)


# ------------------------------------------------------------------------------------------------------ C. the variant forms
@pytest.mark.parametrize("C", [260, 512])
def test_wide_rows_variant_forms(C):
    ops, _, _ = _ops()
    X = tv.make_input(331, 23, C)
    with ops.deterministic_mode():
        for form in tv.SIX_FORMS:
            ref = tv.Ref(X.f, X.nidx, X.posmask, X.a, form)
            with count_calls() as c:
                loss, loss_pt, grad = tv.run_variant(X, form, "rows")
            assert c.get("contrast_variant_backward_csr", 0) == 1 and c.get("contrast_variant_backward", 0) == 0, dict(c)
            ref.check(f"wide form={tv.form_id(form)} m={X.m} k={X.k} C={C} route=rows", loss_pt, grad, factor=4)


# ------------------------------------------------------------------------------------------------- D. bits and boundaries
@pytest.mark.parametrize("C", [260, 512])
def test_wide_rows_repeat_bit_for_bit_and_built_lists_equal_planned_ones(C):
    ops, _, _ = _ops()
    G = tf.graph("crafted")
    f, a = tf.features(G, "gauss", C)
    ins = _inputs(G.plan(a))
    with ops.deterministic_mode():
        runs = [_stage(f, G, a, G.posmask, tf.PARAMS[1], ins["plan"]) for _ in range(3)]
        built = _stage(f, G, a, G.posmask, tf.PARAMS[1], ins["anchors"])
        fallen = _stage(f, G, a, G.posmask, tf.PARAMS[1], ins["mutual"])
    assert float(runs[0][1].abs().max()) > 0
    for loss, grad, _ in runs[1:] + [built, fallen]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(grad, runs[0][1])


def test_default_mode_keeps_the_atomic_kernels_at_512():
    ops, _, _ = _ops()
    ops.set_deterministic(False)
    G = tf.graph("room")
    f, a = tf.features(G, "gauss", 512)
    anchors, rev_csr, mutual, rev_m = G.plan(a)
    with ops.deterministic_mode():
        _, _, c = _stage(f, G, a, G.posmask, tf.PARAMS[0], (anchors, rev_csr))
    assert c.get("contrast_backward_csr", 0) == 1 and c.get("contrast_backward", 0) == 0, c
    assert not ops.deterministic()
    for extra in ((anchors, rev_csr), (anchors, rev_m, mutual)):
        _, _, c = _stage(f, G, a, G.posmask, tf.PARAMS[0], extra)
        assert c.get("contrast_backward", 0) == 1 and c.get("contrast_backward_csr", 0) == 0, c
    X = tv.make_input(331, 23, 512)
    with count_calls() as c:
        tv.run_variant(X, tv.SIX_FORMS[0], "rows")
    assert c.get("contrast_variant_backward", 0) == 1 and c.get("contrast_variant_backward_csr", 0) == 0, dict(c)


def test_a_width_outside_the_row_kernels_still_raises():
    ops, _, _ = _ops()
    G = tf.graph("room")
    f, a = tf.features(G, "gauss", 33)
    anchors, rev_csr, _, _ = G.plan(a)
    X = tv.make_input(331, 23, 33)
    with ops.deterministic_mode():
        with pytest.raises(RuntimeError, match=r"contrast_backward: no deterministic route .*does not cover 33 channels"):
            _stage(f, G, a, G.posmask, tf.PARAMS[0], (anchors, rev_csr))
        with pytest.raises(RuntimeError, match=r"contrast_variant_backward: no deterministic route .*does not cover 33 channels"):
            tv.run_variant(X, tv.SIX_FORMS[0], "rows")


def test_misaligned_rows_raise_on_the_variant_route():
    """features that start 4 bytes into an allocation: contiguous, but no row is 16-byte aligned"""
    ops, _, _ = _ops()
    X = tv.make_input(331, 23, 512)
    anchors, rev = X.plan()
    form = tv.SIX_FORMS[0]
    base = torch.zeros(X.m * X.C + 1, device=DEV)
    base[1:] = X.f.flatten()
    base.requires_grad_(True)
    fg = base[1:].view(X.m, X.C)
    assert fg.is_contiguous() and fg.data_ptr() % 16 == 4
    with ops.deterministic_mode():
        loss = ops.contrast_stage_variant(fg, X.nidx, X.posmask, X.a, *form[:3], tv.MU, tv.NU, form[3], anchors, rev)
        with pytest.raises(RuntimeError, match=r"contrast_variant_backward: no deterministic route .*16-byte aligned rows"):
            loss.backward()


# ------------------------------------------------------------------------------------------------------------ E. whole step
def _build(kind):
    """the shipped models at their shipped width 64 (loss stages 64, 128, 256 and 512 wide): 'XL' AMContrast3D-AA, 'MM'
    AMContrast3D++ (both PointNeXt-XL, blocks [1,4,7,4,4]); 'L64' a shallow model of the same widths"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import configs
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(0)
    c = EasyConfig()
    if kind == "XL":
        c.update(configs.model_cfg("XL", dropout=0))
    elif kind == "MM":
        c.update(configs.model_cfg_mm(dropout=0, threshold=0.5))
    else:
        c.update(configs.model_cfg("L", dropout=0, width=64, blocks=[1, 2, 2, 2, 2]))
    assert c["encoder_args"]["width"] == 64
    if kind != "L64":
        assert list(c["encoder_args"]["blocks"]) == [1, 4, 7, 4, 4]
    model = build_model_from_cfg(c).to(DEV).train()
    cc = EasyConfig()
    cc.update(configs.criterion_cfg_mm() if kind == "MM" else configs.criterion_cfg())
    crit = build_criterion_from_cfg(cc).to(DEV)
    aa = EasyConfig()
    aa.update(configs.ambiguity_args_mm("s3dis") if kind == "MM" else configs.ambiguity_args("s3dis"))
    return model, crit, aa


@pytest.mark.parametrize("kind", ["XL", "MM"])
def test_a_train_step_of_the_shipped_xl_has_the_same_bits_on_every_run(kind):
    """2 x 2048 points: the coarsest loss stage is 64 rows x 512 channels"""
    ops, _, _ = _ops()
    ops.set_deterministic(False)
    model, crit, aa = _build(kind)
    state = copy.deepcopy(model.state_dict())
    data = td._batch(2, 2048, 60)
    runs, counts = [], []
    with ops.deterministic_mode():
        for _ in range(3):
            model.load_state_dict(state)
            with count_calls() as c:
                runs.append(td._step(model, crit, aa, dict(data), kind == "MM"))
            counts.append(dict(c))
    for loss, logits, grads in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(logits, runs[0][1])
        for a, b in zip(grads, runs[0][2]):
            assert (a is None and b is None) or torch.equal(a, b)
    assert sum(g is not None for g in runs[0][2]) > 10 and bool(torch.isfinite(runs[0][0]))
    c = counts[0]
    assert counts[1] == c and counts[2] == c
    assert c.get("contrast_backward_csr", 0) + c.get("contrast_variant_backward_csr", 0) >= 1, c
    assert c.get("contrast_variant_backward", 0) == 0, c
    for old in ("library_gemm_conv", "three_interpolate_grad", "local_aggregation_backward", "masked_refine_backward",
                "grouped_conv_backward", "group_points_grad"):
        assert c.get(old, 0) == 0, (old, c)
    with count_calls() as c0:  # default mode after leaving the block: the atomic entries again
        td._step(model, crit, aa, dict(data), kind == "MM")
    assert c0.get("contrast_backward_csr", 0) == 0 and c0.get("contrast_variant_backward_csr", 0) == 0, dict(c0)
    assert c0["three_interpolate_grad"] == 4


# -------------------------------------------------------------------------------------------------------------- F. captured
def test_captured_epochs_at_width_64_end_in_the_same_state():
    ops, _, _ = _ops()
    from amcontrast3d_amd import train
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    ops.set_deterministic(False)
    model, crit, aa = _build("L64")
    cfg = EasyConfig()
    cfg.update({"num_classes": 13, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
                "ambiguity_args": aa, "grad_norm_clip": 10, "sched_on_epoch": False, "fps_lanes": 2, "deterministic": True})

    class Sched:
        def step(self, epoch):
            pass

    def loader():
        out = []
        for k in range(4):
            d = td._batch(2, 2048, 80 + 2 * k)  # resident batches
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
            assert len(train._PIPELINES) == 1 and all(k[-1] is True for k in train._PIPELINES)
            train.release_pipelines()
        for a, b in zip(ends[0], ends[1]):
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]), k
        moved = max(float((ends[0][1][k].float() - m0[k].float()).abs().max()) for k in m0)
        assert moved > 0
    finally:
        train.release_pipelines()
