"""ops.contrast_stages_cm -- every stage of the contrast loss in one call, the gradient written channel-major -- against the
per-stage route, bit for bit.

The reference is the route the fp64 tests hold (tests/test_gpu_contrast_fp64.py): ops.contrast_stage_cm per stage, the
Python sum of ContrastHead.forward, the loss weight as a Python product, backward().  The merged call promises the same
bits for the total, for every stage's mean and for every gradient element, so everything is compared as int32 patterns:
no tolerance, a NaN equals the same NaN.

Plans are built as the model builds them: ops.knnquery_squared per cloud (the self match dropped as a view),
ops.posmask_from_labels, the ambiguity of AEF.ambiguity_function, ops.select_anchors, ops.contrast_mutual.  Every cloud has
n > k + 2 points.  Shapes: every width of the row kernels; n = 70, 100, 257 (no multiple of a 16-, 32- or 64-point tile of
the unit rows; the gradient's tiles are 16, 8 and 4 points: 70 and 257 are multiples of none, and 256 channels, the 4-point
width, also run at n = 70) and n = 10 (shorter than most tiles, no multiple of 4); B = 3, so tiles end at cloud boundaries;
k = 24 and k = 5.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRM = (-1.0, 0.5, 0.3)  # mu, nu, temperature
B = 3


class Stage:
    """one loss stage: B clouds of n random points, k neighbours, C channels.  select: 'mixed' (the ambiguity function's
    values, every fifth anchor set to 0), 'none' (no anchor has 0 < a <= 1) or 'all'.  clump: a third of the first cloud
    sits in a ball of radius 1e-3, so the rows of the clump are named by many lists they do not name back."""

    def __init__(self, C, n, k, seed, select="mixed", clump=False):
        import amcontrast3d_amd
        amcontrast3d_amd.activate()
        from amcontrast3d_amd import configs, ops
        from openpoints.AMContrast3D.AEF.ambiguity import ambiguity_function
        assert n > k + 2
        g = torch.Generator().manual_seed(seed)
        p = torch.rand(B * n, 3, generator=g)
        if clump:
            c = max(n // 3, 2)
            p[:c] = p[0] + 1e-3 * torch.rand(c, 3, generator=g)
        self.C, self.n, self.k, self.m = C, n, k, B * n
        self.p = p.to(DEV)
        self.offset = (torch.arange(1, B + 1, dtype=torch.int32) * n).to(DEV)
        idx, _ = ops.knnquery_squared(k + 1, self.p, self.p, self.offset, self.offset)
        self.nidx = idx[:, 1:]  # a strided view, as the plan holds it
        lab = torch.randint(0, 4, (self.m,), generator=g, dtype=torch.int32).to(DEV)
        self.posmask = ops.posmask_from_labels(lab, self.nidx)
        aa = configs.ambiguity_args("s3dis")
        a, _ = ambiguity_function(self.p, self.posmask, k, self.nidx, aa["cctype"], aa["ccbeta"], aa["vis"], aa["nu"])
        a = a.clone()
        if select == "mixed":
            a[::5] = 0.0
        elif select == "none":
            a.zero_()
        else:
            a.fill_(0.5)
        self.a = a.contiguous()
        keep = (0 < self.a) & (self.a <= 1)
        self.selected = int(keep.sum())
        assert {"none": self.selected == 0, "all": self.selected == self.m}.get(select, 0 < self.selected < self.m)
        self.anchors = ops.select_anchors(self.a)
        self.mutual, self.rev = ops.contrast_mutual(self.nidx, self.a)
        self.f_cm = torch.randn(B, C, n, generator=g).to(DEV)
        if clump:  # (from the plan alone) a row with several non-mutual incoming edges; with k = 24, more than k of them
            deg = (self.rev[1:self.m + 1] - self.rev[:self.m]).max()
            assert int(deg) >= (12 if k == 24 else 2), int(deg)

    def plan(self):
        return (self.nidx, self.posmask, self.a, self.anchors, self.rev, self.mutual)


@functools.lru_cache(None)
def stage(C, n, k, seed=0, select="mixed", clump=False):
    return Stage(C, n, k, 1000 * C + 10 * n + k + seed, select, clump)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = bits(got) != bits(want)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits"


def per_stage(stages, scale, grad_out, embeddings=None):
    """the reference route -> (total, [stage losses], [gradients])"""
    from amcontrast3d_amd import ops
    fs = [(s.f_cm if e is None else e).clone().requires_grad_(True) for s, e in zip(stages, embeddings or [None] * len(stages))]
    loss_sum, losses = 0, []
    for s, f in zip(stages, fs):
        nidx, posmask, a, anchors, rev, mutual = s.plan()
        loss = ops.contrast_stage_cm(f, nidx, posmask, a, *PRM, anchors, rev, mutual)
        losses.append(loss.detach().clone())
        loss_sum += loss
    total = scale * loss_sum
    total.backward(torch.tensor(grad_out, device=DEV))
    return total.detach(), losses, [f.grad for f in fs]


def merged(stages, scale, grad_out, embeddings=None):
    from amcontrast3d_amd import ops
    fs = [(s.f_cm if e is None else e).clone().requires_grad_(True) for s, e in zip(stages, embeddings or [None] * len(stages))]
    total, means = ops.contrast_stages_cm([(f, *s.plan()) for s, f in zip(stages, fs)], *PRM, scale)
    assert not means.requires_grad
    total.backward(torch.tensor(grad_out, device=DEV))
    return total.detach(), means, [f.grad for f in fs]


def check(stages, scale, grad_out, tag):
    want_total, want_losses, want_grads = per_stage(stages, scale, grad_out)
    total, means, grads = merged(stages, scale, grad_out)
    same_bits(f"{tag} total", total, want_total)
    for i, s in enumerate(stages):
        same_bits(f"{tag} stage {i} mean", means[i, 0], want_losses[i])
        assert float(means[i, 1]) == s.selected, (tag, i)
        assert grads[i].shape == (B, s.C, s.n) and grads[i].is_contiguous(), (tag, i)
        same_bits(f"{tag} stage {i} C={s.C} n={s.n} k={s.k} gradient", grads[i], want_grads[i])
    return total, grads


# every width, every n, both k, both scales; the clumps bring rows with many non-mutual incoming edges
ONE_STAGE = [(16, 70, 24, False), (16, 257, 5, True), (32, 100, 24, True), (32, 10, 5, False), (64, 257, 24, False),
             (64, 100, 5, True), (128, 70, 5, True), (128, 257, 24, False), (256, 100, 24, True), (256, 10, 5, False),
             (256, 70, 5, False)]


@pytest.mark.parametrize("C,n,k,clump", ONE_STAGE)
def test_one_stage_equals_the_per_stage_route(C, n, k, clump):
    s = stage(C, n, k, clump=clump)
    scale = 1.0 if (C // 16 + n) % 2 else 0.1
    total, grads = check([s], scale, 0.7, f"one stage scale={scale}")
    assert bool(torch.isfinite(total)) and float(grads[0].abs().max()) > 0


FOUR = ((32, 257, 24), (64, 100, 24), (128, 70, 5), (256, 10, 5))
TWO = ((16, 70, 24), (256, 100, 24))


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("shapes", [TWO, FOUR], ids=["two", "four"])
@pytest.mark.parametrize("scale,grad_out", [(1.0, 1.0), (0.1, 0.7)])
def test_mixed_widths_in_one_call(shapes, order, scale, grad_out):
    stages = [stage(*s) for s in (shapes if order == "ascending" else shapes[::-1])]
    total, _ = check(stages, scale, grad_out, f"{len(stages)} stages {order}")
    assert bool(torch.isfinite(total))


def test_eight_stages_fill_the_descriptor():
    stages = [stage(*s, seed=i) for i, s in enumerate(FOUR + TWO + ((16, 10, 5), (64, 70, 24)))]
    check(stages, 0.1, 0.7, "eight stages")


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_stage_without_a_selected_anchor_gives_nan_and_a_zero_gradient(where):
    stages = [stage(32, 100, 24), stage(64, 70, 5), stage(128, 10, 5)]
    stages[where] = stage(stages[where].C, stages[where].n, stages[where].k, select="none")
    total, grads = check(stages, 0.1, 0.7, f"empty stage {where}")
    assert bool(torch.isnan(total))
    assert not bool(grads[where].any()), "the stage without anchors has an all-zero gradient"
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for i, g in enumerate(grads) if i != where)


def test_every_anchor_selected():
    stages = [stage(16, 70, 24, select="all"), stage(256, 100, 24, select="all"), stage(64, 10, 5, select="all")]
    total, _ = check(stages, 1.0, 0.7, "all selected")
    assert bool(torch.isfinite(total))


# ------------------------------------------------------------------------------------------------------------- the head
def _head_case(widths, ns=(40, 30, 20, 12), k=5):
    """-> (head, args, stages, make_list): make_list() builds a fresh stageACE_list over new leaf embeddings"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import configs
    from openpoints.AMContrast3D.MarginContrast import ContrastHead
    from openpoints.models.backbone.pointnext_AA import _Stage
    from openpoints.utils import EasyConfig
    stages = []
    for C, n in zip(widths, ns):
        s = stage(min(C, 256), n, k, seed=7)
        if C > 256:  # a width without row kernels on the plan of a supported one
            s = _Wide(s, C)
        stages.append(s)
    args = EasyConfig()
    args.update(dict(configs.ambiguity_args("s3dis"), nsample=k + 1, stages_num=len(stages)))
    plans = [dict(neighbor_idx=s.nidx, posmask=s.posmask, ambiguity=s.a, anchors=s.anchors, rev=s.rev, mutual=s.mutual,
                  shares=None) for s in stages]

    def make_list():
        leaves, up = [], []
        for s in stages:
            f = s.f_cm.clone().requires_grad_(True)
            entry = _Stage(s.p, None, s.offset)
            entry.set_features(f)
            leaves.append(f)
            up.append(entry)
        return {"up": up, "down": up, "geometry": {"loss": plans}}, leaves

    return ContrastHead(), args, stages, make_list


class _Wide:
    def __init__(self, s, C):
        self.__dict__.update(s.__dict__)
        self.C = C
        self.f_cm = torch.randn(B, C, s.n, generator=torch.Generator().manual_seed(C)).to(DEV)


def _loop_over_stages(head, args, make_list, scale):
    """ContrastHead.forward as it was: one point_contrast_margin per stage, added up in Python"""
    stage_list, leaves = make_list()
    loss_sum = 0
    for i in range(args.stages_num):
        loss, _, _ = head.point_contrast_margin(args.stages, i, stage_list, None, 13, None, args)
        loss_sum += loss
    total = scale * loss_sum
    total.backward()
    return total.detach(), [f.grad for f in leaves]


def test_the_head_hands_every_stage_to_one_call():
    from amcontrast3d_amd import timing
    head, args, stages, make_list = _head_case((32, 64, 128, 256))
    want_total, want_grads = _loop_over_stages(head, args, make_list, args.w2)
    stage_list, leaves = make_list()
    with timing.count_calls() as c:
        total, ai_cat, ai_list = head(None, None, stage_list, 13, None, args, scale=args.w2)
        total.backward()
    assert c["contrast_stages_forward"] == 1 and c["contrast_stages_backward"] == 1, dict(c)  # one call each way ...
    assert c["contrast_forward"] == 4 and c["contrast_backward"] == 4, dict(c)                # ... counted once per stage
    same_bits("head total", total, want_total)
    for i, (f, w) in enumerate(zip(leaves, want_grads)):
        same_bits(f"head stage {i} gradient", f.grad, w)
    assert len(ai_list) == 4 and all(a is s.a for a, s in zip(ai_list, stages)) and ai_cat.numel() == sum(s.m for s in stages)
    # without a weight the head returns the plain sum
    stage_list, _ = make_list()
    plain, _, _ = head(None, None, stage_list, 13, None, args)
    same_bits("head sum", plain, _loop_over_stages(head, args, make_list, 1.0)[0])


def test_a_last_stage_of_512_channels_keeps_its_route():
    from amcontrast3d_amd import ops, timing
    head, args, stages, make_list = _head_case((64, 128, 256, 512))
    with ops.deterministic_mode():  # (the 512-wide stage then gathers too: both runs have one summation order)
        want_total, want_grads = _loop_over_stages(head, args, make_list, args.w2)
        stage_list, leaves = make_list()
        with timing.count_calls() as c:
            total, _, ai_list = head(None, None, stage_list, 13, None, args, scale=args.w2)
            total.backward()
    assert c["contrast_stages_forward"] == 1 and c["contrast_forward"] == 3 + 1, dict(c)  # one call for the first three stages
    assert c["contrast_backward"] == 3 and c["contrast_backward_csr"] == 1, dict(c)       # the last on its gather route
    same_bits("head total", total, want_total)
    for i, (f, w) in enumerate(zip(leaves, want_grads)):
        same_bits(f"head stage {i} gradient", f.grad, w)
        assert f.grad.shape == (B, stages[i].C, stages[i].n)
    assert len(ai_list) == 4


# ------------------------------------------------------------------------------------------------------------- capture
def test_captured_forward_and_backward_replay_with_new_embeddings():
    from amcontrast3d_amd import ops
    stages = [stage(*s) for s in FOUR]
    static = [s.f_cm.clone().requires_grad_(True) for s in stages]

    def step():
        for f in static:
            f.grad = None
        total, _ = ops.contrast_stages_cm([(f, *s.plan()) for s, f in zip(stages, static)], *PRM, 0.1)
        total.backward()
        return total

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total = step()
    grads = [f.grad for f in static]
    for it in range(2):
        new = [torch.randn(s.f_cm.shape, generator=torch.Generator().manual_seed(50 + 10 * it + i)).to(DEV)
               for i, s in enumerate(stages)]
        with torch.no_grad():
            for f, e in zip(static, new):
                f.copy_(e)
        graph.replay()
        want_total, _, want_grads = merged(stages, 0.1, 1.0, new)
        same_bits(f"replay {it} total", total, want_total)
        for i, (g, w) in enumerate(zip(grads, want_grads)):
            same_bits(f"replay {it} stage {i} gradient", g, w)


# ------------------------------------------------------------------------------------------------------- bad arguments
def _descs(stages, **override):
    """the forward's descriptors over fresh buffers, `override` applied to the last stage -> (descs, buffers kept alive)"""
    from amcontrast3d_amd import ops
    out, keep = [], []
    for s in stages:
        e = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=DEV)  # noqa: E731
        nidx = s.nidx
        d = dict(b=B, C=s.C, n=s.n, k=s.k, nbr_stride=nidx.stride(0), f_cm=s.f_cm, nbr=nidx, posmask=s.posmask, a=s.a,
                 sel=s.anchors, mutual=s.mutual, rev=s.rev, norm=e(s.m), unit=e(s.m, s.C), stats=e(s.m, 2), loss_pt=e(s.m),
                 mean_cnt=e(2), grad_cm=e(B, s.C, s.n))
        out.append(d)
        keep.append(d)
    out[-1] = dict(out[-1], **override)
    return ops._contrast_stage_descs(out), keep


@pytest.mark.parametrize("case", ["misaligned", "width24", "nine"])
def test_bad_arguments_are_refused_before_any_launch(case):
    from amcontrast3d_amd import _lib, ops
    lib = _lib.load()
    good = [stage(32, 100, 24), stage(64, 70, 5)]
    if case == "misaligned":
        flat = torch.zeros(B * 64 * 70 + 1, dtype=torch.float32, device=DEV)
        descs, keep = _descs(good, f_cm=flat[1:])
        nst = 2
    elif case == "width24":
        descs, keep = _descs(good, C=24)
        nst = 2
    else:
        descs, keep = _descs([stage(16, 10, 5)] * 9)
        nst = 9
    total = torch.full((), -7.0, dtype=torch.float32, device=DEV)
    status = lib.amc3d_contrast_stages_forward_cm(nst, descs, *PRM, 1.0, ops._ptr(total), ops._stream(total))
    assert status != 0 and b"amc3d_contrast_stages_forward_cm" in lib.amc3d_last_error()
    if case != "misaligned":  # (the backward does not read f_cm)
        work = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        g = torch.ones(1, device=DEV)
        status = lib.amc3d_contrast_stages_backward_cm(nst, descs, *PRM, 1.0, ops._ptr(g), ops._ptr(work), work.numel(),
                                                       ops._stream(total))
        assert status != 0 and b"amc3d_contrast_stages_backward_cm" in lib.amc3d_last_error()
    torch.cuda.synchronize()
    assert float(total) == -7.0
    for d in keep:  # nothing ran: every buffer of every stage, the good first stage's included, is as it was
        for name in ("norm", "unit", "stats", "loss_pt", "mean_cnt", "grad_cm"):
            assert bool((d[name] == -7.0).all()), (case, name)
    if case == "nine":
        with pytest.raises(ValueError):
            ops.contrast_stages_cm([(s.f_cm, *s.plan()) for s in [stage(16, 10, 5)] * 9], *PRM)
    assert lib.amc3d_contrast_stages_forward_cm(0, None, *PRM, 1.0, None, None) == 0
