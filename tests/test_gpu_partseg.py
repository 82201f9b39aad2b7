"""Part segmentation on the GPU against what the reference's own classes computed on the CPU (tests/golden/partseg.npz,
tools/record_partseg_fixtures.py): per variant the logits in eval and train mode, the loss and the recorded gradients with the
recorded weights; the per-cloud-term route of the class-conditioned FP conv against the reference's composition on the same
weights; the route predicate; MultiSegHead and MultiShapeCrossEntropy; supplied geometry; two training iterations per head;
deterministic mode.

Tolerances.  Eval logits: 1e-5 of the recorded logits' range.  Train logits: 1e-4 of their range; the loss: 1e-4 of
max(1, |loss|) (the bound of tests/test_gpu_baseline.py).  Gradients: 4 x the deviation of the reference's own fp32 step from
the same step in fp64, measured when the fixture was recorded and stored in it (<variant>_fp64_dev; the rule of
tests/test_gpu_pointnet2.py).  Fused route against composition: 1e-4 of each tensor's range.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.utils._python_dispatch

from test_partseg_host import SEG_VARIANTS, class_conv, fixture_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
from conftest import GOLDEN  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    import json
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    z = np.load(os.path.join(GOLDEN, "partseg.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "partseg_state_keys.json")) as fh:
        d["keys"] = json.load(fh)
    return d


def _data(fix):
    return {"pos": torch.from_numpy(fix["pos"]).to(DEV), "x": torch.from_numpy(fix["x"]).to(DEV),
            "cls": torch.from_numpy(fix["cls"]).to(DEV)}


def _thinned(g):
    return g[::8] if g.numel() > 4096 else g  # as the recorder stores the wide global_conv gradients


@pytest.mark.parametrize("tag", SEG_VARIANTS)
def test_recorded_step(fix, tag):
    stride = int(fix["meta"][4])
    range_eval, range_train = (float(v) for v in fix[f"{tag}_logits_range"])
    model = fixture_model(tag, fix).to(DEV)
    model.eval()
    with torch.no_grad():
        got = model(_data(fix))
    want = fix[f"{tag}_logits_eval"]
    err = float(np.abs(got[:, :, ::stride].cpu().numpy() - want).max())
    print(f"{tag}: eval logits differ by {err:.2e} (allowed {1e-5 * range_eval:.2e})")
    loss_eval = float(got.square().mean())
    print(f"{tag}: eval loss {loss_eval:.7f} against {float(fix[f'{tag}_loss_eval']):.7f}")
    assert got.shape == (3, 50, 512) and err <= 1e-5 * range_eval
    assert abs(loss_eval - float(fix[f"{tag}_loss_eval"])) <= 1e-4

    model.train()
    logits = model(_data(fix))
    loss = logits.square().mean()
    loss.backward()
    err = float(np.abs(logits.detach()[:, :, ::stride].cpu().numpy() - fix[f"{tag}_logits_train"]).max())
    print(f"{tag}: train logits differ by {err:.2e} (allowed {1e-4 * range_train:.2e})")
    want_loss = float(fix[f"{tag}_loss"])
    print(f"{tag}: loss {float(loss.detach()):.7f} against {want_loss:.7f}")
    assert err <= 1e-4 * range_train
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    tol = 4 * float(fix[f"{tag}_fp64_dev"][2])
    grads = {k: p.grad for k, p in model.named_parameters()}
    errors = {}
    for k in fix[f"{tag}_grad_names"].tolist():
        want = fix[f"{tag}_grad::{k}"]
        scale = float(np.abs(want).max())
        assert scale > 0, k
        errors[k] = float(np.abs(_thinned(grads[k]).cpu().numpy() - want).max()) / scale
        print(f"{tag}: gradient of {k} differs by {errors[k]:.2e} of its range (allowed {tol:.2e})")
    worst = max(errors, key=errors.get)
    assert errors[worst] <= tol, worst


def _same_within(a, b, what, tol=1e-4, scale=None):
    scale = float(b.abs().max()) if scale is None else scale
    err = float((a - b).abs().max()) / scale
    print(f"{what}: {err:.2e} of the range")
    assert scale > 0 and err <= tol, what


@pytest.mark.parametrize("tag", ["pointnet2", "curvenet", "pointnext", "pointnext1", "pn2"])
def test_fused_route_against_the_composition(fix, tag, monkeypatch):
    """the same module and weights with the route declined: the class channels are expanded along the points and concatenated
    in front of the skip features, and the FP module runs as it does for any input (the parent's kernels)"""
    from openpoints.models.layers import blocks
    model = fixture_model(tag, fix).to(DEV).train()
    twin = copy.deepcopy(model)
    taken = []
    inner = blocks.cloud_term_route
    monkeypatch.setattr(blocks, "cloud_term_route", lambda *a: taken.append(inner(*a)) or taken[-1])
    got = model(_data(fix))
    assert taken == ["cloud_term"]
    monkeypatch.setattr(blocks, "cloud_term_route", lambda *a: taken.append("composition") or "composition")
    want = twin(_data(fix))
    assert taken == ["cloud_term", "composition"]
    _same_within(got, want, f"{tag} logits")
    r = torch.randn(want.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (got * r).sum().backward()
    (want * r).sum().backward()
    want_grads = {k: q.grad for k, q in twin.named_parameters()}
    for k, p in model.named_parameters():
        q = want_grads[k]
        scale = float(q.abs().max())
        gamma = want_grads.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if gamma is not None and gamma.dim() == 1:  # a BatchNorm's d(beta) is judged on d(gamma)'s scale (sums of the same
            scale = max(scale, float(gamma.abs().max()))  # terms; before another BatchNorm d(beta) cancels to ~0)
        _same_within(p.grad, q, f"{tag} {k}", scale=scale)
    for a, b in zip(model.buffers(), twin.buffers()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), "running statistics advance alike"


class _NoTensorWork(torch.utils._python_dispatch.TorchDispatchMode):
    """records every tensor operator dispatched while it is active"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen.append(str(func))
        return func(*args, **(kwargs or {}))


def test_route_predicate(fix, monkeypatch):
    from amcontrast3d_amd import _lib
    from openpoints.models.layers import cloud_term_form, cloud_term_route, create_convblock1d
    f1, f2, e = torch.rand(2, 4, 10, device=DEV), torch.rand(2, 6, 5, device=DEV), torch.rand(2, 16, device=DEV)
    norm, act = {"norm": "bn1d"}, {"act": "relu"}
    blk = create_convblock1d(26, 8, norm_args=norm, act_args=act).to(DEV)
    wide16 = create_convblock1d(16 + 4 + 6, 128, norm_args=norm, act_args=act).to(DEV)
    before, f1_host = copy.deepcopy(blk.state_dict()), f1.cpu()
    # launches nothing: no tensor operator is dispatched and the kernel library is not reached while the predicates answer
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the predicate reached the kernel library")))
        with _NoTensorWork() as mode:
            answers = (cloud_term_route(blk, f1, f2, e), cloud_term_form(blk, f1, f2, e), cloud_term_route(wide16, f1, f2, e),
                       cloud_term_route(blk, f1_host, f2, e))
    assert answers == ("cloud_term", True, "composition", "composition") and mode.seen == [], mode.seen
    with _NoTensorWork() as mode:
        f1 + 1
    assert mode.seen, "the recorder sees tensor work when there is some"
    assert cloud_term_route(blk, f1, f2, e) == "cloud_term"
    assert all(torch.equal(v, before[k]) for k, v in blk.state_dict().items()), "asking moves no statistics"
    assert cloud_term_route(create_convblock1d(26, 8, norm_args=None, act_args=act).to(DEV), f1, f2, e) == "composition"  # bias, no norm
    assert cloud_term_route(create_convblock1d(26, 8, norm_args=norm, act_args=None).to(DEV), f1, f2, e) == "composition"
    assert cloud_term_route(create_convblock1d(26, 8, norm_args=norm, act_args={"act": "gelu"}).to(DEV), f1, f2, e) == "composition"
    assert cloud_term_route(create_convblock1d(27, 8, norm_args=norm, act_args=act).to(DEV), f1, f2, e) == "composition"  # widths
    assert cloud_term_route(blk, f1.double(), f2, e) == "composition" and cloud_term_route(blk, f1, f2, e.cpu()) == "composition"
    # shape dispatch: E >= 32 or 2 E >= Cout -- the 16-way one-hot in front of a 64- or 128-wide level composes
    for E, cout, want in ((16, 32, "cloud_term"), (16, 64, "composition"), (32, 64, "cloud_term"), (32, 128, "cloud_term")):
        b = create_convblock1d(E + 4 + 6, cout, norm_args=norm, act_args=act).to(DEV)
        assert cloud_term_route(b, f1, f2, torch.rand(2, E, device=DEV)) == want, (E, cout)
    assert cloud_term_route(wide16, f1, f2, e) == "composition" and cloud_term_form(wide16, f1, f2, e)
    wide = create_convblock1d(64 + 4 + 6, 128, norm_args=norm, act_args=act).to(DEV)
    assert cloud_term_route(wide, f1, f2, torch.rand(2, 64, device=DEV)) == "cloud_term"
    for tag in SEG_VARIANTS:  # every fixture model's class-conditioned block has the form
        model = fixture_model(tag)
        dec = model.decoder
        first = (dec.FP_modules[0] if hasattr(dec, "FP_modules") else dec.decoder[0][0]).convs[0].to(DEV)
        conv = class_conv(model)
        E = {"pn2": 16, "curvenet": 208, "pointnext": 242}.get(tag, 64)
        c1 = 7 if tag == "pn2" else 8
        c2 = conv.in_channels - E - c1
        assert cloud_term_route(first, torch.rand(2, c1, 9, device=DEV), torch.rand(2, c2, 4, device=DEV), torch.rand(2, E, device=DEV)) \
            == "cloud_term", tag


def _multi_loss(fix):
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.utils import EasyConfig
    cc = EasyConfig()
    cc.update({"NAME": "MultiShapeCrossEntropy", "criterion_args": {"NAME": "CrossEntropy"}})
    crit = build_criterion_from_cfg(cc).to(DEV)
    parts = torch.from_numpy(fix["parts"].astype(np.int64)).to(DEV)
    shapes = torch.from_numpy(fix["cls"]).reshape(-1).to(DEV)
    return lambda logits: crit(logits, parts, shapes)


def test_multi_seg_head(fix):
    loss_of = _multi_loss(fix)
    model = fixture_model("multi", fix).to(DEV)
    model.eval()
    with torch.no_grad():
        logits = model(_data(fix))
        loss = float(loss_of(logits))
    assert isinstance(logits, list) and len(logits) == 16
    assert [tuple(t.shape) for t in logits] == [(3, n, 512) for n in model.head.num_parts]
    print(f"MultiShapeCrossEntropy, eval: {loss:.7f} against {float(fix['multi_loss_eval']):.7f}")
    assert abs(loss - float(fix["multi_loss_eval"])) <= 1e-4 * max(1.0, abs(float(fix["multi_loss_eval"])))
    model.train()
    loss = loss_of(model(_data(fix)))
    loss.backward()
    print(f"MultiShapeCrossEntropy, train: {float(loss):.7f} against {float(fix['multi_loss']):.7f}")
    assert abs(float(loss) - float(fix["multi_loss"])) <= 1e-4 * max(1.0, abs(float(fix["multi_loss"])))
    k = fix["multi_grad_names"].tolist()[0]
    want = fix[f"multi_grad::{k}"]
    err = float(np.abs(dict(model.named_parameters())[k].grad.cpu().numpy() - want).max()) / float(np.abs(want).max())
    print(f"gradient of {k}: {err:.2e} of its range")
    assert err <= 1e-4
    unused = dict(model.named_parameters())["head.multi_shape_heads.0.0.0.weight"].grad
    assert unused is None or float(unused.abs().max()) == 0.0, "no cloud of the batch has shape 0"


def _geometry(model, pos):
    enc = model.encoder.plan_geometry(pos)
    if isinstance(enc, dict):  # PointNet2Encoder
        clouds = [pos] + [g["new_p"] for g in enc["modules"]]
    else:
        clouds = [pos] + [stage[0]["new_p"] for stage in enc]
    return {"encoder": enc, "decoder": model.decoder.plan_geometry(clouds)}


@pytest.mark.parametrize("tag", ["curvenet", "blocks", "pn2"])
def test_supplied_geometry_gives_the_same_bits(fix, tag):
    model = fixture_model(tag, fix).to(DEV).eval()
    data = _data(fix)
    with torch.no_grad():
        a = model(dict(data))
        b = model({**data, "_geometry": _geometry(model, data["pos"])})
        c = model(data["pos"], data["x"], data["cls"])  # the positional form
    assert torch.equal(a, b) and torch.equal(a, c)
    if tag == "blocks":
        plan = model.decoder.plan_geometry(model.encoder.forward_seg_feat(data["pos"], data["x"])[0])
        assert sorted(plan) == [-3, -2, -1, 0] and [len(plan[i]["blocks"]) for i in (0, -3, -2, -1)] == [1, 1, 0, 0]
        assert plan[0]["blocks"][0]["idx"].shape[:2] == (3, 512) and plan[-3]["blocks"][0]["idx"].shape[:2] == (3, 256)


def _loader(B, N, with_y_parts=50, batches=2, seed=4):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batches):
        pos = rng.uniform(0, 0.7, (B, N, 3)).astype(np.float32)
        out.append({"pos": torch.from_numpy(pos), "x": torch.from_numpy(rng.uniform(-1, 1, (B, N, 4)).astype(np.float32)),
                    "cls": torch.from_numpy(rng.integers(0, 16, (B, 1))), "y": torch.from_numpy(rng.integers(0, with_y_parts, (B, N)))})
    return out


@pytest.mark.parametrize("tag", ["curvenet", "pn2"])
def test_two_iterations_of_train_one_epoch(fix, tag):
    """SegHead + CrossEntropy with a 'cls' key in the batch: the eager loop of train_one_epoch, every parameter moves"""
    from amcontrast3d_amd import train
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    train.release_pipelines()
    torch.manual_seed(1)
    model = fixture_model(tag).to(DEV)
    cc = EasyConfig()
    cc.update({"NAME": "CrossEntropy"})
    crit = build_criterion_from_cfg(cc).to(DEV)
    cfg = EasyConfig()
    cfg.update({"num_classes": 50, "ignore_index": None, "feature_keys": "pos,x", "use_amp": False, "step_per_update": 1,
                "grad_norm_clip": 10, "sched_on_epoch": False, "criterion_args": {"NAME": "CrossEntropy"}})
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=1e-4)

    class Sched:
        calls = 0

        def step(self, epoch):
            Sched.calls += 1
    before = [p.detach().clone() for p in model.parameters()]
    out = train.train_one_epoch(model, _loader(3, 512), crit, opt, Sched(), None, 1, cfg)
    torch.cuda.synchronize()
    assert not train._PIPELINES, "part models train in the eager loop"
    assert np.isfinite(out[0]) and Sched.calls == 2
    unmoved = [k for (k, p), q in zip(model.named_parameters(), before) if torch.equal(p.detach(), q)]
    assert not unmoved, unmoved


def test_two_steps_with_multi_seg_head(fix):
    """MultiSegHead + MultiShapeCrossEntropy in a hand-written loop: the encoder, the decoder and the heads of the shapes in
    the batches move; the other heads get no gradient"""
    from openpoints.optim import build_optimizer_from_cfg
    torch.manual_seed(2)
    model = fixture_model("multi").to(DEV).train()
    loss_of = _multi_loss(fix)
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=0)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = loss_of(model(_data(fix)))
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(v) for v in losses)
    shapes = set(fix["cls"].reshape(-1).tolist())
    for k, p in model.named_parameters():
        head = int(k.split(".")[2]) if k.startswith("head.multi_shape_heads.") else None
        moved = not torch.equal(p.detach(), before[k])
        assert moved == (head is None or head in shapes), k


def test_deterministic_mode_repeats_the_bits(fix):
    """with 32 neighbours, where every SetAbstraction layer has a deterministic route (at the fixture's 16 the gather + conv
    kernel's backward scatters with float atomics and raises in this mode, as tests/test_gpu_pointnet2.py notes); the
    recorded weights fit: no shape depends on nsample"""
    from amcontrast3d_amd import ops
    runs = []
    for _ in range(2):
        model = fixture_model("pointnext", fix, nsample=32).to(DEV).train()
        with ops.deterministic_mode():
            logits = model(_data(fix))
            logits.square().mean().backward()
        runs.append([logits.detach()] + [p.grad for p in model.parameters()])
    assert all(g is not None for g in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
