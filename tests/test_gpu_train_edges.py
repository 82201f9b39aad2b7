"""train.train_one_epoch / train_one_epoch_mm on the routes of `_run_epoch` that tests/test_gpu_train.py never takes: a learning-rate
schedule on a captured torch optimizer, a ragged last batch followed by another epoch, the first batch of a later epoch, gradient
accumulation, use_amp with a GradScaler, an empty loader and a loader whose only batch is the odd one.

The reference in every test is the hand-written loop of test_gpu_train.py::test_train_one_epoch_matches_hand_written_loop
(`_hand_loop`: model, criterion, backward, clip_grad_norm_, opt.step(), opt.zero_grad(), scheduler.step(epoch); no pipeline, no
prefetcher) on a second, identically seeded model -- never the pipeline against itself.  Assertions are exact by construction
wherever the arithmetic allows it:

  * lr = 0 freezes the weights (SGD: p - 0 * g; Adam / AdamW: decay factor 1 - 0 * wd = 1, step size 0), so logits, confusion
    matrix and BatchNorm statistics are bit-identical between the loops and "a parameter moved" / "no parameter moved" are
    bit-wise statements;
  * gradients are compared with the bound of test_gpu_graph_pipeline.py::test_every_variants_gradient_reaches_the_static_tensors,
    2e-3 of each tensor's range (the interpolation backward adds rows with float atomics in BOTH loops), with its companion
    assertion that the gradients of two consecutive updates differ by more than 5e-2 of range -- a leftover or missing
    gradient cannot hide inside the bound.

Epochs with lr > 0 on the eager routes are compared update by update, not at their end.  Measured on the MI355X, the
hand-written loop run twice from the same seed ends one epoch 2.7e-2 of a tensor's range apart from ITSELF with gradient
accumulation (3 updates, which moved the parameters by 0.64 of range) and 2.2e-1 apart under bf16 autocast (3 updates, 0.38):
the atomic order differs from run to run, the next forward pass carries the rounding on and a max-pool pick or ReLU mask flips.
Ten times that spread is no allowance a skipped update would land a hundred times above, so there is none: before each of its
updates the hand-written loop is given the weights the product had before ITS update of the same number, and the two
applied updates (weights after - weights before) are compared -- a one-step statement with the gradient bound above, plus two
ulps of the parameter (p - lr * g is rounded to fp32 in both loops); measured: 8.5e-5 of an update's range.  Under bf16 autocast
even one update of the hand-written loop differs from its own of a second run by 1.9e-1 of range: there the statements are
exact ones about the product's own update (see the test).
"""
import functools

import numpy as np
import pytest
import torch

from amcontrast3d_amd import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_BOUND, GRAD_DISTINCT = 2e-3, 5e-2  # (of a tensor's range: see the module docstring)


# ---- set-up -------------------------------------------------------------------------------------------------------------
def _make(opt_name, lr, monkeypatch=None, mm=False, width=16, **cfg_kw):
    """model, criterion, cfg, optimizer -- seeded, so that two calls give twins.  opt_name: 'sgd', or one of the ways
    build_optimizer_from_cfg yields an Adam-type optimizer: 'fused' (this library's FusedAdamW) and the three torch ones,
    'adam', 'torch_adamw' (AMC3D_TORCH_ADAMW=1), 'adamw_kwarg' (an argument FusedAdamW does not take)"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(0)
    c = EasyConfig()
    c.update(configs.model_cfg_mm("S", dropout=0, width=width, threshold=0.5) if mm else configs.model_cfg("S", dropout=0, width=width))
    model = build_model_from_cfg(c).to(DEV)
    cc = EasyConfig(); cc.update(configs.criterion_cfg_mm() if mm else configs.criterion_cfg())
    crit = build_criterion_from_cfg(cc).to(DEV)
    cfg = EasyConfig()
    cfg.update({"num_classes": 13, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
                "ambiguity_args": configs.ambiguity_args_mm("s3dis") if mm else configs.ambiguity_args("s3dis"),
                "grad_norm_clip": 10, "sched_on_epoch": False, "fps_lanes": 2, "mm": mm})
    cfg.update(cfg_kw)
    if opt_name == "sgd":
        opt = torch.optim.SGD(model.parameters(), lr=lr)
    elif opt_name == "fused":
        opt = build_optimizer_from_cfg(model, NAME="adamw", lr=lr, weight_decay=1e-4)
        assert type(opt).__name__ == "FusedAdamW"
    else:
        if opt_name == "torch_adamw":
            monkeypatch.setenv("AMC3D_TORCH_ADAMW", "1")
        kw = {"amsgrad": False} if opt_name == "adamw_kwarg" else {}
        opt = build_optimizer_from_cfg(model, NAME="adam" if opt_name == "adam" else "adamw", lr=lr, weight_decay=1e-4, **kw)
        if opt_name == "torch_adamw":
            monkeypatch.delenv("AMC3D_TORCH_ADAMW")
        assert type(opt) is (torch.optim.Adam if opt_name == "adam" else torch.optim.AdamW)
        assert all(g["capturable"] and g["fused"] for g in opt.param_groups)
    return model, crit, cfg, opt


@functools.lru_cache(maxsize=None)
def _scene(b, n, first_id):
    from amcontrast3d_amd import synthetic
    return synthetic.make_batch(b, n, first_id=first_id)


def _loader(shapes, first=80, pin=False):
    """the reference's collated layout (point-major feature keys, y (B,N)), one fresh dict per batch: the loops write into them"""
    out = []
    for k, (b, n) in enumerate(shapes):
        nb = _scene(b, n, first + 2 * k)
        d = {"pos": torch.from_numpy(nb["pos"].copy()), "y": torch.from_numpy(nb["y"].copy()),
             "x": torch.from_numpy(np.ascontiguousarray(nb["x"][:, :3].transpose(0, 2, 1))),
             "heights": torch.from_numpy(np.ascontiguousarray(nb["x"][:, 3:4].transpose(0, 2, 1)))}
        out.append({k2: v.pin_memory() for k2, v in d.items()} if pin else d)
    return out


class _Probe:
    """a scheduler: step(epoch) is what the loops call after every update.  Calls `fn(number of the update, from 1)`, then the
    wrapped scheduler's step, if there is one."""

    def __init__(self, fn=None, inner=None):
        self.fn, self.inner, self.calls, self.epochs = fn, inner, 0, []

    def step(self, epoch):
        self.calls += 1
        self.epochs.append(epoch)
        if self.fn is not None:
            self.fn(self.calls)
        if self.inner is not None:
            self.inner.step(epoch)


def _set_lr(opt, lr):
    for g in opt.param_groups:
        g["lr"] = lr


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def _grads(model):
    return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def _fused(opt):
    return type(opt).__name__ == "FusedAdamW"


def _forward(model, crit, cfg, data):
    """-> logits, the loss the step minimises, the row of quantities train_one_epoch(_mm) averages"""
    if cfg.mm:
        logits, stage, rate = model(data)
        seg, ce, am, reg = crit(logits, data["y"], stage, cfg.num_classes, cfg.ignore_index, cfg.ambiguity_args)
        loss = seg + reg
        return logits, loss, [loss, seg, ce, am, reg, rate if torch.is_tensor(rate) else torch.tensor(float(rate))]
    logits, stage = model(data)
    loss = crit(logits, data["y"], stage, cfg.num_classes, cfg.ignore_index, cfg.ambiguity_args)
    return logits, loss, [loss]


def _hand_loop(model, crit, cfg, opt, loader, scheduler=None, scaler=None, epoch=1, before=None):
    """The reference's loop written out (main_AA.py:370-428 / main_MM.py:370-449), nothing of this package's train.py in it
    except get_features_by_keys.  -> (the tuple train_one_epoch returns, per-batch logits, per update: the gradients before
    the clipping and after it).  `before(i)`, if given, runs ahead of batch i's forward pass."""
    from amcontrast3d_amd import train
    from openpoints.utils import ConfusionMatrix
    cm = ConfusionMatrix(num_classes=cfg.num_classes, ignore_index=cfg.ignore_index)
    model.train()
    rows, all_logits, raw, clipped, pending = [], [], [], [], 0
    for i, data in enumerate(loader):
        if before is not None:
            before(i)
        data = {k: v.to(DEV) for k, v in data.items()}
        data["y"] = data["y"].squeeze(-1) if data["y"].dim() == 3 else data["y"]
        data["x"] = train.get_features_by_keys(data, cfg.feature_keys)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(cfg.use_amp)):
            logits, loss, row = _forward(model, crit, cfg, data)
        (scaler.scale(loss) if cfg.use_amp else loss).backward()
        pending += 1
        if pending == cfg.step_per_update:
            pending = 0
            raw.append(_grads(model))
            if cfg.grad_norm_clip:
                torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.grad_norm_clip, norm_type=2)
            clipped.append(_grads(model))
            if cfg.use_amp:
                scaler.step(opt)
                scaler.update()
            else:
                opt.step()
            opt.zero_grad()
            if scheduler is not None and not cfg.sched_on_epoch:
                scheduler.step(epoch)
        cm.update(logits.argmax(dim=1), data["y"])
        all_logits.append(logits.detach().clone())
        rows.append([float(v) for v in row])
    mean = np.sum(np.array(rows, dtype=np.float64).reshape(len(rows), -1), axis=0) / max(1, len(rows)) if rows else np.zeros(6 if cfg.mm else 1)
    return tuple(mean.tolist()) + tuple(cm.all_metrics()), all_logits, raw, clipped


def _same_results(got, want, n_avg=1):
    """the returned tuples: averages to 1e-6 relative (the product sums in fp64 on the device, the hand loop floats on the
    host), metrics of the same integer confusion matrix"""
    assert len(got) == len(want) == n_avg + 5
    np.testing.assert_allclose(got[:n_avg], want[:n_avg], rtol=2e-6 if n_avg > 1 else 1e-6, atol=1e-7 if n_avg > 1 else 0)
    np.testing.assert_allclose(got[n_avg:n_avg + 3], want[n_avg:n_avg + 3], rtol=1e-6)
    np.testing.assert_array_equal(got[n_avg + 3], want[n_avg + 3])
    np.testing.assert_array_equal(got[n_avg + 4], want[n_avg + 4])


def _same_state(model, model2):
    for (k, a), b in zip(model.state_dict().items(), model2.state_dict().values()):
        assert torch.equal(a, b), k


def _grad_error(got, want, what):
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, i)
        if g is not None:
            worst = max(worst, float((g - w).abs().max()) / max(float(w.abs().max()), 1e-2))
    print(f"{what}: worst gradient difference {worst:.2e} of a tensor's range (bound {GRAD_BOUND:.0e})")
    return worst


def _grad_distance(a, b):
    return max(float((x - y).abs().max()) / max(float(y.abs().max()), 1e-2) for x, y in zip(a, b) if x is not None)


def _param_distance(a, b):
    return max(float((x - y).abs().max()) / max(float(y.abs().max()), 1e-2) for x, y in zip(a, b))


def _the_pipeline():
    from amcontrast3d_amd import train
    assert len(train._PIPELINES) == 1
    return next(iter(train._PIPELINES.values()))[0]


@pytest.fixture(autouse=True)
def _fresh_pipelines():
    from amcontrast3d_amd import train
    train.release_pipelines()
    yield
    train.release_pipelines()


def _epoch(mm):
    from amcontrast3d_amd import train
    return train.train_one_epoch_mm if mm else train.train_one_epoch


# ---- 1. a schedule reaches the captured update -------------------------------------------------------------------------------
def _schedule_case(opt_name, monkeypatch, mm=False, cosine=False):
    """lr -> 0 through the scheduler while the epoch runs: the parameters move as long as lr > 0 and are bit-identical after every
    later update.  An update captured with the lr of its capture keeps moving them."""
    n = 6
    model, crit, cfg, opt = _make(opt_name, 0.01, monkeypatch, mm=mm)
    snaps = []
    if cosine:
        # the project's own scheduler: one cycle of 2 epochs down to min_lr = 0; stepped with epoch = 2 it writes 0 into every
        # group (before its first step the groups hold the initial lr: update 1 runs at 0.01, all later ones at 0)
        from openpoints.scheduler.cosine_lr import build_scheduler_from_cfg
        from openpoints.utils import EasyConfig
        args = EasyConfig(); args.update({"sched": "cosine", "epochs": 2, "lr": 0.0, "min_lr": 0, "warmup_epochs": 0})
        inner, epoch, last_moving = build_scheduler_from_cfg(args, opt), 2, 1
        assert [g["lr"] for g in opt.param_groups] == [0.01] * len(opt.param_groups)
        sched = _Probe(lambda k: snaps.append(_params(model)), inner)
    else:
        epoch, last_moving = 1, 2
        sched = _Probe(lambda k: (snaps.append(_params(model)), _set_lr(opt, 0.0) if k >= 2 else None))
    start = _params(model)
    _epoch(mm)(model, _loader([(2, 2048)] * n), crit, opt, sched, None, epoch, cfg)
    torch.cuda.synchronize()
    pipe = _the_pipeline()
    assert pipe.g_update is not None or pipe.update_in_feature_graph, f"the {type(opt).__name__} update is captured: the route under test"
    assert sched.calls == n == len(snaps) and sched.epochs == [epoch] * n, "the scheduler steps once per iteration (sched_on_epoch = False)"
    assert all(float(g["lr"]) == 0.0 for g in opt.param_groups)
    states = [start] + snaps
    for k in range(1, last_moving + 1):
        assert any(not torch.equal(x, y) for x, y in zip(states[k - 1], states[k])), f"update {k} ran with lr 0.01"
    for k in range(last_moving + 1, n + 1):
        moved = sum(not torch.equal(x, y) for x, y in zip(states[last_moving], states[k]))
        assert moved == 0, f"update {k} ran with lr = 0 and moved {moved} parameter tensors: the captured update did not see the new lr"


@pytest.mark.parametrize("opt_name", ["adam", "torch_adamw", "adamw_kwarg", "fused"])
def test_a_schedule_reaches_the_captured_optimizer(opt_name, monkeypatch):
    _schedule_case(opt_name, monkeypatch)


def test_the_cosine_schedule_reaches_a_captured_torch_optimizer(monkeypatch):
    _schedule_case("torch_adamw", monkeypatch, cosine=True)


def test_mm_a_schedule_reaches_the_captured_optimizer(monkeypatch):
    _schedule_case("torch_adamw", monkeypatch, mm=True)


# ---- 2. a ragged last batch, then another epoch ------------------------------------------------------------------------------
def _ragged_case(opt_name, odd_shape, monkeypatch, mm=False, n_same=4, second_epoch=True):
    from amcontrast3d_amd import train
    shapes = [(2, 2048)] * n_same + [odd_shape]
    lr2 = 0.02 if opt_name == "sgd" else 1e-3
    model, crit, cfg, opt = _make(opt_name, 0.0, monkeypatch, mm=mm)
    model2, crit2, cfg2, opt2 = _make(opt_name, 0.0, monkeypatch, mm=mm)
    seen, captured = [], {}
    hook = opt.register_step_pre_hook(lambda o, args, kwargs: seen.append(_grads(model)))

    def first_yield(k):  # after the first captured step: .grad is what the pipeline captured
        if k == 1:
            captured["ptr"] = [None if p.grad is None else p.grad.data_ptr() for p in model.parameters()]
    got = _epoch(mm)(model, _loader(shapes), crit, opt, _Probe(first_yield), None, 1, cfg)
    hook.remove()
    torch.cuda.synchronize()
    want, _, raw, clipped = _hand_loop(model2, crit2, cfg2, opt2, _loader(shapes), _Probe())
    # the gradient the optimizer read for the odd batch (its last step; FusedAdamW clips inside its launch: it reads the raw one)
    ref = raw if _fused(opt) else clipped
    assert _grad_distance(ref[-2], ref[-1]) > GRAD_DISTINCT, "consecutive batches have different gradients: the bound distinguishes them"
    assert _grad_error(seen[-1], ref[-1], f"odd batch {odd_shape}, {opt_name}") <= GRAD_BOUND, \
        "the optimizer stepped on something else than the odd batch's gradient"
    _same_results(got, want, 6 if mm else 1)
    _same_state(model, model2)  # lr = 0: weights untouched, running statistics advanced identically over all batches
    if not second_epoch:
        return
    # another epoch on the cached pipeline, now training
    pipe = _the_pipeline()
    assert (pipe.g_update is not None or pipe.update_in_feature_graph) == (opt_name != "sgd")
    _set_lr(opt, lr2); _set_lr(opt2, lr2)
    snaps, first_grads, ptrs = [], [], []

    def each(k):
        snaps.append(_params(model))
        ptrs.append([None if p.grad is None else p.grad.data_ptr() for p in model.parameters()])
        if k == 1:
            first_grads.extend(_grads(model))
    start = _params(model)
    model2.load_state_dict(model.state_dict())
    _epoch(mm)(model, _loader([(2, 2048)] * 4, first=300), crit, opt, _Probe(each), None, 2, cfg)
    torch.cuda.synchronize()
    assert _the_pipeline() is pipe and len(snaps) == 4
    for k, now in enumerate(ptrs):
        assert now == captured["ptr"], f"epoch 2, iteration {k + 1}: .grad is not the tensor the pipeline captured"
    states = [start] + snaps
    for k in range(1, 5):
        assert any(not torch.equal(x, y) for x, y in zip(states[k - 1], states[k])), f"epoch 2, iteration {k} (lr {lr2}) moved no parameter"
    _, _, raw, clipped = _hand_loop(model2, crit2, cfg2, opt2, _loader([(2, 2048)], first=300), _Probe())
    assert _grad_error(first_grads, (raw if _fused(opt) else clipped)[0], f"epoch 2, first iteration, {opt_name}") <= GRAD_BOUND


@pytest.mark.parametrize("opt_name,odd_shape", [("sgd", (1, 2048)), ("torch_adamw", (1, 2048)), ("fused", (1, 2048)), ("sgd", (2, 1024))],
                         ids=["sgd-1x2048", "torch_adamw-1x2048", "fused-1x2048", "sgd-2x1024"])
def test_a_ragged_last_batch_then_another_epoch(opt_name, odd_shape, monkeypatch):
    """Four 2 x 2048 batches on the pipeline, a fifth of another shape trained eagerly after the drain.  The pipeline's static
    .grad tensors still hold batch 4's gradient then: the odd batch's backward must not add to it.  And whatever the eager loop's
    zero_grad() does to .grad (torch's default drops the tensors), the next epoch's replays write into the tensors the update reads."""
    _ragged_case(opt_name, odd_shape, monkeypatch)


def test_mm_a_ragged_last_batch(monkeypatch):
    _ragged_case("sgd", (1, 2048), monkeypatch, mm=True, n_same=3, second_epoch=False)


# ---- 3. the first batch of a later epoch -------------------------------------------------------------------------------------
def test_the_first_batch_of_a_later_epoch_is_complete_when_the_pipeline_reads_it(monkeypatch):
    """The first batch of an epoch is produced on the caller's stream (host-to-device copies from pinned memory, feature
    assembly) and read by the geometry queue.  Epoch 1 hides a missing wait (building the pipeline ends with a device-wide
    synchronisation); from epoch 2 on nothing does.  Here the caller's stream is busy for tens of milliseconds when epoch 2
    starts, so the batch's copies are still pending when the pipeline's first tick is issued; the allocator hands epoch 2's first
    batch the blocks epoch 1's batches lived in, so a queue that does not wait reads another batch's (or a half-written)
    coordinates, features and labels.  With lr = 0 every batch's logits are bit-identical to the eager loop's on that batch
    (as in test_gpu_graph_pipeline.py::test_every_result_belongs_to_one_batch_in_order): a first batch read early shows as logits
    and targets of something else.  The test is only meaningful with the wait in place; it is not a demonstration of the race."""
    from amcontrast3d_amd import train
    from openpoints.utils import ConfusionMatrix
    monkeypatch.setenv("AMC3D_EAGER_BOOKKEEPING", "1")  # the loop then sees every batch's logits (update_from_logits)
    model, crit, cfg, opt = _make("sgd", 0.0)
    model2, crit2, cfg2, opt2 = _make("sgd", 0.0)
    train.train_one_epoch(model, _loader([(2, 2048)] * 4), crit, opt, _Probe(), None, 1, cfg)
    assert _the_pipeline().tail is None
    _hand_loop(model2, crit2, cfg2, opt2, _loader([(2, 2048)] * 4), _Probe())
    seen = []
    orig = ConfusionMatrix.update_from_logits

    def record(self, logits, true):
        seen.append((logits.detach().clone(), true.clone()))
        return orig(self, logits, true)
    monkeypatch.setattr(ConfusionMatrix, "update_from_logits", record)
    second = _loader([(2, 2048)] * 5, first=400, pin=True)
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)  # the caller's stream: busy while the epoch's first batch is queued behind it
    got = train.train_one_epoch(model, second, crit, opt, _Probe(), None, 2, cfg)
    torch.cuda.synchronize()
    monkeypatch.setattr(ConfusionMatrix, "update_from_logits", orig)
    fresh = _loader([(2, 2048)] * 5, first=400)
    want, logits, _, _ = _hand_loop(model2, crit2, cfg2, opt2, fresh, _Probe(), epoch=2)
    assert len(seen) == 5
    for i, ((lg, y), wl) in enumerate(zip(seen, logits)):
        assert torch.equal(y.cpu(), _loader([(2, 2048)] * 5, first=400)[i]["y"]), f"epoch 2, result {i}: not batch {i}'s labels"
        assert torch.equal(lg, wl), f"epoch 2, batch {i}: logits differ from the eager loop's (max {float((lg - wl).abs().max()):.2e})"
    _same_results(got, want)
    _same_state(model, model2)


# ---- 4. the eager routes -----------------------------------------------------------------------------------------------------
def _updates_match(name, sides, shapes, lr, bound):
    """One epoch with lr > 0: every update the product applies against the update the hand-written loop applies from the same
    weights (module docstring).  sides: (model, crit, cfg, opt) of the product and of the hand-written loop."""
    from amcontrast3d_amd import train
    (model, crit, cfg, opt), (model2, crit2, cfg2, opt2) = sides
    _set_lr(opt, lr); _set_lr(opt2, lr)
    model2.load_state_dict(model.state_dict())
    states, hand, per = [_params(model)], [], cfg.step_per_update
    train.train_one_epoch(model, _loader(shapes), crit, opt, _Probe(lambda k: states.append(_params(model))), None, 2, cfg)

    def before(i):
        if i % per == 0:
            with torch.no_grad():
                for p, w in zip(model2.parameters(), states[i // per]):
                    p.copy_(w)
    _hand_loop(model2, crit2, cfg2, opt2, _loader(shapes), _Probe(lambda k: hand.append(_params(model2))), epoch=2, before=before)
    assert len(hand) == len(states) - 1 == len(shapes) // per
    worst = 0.0
    for k, after in enumerate(hand):
        assert any(not torch.equal(x, y) for x, y in zip(states[k], states[k + 1])), f"{name}: update {k + 1} (lr {lr}) moved no parameter"
        for i, (p0, p1, h1) in enumerate(zip(states[k], states[k + 1], after)):
            den = max(float((h1 - p0).abs().max()), lr * 1e-2)
            err = float(((p1 - p0) - (h1 - p0)).abs().max()) / den
            worst = max(worst, err)
            assert err <= bound + 2 * 2.0 ** -23 * float(p0.abs().max()) / den, (name, k + 1, i, err)
    print(f"{name}: worst difference between the applied updates {worst:.2e} of an update's range (bound {bound:.1e} + 2 ulp of the parameter)")


def test_gradient_accumulation_matches_the_hand_written_loop():
    """step_per_update = 2 over six batches: three updates, each on the sum of two batches' gradients, the scheduler stepped
    three times.  lr = 0: results and the gradient of every update against the hand loop; then one epoch with lr > 0."""
    from amcontrast3d_amd import train
    shapes = [(2, 2048)] * 6
    model, crit, cfg, opt = _make("sgd", 0.0, step_per_update=2)
    model2, crit2, cfg2, opt2 = _make("sgd", 0.0, step_per_update=2)
    seen = []
    hook = opt.register_step_pre_hook(lambda o, args, kwargs: seen.append(_grads(model)))
    sched = _Probe()
    got = train.train_one_epoch(model, _loader(shapes), crit, opt, sched, None, 1, cfg)
    hook.remove()
    assert not train._PIPELINES, "gradient accumulation runs eagerly"
    want, _, raw, clipped = _hand_loop(model2, crit2, cfg2, opt2, _loader(shapes), _Probe())
    assert sched.calls == 3 == len(seen) == len(clipped)
    _same_results(got, want)
    _same_state(model, model2)
    for k in range(3):
        assert _grad_error(seen[k], clipped[k], f"update {k + 1} of 3") <= GRAD_BOUND
    # one batch's gradient is not the sum of two: an update applied every iteration is seen
    cfg1 = type(cfg2)(); cfg1.update(cfg2); cfg1.step_per_update = 1
    _, _, _, single = _hand_loop(model2, crit2, cfg1, opt2, _loader(shapes[:1]), _Probe())
    assert _grad_distance(single[0], clipped[0]) > GRAD_DISTINCT and _grad_distance(clipped[0], clipped[1]) > GRAD_DISTINCT
    _updates_match("accumulate", ((model, crit, cfg, opt), (model2, crit2, cfg2, opt2)), shapes, 0.02, GRAD_BOUND)


def test_use_amp_is_the_bf16_route_and_matches_the_hand_written_loop(monkeypatch):
    """cfg.use_amp with a GradScaler: the eager loop under torch.autocast(bfloat16) -- the arithmetic ops.mixed_precision() selects
    and tests/test_gpu_bf16.py pins (fp32 tensors between the kernels, bf16 MFMA operands), at a width where those routes engage.
    The hand-written loop runs under the same context; with lr = 0 the logits are the same bits, hence the same confusion matrix."""
    from amcontrast3d_amd import ops, train
    shapes = [(2, 2048)] * 3
    model, crit, cfg, opt = _make("sgd", 0.0, width=64, use_amp=True)
    model2, crit2, cfg2, opt2 = _make("sgd", 0.0, width=64, use_amp=True)
    scaler, scaler2 = torch.amp.GradScaler("cuda"), torch.amp.GradScaler("cuda")
    calls, orig = [], ops._pw
    monkeypatch.setattr(ops, "_pw", lambda lib, bf16: calls.append(bool(bf16)) or orig(lib, bf16))
    sched = _Probe()
    got = train.train_one_epoch(model, _loader(shapes), crit, opt, sched, scaler, 1, cfg)
    assert calls.count(True) > 0, "use_amp took no bf16 kernel: the loop computed in fp32"
    monkeypatch.setattr(ops, "_pw", orig)
    assert not train._PIPELINES and sched.calls == 3
    want, _, _, _ = _hand_loop(model2, crit2, cfg2, opt2, _loader(shapes), _Probe(), scaler=scaler2)
    _same_results(got, want)
    _same_state(model, model2)
    assert scaler.get_scale() == scaler2.get_scale()
    # a fp32 run is another computation: the comparison above would see a loop that ignored use_amp
    model3, crit3, cfg3, opt3 = _make("sgd", 0.0, width=64, use_amp=False)
    full = _hand_loop(model3, crit3, cfg3, opt3, _loader(shapes), _Probe())[0]
    assert abs(full[0] - want[0]) > 1e-4 * abs(want[0])
    # One epoch with lr > 0.  Under bf16 not even ONE update compares between two runs: measured on the MI355X, the hand-written
    # loop's update differs from its own of a second run from the same weights by 1.9e-1 of the update's range (the float atomics
    # of the interpolation backward move fp32 values by an ulp, bf16 roundings downstream fall the other way).  Ten times that is
    # no allowance, so the statements are exact ones: every update moves the parameters, each is bit for bit SGD's formula (the
    # launch torch.optim.SGD itself makes) on the gradient the optimizer read, and that gradient is the unscaled one -- its norm
    # is within a factor of 2 of the hand-written loop's at the same weights (five times the spread above; a gradient left at the
    # scaler's 65536 is 3e4 times outside).  Without clipping: the reference clips the still-scaled gradients (to a norm of 10
    # before the division by 65536), which leaves updates of 1e-6 of a parameter's range.
    cfg.grad_norm_clip = cfg2.grad_norm_clip = 0
    _set_lr(opt, 0.02); _set_lr(opt2, 0.02)
    states, seen = [_params(model)], []
    hook = opt.register_step_pre_hook(lambda o, args, kwargs: seen.append(_grads(model)))
    train.train_one_epoch(model, _loader(shapes), crit, opt, _Probe(lambda k: states.append(_params(model))),
                          torch.amp.GradScaler("cuda"), 2, cfg)
    hook.remove()
    assert len(seen) == 3 == len(states) - 1
    for k in range(3):
        assert any(not torch.equal(x, y) for x, y in zip(states[k], states[k + 1])), f"update {k + 1} moved no parameter"
        for x, y in zip(torch._foreach_add(states[k], seen[k], alpha=-0.02), states[k + 1]):
            assert torch.equal(x, y), f"update {k + 1} is not p - lr * (the gradient the optimizer read)"
    scaler2 = torch.amp.GradScaler("cuda")
    _, _, scaled, _ = _hand_loop(model2, crit2, cfg2, opt2, _loader(shapes[:1]), _Probe(), scaler=scaler2, epoch=2)
    norm = lambda gs: float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs if g is not None)))
    ratio = norm(seen[0]) / (norm(scaled[0]) / 65536.0)
    print(f"use_amp, first update: norm of the gradient the optimizer read / the hand-written loop's unscaled one = {ratio:.4f}")
    assert 0.5 <= ratio <= 2.0


# ---- 5. loaders without a recurring shape ------------------------------------------------------------------------------------
def test_an_empty_loader_gives_what_the_hand_written_loop_gives():
    from amcontrast3d_amd import train
    model, crit, cfg, opt = _make("sgd", 0.0)
    model2, crit2, cfg2, opt2 = _make("sgd", 0.0)
    try:
        want = _hand_loop(model2, crit2, cfg2, opt2, [], _Probe())[0]
    except Exception as e:  # (the metrics of a confusion matrix nothing was added to: whatever the hand-written loop meets)
        with pytest.raises(type(e)):
            train.train_one_epoch(model, [], crit, opt, _Probe(), None, 1, cfg)
    else:
        _same_results(train.train_one_epoch(model, [], crit, opt, _Probe(), None, 1, cfg), want)
    _same_state(model, model2)


def test_a_loader_whose_only_batch_is_the_odd_one():
    from amcontrast3d_amd import train
    model, crit, cfg, opt = _make("sgd", 0.0)
    model2, crit2, cfg2, opt2 = _make("sgd", 0.0)
    sched = _Probe()
    got = train.train_one_epoch(model, _loader([(1, 2048)]), crit, opt, sched, None, 1, cfg)
    want = _hand_loop(model2, crit2, cfg2, opt2, _loader([(1, 2048)]), _Probe())[0]
    assert sched.calls == 1
    _same_results(got, want)
    _same_state(model, model2)
