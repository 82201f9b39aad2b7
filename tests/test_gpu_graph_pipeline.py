"""pipeline.GraphPipeline -- the hipGraph schedule that train.train_one_epoch and bench.py run -- against the plain eager loop
on the same batches:

  * ownership: with frozen weights (lr = 0) every result the pipeline yields belongs to ONE batch -- the batches come out in
    the order they went in, the logits are bit-identical to the eager model's on that batch (the searches, sampling and every
    forward kernel are deterministic) and the loss agrees: the sampling plan, the neighbourhood / loss geometry and the
    features that met in a feature graph all belonged to the same batch, for every lane, both joint buffers and both
    ping-pong variants (the former AMC3D_CHECK_BATCHES switch of bench.py as a test);
  * training: the gradients the update reads after each step equal the eager loop's on that batch (frozen weights; not bit
    for bit: the interpolation backward adds rows with float atomics whose order differs from run to run in BOTH loops);
  * a scheduler's new learning rate reaches the captured update (FusedAdamW.sync_hyperparameters);
  * building the pipeline leaves parameters, BatchNorm buffers and optimizer state as they were.
"""
import itertools

import pytest
import torch

from amcontrast3d_amd import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N = 2, 2048


def _setup(lr, fused=True, seed=0, width=16):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(seed)
    c = EasyConfig(); c.update(configs.model_cfg("S", dropout=0, width=width))
    model = build_model_from_cfg(c).to(DEV).train()
    cc = EasyConfig(); cc.update(configs.criterion_cfg())
    crit = build_criterion_from_cfg(cc).to(DEV)
    aa = EasyConfig(); aa.update(configs.ambiguity_args("s3dis"))
    opt = (build_optimizer_from_cfg(model, NAME="adamw", lr=lr, weight_decay=1e-4) if fused
           else torch.optim.SGD(model.parameters(), lr=lr))
    return model, crit, aa, opt


def _batches(n, first=500):
    from amcontrast3d_amd import synthetic
    return [{k: torch.from_numpy(v).to(DEV) for k, v in synthetic.make_batch(B, N, first_id=first + 7 * i).items()} for i in range(n)]


def _pipeline(model, crit, aa, opt, example, lanes, **kw):
    from amcontrast3d_amd.pipeline import GraphPipeline

    def step_loss(data):
        logits, stage = model(data)
        return logits, crit(logits, data["y"], stage, 13, None, aa), ()
    main = torch.cuda.Stream()
    main.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(main):
        pipe = GraphPipeline(model, step_loss, crit.contrast_head, opt, example, 13, None, aa, lanes=lanes, max_grad_norm=10, **kw)
    return pipe, main


def _eager_step(model, crit, aa, opt, data, clip=10, amp_dtype=None):
    with torch.autocast("cuda", dtype=amp_dtype or torch.bfloat16, enabled=amp_dtype is not None):
        logits, stage = model(dict(data))
        loss = crit(logits, data["y"], stage, 13, None, aa)
    opt.zero_grad()
    loss.backward()
    if type(opt).__name__ == "FusedAdamW":
        opt.step(max_grad_norm=clip)
    else:
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
    return logits.detach(), loss.detach()


@pytest.mark.parametrize("lanes,nb", [(2, 11), (3, 14), (4, 9)])
def test_every_result_belongs_to_one_batch_in_order(lanes, nb):
    model, crit, aa, opt = _setup(0.0, fused=False)
    src = _batches(nb)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    pipe, main = _pipeline(model, crit, aa, opt, src[0], lanes)
    for k, v in model.state_dict().items():  # three warm-up steps ran on the example batch: nothing of them may remain
        assert torch.equal(v, before[k]), k
    got = []
    with torch.cuda.stream(main):
        for out in pipe.run(iter(src)):
            got.append((out["data"]["pos"].clone(), out["logits"].clone(), float(out["loss"]), out["target"].clone()))
    torch.cuda.synchronize()
    assert len(got) == nb
    model2, crit2, aa2, opt2 = _setup(0.0, fused=False)
    for i, (pos, logits, loss, target) in enumerate(got):
        assert torch.equal(pos, src[i]["pos"]) and torch.equal(target, src[i]["y"]), f"result {i} is not batch {i}"
        want_logits, want_loss = _eager_step(model2, crit2, aa2, opt2, src[i])
        assert torch.equal(logits, want_logits), f"batch {i}: logits differ from the eager model's (max {float((logits - want_logits).abs().max()):.2e})"
        assert abs(loss - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (i, loss, float(want_loss))
    # the BatchNorm running statistics advanced exactly as in the eager loop (every batch normalised once, in order)
    for (k, a), b in zip(model.state_dict().items(), model2.state_dict().values()):
        assert torch.equal(a, b), k
    # a second pass over other batches on the same graphs (the next epoch)
    src2 = _batches(5, first=900)
    with torch.cuda.stream(main):
        outs = [(o["data"]["pos"].clone(), o["logits"].clone()) for o in pipe.run(iter(src2))]
    assert len(outs) == 5
    for i, (pos, logits) in enumerate(outs):
        assert torch.equal(pos, src2[i]["pos"])
        assert torch.equal(logits, _eager_step(model2, crit2, aa2, opt2, src2[i])[0])


def test_captured_bf16_step_matches_the_eager_autocast_step(monkeypatch):
    """GraphPipeline(amp_dtype=torch.bfloat16) -- the step bench.py --dtype bf16 times -- at a width where the bf16 routes
    engage (the conv before the gather from SA1 on, the library GEMMs of the deep layers): every result belongs to one
    batch, in order, with logits bit-identical to the eager step under autocast on that batch"""
    from amcontrast3d_amd import ops
    model, crit, aa, opt = _setup(0.0, fused=False, width=64)
    src = _batches(5)
    pipe, main = _pipeline(model, crit, aa, opt, src[0], 2, amp_dtype=torch.bfloat16)
    got = []
    with torch.cuda.stream(main):
        for out in pipe.run(iter(src)):
            got.append((out["data"]["pos"].clone(), out["logits"].clone(), float(out["loss"])))
    torch.cuda.synchronize()
    assert len(got) == len(src)
    model2, crit2, aa2, opt2 = _setup(0.0, fused=False, width=64)
    calls = []
    orig = ops._pw
    monkeypatch.setattr(ops, "_pw", lambda lib, bf16: calls.append(bool(bf16)) or orig(lib, bf16))
    for i, (pos, logits, loss) in enumerate(got):
        assert torch.equal(pos, src[i]["pos"]), f"result {i} is not batch {i}"
        want_logits, want_loss = _eager_step(model2, crit2, aa2, opt2, src[i], amp_dtype=torch.bfloat16)
        assert torch.equal(logits, want_logits), f"batch {i}: logits differ from the eager autocast step's (max {float((logits - want_logits).abs().max()):.2e})"
        assert abs(loss - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (i, loss, float(want_loss))
    assert calls.count(True) > 0  # the eager step took the bf16 MFMA


def test_every_variants_gradient_reaches_the_static_tensors():
    """What the update reads after step t is the gradient of batch t on the current weights, whichever captured variant ran:
    with frozen weights (SGD, lr = 0 -- so that nothing is amplified from step to step: at lr = 1e-3 the rounding of the float
    atomics in the interpolation backward, carried into the next forward pass, flips a max-pool pick or a ReLU mask at a
    near-tie in some runs of EITHER loop and the K-step parameters fall into discrete outcomes up to 0.1 of an update apart)
    the .grad tensors after every yielded step equal the eager loop's gradients on that batch at the level of those atomics.
    A variant whose copy into the static tensors was missing would hand the update the gradient of another batch.  (The captured
    FusedAdamW update itself is pinned by the learning-rate test below, tests/test_gpu_optim.py::test_replays_in_a_hip_graph
    and, through the BatchNorm buffers, by the ownership test above.)"""
    K = 5  # three captured variants, and round again
    model, crit, aa, opt = _setup(0.0, fused=False)
    src = _batches(K, first=300)
    pipe, main = _pipeline(model, crit, aa, opt, src[0], 2)
    got = []
    with torch.cuda.stream(main):
        for out in pipe.run(iter(src)):
            got.append([None if p.grad is None else p.grad.detach().clone() for p in model.parameters()])
    torch.cuda.synchronize()
    assert len(got) == K
    model2, crit2, aa2, opt2 = _setup(0.0, fused=False)
    worst = 0.0
    for i in range(K):
        _eager_step(model2, crit2, aa2, opt2, src[i])  # (clips at 10 like the pipeline of _pipeline: .grad holds the clipped gradient)
        for (name, p), g in zip(model2.named_parameters(), got[i]):
            assert (g is None) == (p.grad is None), name
            if g is None:
                continue
            # (a conv bias in front of a BatchNorm has a zero true gradient: what it receives is ~1e-5 of rounding noise)
            err = float((g - p.grad).abs().max()) / max(float(p.grad.abs().max()), 1e-2)
            worst = max(worst, err)
            assert err <= 2e-3, (i, name, err)
    # consecutive batches have different gradients: the comparison above distinguishes them
    assert max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-2) for a, b in zip(got[0], got[1]) if a is not None) > 5e-2
    print(f"gradients after each of {K} pipelined steps vs the eager loop: worst {worst:.2e} of a tensor's range")


def test_a_schedulers_learning_rate_reaches_the_captured_update():
    model, crit, aa, opt = _setup(0.01)
    src = _batches(6, first=40)
    pipe, main = _pipeline(model, crit, aa, opt, src[0], 2)
    assert pipe.g_update is not None or pipe.update_in_feature_graph, "FusedAdamW's step is captured"
    lrs = [0.01, 0.01, 0.0, 0.0, 0.0, 0.0]   # lr -> 0 after the second step: later steps may only apply weight decay * 0 = nothing
    snaps = []
    with torch.cuda.stream(main):
        for i, out in enumerate(pipe.run(iter(src))):
            snaps.append([p.detach().clone() for p in model.parameters()])
            for g in opt.param_groups:
                g["lr"] = lrs[min(i + 1, len(lrs) - 1)]
    torch.cuda.synchronize()
    assert any(not torch.equal(x, y) for x, y in zip(snaps[0], snaps[1])), "step 2 ran with lr 0.01"
    for later in snaps[2:]:
        for x, y in zip(snaps[1], later):
            assert torch.equal(x, y), "a step with lr = 0 moved a parameter: the captured update did not see the new lr"


def test_endless_feed_and_describe():
    model, crit, aa, opt = _setup(0.01)
    pool = _batches(3, first=70)
    pipe, main = _pipeline(model, crit, aa, opt, pool[0], 2, keep_state=False)
    with torch.cuda.stream(main):
        run = pipe.run(itertools.cycle(pool))
        losses = [float(next(run)["loss"]) for _ in range(9)]
    assert all(torch.isfinite(torch.tensor(losses)))
    d = pipe.describe()
    assert d["launch"].startswith("hipGraph") and d["batches_per_joint_fps_launch"] == 2 and d["update"].startswith("captured")
    parts = pipe.parts_alone(reps=2)
    assert parts["features_ms"] > 0 and pipe.serial_ms(reps=2) > 0


@pytest.mark.parametrize("mm", [False, True])
def test_no_memset_node_in_any_graph_of_the_pipeline(mm):
    """On ROCm 7.2 a memset NODE is not reliably ordered before the kernel nodes behind it when a graph is replayed (the GPU
    fault of DESIGN.md section 0: rocPRIM's radix sort zeroes its counters with hipMemsetAsync; torch's multi-block reductions do
    the same -- AMContrast3D++'s L1 regression term was one).  GraphPipeline(audit=True) keeps every captured graph's node list:
    the geometry, feature (+ update), hand-down and sampling graphs of both model families hold kernels and copies only, and
    the audited pipeline still trains."""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    if mm:
        torch.manual_seed(0)
        c = EasyConfig(); c.update(configs.model_cfg_mm("S", dropout=0, width=16, threshold=0.5))
        model = build_model_from_cfg(c).to(DEV).train()
        cc = EasyConfig(); cc.update(configs.criterion_cfg_mm())
        crit = build_criterion_from_cfg(cc).to(DEV)
        aa = EasyConfig(); aa.update(configs.ambiguity_args_mm("s3dis"))
        opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=1e-4)

        def step_loss(data):
            logits, stage, rate = model(data)
            seg, ce, am, reg = crit(logits, data["y"], stage, 13, None, aa)
            return logits, seg + reg, (seg, ce, am, reg)
        from amcontrast3d_amd.pipeline import GraphPipeline
        batches = _batches(5)
        main = torch.cuda.Stream()
        main.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(main):
            pipe = GraphPipeline(model, step_loss, crit.contrast_head, opt, batches[0], 13, None, aa, lanes=2, max_grad_norm=10, audit=True)
    else:
        model, crit, aa, opt = _setup(1e-3)
        batches = _batches(5)
        pipe, main = _pipeline(model, crit, aa, opt, batches[0], 2, audit=True)
    assert set(pipe.graph_nodes) >= {"geometry", "features", "hand_down", "sampling"}, pipe.graph_nodes.keys()
    for name, graphs_ in pipe.graph_nodes.items():
        for counts in graphs_:
            assert counts.get("kernel", 0) + counts.get("memcpy", 0) > 0 and not counts.get("memset"), (name, counts)
            assert set(counts) <= {"kernel", "memcpy", "empty", "event_record", "wait_event"}, (name, counts)
    with torch.cuda.stream(main):
        losses = [float(out["loss"]) for out in pipe.run(iter(batches))]
    assert len(losses) == 5 and all(l == l and l < 1e3 for l in losses)
