"""What deterministic mode costs: GraphPipeline ms per step with the mode off and on, and the reverse-list kernels (three
gathers and the contrast backward at the coarsest loss stage) beside the float-atomic kernels they stand in for at the shapes
of that step (device events, 50 calls each).

    python tools/determinism_bench.py [--config S|XL|both] [--steps K] [--warmup W] [--kernels-only] [--steps-only]

S is PointNeXt-S + AMContrast3D-AA at 8 x 24000, XL the shipped XL at 2 x 64000 (bench.py's workloads).  One JSON line per
measurement.  The step numbers of the two modes come from two pipelines built one after the other in this process."""
import argparse, ctypes, itertools, json, os, sys, time
import torch
sys.path.insert(0, os.getcwd())
import amcontrast3d_amd
amcontrast3d_amd.activate()
from amcontrast3d_amd import _lib, configs, ops, synthetic
from amcontrast3d_amd.pipeline import GraphPipeline
from openpoints.loss import build_criterion_from_cfg
from openpoints.models import build_model_from_cfg
from openpoints.optim import build_optimizer_from_cfg
from openpoints.utils import EasyConfig

DEV = torch.device("cuda:0")
CONFIGS = {"S": ("S", 8, 24000), "XL": ("XL", 2, 64000)}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def step_ms(variant, batch, points, det, steps, warmup):
    torch.manual_seed(0)
    c = EasyConfig(); c.update(configs.model_cfg(variant, dropout=0.5))
    model = build_model_from_cfg(c).to(DEV).train()
    cc = EasyConfig(); cc.update(configs.criterion_cfg()); crit = build_criterion_from_cfg(cc).to(DEV)
    aa = EasyConfig(); aa.update(configs.ambiguity_args("s3dis"))
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=1e-4)
    pool = [{k: torch.from_numpy(v).to(DEV) for k, v in synthetic.make_batch(batch, points, first_id=1000 + 16 * j).items()}
            for j in range(4)]

    def step_loss(data):
        logits, stage = model(data)
        return logits, crit(logits, data["y"], stage, 13, None, aa), ()

    main = torch.cuda.Stream()
    main.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(main), ops.deterministic_mode(det):
        pipe = GraphPipeline(model, step_loss, crit.contrast_head, opt, pool[0], 13, None, aa, max_grad_norm=10, keep_state=False)
        runner = pipe.run(itertools.cycle(pool))
        for _ in range(warmup):
            next(runner)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = next(runner)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        loss = float(out["loss"])
    del pipe, runner
    return ms, loss


def timed(fn, calls=50):
    for _ in range(3):
        fn()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    e[0].record()
    for i in range(calls):
        fn()
        e[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(e[i].elapsed_time(e[i + 1]) * 1e3 for i in range(calls))
    return {"median_us": round(ts[calls // 2], 1), "min_us": round(ts[0], 1)}


def kernels(variant, batch, points):
    """the levels of the model's step: interpolation onto every decoder level, the local aggregations of every stage"""
    lib = _lib.load()
    cfg = configs.model_cfg(variant)["encoder_args"]
    width, blocks, sa_layers = cfg["width"], cfg["blocks"], cfg["sa_layers"]
    g = torch.Generator().manual_seed(0)
    data = synthetic.make_batch(batch, points, first_id=1000)
    p = [torch.from_numpy(data["pos"]).to(DEV).contiguous()]
    for _ in range(4):
        n = p[-1].shape[1] // 4
        pick = ops.furthest_point_sample(p[-1], n).long()
        p.append(torch.gather(p[-1], 1, pick.unsqueeze(-1).expand(-1, -1, 3)).contiguous())
    out = []
    for lvl in range(4):  # grad of three_interpolate: coarse features (B, c, m) onto the n finer points
        fine, coarse = p[lvl], p[lvl + 1]
        n, m, c = fine.shape[1], coarse.shape[1], width * 2 ** (lvl + 1)
        dist, idx = ops.three_nn(fine, coarse)
        w = 1.0 / (dist + 1e-8)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        go = torch.randn(batch, c, n, generator=g).to(DEV)
        rs, re = ops.group_csr(idx, m)
        gp, work = torch.empty(batch, c, m, device=DEV), torch.empty(batch * c * m, device=DEV)

        def atomic():
            gp.zero_()
            _lib.check(lib.amc3d_three_interpolate_grad(batch, c, n, m, _p(go), _p(idx), _p(w), _p(gp), _p(work), work.numel() * 4, _s()), "a")

        def lists():
            _lib.check(lib.amc3d_three_interpolate_grad_csr(batch, c, n, m, _p(go), _p(idx), _p(w), _p(rs), _p(re), _p(gp), _s()), "l")
        out.append({"kernel": "three_interpolate_grad", "variant": variant, "shape": {"b": batch, "c": c, "n": n, "m": m},
                    "atomic": timed(atomic), "csr": timed(lists), "group_csr": timed(lambda: ops.group_csr(idx, m))})
    if sa_layers == 1 or max(blocks[1:]) > 1:  # LocalAggregation / single-layer SetAbstraction backward per stage
        radius = 0.1
        for lvl in range(1, 5):
            radius *= 2
            C, N = width * 2 ** lvl, p[lvl].shape[1]
            if not ops.local_aggregation_supported(C, 32):
                continue
            pts = p[lvl]
            idx = ops.ball_query(radius, 32, pts, pts)
            dp = ((ops.grouping_operation(pts.transpose(1, 2).contiguous(), idx) - pts.transpose(1, 2).unsqueeze(-1)) / radius).contiguous()
            f = torch.randn(batch, C, N, generator=g).to(DEV).requires_grad_(True)
            wgt = (torch.randn(C, C + 3, 1, 1, generator=g) * 0.1).to(DEV).requires_grad_(True)
            gamma, beta = torch.ones(C, device=DEV, requires_grad=True), torch.zeros(C, device=DEV, requires_grad=True)
            go = torch.randn(batch, C, N, generator=g).to(DEV)
            mom = ops.group_moments(idx, dp, N)
            csr = ops.group_csr(idx, N)
            res = {}
            for name, det in (("atomic", False), ("csr", True)):
                with ops.deterministic_mode(det):
                    y = ops.LocalAggregationFused.apply(f, dp, idx, mom, wgt, gamma, beta, 1e-5, True, None, None, csr if det else None)
                res[name] = timed(lambda: torch.autograd.grad(y, (f, wgt, gamma, beta), go, retain_graph=True))
            out.append({"kernel": "local_aggregation_backward (+ the conv's backward, both forms alike)", "variant": variant,
                        "shape": {"b": batch, "c": C, "n": N, "npoints": N, "nsample": 32}, **res,
                        "group_csr": timed(lambda: ops.group_csr(idx, N))})
    # contrast loss backward at the coarsest loss stage (N / 64 points per cloud, 8 x width channels, 23 neighbours):
    # float atomics (default mode at a width without a power-of-two row kernel) against the gather over reverse lists
    xyz = p[3].view(-1, 3).contiguous()
    m, C, k = xyz.shape[0], width * 8, 23
    o = torch.arange(1, batch + 1, dtype=torch.int32, device=DEV) * p[3].shape[1]
    nbr = ops.knnquery(k + 1, xyz, xyz, o, o)[0][:, 1:]
    lab = torch.randint(0, 13, (m,), generator=g, dtype=torch.int32).to(DEV)
    posmask = ops.posmask_from_labels(lab, nbr)
    a = torch.rand(m, generator=g).to(DEV)
    anchors = ops.select_anchors(a)
    rev = ops.contrast_csr(nbr, anchors)
    f = torch.randn(m, C, generator=g).to(DEV).requires_grad_(True)
    res = {}
    for name, det, extra in (("atomic", False, (anchors,)), ("csr", True, (anchors, rev))):
        with ops.deterministic_mode(det):
            y = ops.contrast_stage(f, nbr, posmask, a, -1.0, 0.5, 0.3, *extra)
        res[name] = timed(lambda: torch.autograd.grad(y, f, retain_graph=True))
    out.append({"kernel": "contrast_backward", "variant": variant, "shape": {"m": m, "C": C, "k": k}, **res,
                "contrast_csr": timed(lambda: ops.contrast_csr(nbr, anchors))})
    # refinement backward at the decoder's finest level
    D, n, k = width, points, 11
    B = batch
    f = torch.randn(B, D, n, generator=g).to(DEV).requires_grad_(True)
    a = torch.rand(B * n, generator=g).to(DEV)
    xyz = p[0].view(-1, 3).contiguous()
    o = torch.tensor([B * n], dtype=torch.int32, device=DEV)
    nbr = ops.knnquery(k + 1, xyz, xyz, o, o)[0][:, 1:].contiguous()
    go = torch.randn(B, D, n, generator=g).to(DEV)
    res = {}
    for name, det in (("atomic", False), ("csr (lists built in the call)", True)):
        with ops.deterministic_mode(det):
            y, _ = ops.MaskedRefineDual.apply(f, a, nbr, 0.5, 1.0, 1.0)
        res[name] = timed(lambda: torch.autograd.grad(y, f, go, retain_graph=True))
    out.append({"kernel": "masked_refine_backward", "variant": variant, "shape": {"B": B, "D": D, "n": n, "k": k}, **res})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["S", "XL", "both"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    args = ap.parse_args()
    for name in (("S", "XL") if args.config == "both" else (args.config,)):
        variant, batch, points = CONFIGS[name]
        if not args.kernels_only:
            for det in (False, True, False, True):
                try:
                    ms, loss = step_ms(variant, batch, points, det, args.steps, args.warmup)
                except RuntimeError as e:  # an operator of this configuration without a deterministic route says so
                    if not det or "no deterministic route" not in str(e):
                        raise
                    print(json.dumps({"step": f"PointNeXt-{variant} {batch} x {points}", "deterministic": det, "error": str(e)}), flush=True)
                    break
                print(json.dumps({"step": f"PointNeXt-{variant} {batch} x {points}", "deterministic": det, "ms_per_step": round(ms, 3),
                                  "loss": loss}), flush=True)
        if not args.steps_only:
            for row in kernels(variant, batch, points):
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
