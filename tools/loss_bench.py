"""Each plain criterion of openpoints.loss (the registry's CrossEntropy with smoothing / weights among them), forward +
backward, on the point-loss kernels against the torch composition of the same module on the same inputs (the route CPU tensors and (M, C) rows take, here run on the device), at 8 x 13 x 24000 and
2 x 20 x 64000 logits: device-event times, median of --repeats calls after --warmup untimed ones.

    python tools/loss_bench.py [--repeats 50] [--warmup 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from openpoints.loss import build as loss_build  # noqa: E402
from openpoints.loss import build_criterion_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=50)
opt = ap.parse_args()
dev = torch.device("cuda:0")


def forms(C):
    w = 0.5 + 1.5 * ((np.arange(C) * 7) % 5) / 4.0
    return [("CrossEntropy label_smoothing=0.2", {"label_smoothing": 0.2}),
            ("CrossEntropy label_smoothing=0.2 weight", {"label_smoothing": 0.2, "weight": torch.tensor(w, dtype=torch.float32)}),
            ("SmoothCrossEntropy", {}), ("SmoothCrossEntropy eps=0 weight", {"label_smoothing": 0, "weight": w}),
            ("SmoothCrossEntropy ignore_index=3 weight", {"ignore_index": 3, "num_classes": C, "weight": w}),
            ("MaskedCrossEntropy", {}), ("BCELogits", {}), ("FocalLoss gamma=2", {"gamma": 2}),
            ("FocalLoss gamma=0.5 alpha", {"gamma": 0.5, "alpha": [0.5] * C}), ("Poly1CrossEntropyLoss", {"num_classes": C}),
            ("Poly1FocalLoss", {}), ("Poly1FocalLoss gamma=1.5", {"alpha": -1, "gamma": 1.5, "epsilon": 0.5})]


def timed(step):
    """median ms of step() between two events"""
    for _ in range(opt.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(opt.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


kernel_route = loss_build._kernel_route
print("| criterion | B x C x N | kernels fwd+bwd (us) | torch composition fwd+bwd (us) | ratio | bytes 4BCN x 3 at kernel time (TB/s) |")
print("|---|---|---|---|---|---|")
for B, C, N in ((8, 13, 24000), (2, 20, 64000)):
    g = torch.Generator().manual_seed(C)
    logits = (torch.randn(B, C, N, generator=g) * 3).to(dev).requires_grad_(True)
    target = torch.randint(0, C, (B, N), generator=g).to(dev)
    mask = (torch.rand(B, N, generator=g) >= 0.3).long().to(dev)
    for label, kwargs in forms(C):
        name = label.split()[0]
        cfg = EasyConfig(); cfg.update(dict(kwargs, NAME=name))
        crit = build_criterion_from_cfg(cfg).to(dev)
        args = (logits, target, mask) if name == "MaskedCrossEntropy" else (logits, target)

        def step():
            logits.grad = None
            crit(*args).backward()
        values, times = [], []
        for route in (kernel_route, lambda *a: False):
            loss_build._kernel_route = route
            values.append(float(crit(*args).detach()))
            times.append(timed(step))
        loss_build._kernel_route = kernel_route
        assert abs(values[0] - values[1]) <= 1e-4 * max(1.0, abs(values[1])), (label, values)
        tbs = 3 * 4 * B * C * N / (times[0] * 1e-3) / 1e12  # one read forward, one read and one write backward
        print(f"| {label} | {B} x {C} x {N} | {times[0] * 1e3:.0f} | {times[1] * 1e3:.0f} | {times[1] / times[0]:.1f}x | {tbs:.2f} |")
