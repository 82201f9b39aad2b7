"""ms per train step of the plain PointNeXt baseline beside AMContrast3D's -- and, with --models, beside the PointNet++ and
ASSANet baselines (configs.model_cfg_pointnet2) -- through the same loop in one run.

Both models are PointNeXt-S on synthetic rooms (amcontrast3d_amd.synthetic), 8 x 24000 points by default; each is trained by
train.train_one_epoch with FusedAdamW on the captured pipeline: one epoch that builds the pipeline and warms it up, then timed
epochs, the two models taking turns.  The time is the host clock around an epoch that ends in a device synchronise, over its
batches -- pipeline fill and drain included, which is why an epoch is long.  Prints one JSON line.
PointNet++ / ASSANet ('pointnet++', 'pointnet++msg', 'assanet') have no captured pipeline yet and run train_one_epoch's eager
loop; 'pointnext-eager' is PointNeXt-S through that same eager loop (cfg.graph_pipeline = False), the like-for-like neighbour.

    python tools/baseline_step_bench.py [--batch 8] [--points 24000] [--steps 60] [--epochs 3]
                                        [--models amcontrast3d,pointnext,pointnext-eager,pointnet++,pointnet++msg,assanet]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import amcontrast3d_amd  # noqa: E402
from amcontrast3d_amd import configs, synthetic, train  # noqa: E402


class Loader:
    """`steps` batches per epoch cycling over a few rooms, in the reference's collated layout; a fresh dict per batch (the
    loop writes into it)"""

    def __init__(self, batch, points, steps, distinct=4):
        self.steps, self.rooms = steps, []
        for k in range(distinct):
            nb = synthetic.make_batch(batch, points, first_id=500 + batch * k)
            x = torch.from_numpy(nb["x"]).transpose(1, 2).contiguous()
            self.rooms.append({"pos": torch.from_numpy(nb["pos"]).cuda(), "y": torch.from_numpy(nb["y"]).cuda(),
                               "x": x[..., :3].contiguous().cuda(), "heights": x[..., 3:4].contiguous().cuda()})

    def __iter__(self):
        return (dict(self.rooms[k % len(self.rooms)]) for k in range(self.steps))


def make(kind):
    amcontrast3d_amd.activate()
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(0)
    m = configs.model_cfg("S")
    crit = configs.criterion_cfg()
    if kind in ("pointnet++", "pointnet++msg", "assanet", "assanet-l"):
        m = configs.model_cfg_pointnet2(kind)
        crit = {"NAME": "CrossEntropy", "label_smoothing": 0.2}
    elif kind in ("pointnext", "pointnext-eager"):
        m["NAME"], m["encoder_args"]["NAME"], m["decoder_args"]["NAME"] = "BaseSeg", "PointNextEncoder", "PointNextDecoder"
        crit = {"NAME": "CrossEntropy", "label_smoothing": 0.2}  # cfgs/s3dis/default.yaml criterion_args
    c = EasyConfig(); c.update(m)
    model = build_model_from_cfg(c).cuda()
    cc = EasyConfig(); cc.update(crit)
    cfg = EasyConfig()
    cfg.update({"num_classes": 13, "ignore_index": None, "ambiguity_args": configs.ambiguity_args("s3dis"), "feature_keys": "x,heights",
                "use_amp": False, "step_per_update": 1, "grad_norm_clip": 10, "sched_on_epoch": True,
                "graph_pipeline": kind != "pointnext-eager"})
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=1e-4)
    return model, build_criterion_from_cfg(cc).cuda(), opt, cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--models", default="amcontrast3d,pointnext")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    loader = Loader(a.batch, a.points, a.steps)
    sides = {k: make(k) for k in a.models.split(",")}
    ms = {k: [] for k in sides}
    for epoch in range(a.epochs + 1):  # epoch 0 builds and warms the pipelines
        for k, (model, crit, opt, cfg) in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = train.train_one_epoch(model, loader, crit, opt, None, None, epoch + 1, cfg)
            torch.cuda.synchronize()
            if epoch:
                ms[k].append(round((time.perf_counter() - t0) / a.steps * 1e3, 3))
            assert out[0] == out[0], "the loss is NaN"
    print(json.dumps({"model": "PointNeXt-S" if a.models == "amcontrast3d,pointnext" else a.models, "batch": a.batch, "points": a.points, "steps_per_epoch": a.steps,
                      "ms_per_step_epochs": ms, "ms_per_step": {k: min(v) for k, v in ms.items()},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
