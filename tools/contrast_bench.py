"""contrast_stage forward / backward on the loss stages of one synthetic S3DIS-like batch (8 x 24000), per stage, HIP-event
times; AMC3D_LIB selects another build of the library with the same C ABI (an A/B against a parent commit's).

    python tools/contrast_bench.py                               the default (fused) stage, then all four stages of the batch on
        channel-major embeddings: ops.contrast_stage_cm per stage with the head's additions and the loss weight (the route one
        call replaces, glue included), and ops.contrast_stages_cm, the one call
    python tools/contrast_bench.py --form constant,-m,Method1,0.3   another form of the loss (margin,db,method,T; T may be None):
        ops.contrast_stage_variant with reverse lists (gather), without (float atomics), the torch composition of
        ContrastHead.point_contrast_margin's CPU branch run on the device (with its peak memory), and the default stage for scale
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from amcontrast3d_amd import configs, geometry, ops, synthetic  # noqa: E402
from openpoints.loss import build_criterion_from_cfg  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--form", default=None, help="margin,db,method,T  e.g. learned,+m,Method2,None")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
opt = ap.parse_args()

dev = torch.device("cuda:0")
c = EasyConfig(); c.update(configs.model_cfg("S", dropout=0.5)); model = build_model_from_cfg(c).to(dev).train()
cc = EasyConfig(); cc.update(configs.criterion_cfg()); crit = build_criterion_from_cfg(cc).to(dev)
aa = EasyConfig(); aa.update(configs.ambiguity_args("s3dis"))
data = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(8, 24000).items()}
plan = geometry.precompute(model, crit.contrast_head, data, 13, None, aa)
torch.manual_seed(0)


def timed(f, fwd):
    """-> (forward ms, backward ms): medians over opt.repeats after opt.warmup untimed passes; f: the leaf or leaves"""
    leaves = f if isinstance(f, (list, tuple)) else [f]
    for _ in range(opt.warmup):
        for x in leaves:
            x.grad = None
        fwd().backward()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf, tb = [], []
    for _ in range(opt.repeats):
        for x in leaves:
            x.grad = None
        e[0].record(); l = fwd(); e[1].record(); l.backward(); e[2].record(); torch.cuda.synchronize()
        tf.append(e[0].elapsed_time(e[1])); tb.append(e[1].elapsed_time(e[2]))
    return sorted(tf)[len(tf) // 2], sorted(tb)[len(tb) // 2]


form = None
if opt.form:
    margin, db, method, T = opt.form.split(",")
    form = (margin, db, method, None if T in ("None", "null", "") else float(T))
    fa = EasyConfig(); fa.update(dict(configs.ambiguity_args("s3dis"), margin=form[0], db=form[1], supervisedCL=form[2], temperature=form[3]))

for i, (g, C) in enumerate(zip(plan["loss"], (32, 64, 128, 256))):
    m = g["neighbor_idx"].shape[0]
    f = torch.randn(m, C, device=dev, requires_grad=True)
    sel = int(g["anchors"][0])

    def fwd():
        return ops.contrast_stage(f, g["neighbor_idx"], g["posmask"], g["ambiguity"], aa.mu, aa.nu, aa.temperature, g["anchors"], g.get("rev"), g.get("mutual"))
    tf, tb = timed(f, fwd)
    mb = sel * 24 * C * 4 / 1e6
    if form is None:
        print(f"stage {i}: m={m} C={C} selected={sel} ({100*sel/m:.1f} %)  fwd {tf*1e3:.0f} us  bwd {tb*1e3:.0f} us  rows {mb:.0f} MB -> bwd atomics at {mb/tb/1e3:.2f} TB/s")
        continue
    print(f"form {opt.form} stage {i}: m={m} C={C} selected={sel}  default-fused  fwd {tf*1e3:.0f} us  bwd {tb*1e3:.0f} us  total {(tf+tb)*1e3:.0f} us")
    rev = ops.contrast_csr(g["neighbor_idx"], g["anchors"])
    for name, r in (("variant-rev", rev), ("variant-atomic", None)):
        def fwd_v():
            return ops.contrast_stage_variant(f, g["neighbor_idx"], g["posmask"], g["ambiguity"], *form[:3], aa.mu, aa.nu, form[3], g["anchors"], r)
        tf, tb = timed(f, fwd_v)
        print(f"form {opt.form} stage {i}: m={m} C={C} selected={sel}  {name}  fwd {tf*1e3:.0f} us  bwd {tb*1e3:.0f} us  total {(tf+tb)*1e3:.0f} us")

    def fwd_t():  # the torch composition (MarginContrast.py: the branch CPU tensors take), on the device
        keep = torch.logical_and(0 < g["ambiguity"], g["ambiguity"] <= 1)
        k = g["neighbor_idx"].shape[1]
        nf = f[g["neighbor_idx"].reshape(-1).long(), :].view(m, k, C)
        dist = crit.contrast_head.dist_func(f[keep], nf[keep])
        return torch.mean(crit.contrast_head.contrast_func(dist, g["posmask"][keep], g["ambiguity"][keep], fa))
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    tf, tb = timed(f, fwd_t)
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    print(f"form {opt.form} stage {i}: m={m} C={C} selected={sel}  torch-composition  fwd {tf*1e3:.0f} us  bwd {tb*1e3:.0f} us  total {(tf+tb)*1e3:.0f} us  peak +{peak:.0f} MB")

if form is None:
    widths = (32, 64, 128, 256)
    fs = [torch.randn(8, C, g["neighbor_idx"].shape[0] // 8, device=dev, requires_grad=True) for g, C in zip(plan["loss"], widths)]
    plans = [(g["neighbor_idx"], g["posmask"], g["ambiguity"], g["anchors"], g["rev"], g["mutual"]) for g in plan["loss"]]

    def fwd_loop():
        loss_sum = 0
        for f, (nidx, posmask, a, anchors, rev, mutual) in zip(fs, plans):
            loss_sum += ops.contrast_stage_cm(f, nidx, posmask, a, aa.mu, aa.nu, aa.temperature, anchors, rev, mutual)
        return aa.w2 * loss_sum
    tf, tb = timed(fs, fwd_loop)
    print(f"four stages, channel-major, one call per stage + additions + weight: fwd {tf*1e3:.0f} us  bwd {tb*1e3:.0f} us  total {(tf+tb)*1e3:.0f} us")
    if hasattr(ops, "contrast_stages_cm"):
        def fwd_merged():
            return ops.contrast_stages_cm([(f, *p) for f, p in zip(fs, plans)], aa.mu, aa.nu, aa.temperature, aa.w2)[0]
        tf, tb = timed(fs, fwd_merged)
        print(f"four stages, channel-major, one call (contrast_stages_cm): fwd {tf*1e3:.0f} us  bwd {tb*1e3:.0f} us  total {(tf+tb)*1e3:.0f} us")
        # the backward entry per width, one stage per call, opt.repeats calls back to back between two events: what a build
        # with another gradient tile changes (profiles/contrast_stages_tile_sweep.txt)
        from amcontrast3d_amd import _lib
        lib, P = _lib.load(), ops._ptr
        sts = []
        for f, (nidx, posmask, a, anchors, rev, mutual) in zip(fs, plans):
            b, C, n = f.shape
            e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
            sts.append(dict(b=b, C=C, n=n, k=nidx.shape[1], nbr_stride=nidx.stride(0), f_cm=f.detach(), nbr=nidx, posmask=posmask,
                            a=a, sel=anchors, mutual=mutual, rev=rev, norm=e(b * n), unit=e(b * n, C), stats=e(b * n, 2),
                            loss_pt=e(b * n), mean_cnt=e(2), grad_cm=e(b, C, n)))
        prm = (float(aa.mu), float(aa.nu), float(aa.temperature), float(aa.w2))
        total, g = torch.empty(1, device=dev), torch.ones(1, device=dev)
        for group in [[st] for st in sts] + [sts]:
            descs = ops._contrast_stage_descs(group)
            wb = int(lib.amc3d_contrast_stages_backward_cm_workspace_bytes(len(group), descs))
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
            _lib.check(lib.amc3d_contrast_stages_forward_cm(len(group), descs, *prm, P(total), ops._stream(total)), "forward")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(2):  # (the second pass is the timed one)
                ev[0].record()
                for _ in range(opt.repeats):
                    _lib.check(lib.amc3d_contrast_stages_backward_cm(len(group), descs, *prm, P(g), P(work), wb, ops._stream(total)),
                               "backward")
                ev[1].record(); torch.cuda.synchronize()
            what = f"C={group[0]['C']} n={group[0]['n']}" if len(group) == 1 else "the four stages in one call"
            print(f"backward entry alone, {what}: {ev[0].elapsed_time(ev[1]) / opt.repeats * 1e3:.1f} us per call (records + gather)")
    else:
        print("four stages, channel-major, one call (contrast_stages_cm): not in this build")
