"""Times the compiled transform chain (amcontrast3d_amd.transforms, csrc/transforms.hip) against what it replaces.

    python tools/transform_bench.py [--rounds 30] [--inner 5] [--out profiles/transform_chain_bench.txt]

Cases: the S3DIS default chain on a dense 8 x 24000 batch; the upstream-style ScanNet chain and the ScanNet default chain on
two ragged rooms of about 150 k points.  Candidates per case: the chain; the same chain as a composition of torch ops on the
device (what a user could write without this module); the fixed class (S3DISTrainAugment / ScanNetTrainAugment) where the
chain equals theirs.  Every candidate gets its draws ready-made, so the time is the transform's own: the per-cloud tables and
the kernels.  Device events around `inner` calls; the candidates alternate inside every round of one process; after warm-up.
Reported: median and the 10th .. 90th percentile over the rounds (the spread), per call, and the number of GPU kernels one
call launches."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from amcontrast3d_amd.augment import S3DISTrainAugment, ScanNetTrainAugment  # noqa: E402
from amcontrast3d_amd.transforms import TransformChain  # noqa: E402

DEV = "cuda:0"
S3DIS = ["ChromaticAutoContrast", "PointsToTensor", "PointCloudScaling", "PointCloudXYZAlign", "PointCloudRotation", "PointCloudJitter",
         "ChromaticDropGPU", "ChromaticNormalize"]
S3DIS_KW = {"color_drop": 0.2, "gravity_dim": 2, "scale": [0.9, 1.1], "angle": [0, 0, 1], "jitter_sigma": 0.005, "jitter_clip": 0.02}
SCANNET = ["RandomRotateZ", "RandomScale", "ChromaticAutoContrast", "RandomDropFeature", "NumpyChromaticNormalize"]
UPSTREAM = ["RandomRotateZ", "RandomScale", "RandomFlip", "RandomJitter", "ChromaticAutoContrast", "ChromaticTranslation", "ChromaticJitter",
            "HueSaturationTranslation", "RandomDropFeature", "NumpyChromaticNormalize"]
SCANNET_KW = {"color_drop": 0.2, "gravity_dim": 2, "rotate_dim": 2, "scale": [0.8, 1.2], "mirror": [0.2, -1, -1], "angle": 1,
              "color_mean": [0.46259782, 0.46253258, 0.46253258], "color_std": [0.693565, 0.6852543, 0.68061745]}
MEAN = (0.5136457, 0.49523646, 0.44921124)
STD = (0.18308958, 0.18415008, 0.19252081)


def torch_s3dis(pos, x, d):
    """the S3DIS default chain as batched torch ops, (B,N,3)"""
    B = pos.shape[0]
    taken = (d["0.u"] < 0.2).view(B, 1, 1)
    lo, hi = x.min(1, keepdim=True).values, x.max(1, keepdim=True).values
    blend = d["0.blend"].float().view(B, 1, 1)
    x = torch.where(taken, (1 - blend) * x + blend * ((x - lo) * (255 / (hi - lo))), x)
    pos = pos * (d["2.scale_u"] * (1.1 - 0.9) + 0.9).view(B, 1, 3)
    pos = pos - pos.mean(1, keepdim=True)
    pos[..., 2] -= pos[..., 2].min(1, keepdim=True).values
    t = d["4.theta"][:, 2]
    c, s, z, o = torch.cos(t), torch.sin(t), torch.zeros_like(t), torch.ones_like(t)
    rot = torch.stack([c, -s, z, s, c, z, z, z, o], 1).view(B, 3, 3).float()
    pos = pos @ rot.transpose(1, 2)
    pos = pos + (d["5.noise"].view(B, -1, 3) * 0.005).clamp_(-0.02, 0.02)
    x = torch.where((d["6.u"] < 0.2).view(B, 1, 1), torch.zeros_like(x), x)
    big = x.amax((1, 2), keepdim=True) > 1
    x = torch.where(big, x / 255., x)
    mean, std = x.new_tensor(MEAN), x.new_tensor(STD)  # a user's code would keep these on the device
    return pos, (x - mean) / std


def hsv_torch(x, hue_val, sat_ratio):
    rgb = x.double()
    r, g, b = rgb.unbind(-1)
    v, lo = rgb.max(-1).values, rgb.min(-1).values
    span = torch.where(v == lo, torch.ones_like(v), v - lo)
    s = torch.where(v == lo, torch.zeros_like(v), (v - lo) / torch.where(v == lo, torch.ones_like(v), v))
    rc, gc, bc = (v - r) / span, (v - g) / span, (v - b) / span
    h = torch.where(r == v, bc - gc, torch.where(g == v, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.remainder(h / 6.0, 1.0)
    h = torch.remainder(hue_val + h + 1, 1.0)
    s = (sat_ratio * s).clamp(0, 1)
    i = (h * 6.0).to(torch.uint8)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i % 6
    pick = lambda opts: torch.stack(opts, 0).gather(0, i.long().unsqueeze(0)).squeeze(0)  # noqa: E731
    out = torch.stack([pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])], -1)
    out = torch.where((s == 0).unsqueeze(-1), v.unsqueeze(-1).expand_as(out), out)
    return out.to(torch.uint8).float()


def torch_scannet(names, coord, feat, sizes, d):
    """a ScanNet chain as torch ops, room by room (the rooms are ragged)"""
    P, X, beg = [], [], 0
    for b, n in enumerate(sizes):
        pos, x = coord[beg:beg + n], (feat[beg:beg + n] + 1) * 127.5
        for i, name in enumerate(names):
            k = f"{i}."
            if name == "RandomRotateZ":
                t = d[k + "angle"][b]
                c, s, z, o = torch.cos(t), torch.sin(t), torch.zeros_like(t), torch.ones_like(t)
                pos = pos.double() @ torch.stack([c, -s, z, s, c, z, z, z, o]).view(3, 3)
            elif name == "RandomScale":
                m = (d[k + "mirror_u"][b] > d["_mirror"]).double() * 2 - 1
                pos = pos * (d[k + "scale"][b] * m)
            elif name == "RandomFlip":
                pos = pos * torch.cat([1 - 2 * (d[k + "u"][b] < 0.5).double(), d["_one"]])
            elif name == "RandomJitter":
                pos = pos + (0.01 * d[k + "noise"][beg:beg + n]).clamp(-0.05, 0.05)
            elif name == "ChromaticAutoContrast":
                lo, hi = x.min(0, keepdim=True).values, x.max(0, keepdim=True).values
                blend = d[k + "blend"][b].float()
                x = torch.where(d[k + "u"][b] < 0.2, (1 - blend) * x + blend * ((x - lo) * (255 / (hi - lo))), x)
            elif name == "ChromaticTranslation":
                tr = (d[k + "tr_u"][b] - 0.5) * 255 * 2 * 0.05
                x = torch.where(d[k + "u"][b] < 0.95, (tr + x).clamp(0, 255).float(), x)
            elif name == "ChromaticJitter":
                x = torch.where(d[k + "u"][b] < 0.95, (d[k + "noise"][beg:beg + n] * (0.005 * 255) + x).clamp(0, 255).float(), x)
            elif name == "HueSaturationTranslation":
                x = hsv_torch(x, (d[k + "hue_u"][b] - 0.5) * 2 * 0.5, 1 + (d[k + "sat_u"][b] - 0.5) * 2 * 0.2)
            elif name == "RandomDropFeature":
                x = torch.where(d[k + "u"][b] < 0.2, torch.zeros_like(x), x)
            elif name == "NumpyChromaticNormalize":
                x = torch.where(x.max() > 1, x / 255., x)
                x = (x - d["_mean"]) / d["_std"]
        P.append(pos)
        X.append(x)
        beg += n
    return torch.cat(P), torch.cat(X)


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:  # the profiler is a convenience here, not the measurement
        return f"n/a ({type(e).__name__})"


def measure(cands, rounds, inner, warmup=10):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for r in range(rounds):
        order = list(cands) if r % 2 == 0 else list(cands)[::-1]
        for k in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                cands[k]()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner * 1000.0)
    return times


def big_room(seed, side=275):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * 0.022
    base = np.concatenate([g, (0.4 * np.sin(g[:, 0]) + rng.choice([0.0, 0.8], len(g)))[:, None]], 1)
    coord = np.concatenate([base + rng.uniform(-0.003, 0.003, base.shape) for _ in range(2)], 0).astype(np.float32)
    return torch.from_numpy(coord).to(DEV), torch.from_numpy(rng.uniform(-1, 1, coord.shape).astype(np.float32)).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = [f"device {torch.cuda.get_device_name(0)}; rounds {a.rounds} x inner {a.inner}; microseconds per call: median [p10 .. p90]"]
    cases = []

    # ---- S3DIS default, dense 8 x 24000
    B, N = 8, 24000
    pos = torch.rand(B, N, 3, device=DEV, generator=gen) * 6
    col = torch.round(torch.rand(B, N, 3, device=DEV, generator=gen) * 255)
    chain = TransformChain(S3DIS, S3DIS_KW)
    d = chain.draw([N] * B, DEV, gen)
    d["0.u"][::2] = 0.0  # contrast taken in half of the clouds
    aug = S3DISTrainAugment(**S3DIS_KW)
    fd = {"contrast": d["0.u"] < 0.2, "blend": d["0.blend"].float(), "scale_u": d["2.scale_u"], "theta": d["4.theta"],
          "noise": d["5.noise"].view(B, N, 3), "drop": d["6.u"] < 0.2}
    cases.append((f"S3DIS default chain, dense {B} x {N}", chain.plan(), {
        "chain": lambda: chain({"pos": pos, "x": col}, draws=d),
        "torch composition": lambda: torch_s3dis(pos, col, d),
        "S3DISTrainAugment": lambda: aug(pos, col, draws=fd)}))

    # ---- ScanNet chains, two ragged rooms
    rooms = [big_room(1), big_room(2, 270)]
    sizes = [int(c.shape[0]) for c, _ in rooms]
    coord, feat = torch.cat([c for c, _ in rooms]), torch.cat([f for _, f in rooms])
    off = torch.tensor([0, sizes[0], sum(sizes)], dtype=torch.int64, device=DEV)
    extra = {"_mirror": torch.tensor([0.2, -1, -1], dtype=torch.float64, device=DEV), "_one": torch.ones(1, dtype=torch.float64, device=DEV),
             "_mean": torch.tensor(SCANNET_KW["color_mean"], device=DEV), "_std": torch.tensor(SCANNET_KW["color_std"], device=DEV)}
    for title, names in ((f"upstream-style ScanNet chain, ragged rooms {sizes}", UPSTREAM), (f"ScanNet default chain, ragged rooms {sizes}", SCANNET)):
        ch = TransformChain(names, SCANNET_KW)
        dd = ch.draw(sizes, DEV, gen)
        data = {"pos": coord, "x": feat, "offsets": off, "sizes": sizes}
        cands = {"chain": (lambda ch=ch, dd=dd: ch(data, draws=dd, scannet_colour=True, want_heights=False)),
                 "torch composition": (lambda names=names, dd=dd: torch_scannet(names, coord, feat, sizes, dict(dd, **extra)))}
        if names == SCANNET:
            fa = ScanNetTrainAugment(**SCANNET_KW)
            hd = {"angle": dd["0.angle"].cpu(), "scale": dd["1.scale"].reshape(-1).cpu(), "mirror_u": dd["1.mirror_u"].cpu(),
                  "contrast_u": dd["2.u"].cpu(), "blend": dd["2.blend"].cpu(), "drop_u": dd["3.u"].cpu()}
            cands["ScanNetTrainAugment"] = lambda fa=fa, hd=hd: fa(coord, feat, off, draws=hd)
        cases.append((title, ch.plan(), cands))

    for title, plan, cands in cases:
        lines.append("")
        lines.append(f"{title}: {len(plan['micro'])} micro-ops, {plan['phases']} reduction phases, {plan['launches']} launches of the chain kernel")
        times = measure(cands, a.rounds, a.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        q = {k: (float(np.percentile(v, 10)), float(np.percentile(v, 90))) for k, v in times.items()}
        for k, v in times.items():
            lines.append(f"  {k:22s} {med[k]:9.1f} [{q[k][0]:9.1f} .. {q[k][1]:9.1f}]   GPU kernels per call: {count_kernels(cands[k])}")
        spread = max(hi - lo for lo, hi in q.values())
        lines.append(f"  chain vs torch composition: {med['torch composition'] / med['chain']:.2f}x faster "
                     f"(difference {med['torch composition'] - med['chain']:.1f} us, largest spread {spread:.1f} us: "
                     f"{'beyond' if q['torch composition'][0] > q['chain'][1] else 'NOT beyond'} the spread)")
        for k in cands:
            if k.endswith("TrainAugment"):
                lines.append(f"  chain / {k}: {med['chain'] / med[k]:.2f} (time ratio; above 1: the fixed kernels are faster)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
