"""One line `name sha256` per deterministic output of the contrast loss, for the library AMC3D_LIB names (default: the
tree's own build).  Two libraries with the same C ABI are compared by running this twice, each in a fresh process, and
diffing the outputs: a differing line means the order of some floating-point operation differs.

    AMC3D_LIB=/path/to/libamc3d_hip.so python tools/contrast_bits.py > bits.txt

Inputs come from amcontrast3d_amd.synthetic and fixed seeds only.  Graph A: 2 x 1,200 points, k = 23 (the `room` graph
of tests/test_gpu_contrast_fp64.py: spatially coherent labels, ambiguities with fixed shares of 0, 1, just above 1, 1e-30 and
a negative value).  Graph B: 257 points, k = 33 (the second chunk of every 32-wide loop).  Only what the kernels write is
hashed: sim, loss_pt and stats are torch.empty and filled for the selected anchors, so they are indexed by the selection
first.  The float-atomic routes are left out: their sums are unordered by design.
The `stages` lines are the five widths of a graph as five stages of one loss: by ops.contrast_stages_cm where the build
has it, otherwise by ops.contrast_stage_cm per stage, the head's additions and the weight as a Python product -- the same
lines from both, so the two builds' files are compared whole.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from amcontrast3d_amd import _lib, ops, synthetic  # noqa: E402

DEV = "cuda:0"
PRM = (-1.0, 0.5, 0.3)  # mu, nu, temperature
DEFAULT = ("adaptive", "-m", "Method1", 0.3)
VARIANTS = (("constant", "-m", "Method1", 0.3), ("adaptive", "+m", "Method2", 0.07), ("learned", "-m", "Method1", None))
A_SPECIAL = (0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 1e-30, -0.25)


def emit(name, t):
    print(name, hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest())


class Graph:
    def __init__(self, name, p, k, base, seed, B):
        self.name, self.B, self.k = name, B, k
        o = torch.tensor([p.shape[0]], dtype=torch.int32, device=DEV)
        idx, dist = ops.knnquery(k + 1, p, p, o, o)
        self.nidx, self.dist = idx[:, 1:], dist[:, 1:]
        m = self.m = p.shape[0]
        g = torch.Generator().manual_seed(seed)
        lab = torch.where(torch.rand(m, generator=g) < 0.25, torch.randint(0, 4, (m,), generator=g), base % 4)
        lab[p.cpu()[:, 0] < torch.quantile(p.cpu()[:, 0], 0.2)] = 0
        a = torch.rand(m, generator=g)
        u = torch.rand(m, generator=g)
        for lo, v in zip((0.0, 0.25, 0.30, 0.35, 0.40), A_SPECIAL):
            a[(u >= lo) & (u < (0.25 if lo == 0.0 else lo + 0.05))] = v
        self.a = a.to(DEV)
        self.keep = (0 < self.a) & (self.a <= 1)
        self.posmask = ops.posmask_from_labels(lab.int().to(DEV), self.nidx)
        self.anchors = ops.select_anchors(self.a)
        self.rev = ops.contrast_csr(self.nidx, self.anchors)
        self.mutual, self.rev_m = ops.contrast_mutual(self.nidx, self.a, self.dist)

    def features(self, C):
        return torch.randn(self.m, C, generator=torch.Generator().manual_seed(1000 + C)).to(DEV)


def stage_forward(G, f, tag, cm=False):
    """What contrast_stage's forward (cm: contrast_stage_cm's) writes per anchor -- sim (cm: stats, the cosines are not
    stored there) and loss_pt, which the autograd Functions keep to themselves or drop: the library entry they call, on
    buffers of this tool's own, with their arguments."""
    m, C, k = G.m, f.shape[1], G.k
    lib, P = _lib.load(), ops._ptr
    nidx = G.nidx if G.nidx.stride(1) == 1 else G.nidx.contiguous()
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=DEV)  # noqa: E731
    norm, sim, stats, loss_pt, mean_cnt = e(m), e(m, k), e(m, 2), e(m), e(2)
    unit = e(m, C) if lib.amc3d_contrast_backward_csr_supported(C) else None
    tail = (*PRM, P(norm), P(unit) if unit is not None else None, None if cm else P(sim), P(stats) if cm else None, P(loss_pt),
            P(mean_cnt), ops._stream(f))
    if cm:
        f_cm = f.view(G.B, m // G.B, C).transpose(1, 2).contiguous()
        _lib.check(lib.amc3d_contrast_forward_cm(G.B, C, m // G.B, k, nidx.stride(0), P(f_cm), P(nidx), P(G.posmask), P(G.a),
                                                 P(G.anchors), *tail), "contrast_forward_cm")
    else:
        _lib.check(lib.amc3d_contrast_forward(m, C, k, nidx.stride(0), P(f), P(nidx), P(G.posmask), P(G.a), P(G.anchors), *tail),
                   "contrast_forward")
    emit(f"{tag} {'stats' if cm else 'sim'}", (stats if cm else sim)[G.keep])
    emit(f"{tag} loss_pt", loss_pt[G.keep])
    emit(f"{tag} mean_cnt", mean_cnt)


def stage_grad(G, f, *plan):
    fg = f.clone().requires_grad_(True)
    loss = ops.contrast_stage(fg, G.nidx, G.posmask, G.a, *PRM, *plan)
    (loss * 0.9).backward()
    return loss.detach(), fg.grad


def stages(G, widths, scale=0.9):
    """total, per-stage loss and channel-major gradient of the stages (G, C), C in widths"""
    fs = [G.features(C).view(G.B, G.m // G.B, C).transpose(1, 2).contiguous().requires_grad_(True) for C in widths]
    plan = (G.nidx, G.posmask, G.a, G.anchors, G.rev_m, G.mutual)
    if hasattr(ops, "contrast_stages_cm"):
        total, means = ops.contrast_stages_cm([(f, *plan) for f in fs], *PRM, scale)
        losses = [means[i, 0] for i in range(len(fs))]
    else:
        loss_sum, losses = 0, []
        for f in fs:
            loss = ops.contrast_stage_cm(f, G.nidx, G.posmask, G.a, *PRM, G.anchors, G.rev_m, G.mutual)
            losses.append(loss.detach().clone())
            loss_sum += loss
        total = scale * loss_sum
    total.backward(torch.tensor(0.7, device=DEV))
    emit(f"graph={G.name} stages total", total)
    for C, loss, f in zip(widths, losses, fs):
        emit(f"graph={G.name} stages C={C} loss", loss)
        emit(f"graph={G.name} stages C={C} grad_cm", f.grad)


def variant(G, f, form, tag, grad=True):
    b = ops.contrast_variant_forward(f, G.nidx, G.posmask, G.a, ops.contrast_form(*form), PRM[0], PRM[1], G.anchors)
    emit(f"{tag} sim", b["sim"][G.keep])
    emit(f"{tag} loss_pt", b["loss_pt"][G.keep])
    emit(f"{tag} loss", b["mean_cnt"])
    if grad:
        fg = f.clone().requires_grad_(True)
        loss = ops.contrast_stage_variant(fg, G.nidx, G.posmask, G.a, *form[:3], PRM[0], PRM[1], form[3], G.anchors, G.rev)
        (loss * 0.9).backward()
        emit(f"{tag} grad_rev", fg.grad)


def main():
    nb = synthetic.make_batch(2, 1200)
    pA = torch.from_numpy(nb["pos"]).reshape(-1, 3).contiguous().to(DEV)
    graphs = [Graph("A", pA, 23, torch.from_numpy(nb["y"]).reshape(-1), 11, 2),
              Graph("B", pA[:257].contiguous(), 33, torch.from_numpy(nb["y"]).reshape(-1)[:257], 12, 1)]
    for G in graphs:
        for C in (16, 32, 64, 128, 256):
            f, tag = G.features(C), f"graph={G.name} C={C} default"
            variant(G, f, DEFAULT, tag + " variant_forward", grad=False)
            stage_forward(G, f, tag + " stage_forward")
            stage_forward(G, f, tag + " cm_forward", cm=True)
            loss, grad = stage_grad(G, f, G.anchors, G.rev)
            emit(f"{tag} stage loss", loss)
            emit(f"{tag} grad_csr", grad)
            emit(f"{tag} grad_mutual", stage_grad(G, f, G.anchors, G.rev_m, G.mutual)[1])
            f_cm = f.view(G.B, G.m // G.B, C).transpose(1, 2).contiguous().requires_grad_(True)
            loss = ops.contrast_stage_cm(f_cm, G.nidx, G.posmask, G.a, *PRM, G.anchors, G.rev_m, G.mutual)
            (loss * 0.9).backward()
            emit(f"{tag} cm loss", loss.detach())
            emit(f"{tag} grad_cm", f_cm.grad)
        stages(G, (16, 32, 64, 128, 256))
        stages(G, (256, 64))
        for C in (5, 33):  # the general forward kernels
            f = G.features(C)
            emit(f"graph={G.name} C={C} default stage loss", stage_grad(G, f, G.anchors)[0])
            stage_forward(G, f, f"graph={G.name} C={C} default stage_forward")
            variant(G, f, DEFAULT, f"graph={G.name} C={C} default variant_forward", grad=False)
        for form in VARIANTS:
            variant(G, G.features(64), form, f"graph={G.name} C=64 form={','.join(map(str, form))}")
        with ops.deterministic_mode():  # the wide rows kernel
            for C in (20, 260, 512):
                f = G.features(C)
                emit(f"graph={G.name} C={C} deterministic default grad", stage_grad(G, f, G.anchors, G.rev)[1])
                fg = f.clone().requires_grad_(True)
                form = VARIANTS[1]
                loss = ops.contrast_stage_variant(fg, G.nidx, G.posmask, G.a, *form[:3], PRM[0], PRM[1], form[3], G.anchors, G.rev)
                (loss * 0.9).backward()
                emit(f"graph={G.name} C={C} deterministic form={','.join(map(str, form))} grad", fg.grad)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
