"""The class-conditioned first feature-propagation block of the part-segmentation decoders, both ways:

    fused        blocks.feature_propagation_first_block(..., cloud=(e, E)): W_skip . f1 + c[b] in one kernel
                 (ops.pointwise_conv_cloud_term), + up(W_up . f2), BatchNorm, ReLU -- no (B, E + C1, N) tensor
    composition  the reference's expand + concatenate of e in front of f1, then the same block as it runs for any input
                 (W . [e ; f1] + up(W_up . f2): the kernels the library had before the per-cloud term)

forward alone (no autograd) and forward + backward to f1, f2, e and the block's parameters, for E in {16, 64, 208, 242} -- the
one-hot of PointNet2PartDecoder and the cls_map forms pointnet2 / pointnext1, curvenet, pointnext of PointNextPartDecoder -- and
E = 32, at 32 clouds of 2048 points (ShapeNetPart's shape class) and 8 clouds of 24000 (a scene-sized batch), with output widths
32, 64 and 128.  The fused route is FORCED (force_cloud_term) wherever the block has the form for it, so that both sides of the
shape dispatch of blocks.cloud_term_route are timed; the last column says what that rule chooses at the row's shape.  The
coarse cloud has half (PointNeXt at stride 2) or a quarter (stride 4) of the points.  Each is captured into a graph once and
replayed; the figure is the median HIP-event time of --repeats replays after --warmup.  Run it from the root of the tree whose
build it is to time:

    python tools/cloud_term_bench.py [--repeats 30]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from openpoints.models.backbone import FeaturePropogation  # noqa: E402
from openpoints.models.layers import (cloud_term_form, cloud_term_route, expand_cloud_channels,  # noqa: E402
                                      feature_propagation_first_block)

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=30)
opt = ap.parse_args()
assert opt.repeats >= 30
dev = torch.device("cuda:0")

# label, B, N, M (coarse points), C1 (skip), C2 (coarse), Cout
SHAPES = [("32 x 2048, PointNeXt-S", 32, 2048, 1024, 32, 64, 32),
          ("32 x 2048, width 64", 32, 2048, 1024, 16, 64, 64),
          ("32 x 2048, PointNet++", 32, 2048, 512, 7, 128, 128),
          ("8 x 24000, PointNeXt-S", 8, 24000, 12000, 32, 64, 32),
          ("8 x 24000, width 64", 8, 24000, 12000, 16, 64, 64),
          ("8 x 24000, PointNet++", 8, 24000, 6000, 7, 128, 128)]


def replay_us(fn):
    """median microseconds of a replay of fn() captured as a graph"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(opt.warmup):
        graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(opt.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); graph.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    del graph
    return ts[len(ts) // 2]


def fused(blk, f1, f2, geom, e):
    return feature_propagation_first_block(blk, f1, f2, geom, (e, e.shape[1]), force_cloud_term=True)


def composition(blk, f1, f2, geom, e):
    return feature_propagation_first_block(blk, expand_cloud_channels(e, f1), f2, geom)


def with_backward(route, blk, tensors, geom, g):
    """forward + backward on leaves made inside the call (a leaf autograd has seen on another stream would make it synchronise
    with that stream inside the capture)"""
    params = [p for p in blk.parameters()]

    def fn():
        leaves = [t.detach().requires_grad_(True) for t in tensors]
        return torch.autograd.grad(route(blk, leaves[0], leaves[1], geom, leaves[2]), leaves + params, g)
    return fn


print(f"{'shape':<24} {'E':>4} {'C1':>3} {'C2':>4} {'Cout':>4} | {'fwd fused':>9} {'compose':>8} | {'f+b fused':>9} {'compose':>8}   (us) | dispatched")
for label, B, N, M, C1, C2, Cout in SHAPES:
    gen = torch.Generator().manual_seed(0)
    p1 = torch.rand(B, N, 3, generator=gen).to(dev)
    p2 = p1[:, :M].contiguous()
    geom = FeaturePropogation.plan(p1, p2)
    f1 = torch.randn(B, C1, N, generator=gen).to(dev)
    f2 = torch.randn(B, C2, M, generator=gen).to(dev)
    g = torch.randn(B, Cout, N, generator=gen).to(dev)
    for E in (16, 32, 64, 208, 242):
        torch.manual_seed(1)
        blk = FeaturePropogation([E + C1 + C2, Cout, Cout]).to(dev).train().convs[0]
        e = torch.randn(B, E, generator=gen).to(dev)
        assert cloud_term_form(blk, f1, f2, e)
        with torch.no_grad():
            t_fused = replay_us(lambda: fused(blk, f1, f2, geom, e))
            t_comp = replay_us(lambda: composition(blk, f1, f2, geom, e))
        t_fused_fb = replay_us(with_backward(fused, blk, (f1, f2, e), geom, g))
        t_comp_fb = replay_us(with_backward(composition, blk, (f1, f2, e), geom, g))
        print(f"{label:<24} {E:>4} {C1:>3} {C2:>4} {Cout:>4} | {t_fused:9.1f} {t_comp:8.1f} | {t_fused_fb:9.1f} {t_comp_fb:8.1f}        | {cloud_term_route(blk, f1, f2, e)}", flush=True)
