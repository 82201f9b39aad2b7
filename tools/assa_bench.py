"""The separable aggregation of ASSA (ops.SeparableAggregation, csrc/assa.hip) alone, at the shapes and on the geometry of a
real step: every ASSA layer of configs.model_cfg_pointnet2('assanet') on one synthetic S3DIS-like batch of 8 x 24000 points
(the stem's self query of 24000 points, per stage one strided query N -> N/4 and the self queries of the sampled cloud),
radius 0.1 doubling per stage, 32 neighbours, the plan of PointNet2Encoder.plan_geometry.  Each distinct (C, N, M) is timed:

    kernel       the forward entry alone, with its achieved bytes per second over the algorithmic bytes (f rows once, idx,
                 dp, output) against the HBM roof
    fwd          the operator (point-major copy of f + the kernel) beside the reference's expression on the device:
                 grouping_operation, expand, multiply, mean / max over (B,3C,M,K)
    f+b          forward + backward of both through autograd (the operator's backward in its default dispatch)
    bwd          the two backward entries alone on a point-major gradient: float atomics (zero-fill included) and the gather
                 over reverse lists, and what building those lists costs when the plan does not carry them (group_csr)

Each is captured into a graph once and replayed; the figure is the median HIP-event time of --repeats replays after --warmup.
Run it from the root of the tree whose build it is to time:

    python tools/assa_bench.py [--reductions mean,max] [--repeats 30]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from amcontrast3d_amd import _lib, configs, ops, roofline, synthetic  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.models.layers import ASSA, grouping_operation  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reductions", default="mean,max")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--points", type=int, default=24000)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=30)
opt = ap.parse_args()
assert opt.repeats >= 30

dev = torch.device("cuda:0")
lib, P = _lib.load(), ops._ptr


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


def shapes():
    """-> [(label, C, N, idx, dp)]: one entry per distinct (C, N, M) of the model's ASSA layers, on their real geometry"""
    c = EasyConfig()
    c.update(configs.model_cfg_pointnet2("assanet", nsample=32))
    enc = build_model_from_cfg(c).encoder.to(dev)
    pos = torch.from_numpy(synthetic.make_batch(opt.batch, opt.points)["pos"]).to(dev)
    plan = enc.plan_geometry(pos)
    out, seen = [], set()

    def add(label, op, g, n):
        assert isinstance(op, ASSA)
        C = op.convs[op.num_preconv - 1][0].out_channels
        key = (C, n, g["idx"].shape[1])
        if key not in seen:
            seen.add(key)
            out.append((label, C, n, g["idx"], g["dp"]))
    add("stem", enc.stem.SA_CONFIG_operator, plan["stem"], pos.shape[1])
    n = pos.shape[1]
    for s, (sa, g) in enumerate(zip(enc.SA_modules, plan["modules"])):
        for j, (la, gb) in enumerate(zip(sa.local_aggregations, g["blocks"])):
            add(f"stage {s} block {j}", la.SA_CONFIG_operator, gb, n if j == 0 else g["new_p"].shape[1])
        n = g["new_p"].shape[1]
    return out


def composition(f, idx, dp, reduction):
    fj = grouping_operation(f, idx)
    B, C, M, K = fj.shape
    x = (fj.unsqueeze(1).expand(-1, 3, -1, -1, -1) * dp.unsqueeze(2)).reshape(B, -1, M, K)
    return x.mean(-1) if reduction == "mean" else x.max(-1)[0]


def with_backward(op, f0, g):
    """forward + backward of op on a leaf made inside the call: a leaf autograd has seen on another stream would make it
    synchronise with that stream inside the capture"""
    def fn():
        leaf = f0.detach().requires_grad_(True)
        return torch.autograd.grad(op(leaf), leaf, g)
    return fn


print(f"{'layer':<16} {'C':>4} {'N':>6} {'M':>6} {'red':>5} | {'kernel':>7} {'GB/s':>6} {'roof':>6} | {'fwd op':>7} {'compose':>8} | "
      f"{'f+b op':>7} {'compose':>8} | {'bwd atom':>8} {'bwd list':>8} {'lists':>7}   (us)")
for label, C, N, idx, dp in shapes():
    B, M, K = idx.shape
    gen = torch.Generator().manual_seed(0)
    f = torch.randn(B, C, N, generator=gen).to(dev)
    g = torch.randn(B, 3 * C, M, generator=gen).to(dev)
    f_pm, g_pm = f.transpose(1, 2).contiguous(), g.transpose(1, 2).contiguous()
    csr = ops.group_csr(idx, N)
    t_lists = replay_us(lambda: ops.group_csr(idx, N))
    nbytes = (B * N * C + B * M * K * 4 + B * 3 * C * M) * 4
    out = torch.empty(B, 3 * C, M, device=dev)
    arg = torch.empty(B, M, 3 * C, dtype=torch.uint8, device=dev)
    df_pm = torch.empty(B, N, C, device=dev)
    for reduction in opt.reductions.split(","):
        red = ops._ASSA_REDUCTION[reduction]
        t_kernel = replay_us(lambda: _lib.check(lib.amc3d_assa_aggregate_forward(
            B, C, N, M, K, red, P(f_pm), P(idx), P(dp), P(out), P(arg), ops._stream(f)), "assa_aggregate_forward"))
        t_atom = replay_us(lambda: _lib.check(lib.amc3d_assa_aggregate_backward(
            B, C, N, M, K, red, P(g_pm), P(idx), P(dp), P(arg), P(df_pm), ops._stream(f)), "assa_aggregate_backward"))
        t_list = replay_us(lambda: _lib.check(lib.amc3d_assa_aggregate_backward_csr(
            B, C, N, M, K, red, P(g_pm), P(dp), P(arg), P(csr[0]), P(csr[1]), P(df_pm), ops._stream(f)), "assa_aggregate_backward_csr"))
        with torch.no_grad():
            t_op = replay_us(lambda: ops.separable_aggregation(f, idx, dp, reduction))
            t_comp = replay_us(lambda: composition(f, idx, dp, reduction))
        t_op_fb = replay_us(with_backward(lambda x: ops.separable_aggregation(x, idx, dp, reduction), f, g))
        t_comp_fb = replay_us(with_backward(lambda x: composition(x, idx, dp, reduction), f, g))
        gbs = nbytes / (t_kernel * 1e-6) / 1e9
        print(f"{label:<16} {C:>4} {N:>6} {M:>6} {reduction:>5} | {t_kernel:7.1f} {gbs:6.0f} {gbs / roofline.HBM_PEAK_GBS:6.1%} | "
              f"{t_op:7.1f} {t_comp:8.1f} | {t_op_fb:7.1f} {t_comp_fb:8.1f} | {t_atom:8.1f} {t_list:8.1f} {t_lists:7.1f}", flush=True)
