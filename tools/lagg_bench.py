"""The convolve-before-gather layers (ops.GroupedConvBN, ops.LocalAggregationFused) alone, at the shapes and on the geometry
of a real step: PointNeXt-S's four SetAbstraction first blocks and the neighbourhood layers of configs.model_cfg("L"), one
synthetic S3DIS-like batch of 8 x 24000 points, the plan of geometry.precompute (reverse lists included).

A forward of the model records every call of the two layers with its inputs; each distinct shape is then timed on its own:

    forward   the layer's forward as the model calls it: conv on the source points + statistics + finalize + expand / pool
    backward  the layer kernels' backward entry alone (Q + partial sums, finalize, dG), without the conv's backward products:
              the reverse-list form for GroupedConvBN on a gradient that arrives as rows (what the step runs), the atomic form
              for LocalAggregationFused

Each is captured into a graph once and replayed; the figure is the median HIP-event time of --repeats replays after --warmup
(no launch gaps of the host in it).  Run it from the root of the tree whose build it is to time:

    python tools/lagg_bench.py [--variants S,L] [--repeats 30]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from amcontrast3d_amd import _lib, configs, geometry, ops, synthetic  # noqa: E402
from openpoints.loss import build_criterion_from_cfg  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--variants", default="S,L")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=30)
opt = ap.parse_args()
assert opt.repeats >= 20

dev = torch.device("cuda:0")
lib, P = _lib.load(), ops._ptr


def record(variant):
    """-> {shape key: (layer, args, number of calls)} of one training forward of the variant"""
    torch.manual_seed(0)
    c = EasyConfig(); c.update(configs.model_cfg(variant, dropout=0.5)); model = build_model_from_cfg(c).to(dev).train()
    cc = EasyConfig(); cc.update(configs.criterion_cfg()); crit = build_criterion_from_cfg(cc).to(dev)
    aa = EasyConfig(); aa.update(configs.ambiguity_args("s3dis"))
    data = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(8, 24000).items()}
    data["_geometry"] = geometry.precompute(model, crit.contrast_head, data, 13, None, aa)
    seen = {}
    originals = {}

    def wrap(name):
        layer = getattr(ops, name)
        originals[name] = layer.apply

        def apply(*args):
            f, idx, w = args[0], args[2], args[4]
            key = (name, f.shape[0], f.shape[1], w.shape[0], f.shape[2], idx.shape[1], idx.shape[2])
            if key in seen:
                seen[key][2] += 1
            else:
                seen[key] = [layer, tuple(a.detach().clone() if torch.is_tensor(a) and a.is_floating_point() else a for a in args), 1]
            return originals[name](*args)
        layer.apply = apply

    for name in ("GroupedConvBN", "LocalAggregationFused"):
        wrap(name)
    try:
        with torch.no_grad():
            model(data)
    finally:
        for name, fn in originals.items():
            getattr(ops, name).apply = fn
    torch.cuda.synchronize()
    return seen


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
    return ts[len(ts) // 2], ts[0]


def backward_entry(layer, saved, csr, relu):
    """the layer kernels' backward entry on the saved tensors of a forward, as a closure without allocations"""
    grouped = layer is ops.GroupedConvBN
    f, w_f, w_dp, g_pm, idx, dp, moments, gamma, beta, mean, invstd, gd = saved[:12]
    B, Cin, N = f.shape
    _, M, K = idx.shape
    C, ldw = w_f.shape[0], w_dp.shape[1]
    g = torch.Generator().manual_seed(1)
    dg = torch.empty(B, C, N, device=dev)
    dw = torch.empty(C, ldw, device=dev)
    dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
    stream = lambda: ops._stream(f)  # noqa: E731  (the stream current at the call: the capturing one inside a capture)
    if grouped:
        go = torch.randn(B, M, K, C, generator=g).to(dev)  # position-major rows, as SATailActivated hands them over
        if csr is not None:
            wb = int(lib.amc3d_grouped_conv_bn_csr_workspace_bytes(B, C, N, M, K))
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
            edge_dp = P(csr[2]) if len(csr) > 2 and csr[2] is not None else None
            return lambda: _lib.check(lib.amc3d_grouped_conv_bn_backward(
                B, C, N, M, K, int(relu), P(go), 1, P(g_pm), P(idx), P(csr[0]), P(csr[1]), edge_dp, P(dp), P(w_dp), ldw, P(moments),
                P(gd), P(mean), P(invstd), P(gamma), P(beta), P(dg), P(dw), ldw, P(dgamma), P(dbeta), 0, None, None, P(work), wb,
                stream()), "grouped_conv_bn_backward with lists")
        go = go.permute(0, 3, 1, 2).contiguous()
        wb = int(lib.amc3d_local_aggregation_workspace_bytes(B, C, N, M))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        return lambda: _lib.check(lib.amc3d_grouped_conv_bn_backward(
            B, C, N, M, K, int(relu), P(go), 0, P(g_pm), P(idx), None, None, None, P(dp), P(w_dp), ldw, P(moments), P(gd), P(mean),
            P(invstd), P(gamma), P(beta), P(dg), P(dw), ldw, P(dgamma), P(dbeta), 0, None, None, P(work), wb, stream()),
            "grouped_conv_bn_backward")
    ystar, arg = saved[12], saved[13]
    go = torch.randn(B, C, M, generator=g).to(dev)
    wb = int(lib.amc3d_local_aggregation_workspace_bytes(B, C, N, M))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    return lambda: _lib.check(lib.amc3d_local_aggregation_backward(
        B, C, N, M, K, int(relu), P(go), P(ystar), P(arg), P(g_pm), P(idx), P(dp), P(w_dp), ldw, P(moments), P(gd), P(mean),
        P(invstd), P(gamma), P(beta), None, None, P(dg), P(dw), ldw, P(dgamma), P(dbeta), 0, None, None, P(work), wb, stream()),
        "local_aggregation_backward")


print(f"library: {os.path.relpath(_lib._SO)}   repeats {opt.repeats}, warm-up {opt.warmup}; microseconds, median (minimum)")
totals = {}
for variant in opt.variants.split(","):
    fwd_sum = bwd_sum = 0.0
    for key, (layer, args, ncalls) in record(variant).items():
        name, B, Cin, C, N, M, K = key
        grouped = layer is ops.GroupedConvBN
        relu = bool(args[8])
        csr = args[10] if grouped else None
        leaf = [a.requires_grad_(True) if i in (0, 4, 5, 6) else a for i, a in enumerate(args)]
        with torch.cuda.device(dev):
            y = layer.apply(*leaf)
            saved = y.grad_fn.saved_tensors
            with torch.no_grad():
                tf, tf_min = replay_us(lambda: layer.apply(*args))
            tb, tb_min = replay_us(backward_entry(layer, saved, csr, relu))
        del y, saved
        fwd_sum += tf * ncalls
        bwd_sum += tb * ncalls
        print(f"{variant} {name:22s} B={B} Cin={Cin:3d} C={C:3d} N={N:5d} M={M:5d} K={K} x{ncalls}:  forward {tf:7.1f} ({tf_min:7.1f})   "
              f"backward {tb:7.1f} ({tb_min:7.1f})")
    totals[variant] = (fwd_sum, bwd_sum)
    print(f"{variant} all calls of one step: forward {fwd_sum:8.1f}   backward {bwd_sum:8.1f}   sum {fwd_sum + bwd_sum:8.1f}")
