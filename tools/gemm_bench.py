"""Every launch of gm_gemm_kernel (csrc/gemm.hip) in one train step of bench.py's workload (PointNeXt-S + AMContrast3D-AA,
8 x 24000 synthetic rooms), one line per distinct (product, b, cin, cout, P, pm, splits): workgroups, K chunks per workgroup,
microseconds and TFLOP/s.

    python tools/gemm_bench.py [reps=30] [variant=S] [batch=8] [points=24000]
    python tools/gemm_bench.py 30 sweep          (a grid of shapes instead of a model's: where each tile wins)

The shapes are collected from one eager step: the C entries that can reach the kernel are wrapped where the operators fetch them,
and the library's routing (pw_forward_deep, gemm_conv_short, gemm_short_splits, gemm_wgrad_splits: restated below, with the
128 x 128 tile they count in) says which calls arrive at gm_gemm_kernel and with which K split.  A call is then repeated on
fresh tensors of that shape through the public entry, captured as a graph, and the median of `reps` replays alone on the chip
is reported ("call": the GEMM and, where there is one, the fixed-order sum of its partials or the bias pass; TFLOP/s is
2 b M N K over that time).  With a library that has amc3d_gemm_probe the same call is also timed with every tile forced, and
the dispatch rule's choice (amc3d_gemm_tile_for) is named: that is the sweep the rule's threshold is read from.
"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import amcontrast3d_amd
amcontrast3d_amd.activate()
from amcontrast3d_amd import _lib, configs, synthetic
from openpoints.loss import build_criterion_from_cfg
from openpoints.models import build_model_from_cfg
from openpoints.utils import EasyConfig

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
variant = sys.argv[2] if len(sys.argv) > 2 else "S"
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 8
points = int(sys.argv[4]) if len(sys.argv) > 4 else 24000
TILES = ((128, 128), (64, 128), (64, 64))  # amc3d_gemm_probe's tile_id
PRODUCTS = ("forward", "backward-data", "weight-grad")


def div_up(a, b):
    return (a + b - 1) // b


# ---- the routing of csrc/pwconv.hip and csrc/gemm.hip, restated ---------------------------------------------------------------
def deep(cin, cout, P):
    return cin >= 64 and cout >= 64 and P < 2 ** 31


def short(b, rows, P):
    return div_up(rows, 128) * div_up(P, 128) * b < 192


def short_splits(b, M, N, K):
    tiles = div_up(M, 128) * div_up(N, 128) * b
    if tiles >= 192 or K < 128:
        return 1
    s = min(512 // tiles, 8, K // 64)
    return 1 if s < 2 else s


def split_kper(K, s):
    return K if s == 1 else div_up(div_up(K, s), 16) * 16


def wgrad_splits(b, cin, cout, P):
    if P % 4 == 0 and P >= 128:
        tiles = div_up(cout, 128) * div_up(cin, 64 if cin <= 64 else 128)
        s = max(1, min(512 // (tiles * b), max(P // 128, 1)))
        per = div_up(div_up(P, s), 32) * 32
    else:
        tiles = div_up(cout, 128) * div_up(cin, 128)
        s = max(1, min(1024 // (tiles * b), max(P // 64, 1)))
        per = div_up(div_up(P, s), 16) * 16
    return div_up(P, per), per


def val(p):
    return (p.value if isinstance(p, ctypes.c_void_p) else p) or 0


class Recorder:
    """the ctypes library with the pointwise-conv entries wrapped: every call that reaches gm_gemm_kernel is noted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def note(self, product, b, cin, cout, P, pm, splits, ldw, w_off, bias):
        key = (product, b, cin, cout, P, pm, splits, ldw, w_off, bias)
        self.calls[key] = self.calls.get(key, 0) + 1

    def forward(self, b, cin, cout, P, w, ldw, bias, y, pm, ws, wsb):
        if not (b > 0 and P > 0 and deep(cin, cout, P) and (not val(bias) or short(b, cout, P))):
            return
        need = 4 * b * short_splits(b, cout, P, cin) * cout * P if short_splits(b, cout, P, cin) > 1 else 0
        s = short_splits(b, cout, P, cin) if need and val(ws) and wsb >= need else 1
        if pm:
            pm = 2 if cout % 4 == 0 and val(y) % 16 == 0 else 1
        self.note(0, b, cin, cout, P, pm, s, ldw, val(w) % 16 // 4, int(bool(val(bias))))

    def backward(self, b, cin, cout, P, x, w, ldw, dy, dx, pm, dw, ws, wsb):
        if not (b > 0 and P > 0 and deep(cin, cout, P)):
            return
        if val(dx) and (cout > 128 or short(b, cin, P)):
            sp = short_splits(b, cin, P, cout)
            need = 4 * b * sp * cin * P if sp > 1 else 0
            s = sp if need and val(ws) and wsb >= need else 1
            if pm:
                pm = 2 if cin % 4 == 0 and val(dx) % 16 == 0 else 1
            self.note(1, b, cin, cout, P, pm, s, ldw, val(w) % 16 // 4, 0)
        if val(dw) and not (P % 4 == 0 and P >= 128 and val(dy) % 16 == 0 and val(x) % 16 == 0):
            self.note(2, b, cin, cout, P, 0, wgrad_splits(b, cin, cout, P)[0], cin, 0, 0)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "amc3d_pointwise_conv_forward":
            def wrapped(b, cin, cout, P, x, w, bias, y, stream):
                self.forward(b, cin, cout, P, w, cin, bias, y, 0, None, 0)
                return fn(b, cin, cout, P, x, w, bias, y, stream)
        elif name == "amc3d_pointwise_conv_forward_ws":
            def wrapped(b, cin, cout, P, x, w, bias, y, ws, wsb, stream):
                self.forward(b, cin, cout, P, w, cin, bias, y, 0, ws, wsb)
                return fn(b, cin, cout, P, x, w, bias, y, ws, wsb, stream)
        elif name == "amc3d_pointwise_conv_forward_strided":
            def wrapped(b, cin, cout, P, x, w, ldw, bias, y, ws, wsb, stream):
                self.forward(b, cin, cout, P, w, ldw, bias, y, 0, ws, wsb)
                return fn(b, cin, cout, P, x, w, ldw, bias, y, ws, wsb, stream)
        elif name == "amc3d_pointwise_conv_forward_rows":
            def wrapped(b, cin, cout, P, x, w, ldw, y, ws, wsb, stream):
                self.forward(b, cin, cout, P, w, ldw, None, y, 1, ws, wsb)
                return fn(b, cin, cout, P, x, w, ldw, y, ws, wsb, stream)
        elif name == "amc3d_pointwise_conv_backward":
            def wrapped(b, cin, cout, P, x, w, dy, dx, dw, ws, wsb, stream):
                self.backward(b, cin, cout, P, x, w, cin, dy, dx, 0, dw, ws, wsb)
                return fn(b, cin, cout, P, x, w, dy, dx, dw, ws, wsb, stream)
        elif name == "amc3d_pointwise_conv_backward_strided":
            def wrapped(b, cin, cout, P, x, w, ldw, dy, dx, pm, dw, lddw, ws, wsb, stream):
                self.backward(b, cin, cout, P, x, w, ldw, dy, dx, pm, dw, ws, wsb)
                return fn(b, cin, cout, P, x, w, ldw, dy, dx, pm, dw, lddw, ws, wsb, stream)
        elif name == "amc3d_sa_residual_backward":  # its weight gradient is amc3d_pointwise_conv_backward on (g, fi), inside C
            def wrapped(*a):
                b, cin, cout, _, m = a[:5]
                self.backward(b, cin, cout, m, a[7], None, cin, a[11], None, 0, a[13], 1, 0)
                return fn(*a)
        else:
            return fn
        return wrapped


def eager_step_shapes():
    torch.manual_seed(0)
    c = EasyConfig(); c.update(configs.model_cfg(variant, dropout=0.5))
    model = build_model_from_cfg(c).to(dev).train()
    cc = EasyConfig(); cc.update(configs.criterion_cfg()); crit = build_criterion_from_cfg(cc).to(dev)
    aa = EasyConfig(); aa.update(configs.ambiguity_args("s3dis"))
    data = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(batch, points, first_id=1000).items()}
    real = _lib.load()
    rec = Recorder(real)
    _lib._lib = rec
    try:
        logits, stage = model(data)
        crit(logits, data["y"], stage, 13, None, aa).backward()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return rec.calls


def replay_median(fn):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def P_(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S_():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def main():
    lib = _lib.load()
    probe = hasattr(lib, "amc3d_gemm_probe")
    g = torch.Generator().manual_seed(1)
    if variant == "sweep":  # no model: forward and backward-data as rows over a grid of channel counts and positions
        calls = {}
        for cin, cout, P in ((ci, co, p) for ci in (64, 128, 256, 512) for co in (128, 256, 512) for p in (1500, 6000, 12000, 48000)):
            calls[(0, batch, cin, cout, P, 0, short_splits(batch, cout, P, cin), cin, 0, 0)] = 1
            if cout > 128 or short(batch, cin, P):  # what pw_backward sends to this kernel
                calls[(1, batch, cin, cout, P, 2, short_splits(batch, cin, P, cout), cin, 0, 0)] = 1
        print(f"a grid of shapes, {batch} clouds; medians of {reps} graph replays, us")
    else:
        calls = eager_step_shapes()
        print(f"PointNeXt-{variant} {batch} x {points}: gm_gemm_kernel launches of one train step; medians of {reps} graph replays, us")
    head = f"{'product':13s} {'b':>2s} {'cin':>4s} {'cout':>4s} {'P':>6s} pm sp {'ldw':>4s} al n | {'M':>4s} {'N':>6s} {'K':>6s} {'kper':>5s} |"
    head += "".join(f" {'%dx%d' % t:>7s}: wgs chunks" for t in (TILES if probe else TILES[:1]))
    head += f" | {'call us':>8s} {'TF/s':>6s}"
    if probe:
        head += " | rule |" + "".join(f" {'%dx%d us' % t:>10s}" for t in TILES)
    print(head)
    total = {"call": 0.0, **{t: 0.0 for t in range(len(TILES))}, "best": 0.0}
    per_product = {}
    for key in sorted(calls):
        product, b, cin, cout, P, pm, sp, ldw, w_off, bias = key
        n = calls[key]
        M, N, K = ((cout, P, cin), (cin, P, cout), (cout, cin, P))[product]
        kper = wgrad_splits(b, cin, cout, P)[1] if product == 2 else split_kper(K, sp)
        w = torch.randn(cout * ldw + 4, generator=g).to(dev)[w_off:]  # the (cout, cin) block at row stride ldw, aligned as it was
        xin = torch.randn(b, cin, P, generator=g).to(dev)
        dy = torch.randn(b, cout, P, generator=g).to(dev)
        bias_t = torch.randn(cout, generator=g).to(dev) if bias else None
        out = torch.empty(b * M * N + 4, device=dev)
        wsb = max(int(lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P)),
                  int(lib.amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, bias)), 16)
        if sp == 1 and product != 2:
            wsb = 16  # the recorded call had no room for partials: no K split
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        if product == 0 and pm:
            call = lambda: _lib.check(lib.amc3d_pointwise_conv_forward_rows(b, cin, cout, P, P_(xin), P_(w), ldw, P_(out), P_(ws), wsb, S_()), "f")  # noqa: E731
        elif product == 0:
            call = lambda: _lib.check(lib.amc3d_pointwise_conv_forward_strided(b, cin, cout, P, P_(xin), P_(w), ldw, P_(bias_t), P_(out), P_(ws), wsb, S_()), "f")  # noqa: E731
        elif product == 1:
            call = lambda: _lib.check(lib.amc3d_pointwise_conv_backward_strided(b, cin, cout, P, None, P_(w), ldw, P_(dy), P_(out), int(pm != 0), None, cin, P_(ws), wsb, S_()), "b")  # noqa: E731
        else:
            if P % 4 == 0 and P >= 128:  # only an unaligned operand sends such a shape here
                raise SystemExit("an unaligned streaming-shaped weight gradient: not a case this tool rebuilds")
            call = lambda: _lib.check(lib.amc3d_pointwise_conv_backward_strided(b, cin, cout, P, P_(xin), None, cin, P_(dy), None, 0, P_(out), cin, P_(ws), wsb, S_()), "w")  # noqa: E731
        t_call = replay_median(call)
        flops = 2.0 * b * M * N * K
        line = f"{PRODUCTS[product]:13s} {b:2d} {cin:4d} {cout:4d} {P:6d} {pm:2d} {sp:2d} {ldw:4d} {int(w_off == 0):2d} {n:1d} | {M:4d} {N:6d} {K:6d} {kper:5d} |"
        for tm, tn in (TILES if probe else TILES[:1]):
            line += f" {'':8s} {div_up(M, tm) * div_up(N, tn) * b * sp:4d} {div_up(min(kper, K), 16):6d}"
        line += f" | {t_call:8.1f} {flops / t_call * 1e-6:6.1f}"
        total["call"] += n * t_call
        per_product[product] = per_product.get(product, 0.0) + n * t_call
        if probe:
            src = dy if product else xin
            other = xin if product == 2 else w
            ts = []
            for tile in range(len(TILES)):
                ts.append(replay_median(lambda: _lib.check(lib.amc3d_gemm_probe(  # noqa: B023
                    tile, product, b, cin, cout, P, ldw, int(pm != 0), P_(src), P_(other), P_(out), P_(ws), wsb, S_()), "p")))
                total[tile] += n * ts[-1]
            total["best"] += n * min(ts)
            line += f" | {'%dx%d' % TILES[lib.amc3d_gemm_tile_for(M, N, b, sp)]:>7s} |" + "".join(f" {t:10.1f}" for t in ts)
        print(line, flush=True)
    print("columns: pm 0 channel-major / 1 rows, 4-byte stores / 2 rows, 16-byte stores; sp = K splits; al = weight view 16-byte aligned; "
          "n = launches per step")
    print("per step, us: " + ", ".join(f"{PRODUCTS[p]} {v:.1f}" for p, v in sorted(per_product.items())) + f"; all {total['call']:.1f}")
    if probe:
        print("per step with one tile everywhere, us: " + ", ".join(f"{'%dx%d' % TILES[t]} {total[t]:.1f}" for t in range(len(TILES)))
              + f"; the best tile per shape {total['best']:.1f}")


if __name__ == "__main__":
    main()
