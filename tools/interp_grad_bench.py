"""three_interpolate's backward at the four decoder levels of S (8 x 24000) and XL (2 x 64000): idx / weights from the
product's own 3-NN on synthetic.make_batch clouds sampled down by FPS (bank conflicts and same-address adds depend on the
real neighbour structure), random grad_out.  Median of `reps` calls (device events around each call) of

    entry   out.zero_() + amc3d_three_interpolate_grad with its workspace: what backward ran before the LDS route, and
            on a library with the LDS route whatever that library dispatches to, still with the zero fill
    list    amc3d_three_interpolate_grad_csr (deterministic mode's gather; the lists are built outside the timed call)
    write   amc3d_three_interpolate_grad_write: the dispatched LDS route, no zero fill
    lds     amc3d_three_interpolate_grad_lds per channel group cg and workgroup size (overwrite form)

The last two only where the loaded library has them, so the same file times a library from before the route.

    python tools/interp_grad_bench.py [reps=50]
"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from amcontrast3d_amd import _lib, ops, synthetic

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
lib = _lib.load()
HAS_LDS = "amc3d_three_interpolate_grad_lds" in _lib.SIGNATURES


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def median_us(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def levels(B, N, widths):
    """(c, unknown cloud, known cloud) per decoder level, finest first"""
    pos = torch.from_numpy(synthetic.make_batch(B, N)["pos"]).to(dev)
    clouds = [pos]
    for _ in widths:
        cur = clouds[-1]
        idx = ops.furthest_point_sample(cur, cur.shape[1] // 4).long()
        clouds.append(torch.gather(cur, 1, idx.unsqueeze(-1).expand(-1, -1, 3)).contiguous())
    return [(c, clouds[i], clouds[i + 1]) for i, c in enumerate(widths)]


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: {lib.amc3d_last_error().decode()}")


for name, B, N, widths in (("S  8 x 24000", 8, 24000, (64, 128, 256, 512)), ("XL 2 x 64000", 2, 64000, (128, 256, 512, 1024))):
    for c, unknown, known in levels(B, N, widths):
        n, m = unknown.shape[1], known.shape[1]
        dist, idx = ops.three_nn(unknown, known)
        recip = 1.0 / (dist + 1e-8)
        w = (recip / recip.sum(2, keepdim=True)).contiguous()
        go = torch.randn(B, c, n, device=dev)
        out = torch.empty(B, c, m, device=dev)
        work = torch.empty(B * c * m, device=dev)
        rs, re = ops.group_csr(idx, m)

        def entry():
            out.zero_()
            check(lib.amc3d_three_interpolate_grad(B, c, n, m, _p(go), _p(idx), _p(w), _p(out), _p(work), work.numel() * 4, _s()), "entry")

        def lists():
            check(lib.amc3d_three_interpolate_grad_csr(B, c, n, m, _p(go), _p(idx), _p(w), _p(rs), _p(re), _p(out), _s()), "list")

        line = f"{name} c={c:4d} n={n:5d} m={m:5d}: entry {median_us(entry):7.1f} us  list {median_us(lists):7.1f} us"
        if HAS_LDS:
            cg, th = ctypes.c_int(0), ctypes.c_int(0)
            route = lib.amc3d_three_interpolate_grad_route(B, c, n, m, ctypes.byref(cg), ctypes.byref(th))
            line += f"  route {route} cg {cg.value} threads {th.value}"
            if route == 2:
                t = median_us(lambda: check(lib.amc3d_three_interpolate_grad_write(B, c, n, m, _p(go), _p(idx), _p(w), _p(out), _s()), "write"))
                line += f"  write {t:7.1f} us"
        print(line, flush=True)
        if HAS_LDS:
            for threads in (256, 512, 1024):
                cells = []
                for g in (1, 2, 4, 8, 16, 32):
                    if g > c or g * m * 8 > 160 * 1024:
                        continue
                    t = median_us(lambda: check(lib.amc3d_three_interpolate_grad_lds(B, c, n, m, g, threads, 0, _p(go), _p(idx), _p(w), _p(out), _s()), "lds"))
                    cells.append(f"cg {g:2d} ({g * m * 8 / 1024:5.1f} KiB) {t:7.1f}")
                print(f"    lds, {threads:4d} threads, us: " + "   ".join(cells), flush=True)
