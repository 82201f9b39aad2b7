"""Hardware counters of gm_gemm_kernel (csrc/gemm.hip), per launch shape and per tile.

    python tools/gemm_pmc.py run                      (under `rocprofv3 --pmc ... --output-format csv`, see tools/gemm_pmc.sh)
    python tools/gemm_pmc.py table OUT.txt DIR...     (merge the passes' *counter_collection.csv into one table)

`run` drives amc3d_gemm_probe over the three filled launches of the PointNeXt-S step at 8 x 24000 and four of its short ones
(shapes as tools/gemm_bench.py lists them), every tile forced, three dispatches each.  `table` prints one row per (kernel
instantiation, grid): the mean of each counter over the dispatches and the ratios that name the stall:
    mfma    SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs): share of the launch the MFMA pipe works
    parked  SQ_WAIT_ANY / SQ_WAVE_CYCLES: share of a wave's life parked at s_waitcnt (vector-memory or LDS data) or at a barrier
            -- this ROCm offers no counter that separates the three
    issue   SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES: waiting to issue (mostly behind the MFMAs of the other waves of its SIMD)
    lds     SQ_LDS_IDX_ACTIVE / (256 CUs x GRBM_GUI_ACTIVE / 8): share of the launch the LDS array works
    confl   SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE
    vm/lds  (SQ_INST_LEVEL_VMEM / SQ_INSTS_VMEM) / (SQ_INST_LEVEL_LDS / SQ_INSTS_LDS): a vector-memory instruction's time in
            flight in units of an LDS instruction's
"""
import csv
import ctypes
import glob
import os
import re
import sys

SHAPES = [  # product, b, cin, cout, P, pm, extra floats in front of / between the weight rows (the [W_dp | W_f] view)
    (0, 8, 64, 128, 48000, 0, 0), (0, 8, 128, 256, 12000, 0, 0), (1, 8, 128, 256, 12000, 1, 0),
    (0, 8, 256, 256, 375, 1, 3), (1, 8, 128, 128, 1500, 0, 3), (2, 8, 256, 256, 375, 0, 0), (2, 8, 256, 512, 93, 0, 0)]


def run():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(1)
    for product, b, cin, cout, P, pm, ex in SHAPES:
        ldw = cin + ex
        w = torch.randn(cout * ldw + 4, generator=g).to(dev)[ex:]
        xin = torch.randn(b, cin, P, generator=g).to(dev)
        dy = torch.randn(b, cout, P, generator=g).to(dev)
        M, N = ((cout, P), (cin, P), (cout, cin))[product]
        out = torch.empty((b if product != 2 else 1) * M * N + 4, device=dev)
        wsb = max(int(lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P)),
                  int(lib.amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, 0)), 16)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        src, other = (dy if product else xin), (xin if product == 2 else w)
        for tile in range(3):
            for _ in range(3):
                _lib.check(lib.amc3d_gemm_probe(tile, product, b, cin, cout, P, cin if product == 2 else ldw, pm, ptr(src), ptr(other),
                                                ptr(out), ptr(ws), wsb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "probe")
        torch.cuda.synchronize()


def label(kernel, grid):
    """the launch behind a grid size: workgroups = grid / 256 threads"""
    m = re.search(r"<(\d+), (\d+), (\w+), (\w+)>", kernel)
    tm, tn = int(m.group(1)), int(m.group(2))
    up = lambda a, b: (a + b - 1) // b  # noqa: E731
    names = {("true", "false"): "forward", ("false", "false"): "backward-data", ("true", "true"): "weight-grad"}
    for product, b, cin, cout, P, pm, ex in SHAPES:
        if names[(m.group(3), m.group(4))] != ("forward", "backward-data", "weight-grad")[product]:
            continue
        M, N, K = ((cout, P, cin), (cin, P, cout), (cout, cin, P))[product]
        if product == 2:
            splits = 1 if P < 128 else min(1024 // (up(cout, 128) * up(cin, 128) * b), P // 64)
            per = up(up(P, splits), 16) * 16
            splits = up(P, per)
        else:
            tiles = up(M, 128) * up(N, 128) * b
            splits = 1 if tiles >= 192 or K < 128 else max(1, min(512 // tiles, 8, K // 64))
        if up(M, tm) * up(N, tn) * b * splits * 256 == int(grid):
            return f"{names[(m.group(3), m.group(4))]} {M}<-{K} x {N} b{b} sp{splits}"
    return "?"


def table(out, dirs):
    agg = {}
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                rd = csv.DictReader(fh)
                cols = {c.lower(): c for c in rd.fieldnames}
                for r in rd:
                    m = re.search(r"(gm_gemm_kernel<[^>]*>)", r[cols["kernel_name"]])
                    if m:
                        a = agg.setdefault((m.group(1), r[cols["grid_size"]]), {}).setdefault(r[cols["counter_name"]], [0, 0.0])
                        a[0] += 1
                        a[1] += float(r[cols["counter_value"]])
    write_table(out, {k: {c: s / n for c, (n, s) in v.items()} for k, v in agg.items()})


def write_table(out, rows):
    with open(out, "w") as fh:
        fh.write(f"{'launch':38s} {'tile':>8s} {'waves':>6s} {'cycles':>8s} | {'mfma':>5s} {'parked':>6s} {'issue':>5s} {'active':>6s} | "
                 f"{'lds':>5s} {'confl':>5s} | {'vm/lds':>6s}\n")
        for (kernel, grid), v in sorted(rows.items(), key=lambda kv: (label(*kv[0]), kv[0][0])):
            g = lambda c: v.get(c, float("nan"))  # noqa: E731
            m = re.search(r"<(\d+), (\d+)", kernel)
            cyc, wc = g("GRBM_GUI_ACTIVE") / 8, g("SQ_WAVE_CYCLES")
            fh.write(f"{label(kernel, grid):38s} {m.group(1) + 'x' + m.group(2):>8s} {g('SQ_WAVES'):6.0f} {cyc:8.0f} | "
                     f"{g('SQ_VALU_MFMA_BUSY_CYCLES') / (1024 * cyc):5.2f} {g('SQ_WAIT_ANY') / wc:6.2f} {g('SQ_WAIT_INST_ANY') / wc:5.2f} "
                     f"{g('SQ_ACTIVE_INST_ANY') / wc:6.2f} | {g('SQ_LDS_IDX_ACTIVE') / (256 * cyc):5.2f} "
                     f"{g('SQ_LDS_BANK_CONFLICT') / g('SQ_LDS_IDX_ACTIVE'):5.2f} | "
                     f"{g('SQ_INST_LEVEL_VMEM') / g('SQ_INSTS_VMEM') / (g('SQ_INST_LEVEL_LDS') / g('SQ_INSTS_LDS')):6.1f}\n")
        fh.write("cycles = GRBM_GUI_ACTIVE / 8 (one XCD's clock over the launch); the other columns: see tools/gemm_pmc.py\n")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        table(sys.argv[2], sys.argv[3:])
