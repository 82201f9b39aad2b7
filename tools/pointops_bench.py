"""The offset-layout pointops operators against the torch composition that gives the same values, forward and backward, in
the default mode (float atomics) and in deterministic mode (reverse lists built inside the timed backward, as the Python
layer does): 8 segments of synthetic.make_batch rooms, 192 000 rows in all, c = 64, nsample = 16, w_c = 8, k = 3; queries
are the furthest-sampling picks (a quarter of each segment), neighbourhoods the product's own k-NN.

    grouping / subtraction / aggregation   offset_ops Functions  vs  index_select, broadcasting, sum; autograd's index_add_
    interpolation                          the C-ABI entries on given idx / weights  vs  the reference's loop over k in torch
    ball query                             the ragged kernel  vs  the dense entry on the same (equal) segments as (B,N,3)
    furthest sampling                      the ragged kernel  vs  the dense entry on the same (equal) segments

Median of `reps` calls, device events around each call, three warm-up calls per shape.  Nothing here is a threshold.

    python tools/pointops_bench.py [reps=20]
"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from amcontrast3d_amd import _lib, offset_ops as O, ops, synthetic

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B, N, C, NS, WC, K = 8, 24000, 64, 16, 8, 3
lib = _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def median_us(fn, reps=reps):
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


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: {lib.amc3d_last_error().decode()}")


def row(name, ours, theirs, note=""):
    verdict = "faster" if ours < theirs else "SLOWER"
    print(f"| {name:34s} | {ours:9.1f} | {theirs:9.1f} | {theirs / ours:5.2f}x {verdict} | {note} |", flush=True)


def fwd_bwd(name, ours, theirs, leaves, up):
    """ours / theirs: leaves -> output.  Forward, then backward alone (the graph is kept), in both modes for ours."""
    def prep(fn, det):
        ls = [t.detach().requires_grad_(True) for t in leaves]
        with ops.deterministic_mode(det):
            out = fn(*ls)
        return ls, out

    row(name + " forward", median_us(lambda: ours(*leaves)), median_us(lambda: theirs(*leaves)))
    ls_t, out_t = prep(theirs, False)
    t_bwd = median_us(lambda: torch.autograd.grad(out_t, ls_t, up, retain_graph=True))
    for det in (False, True):
        ls, out = prep(ours, det)
        row(name + " backward" + (" (deterministic)" if det else ""),
            median_us(lambda: torch.autograd.grad(out, ls, up, retain_graph=True)), t_bwd)
        for a, b in zip(torch.autograd.grad(out, ls, up, retain_graph=True), torch.autograd.grad(out_t, ls_t, up, retain_graph=True)):
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), name
    del ls_t, out_t


pos = torch.from_numpy(synthetic.make_batch(B, N)["pos"]).to(dev)  # (B,N,3)
xyz = pos.reshape(B * N, 3).contiguous()
n, M = B * N, N // 4
offset = torch.arange(1, B + 1, dtype=torch.int32, device=dev) * N
new_offset = torch.arange(1, B + 1, dtype=torch.int32, device=dev) * M
print(f"{B} segments x {N} rows = {n} rows, {B * M} queries, c = {C}, nsample = {NS}, w_c = {WC}, k = {K}; median of {reps} calls, us")
print("| operator | ours | composition / dense | ratio | note |\n|---|---|---|---|---|")

# ---- furthest sampling: ragged kernel against the dense entry (equal segments, the case the Python layer sends there)
idx_r = torch.empty(B * M, dtype=torch.int32, device=dev)
tmp = torch.empty(n, device=dev)


def fps_ragged():
    tmp.fill_(1e10)
    check(lib.amc3d_pointops_furthestsampling(B, N, n, _p(xyz), _p(offset), _p(new_offset), _p(tmp), _p(idx_r), _s()), "fps")


fps = O.furthestsampling(xyz, offset, new_offset)  # dense route
fps_ragged()
assert torch.equal(fps, idx_r)
row("furthest sampling (ragged kernel)", median_us(fps_ragged, 5), median_us(lambda: ops.furthest_point_sample(pos, M), 5),
    "dense = amc3d_furthest_point_sampling; ops.FurthestSampling sends equal segments there")
new_xyz = xyz[fps.long()].contiguous()
m = new_xyz.shape[0]
# the same rows as 16 segments of 12 000: within the ragged kernel's register budget (12 points per thread)
off16 = torch.arange(1, 2 * B + 1, dtype=torch.int32, device=dev) * (N // 2)
noff16 = torch.arange(1, 2 * B + 1, dtype=torch.int32, device=dev) * (M // 2)


def fps_ragged16():
    tmp.fill_(1e10)
    check(lib.amc3d_pointops_furthestsampling(2 * B, N // 2, n, _p(xyz), _p(off16), _p(noff16), _p(tmp), _p(idx_r), _s()), "fps")


row("furthest sampling, 16 x 12000", median_us(fps_ragged16, 5),
    median_us(lambda: ops.furthest_point_sample(pos.view(2 * B, N // 2, 3), M // 2), 5), "minima in registers")

# ---- ball query
new_pos = new_xyz.view(B, M, 3)
for radius in (0.1, 0.4):
    a = O.ballquery(radius, NS, xyz, new_xyz, offset, new_offset)
    b = ops.ball_query(radius, NS, pos, new_pos) + (torch.arange(B, dtype=torch.int32, device=dev) * N).view(B, 1, 1)
    hit = (a != 0).any(1)  # rows without a hit are global row 0 in the ragged form
    assert torch.equal(a[hit], b.view(m, NS)[hit])
    row(f"ball query r={radius}", median_us(lambda: O.ballquery(radius, NS, xyz, new_xyz, offset, new_offset)),
        median_us(lambda: ops.ball_query(radius, NS, pos, new_pos)), "dense = amc3d_ball_query (grid search); ragged = all pairs per segment")

# ---- grouping, subtraction, aggregation on the product's k-NN
knn, _ = ops.knnquery(NS, xyz, new_xyz, offset, new_offset)  # (m,NS)
self_knn, _ = ops.knnquery(NS, xyz, xyz, offset, offset)  # (n,NS)
feat, feat2 = torch.randn(n, C, device=dev), torch.randn(n, C, device=dev)
lk, lsk = knn.long().view(-1), self_knn.long().view(-1)
wmap = torch.arange(C, device=dev) % WC

fwd_bwd("grouping", lambda f: O.grouping(f, knn), lambda f: f.index_select(0, lk).view(m, NS, C), [feat], torch.randn(m, NS, C, device=dev))
fwd_bwd("subtraction", lambda a, b: O.subtraction(a, b, self_knn), lambda a, b: a.unsqueeze(1) - b.index_select(0, lsk).view(n, NS, C),
        [feat, feat2], torch.randn(n, NS, C, device=dev))
position, weight = torch.randn(n, NS, C, device=dev), torch.randn(n, NS, WC, device=dev)
fwd_bwd("aggregation", lambda f, p, w: O.aggregation(f, p, w, self_knn),
        lambda f, p, w: ((f.index_select(0, lsk).view(n, NS, C) + p) * w.index_select(2, wmap)).sum(1),
        [feat, position, weight], torch.randn(n, C, device=dev))
del position, weight

# ---- interpolation: m sampled rows up to all n rows, on given idx / weights
up_idx, dist = ops.knnquery(K, new_xyz, xyz, new_offset, offset)
recip = 1.0 / (dist + 1e-8)
w = (recip / recip.sum(1, keepdim=True)).contiguous()
feat_m, go = torch.randn(m, C, device=dev), torch.randn(n, C, device=dev)
out, gin = torch.empty(n, C, device=dev), torch.empty(m, C, device=dev)


def torch_interp(f):
    acc = torch.zeros(n, C, device=dev)
    for i in range(K):
        acc += f[up_idx[:, i].long(), :] * w[:, i].unsqueeze(-1)
    return acc


def ours_bwd():
    gin.zero_()
    check(lib.amc3d_pointops_interpolation_backward(n, C, K, m, _p(go), _p(up_idx), _p(w), _p(gin), _s()), "interpolation_backward")


def ours_bwd_det():
    rs, re = ops.group_csr(up_idx.view(1, n, K), m)
    check(lib.amc3d_pointops_scatter_csr(1, m, C, K, 1, _p(go), _p(w), _p(rs), _p(re), _p(gin), _s()), "scatter_csr")


row("interpolation forward", median_us(lambda: check(lib.amc3d_pointops_interpolation_forward(
    n, C, K, m, 0, _p(feat_m), _p(up_idx), _p(w), _p(out), _s()), "interpolation_forward")), median_us(lambda: torch_interp(feat_m)))
assert torch.allclose(out, torch_interp(feat_m), rtol=1e-5, atol=1e-5)
leaf = feat_m.detach().requires_grad_(True)
res = torch_interp(leaf)
t_bwd = median_us(lambda: torch.autograd.grad(res, [leaf], go, retain_graph=True))
row("interpolation backward", median_us(ours_bwd), t_bwd, "ours includes the zero fill")
row("interpolation backward (deterministic)", median_us(ours_bwd_det), t_bwd, "ours includes building the reverse lists")
