"""The loss's seven k-NN searches at the benchmark shape (8 x 24000 synthetic rooms, one segment): four self searches
(k = 24) over the stage clouds and the three label votes (k = 4, 16, 64) over the finest cloud, whose grid they reuse
as in the training step (the k = 4 and 16 votes as prefixes of stage 0's rows, ops.knn_of_support_points).  Prints
every search's time (device events, mean of `reps` calls) and then, from a kernel trace of one pass over the seven, the
time per kernel family (kg_query*, kg_prefix, knn_exact_list, the grid build).

    python tools/knn_bench.py [reps=20]

    python tools/knn_bench.py --batched B N M k [dilation=1]

the k-NN grouper instead: the kernel route (ops.knn_batch, group.py's KNN layout) against the torch composition the
reference writes (cdist + topk + strided pick), and KNNGroup.forward (normalize_dp, with features) against
grouping_operation + subtract + amax + divide on the same indices.  Queries are an FPS pick of the support (M < N) or the
support itself (M == N).  Both sides warmed up, then timed alternately in five rounds of device-event windows of at least
0.3 s each; the median and the spread over the rounds are printed.

    python tools/knn_bench.py --features C

the feature-space search of DynConv: ops.knn_features on (B,C,N) features in place (self-search) against the reference's
composition on the same device (transposed copy, cdist, topk, strided pick), at 8 x 4096 with k = 20, 8 x 4096 with k = 16 and
dilation 4, and 1 x 24000 with k = 16; same timing scheme, plus the achieved 2 B N^2 C FLOP rate and its share of the 157 TF
fp32 matrix roof, and the share of indices on which the two routes agree.
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from amcontrast3d_amd import ops, synthetic

dev = torch.device("cuda:0")


def batched(B, N, M, k, dilation=1):
    import statistics
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers.group import KNNGroup, grouping_operation
    assert torch.cuda.is_available(), "timings need the GPU"
    sup = torch.from_numpy(synthetic.make_batch(B, N)["pos"]).to(dev)
    if M == N:
        qry = sup
    else:
        pick = ops.furthest_point_sample(sup, M).long()
        qry = torch.gather(sup, 1, pick.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    feat = torch.randn(B, 32, N, device=dev)
    grouper = KNNGroup(k, normalize_dp=True)

    def kernel_search():
        return ops.knn_batch(k, sup, qry, dilation=dilation, dist="bkm")

    def torch_search():
        kd = torch.cdist(sup, qry).topk(k=k * dilation, dim=1, largest=False)
        return kd.values, kd.indices.transpose(1, 2)[:, :, ::dilation].contiguous().int()

    def kernel_group():
        return grouper(qry, sup, feat)

    def torch_group():
        i = ops.knn_batch(k, sup, qry)[1]  # the same search on both sides: the difference is the coordinate arithmetic
        dp = grouping_operation(sup.transpose(1, 2).contiguous(), i)
        dp -= qry.transpose(1, 2).unsqueeze(-1)
        dp /= torch.amax(torch.sqrt(torch.sum(dp ** 2, dim=1)), dim=(1, 2)).view(-1, 1, 1, 1)
        return dp, grouping_operation(feat, i)

    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    def compare(name, new, old):
        for fn in (new, old):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        counts = [max(3, int(0.3e6 / max(window(fn, 3), 1.0))) for fn in (new, old)]
        rounds = [(window(new, counts[0]), window(old, counts[1])) for _ in range(5)]
        tn, to = [statistics.median(r[i] for r in rounds) for i in (0, 1)]
        spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in (0, 1)]
        print(f"{name}: kernel route {tn:9.1f} us (spread {spread[0]:.1f}), torch composition {to:9.1f} us (spread {spread[1]:.1f}), "
              f"ratio {to / tn:.2f}")

    with torch.no_grad():
        print(f"B={B} N={N} M={M} k={k} dilation={dilation} (synthetic rooms)")
        compare("search (B,k,M) distances + (B,M,k) indices", kernel_search, torch_search)
        compare("KNNGroup.forward, normalize_dp, 32 feature channels", kernel_group, torch_group)


FEATURE_SHAPES = [(8, 4096, 20, 1), (8, 4096, 16, 4), (1, 24000, 16, 1)]  # (B, N, k, dilation): DGCNN, DeepGCN, one room


def features(C, shapes=FEATURE_SHAPES):
    """ops.knn_features on (B,C,N) features, self-search, against cdist + topk + strided pick on the same device"""
    import statistics
    assert torch.cuda.is_available(), "timings need the GPU"

    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    for B, N, k, dilation in shapes:
        torch.manual_seed(0)
        x = torch.randn(B, C, N, device=dev)
        rows = x.transpose(1, 2).contiguous()

        def kernel_search():
            return ops.knn_features(k, x, dilation=dilation, channel_major=True)[1]

        def torch_search():  # DilatedKNN as the reference writes it, transposed copy included
            r = x.transpose(1, 2).contiguous()
            return torch.cdist(r, r).topk(k=k * dilation, dim=-1, largest=False).indices[:, :, ::dilation].contiguous().int()

        with torch.no_grad():
            same = float((kernel_search() == torch_search()).float().mean())
            assert torch.equal(kernel_search(), ops.knn_features(k, rows, dilation=dilation)[1])
            for fn in (kernel_search, torch_search):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            counts = [max(3, int(0.3e6 / max(window(fn, 3), 1.0))) for fn in (kernel_search, torch_search)]
            rounds = [(window(kernel_search, counts[0]), window(torch_search, counts[1])) for _ in range(5)]
        tn, to = [statistics.median(r[i] for r in rounds) for i in (0, 1)]
        spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in (0, 1)]
        flops = 2.0 * B * N * N * C
        print(f"features C={C} B={B} N={N} k={k} dilation={dilation}: knn_features {tn:9.1f} us (spread {spread[0]:.1f}, "
              f"{flops / tn / 1e6:6.1f} TFLOP/s = {flops / tn / 1e6 / 157 * 100:4.1f} % of the 157 TF fp32 matrix roof), "
              f"cdist + topk {to:9.1f} us (spread {spread[1]:.1f}), ratio {to / tn:.2f}; {same:.4f} of the indices equal", flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "--batched":
    batched(*[int(v) for v in sys.argv[2:7]])
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[1] == "--features":
    features(int(sys.argv[2]))
    sys.exit(0)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B, N = 8, 24000
pos = torch.from_numpy(synthetic.make_batch(B, N)["pos"]).to(dev)


def flat(p):
    return p.reshape(-1, 3).contiguous()


stages = [flat(pos)]
cur = pos
for m in (6000, 1500, 375):
    idx = ops.furthest_point_sample(cur, m).long()
    cur = torch.gather(cur, 1, idx.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    stages.append(flat(cur))
offs = [torch.tensor([p.shape[0]], dtype=torch.int32, device=dev) for p in stages]
K_SELF = 24
searches = [("self  stage %d" % i, K_SELF, i, i) for i in range(4)] + [("votes stage %d" % i, kr, 0, i) for i, kr in ((1, 4), (2, 16), (3, 64))]


def run(which):
    """the searches `which` as the loss runs them: inside one knn_grid_reuse block, stage 0's self search first"""
    with ops.knn_grid_reuse():
        for j in which:
            _, k, s, q = searches[j]
            if s == q:
                ops.knnquery_squared(k, stages[s], stages[q], offs[s], offs[q])
            else:  # a vote (AEF/utils.py get_subscene_class): prefixes of stage 0's rows where k allows, else the search
                ops.knn_of_support_points(k, stages[s], stages[q], offs[s], offs[q])


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


t_build0 = None
for j, (name, k, s, q) in enumerate(searches):
    if s == q:
        t = timed(lambda: run([j]))
        note = "grid build included"
    else:  # a vote: the time of [stage 0 self, this search] minus the stage 0 self search alone
        t = timed(lambda: run([0, j])) - timed(lambda: run([0]))
        note = "on stage 0's grid"
    print(f"{name}  n={stages[s].shape[0]:7d} m={stages[q].shape[0]:7d} k={k:2d}: {t:8.1f} us  ({note})")
print(f"all seven, as the loss runs them: {timed(lambda: run(range(7))):8.1f} us")

# kernel by kernel: one traced pass over the seven searches
from torch.profiler import ProfilerActivity, profile

run(range(7))
torch.cuda.synchronize()
with profile(activities=[ProfilerActivity.CUDA]) as prof:
    for _ in range(reps):
        run(range(7))
    torch.cuda.synchronize()
fam = collections.OrderedDict((f, [0, 0.0]) for f in ("kg_query_group_kernel", "kg_query_kernel", "kg_prefix_kernel", "knn_exact_list_kernel",
                                                      "knn_exact_kernel", "grid build (other kg_*)", "other"))
for ev in prof.key_averages():
    t = getattr(ev, "device_time_total", None)
    if t is None:
        t = getattr(ev, "cuda_time_total", 0.0)
    if not t:
        continue
    name = ev.key
    f = next((f for f in list(fam)[:5] if f in name), None)
    if f is None:
        f = "grid build (other kg_*)" if ("kg_" in name or "fill_i32" in name) else "other"
    fam[f][0] += ev.count
    fam[f][1] += t
print("per pass over the seven searches (kernel trace):")
for f, (cnt, t) in fam.items():
    print(f"  {f:26s} {cnt / reps:6.1f} launches {t / reps:9.1f} us")
# the query kernel of every search: launch j of a pass belongs to search j
from torch.autograd import DeviceType

for pat in (("kg_query", "kg_prefix"), ("knn_exact_list",)):
    launches = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA and any(s in e.name for s in pat)),
                      key=lambda e: e.time_range.start)
    if len(launches) != reps * len(searches):
        print(f"  ({len(launches)} {pat} launches traced, {reps * len(searches)} expected: no per-search table)")
        continue
    for j, (name, k, s, q) in enumerate(searches):
        mine = launches[j::len(searches)]
        us = sum(e.time_range.elapsed_us() for e in mine) / reps
        print(f"  {name} m={stages[q].shape[0]:7d} k={k:2d}: {mine[0].name.split('(')[0][-40:]:40s} {us:8.1f} us")
