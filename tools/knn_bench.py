"""The loss's seven k-NN searches at the benchmark shape (8 x 24000 synthetic rooms, one segment): four self searches
(k = 24) over the stage clouds and the three label votes (k = 4, 16, 64) over the finest cloud, whose grid they reuse
as in the training step.  Prints every search's time (device events, mean of `reps` calls) and then, from a kernel
trace of one pass over the seven, the time per kernel family (kg_query*, knn_exact_list, the grid build).

    python tools/knn_bench.py [reps=20]
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from amcontrast3d_amd import ops, synthetic

dev = torch.device("cuda:0")
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
            ops.knnquery_squared(k, stages[s], stages[q], offs[s], offs[q])


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
fam = collections.OrderedDict((f, [0, 0.0]) for f in ("kg_query_group_kernel", "kg_query_kernel", "knn_exact_list_kernel",
                                                      "knn_exact_kernel", "grid build (other kg_*)", "other"))
for ev in prof.key_averages():
    t = getattr(ev, "device_time_total", None)
    if t is None:
        t = getattr(ev, "cuda_time_total", 0.0)
    if not t:
        continue
    name = ev.key
    f = next((f for f in list(fam)[:4] if f in name), None)
    if f is None:
        f = "grid build (other kg_*)" if ("kg_" in name or "fill_i32" in name) else "other"
    fam[f][0] += ev.count
    fam[f][1] += t
print("per pass over the seven searches (kernel trace):")
for f, (cnt, t) in fam.items():
    print(f"  {f:26s} {cnt / reps:6.1f} launches {t / reps:9.1f} us")
# the query kernel of every search: launch j of a pass belongs to search j
from torch.autograd import DeviceType

for pat in ("kg_query", "knn_exact_list"):
    launches = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA and pat in e.name),
                      key=lambda e: e.time_range.start)
    if len(launches) != reps * len(searches):
        print(f"  ({len(launches)} {pat} launches traced, {reps * len(searches)} expected: no per-search table)")
        continue
    for j, (name, k, s, q) in enumerate(searches):
        mine = launches[j::len(searches)]
        us = sum(e.time_range.elapsed_us() for e in mine) / reps
        print(f"  {name} m={stages[q].shape[0]:7d} k={k:2d}: {mine[0].name.split('(')[0][-40:]:40s} {us:8.1f} us")
