"""The row passes of the four loss stages at the benchmark shape (8 x 24000 synthetic rooms, one segment), on the stages'
real 24-NN lists and voted labels: amc3d_posmask + amc3d_ambiguity (two passes over the rows) against amc3d_loss_rows (one),
each captured as a graph and replayed alone on the chip.  Prints the median of `reps` replays per stage and route, after
checking that both routes give the same bits.

    python tools/loss_rows_bench.py [reps=30] [cctype=Method1]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from amcontrast3d_amd import ops, synthetic

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
cctype = sys.argv[2] if len(sys.argv) > 2 else "Method1"
B, N, NCLS, BETA = 8, 24000, 13, 0.5
batch = synthetic.make_batch(B, N)
pos = torch.from_numpy(batch["pos"]).to(dev)
labels0 = torch.from_numpy(batch["y"]).to(dev).flatten().to(torch.int32)

stages = [pos.reshape(-1, 3).contiguous()]
cur = pos
for m in (6000, 1500, 375):
    pick = ops.furthest_point_sample(cur, m).long()
    cur = torch.gather(cur, 1, pick.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    stages.append(cur.reshape(-1, 3).contiguous())
offs = [torch.tensor([p.shape[0]], dtype=torch.int32, device=dev) for p in stages]


def two_passes(labels, p, nbr):
    posmask = ops.posmask_from_labels(labels, nbr)
    return posmask, ops.ambiguity(p, posmask, nbr, cctype, BETA)


def one_pass(labels, p, nbr):
    return ops.posmask_and_ambiguity(labels, p, nbr, cctype, BETA)


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
    return statistics.median(times), min(times), max(times)


print(f"cctype {cctype}, medians of {reps} graph replays, us (min .. max)")
total = [0.0, 0.0]
for i, p in enumerate(stages):
    idx, _ = ops.knnquery_squared(24, p, p, offs[i], offs[i])
    nbr = idx[:, 1:]
    labels = labels0
    if i:
        votes, _ = ops.knnquery_squared(4 ** i, stages[0], p, offs[0], offs[i])
        labels = ops.vote_labels(labels0, votes, NCLS)
    want, got = two_passes(labels, p, nbr), one_pass(labels, p, nbr)
    same = torch.equal(want[0], got[0]) and torch.equal(want[1].view(torch.int32), got[1].view(torch.int32))
    t2, t1 = replay_median(lambda: two_passes(labels, p, nbr)), replay_median(lambda: one_pass(labels, p, nbr))
    total[0] += t2[0]
    total[1] += t1[0]
    print(f"stage {i} m={p.shape[0]:7d} k=23: posmask + ambiguity {t2[0]:7.1f} ({t2[1]:.1f} .. {t2[2]:.1f})   "
          f"loss_rows {t1[0]:7.1f} ({t1[1]:.1f} .. {t1[2]:.1f})   same bits: {same}")
print(f"four stages: posmask + ambiguity {total[0]:7.1f}   loss_rows {total[1]:7.1f}")
