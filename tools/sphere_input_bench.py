"""Times the S3DISSphere route on the device against the host route on the same machine:

    python tools/sphere_input_bench.py [--points 1500000] [--batch 8] [--num-points 24000] [--radius 2.0] [--steps 1000]

  batch      one s3dis_sphere_batch of B spheres (B schedule steps, the shuffle and padding draws, the tail), generator draws
  schedule   one epoch's schedule: SpherePotentials.advance(steps)
  host       the same two on the CPU: tests/sphere_ref.py's arithmetic with sklearn's KD-tree for the radius query where sklearn
             is importable (what the reference runs, in its loader workers and before the first step), brute force otherwise; the
             schedule is timed over --host-steps steps and scaled to --steps
The cloud is a synthetic Area: floors, ceilings and walls of a grid of rooms, about --points sub-points.  Device times are
host clocks around work that ends in a synchronise, after a warm-up, median of --repeats.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES_PER_STEP = {"pick": 1, "keys": 1, "sort (library)": 1, "finish + Tukey update": 1, "minima of the touched blocks": 1}


def make_area(n, seed=0):
    """floors, ceilings and walls every 4 m of a 24 x 20 x 3 m storey (about 800 points per square metre at 1.5 M), uniformly
    random points -> (n,3) float32"""
    rng = np.random.default_rng(seed)
    lx, ly, lz = 24.0, 20.0, 3.0
    areas = np.array([2 * lx * ly, (lx / 4 + 1) * ly * lz, (ly / 4 + 1) * lx * lz])
    kind = rng.choice(3, n, p=areas / areas.sum())
    p = rng.uniform(0, 1, (n, 3)) * np.array([lx, ly, lz])
    flat = kind == 0
    p[flat, 2] = rng.integers(0, 2, int(flat.sum())) * lz
    wx = kind == 1
    p[wx, 0] = rng.integers(0, int(lx / 4) + 1, int(wx.sum())) * 4.0
    wy = kind == 2
    p[wy, 1] = rng.integers(0, int(ly / 4) + 1, int(wy.sum())) * 4.0
    return (p + rng.normal(0, 0.01, p.shape)).astype(np.float32)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return statistics.median(out), min(out), max(out)


def host_query(tree, pts, centre, radius):
    if tree is not None:
        return tree.query_radius(centre.reshape(1, 3), r=radius, return_distance=True, sort_results=True)[0][0]
    import sphere_ref as sr
    return sr.radius_query(pts, centre, radius)[0]


def host_step(tree, pts, pot, noise, radius, num_points):
    import sphere_ref as sr
    point = int(np.argmin(pot))
    centre = sr.pick_point(pts, point, noise)
    q = host_query(tree, pts, centre, radius)[:num_points]
    d = np.sum(np.square((pts[q].astype(np.float64) - centre).astype(np.float32)), axis=1)
    t = np.square(1 - d / np.square(radius))
    t[d > np.square(radius)] = 0
    pot[q] += t
    return point


def host_item(tree, pts, colours, labels, point, noise, radius, num_points, rng):
    import sphere_ref as sr
    centre = sr.pick_point(pts, point, noise)
    q = host_query(tree, pts, centre, radius)
    cur = len(q)
    if cur > num_points:
        inds = q[:num_points][rng.permutation(num_points)]
    else:
        q = q[rng.permutation(cur)]
        inds = np.hstack([q, q[rng.choice(cur, num_points - cur)]])
    return (pts[inds].astype(np.float64) - centre).astype(np.float32), colours[inds], labels[inds], inds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1500000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--num-points", type=int, default=24000)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--host-steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the device route needs the GPU; there is no fallback"
    from amcontrast3d_amd import input_pipeline as ip
    dev = "cuda:0"
    pts = make_area(a.points)
    rng = np.random.default_rng(1)
    colours = rng.integers(0, 256, pts.shape).astype(np.float32)
    labels = rng.integers(0, 13, len(pts)).astype(np.int64)
    pot0 = rng.random(len(pts)) * 1e-3
    cloud = [(torch.from_numpy(pts).to(dev), torch.from_numpy(colours).to(dev), torch.from_numpy(labels).to(dev))]
    gen = torch.Generator(device=dev).manual_seed(0)

    st = ip.SpherePotentials(cloud, a.radius, a.num_points, potentials=[pot0], generator=gen)
    batch = timed(lambda: ip.s3dis_sphere_batch(st, a.batch, None), a.repeats)
    counts = ip.s3dis_sphere_batch(st, a.batch, None)["mask"].sum(1).tolist()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ip.s3dis_sphere_batch(st, a.batch, None)
        read_backs = 0
    except RuntimeError:
        read_backs = None  # (a synchronising call was made: not the structure the design states)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = ip.SpherePotentials(cloud, a.radius, a.num_points, potentials=[pot0], generator=gen)
    sched = timed(lambda: st.advance(a.steps), max(a.repeats // 3, 3), warmup=1)

    tree = None
    try:
        from sklearn.neighbors import KDTree
        t = time.perf_counter()
        tree = KDTree(pts, leaf_size=50)
        tree_s = time.perf_counter() - t
    except ImportError:
        tree_s = None
    pot = pot0.copy()
    noise = rng.normal(0, a.radius / 10, (a.host_steps, 3))
    t = time.perf_counter()
    picks = [host_step(tree, pts, pot, noise[s], a.radius, a.num_points) for s in range(a.host_steps)]
    host_step_s = (time.perf_counter() - t) / a.host_steps
    t = time.perf_counter()
    for s in range(a.batch):
        host_item(tree, pts, colours, labels, picks[s % len(picks)], noise[s % len(picks)], a.radius, a.num_points, rng)
    host_batch_s = time.perf_counter() - t

    print(json.dumps({
        "points": len(pts), "batch": a.batch, "num_points": a.num_points, "in_radius": a.radius, "steps": a.steps,
        "points_listed_per_sphere": counts,
        "device_batch_ms": {"median": batch[0] * 1e3, "min": batch[1] * 1e3, "max": batch[2] * 1e3},
        "device_schedule_ms": {"median": sched[0] * 1e3, "min": sched[1] * 1e3, "max": sched[2] * 1e3, "per_step": sched[0] * 1e3 / a.steps},
        "host_route": "sklearn KDTree" if tree is not None else "brute force", "host_tree_build_s": tree_s,
        "host_batch_ms": host_batch_s * 1e3, "host_schedule_ms": host_step_s * a.steps * 1e3, "host_step_ms": host_step_s * 1e3,
        "host_steps_timed": a.host_steps, "launches_per_schedule_step": sum(LAUNCHES_PER_STEP.values()),
        "launches": LAUNCHES_PER_STEP, "read_backs_per_batch": read_backs}))


if __name__ == "__main__":
    main()
