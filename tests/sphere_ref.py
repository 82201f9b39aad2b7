"""Plain-numpy restatement of S3DISSphere (openpoints/dataset/s3dis/s3dis_sphere.py) and of validate_sphere's vote
(examples/segmentation/main.py:436-483): the radius query, one schedule step, one item, the vote.  No sklearn and nothing of the
package: the GPU tests compare the device with this, and tests/test_sphere_oracle.py compares this with what the reference's own
class recorded (tests/golden/s3dis_sphere.npz).

Arithmetic, as the reference evaluates it with numpy >= 2:
  query   sklearn's KDTree holds the float32 coordinates as float64; query_radius(pick, r, sort_results=True) is every j with
          ((dx*dx + dy*dy) + dz*dz) <= r*r in float64, ascending.  Equal distances: ascending index (sklearn: unspecified).
  pick    the reference reads the coordinates back from the KD-tree (`np.array(tree.data)`), which holds them as float64: pick =
          float64(sub_points[point]) + noise, float64; pos = (float64(sub_points[inds]) - pick).astype(float32).
  Tukey   d32 = float32 sum of squares of the float64 differences rounded to float32; np.square(python float) is a float64 scalar, which
          promotes: t = (1 - d32 / r^2)^2 and the test d32 > r^2 are float64.
  vote    per sub-point the float32 sum of its logits rows in ascending (batch, slot) order from +0, divided by their number;
          zero logits for a sub-point no sphere visited (the reference's scatter output would be too short there)."""
import numpy as np


def radius_query(sub_points, pick, radius):
    """-> (indices ascending by (d2, index), d2 of every point) for one centre `pick` (3,) float64"""
    p = np.asarray(sub_points, dtype=np.float32).astype(np.float64)
    c = np.asarray(pick, dtype=np.float64).reshape(3)
    d = p - c
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inside = np.flatnonzero(d2 <= float(radius) * float(radius))
    return inside[np.argsort(d2[inside], kind="stable")], d2


def pick_point(sub_points, point, noise):
    return (np.asarray(sub_points, dtype=np.float32)[int(point)].astype(np.float64).reshape(1, 3)
            + np.asarray(noise, dtype=np.float64).reshape(1, 3)).reshape(3)


def pick(potentials):
    """(cloud, point): argmin of the clouds' minima, then argmin of that cloud's potentials, first minimum in both"""
    cloud = int(np.argmin([float(np.min(p)) for p in potentials]))
    return cloud, int(np.argmin(potentials[cloud]))


def schedule_step(potentials, clouds_points, noise, radius, num_points):
    """s3dis_sphere.py:221-247: updates potentials[cloud] in place -> (cloud, point, query cut to num_points, cur)"""
    cloud, point = pick(potentials)
    pts = np.asarray(clouds_points[cloud], dtype=np.float32)
    centre = pick_point(pts, point, noise)
    q, _ = radius_query(pts, centre, radius)
    cur = len(q)
    q = q[:num_points]
    if cur:
        dists = np.sum(np.square((pts[q].astype(np.float64) - centre.reshape(1, 3)).astype(np.float32)), axis=1)
        assert dists.dtype == np.float32
        r2 = np.float64(radius) * np.float64(radius)
        tukeys = np.square(1 - dists.astype(np.float64) / r2)
        tukeys[dists.astype(np.float64) > r2] = 0
        potentials[cloud][q] += tukeys
    return cloud, point, q, cur


def schedule(potentials, clouds_points, noise, radius, num_points):
    """`len(noise)` steps from `potentials` (a list of float64 arrays, updated in place) -> (cloud_inds, point_inds, curs)"""
    out = [schedule_step(potentials, clouds_points, nz, radius, num_points) for nz in noise]
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int64))


def item(sub_points, sub_colors, sub_labels, cloud, point, noise, radius, num_points, perm, pad, gravity_dim=2):
    """s3dis_sphere.py:288-347 without a transform.  perm: a permutation of min(cur, num_points); pad: num_points - cur indices
    below cur (empty when cur >= num_points).  cur == 0 (the reference raises): the centre's point in every slot, mask 0."""
    pts = np.asarray(sub_points, dtype=np.float32)
    centre = pick_point(pts, point, noise)
    q, _ = radius_query(pts, centre, radius)
    cur = len(q)
    mask = np.zeros(num_points, dtype=np.int32)
    if cur > num_points:
        inds = q[:num_points][np.asarray(perm)]
        mask[:] = 1
    elif cur > 0:
        q = q[np.asarray(perm)]
        inds = np.hstack([q, q[np.asarray(pad, dtype=np.int64)]])
        mask[:cur] = 1
    else:
        inds = np.full(num_points, int(point), dtype=np.int64)
    inds = inds.astype(np.int64)
    original = pts[inds]
    return {"pos": (original.astype(np.float64) - centre.reshape(1, 3)).astype(np.float32), "x": np.asarray(sub_colors)[inds].astype(np.float32),
            "y": np.asarray(sub_labels)[inds].astype(np.int64), "mask": mask, "cloud_index": np.int64(cloud), "input_inds": inds,
            "heights": original[:, gravity_dim:gravity_dim + 1].astype(np.float32), "cur": cur}


def vote(logits, input_inds, n_sub, projections, labels, num_classes, ignore_index=None):
    """logits (M,C) float32 rows in (batch, slot) order, input_inds (M) -> voted (n_sub,C), pred (n_sub), projected pred, the
    confusion matrix (rows: truth, columns: prediction) over the raw points"""
    logits = np.asarray(logits, dtype=np.float32)
    inds = np.asarray(input_inds, dtype=np.int64).reshape(-1)
    total = np.zeros((n_sub, logits.shape[1]), dtype=np.float32)
    np.add.at(total, inds, logits)  # unbuffered: row after row, ascending position
    cnt = np.bincount(inds, minlength=n_sub).astype(np.float32)
    voted = total / np.maximum(cnt, np.float32(1))[:, None]
    pred = voted.argmax(1)
    proj = pred[np.asarray(projections, dtype=np.int64)]
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    keep = np.ones(len(labels), dtype=bool) if ignore_index is None else labels != ignore_index
    cm = np.bincount(labels[keep] * num_classes + proj[keep], minlength=num_classes * num_classes).reshape(num_classes, num_classes)
    return voted, pred, proj, cm


def projections(points, sub_points):
    """per raw point the row minimum of the float32 direct-difference d2 to the sub-points -> (d2 (n,m) float32)"""
    p = np.asarray(points, dtype=np.float32)[:, None, :]
    s = np.asarray(sub_points, dtype=np.float32)[None, :, :]
    d = p - s
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
