"""tests/sphere_ref.py against what the reference's own S3DISSphere recorded (tests/golden/s3dis_sphere.npz, written by
tools/record_sphere_fixtures.py): the schedule table of every step and every output of the recorded items, exactly.

The reference leaves two orders unspecified -- equal distances inside a sphere (sklearn's sort) and, where numpy's argmin would
meet it, a tied potential minimum is at least the FIRST one, but a tie would make the test blind to a wrong rule.  The fixture
contains neither, and that is asserted here, so that a failure cannot hide behind them."""
import numpy as np
import pytest

import sphere_ref as sr
from conftest import load_golden


@pytest.fixture(scope="module")
def fx():
    g = load_golden("s3dis_sphere")
    m = g["meta"]
    g["clouds"] = [{k: g[f"cloud{c}/{k}"] for k in ("sub_points", "sub_colors", "sub_labels", "points", "labels", "potentials",
                                                     "projections")} for c in range(2)]
    assert m["numpy"].split(".")[0] >= "2", "the fixture's Tukey weights are numpy >= 2 arithmetic (float64)"
    return g


def _replay(fx):
    """the schedule from the recorded potentials and noise -> the restatement's table, and per step what the test checks"""
    m = fx["meta"]
    pots = [c["potentials"].copy() for c in fx["clouds"]]
    pts = [c["sub_points"] for c in fx["clouds"]]
    steps = []
    for nz in fx["noise"]:
        before = [p.copy() for p in pots]
        cloud, point, q, cur = sr.schedule_step(pots, pts, nz, m["in_radius"], m["num_points"])
        steps.append((cloud, point, q, cur, before))
    return steps, pots


def test_the_fixture_has_no_tie_the_reference_leaves_open(fx):
    m = fx["meta"]
    steps, _ = _replay(fx)
    for s, (cloud, point, q, cur, before) in enumerate(steps):
        mins = [float(p.min()) for p in before]
        assert len(set(mins)) == len(mins), f"step {s}: two clouds share the minimum potential"
        assert int((before[cloud] == mins[cloud]).sum()) == 1, f"step {s}: a tied potential minimum"
        centre = sr.pick_point(fx["clouds"][cloud]["sub_points"], point, fx["noise"][s])
        allq, d2 = sr.radius_query(fx["clouds"][cloud]["sub_points"], centre, m["in_radius"])
        assert len(np.unique(d2[allq])) == len(allq), f"step {s}: equal distances inside the sphere"
        assert len(np.unique(np.sqrt(d2[allq]))) == len(allq), f"step {s}: equal distances after sklearn's square root"


def test_the_fixture_takes_both_branches(fx):
    m = fx["meta"]
    curs = [s[3] for s in _replay(fx)[0]][:m["items"]]
    assert any(c > m["num_points"] for c in curs) and any(0 < c < m["num_points"] for c in curs), curs


def test_the_schedule_table_is_the_references(fx):
    steps, _ = _replay(fx)
    np.testing.assert_array_equal([s[0] for s in steps], fx["cloud_inds"])
    np.testing.assert_array_equal([s[1] for s in steps], fx["point_inds"])
    assert len(set(fx["cloud_inds"].tolist())) == 2, "both clouds are picked"


def test_every_recorded_item_is_reproduced_exactly(fx):
    m = fx["meta"]
    for i in range(m["items"]):
        c = int(fx["cloud_inds"][i])
        cl = fx["clouds"][c]
        got = sr.item(cl["sub_points"], cl["sub_colors"], cl["sub_labels"], c, fx["point_inds"][i], fx["noise"][i], m["in_radius"],
                      m["num_points"], fx[f"item{i}/perm"], fx[f"item{i}/pad"], m["gravity_dim"])
        for k in ("pos", "x", "y", "mask", "cloud_index", "input_inds", "heights"):
            want = fx[f"item{i}/{k}"]
            assert got[k].dtype == want.dtype and got[k].shape == want.shape, (i, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
            np.testing.assert_array_equal(got[k], want, err_msg=f"item {i}: {k}")
        assert len(fx[f"item{i}/perm"]) == min(got["cur"], m["num_points"])
        assert len(fx[f"item{i}/pad"]) == max(m["num_points"] - got["cur"], 0)


def test_the_recorded_projections_are_nearest_sub_points(fx):
    """sklearn's float64 nearest neighbour; the device route's float32 search may pick another point at an equal float32
    distance, which the GPU test allows for -- here: the recorded index attains the float64 row minimum"""
    for cl in fx["clouds"]:
        p, s = cl["points"].astype(np.float64), cl["sub_points"].astype(np.float64)
        for lo in range(0, len(p), 1000):
            d = ((p[lo:lo + 1000, None, :] - s[None]) ** 2).sum(-1)
            np.testing.assert_array_equal(d[np.arange(d.shape[0]), cl["projections"][lo:lo + 1000]], d.min(1))


def test_the_vote_is_the_mean_in_position_order():
    rng = np.random.default_rng(3)
    inds = rng.integers(0, 50, 400)
    inds[inds == 7] = 8  # sub-point 7 is never visited
    logits = rng.normal(size=(400, 5)).astype(np.float32)
    proj = rng.integers(0, 50, 90)
    labels = rng.integers(0, 5, 90)
    voted, pred, got, cm = sr.vote(logits, inds, 50, proj, labels, 5)
    for j in range(50):
        rows = logits[inds == j]
        acc = np.zeros(5, np.float32)
        for r in rows:
            acc = acc + r
        np.testing.assert_array_equal(voted[j], acc / np.float32(max(len(rows), 1)))
    assert not voted[7].any() and pred[7] == 0
    assert cm.sum() == 90 and cm[labels[0], got[0]] >= 1
    # torch_scatter's mean (sum / count) agrees up to the order of the float32 sum
    want = np.stack([logits[inds == j].astype(np.float64).mean(0) if (inds == j).any() else np.zeros(5) for j in range(50)])
    assert np.abs(voted - want).max() <= 1e-5
