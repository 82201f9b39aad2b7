"""The offset-layout pointops surface, on the host: the NumPy restatement (tests/pointops_offset_ref.py) against the oracle's
dense kernels per segment and against the fixtures recorded from the reference's own pointops.py
(tools/record_pointops_fixtures.py), the module's names and signatures, the compat entry points, and the offset checks that
run before any GPU call."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import pointops_offset_ref as R
from conftest import GOLDEN, load_golden

MIXES = ([40, 300, 7], [2500, 130, 1], [65, 64, 63, 1100], [3, 1, 2], [1030, 2050])


def sample_counts(counts, rule):
    """per segment: the whole segment, a third of it, or one sample, rotating with the segment's position"""
    picks = []
    for s, c in enumerate(counts):
        which = (s + rule) % 3
        picks.append(c if which == 0 else max(1, c // 3) if which == 1 else 1)
    return picks


@pytest.fixture(scope="module")
def fix():
    return load_golden("pointops_offset")


@pytest.mark.parametrize("kind", ["lattice", "dup"])
@pytest.mark.parametrize("counts", MIXES, ids=lambda c: "-".join(map(str, c)))
def test_ragged_fps_is_the_dense_fps_of_each_segment(counts, kind):
    from oracle import pointops_ref as K
    xyz = np.concatenate([R.cloud(5 + i, c, kind) for i, c in enumerate(counts)])
    for rule in (0, 1):
        picks = sample_counts(counts, rule)
        got, tmp = R.furthestsampling(xyz, R.ends(counts), R.ends(picks))
        for (a, b), (ma, mb) in zip(R.segments(R.ends(counts)), R.segments(R.ends(picks))):
            want = K.furthest_point_sample(torch.from_numpy(xyz[a:b])[None], mb - ma)[0].numpy() + a
            np.testing.assert_array_equal(got[ma:mb], want)
        assert tmp.dtype == np.float32 and tmp.shape == (xyz.shape[0],)


@pytest.mark.parametrize("kind,radius,nsample", [("uniform", 0.3, 16), ("lattice", 0.25, 16), ("dup", 10.0, 70), ("uniform", 1e-6, 5),
                                                 ("lattice", 0.25, 1)])
def test_ragged_ball_query_is_the_dense_one_of_each_segment(kind, radius, nsample):
    from oracle import pointops_ref as K
    counts, qcounts = [1, 2, 65, 300, 7], [1, 1, 20, 75, 3]
    xyz = np.concatenate([R.cloud(9 + i, c, kind) for i, c in enumerate(counts)])
    rng = np.random.default_rng(3)
    if radius < 1e-3:  # queries that are no support points: whole rows stay zero
        q = np.concatenate([R.cloud(40 + i, c, kind) + np.float32(0.37) for i, c in enumerate(qcounts)])
    else:
        q = np.concatenate([xyz[a:b][rng.permutation(b - a)[:c]] for (a, b), c in zip(R.segments(R.ends(counts)), qcounts)])
    got = R.ballquery(radius, nsample, xyz, q, R.ends(counts), R.ends(qcounts))
    for (a, b), (qa, qb) in zip(R.segments(R.ends(counts)), R.segments(R.ends(qcounts))):
        dense = K.ball_query(radius, nsample, torch.from_numpy(xyz[a:b])[None], torch.from_numpy(q[qa:qb])[None])[0].numpy()
        hit = (R.dist2(q[qa:qb, None, :], xyz[None, a:b, :]) < np.float32(radius) * np.float32(radius)).any(1)
        want = np.where(hit[:, None], dense + a, 0)  # a row without a hit is global row 0, not the segment's start
        np.testing.assert_array_equal(got[qa:qb], want)
    if radius < 1e-3:
        assert not got.any()


def weights_of(dist):
    """pointops.py:258-260 / 278-280 on the recorded distances, in torch on the CPU as the recorder ran it"""
    d = torch.from_numpy(dist)
    r = 1.0 / (d + 1e-8)
    return (r / torch.sum(r, dim=1, keepdim=True)).numpy()


def test_restatement_reproduces_the_recorded_fixtures(fix):
    xyz, new_xyz, offset, new_offset, feat = fix["xyz"], fix["new_xyz"], fix["offset"], fix["new_offset"], fix["feat"]
    meta = fix["meta"]
    ns, n = meta["nsample"], xyz.shape[0]
    eq = np.testing.assert_array_equal
    idx, _ = R.furthestsampling(xyz, offset, new_offset)
    eq(idx, fix["furthestsampling/idx"])
    eq(xyz[idx], new_xyz)
    ball = R.ballquery(meta["radius"], ns, xyz, new_xyz, offset, new_offset)
    eq(ball, fix["ballquery/idx"])

    eq(R.grouping_forward(feat, ball), fix["grouping/out0"])
    eq(R.grouping_backward(fix["grouping/up0"], ball, n), fix["grouping/grad0"])

    knn = fix["knnquery/idx"]
    for method, nbr in (("knn", knn), ("knnquery", knn), ("ballquery", ball)):
        for norm in (0, 1):
            key = f"querygroup/{method}/{norm}"
            dp = R.grouping_forward(xyz, nbr) - new_xyz[:, None, :]
            if norm and method == "knn":  # each neighbour offset by its own norm: the largest norm afterwards is 1
                got = fix[key + "/out0"]
                assert np.abs(np.linalg.norm(got.astype(np.float64), axis=-1)).max() <= 1.0 + 1e-6
                live = np.linalg.norm(dp, axis=-1) > 1e-4
                np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=-1)[live], 1.0, rtol=1e-5)
            elif norm:
                eq(dp / np.float32(meta["radius"]), fix[key + "/out0"])
            else:
                eq(dp, fix[key + "/out0"])
            eq(R.grouping_forward(feat, nbr), fix[key + "/out1"])
            eq(R.grouping_backward(fix[key + "/up1"], nbr, n), fix[key + "/grad0"])
    eq(R.grouping_backward(fix["querygroup_xyz/up0"], knn, n), fix["querygroup_xyz/grad0"])

    both = np.concatenate([R.grouping_forward(xyz, knn) - new_xyz[:, None, :], R.grouping_forward(feat, knn)], -1)
    eq(both, fix["queryandgroup/1/out0"])
    eq(both[..., 3:], fix["queryandgroup/0/out0"])
    eq(R.grouping_backward(fix["queryandgroup/1/up0"][..., 3:], knn, n), fix["queryandgroup/1/grad0"])
    eq(R.grouping_forward(feat, ball), fix["queryandgroup_idx/out0"][..., 3:])

    sidx = fix["self_idx"]
    eq(R.subtraction_forward(feat, fix["feat2"], sidx), fix["subtraction/out0"])
    g1, g2 = R.subtraction_backward(fix["subtraction/up0"], sidx)
    eq(g1, fix["subtraction/grad0"])
    eq(g2, fix["subtraction/grad1"])

    eq(R.aggregation_forward(feat, fix["position"], fix["weight"], sidx), fix["aggregation/out0"])
    gi, gp, gw = R.aggregation_backward(feat, fix["position"], fix["weight"], sidx, fix["aggregation/up0"])
    eq(gi, fix["aggregation/grad0"])
    eq(gp, fix["aggregation/grad1"])
    eq(gw, fix["aggregation/grad2"])

    w = weights_of(fix["interpolation/dist"])
    up = fix["interpolation/idx"]
    eq(R.interpolation_forward(fix["feat_m"], up, w), fix["interpolation2/out0"])
    eq(R.interpolation_backward(fix["interpolation2/up0"], up, w, fix["feat_m"].shape[0]), fix["interpolation2/grad0"])
    # the torch loop adds the same rounded products in the same order
    eq(fix["interpolation/out0"], fix["interpolation2/out0"])


def test_exact_forms_bound_the_sequential_sums(fix):
    """the fp64 forms return (exact, sum |terms|, in-degree); the sequential fp32 sum lies within the any-order bound"""
    sidx, up = fix["self_idx"], fix["subtraction/up0"]
    _, g2 = R.subtraction_backward(up, sidx)
    exact, mag, deg = R.subtraction_backward_exact(up, sidx)
    assert deg.sum() == sidx.size * up.shape[2] and (mag >= np.abs(exact) - 1e-12).all()
    assert (np.abs(g2 - exact) <= 2 * (deg + 1) * 2.0 ** -24 * mag).all()


def test_module_has_every_name_of_the_reference_with_its_parameters():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.cpp.pointops.functions import pointops as P
    sig = json.load(open(os.path.join(GOLDEN, "pointops_offset_signatures.json")))
    assert {"FurthestSampling", "furthestsampling", "KNNQuery", "knnquery", "BallQuery", "ballquery", "Grouping", "grouping",
            "querygroup", "queryandgroup", "Subtraction", "subtraction", "Aggregation", "aggregation", "interpolation",
            "Interpolation", "interpolation2"} == set(sig)

    def params(fn, drop_first=False):
        ps = list(inspect.signature(fn).parameters.values())[1 if drop_first else 0:]
        return [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in ps]

    for name, want in sig.items():
        obj = getattr(P, name)
        if want["kind"] == "Function":
            assert issubclass(obj, torch.autograd.Function)
            assert params(obj.forward, drop_first=True) == want["forward"], name
        elif want["kind"] == "function":
            assert params(obj) == want["params"], name
        else:
            assert obj.__self__ is getattr(P, want["of"]), name


def test_compat_pointops_module_has_all_eleven_entry_points():
    from amcontrast3d_amd import compat
    assert len(R.ENTRY_POINTS) == 11
    for name in R.ENTRY_POINTS:  # pointops_api.cpp:14-24
        assert callable(getattr(compat.pointops_cuda, name)), name
    ref = R.as_pointops_cuda()
    for name in R.ENTRY_POINTS:
        if name != "knnquery_cuda":  # as many positional parameters as the stand-in that ran under the reference's wrappers
            assert len(inspect.signature(getattr(compat.pointops_cuda, name)).parameters) == \
                len(inspect.signature(getattr(ref, name)).parameters), name


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def test_offsets_are_checked_on_the_host_before_any_gpu_call():
    from amcontrast3d_amd import offset_ops as O
    xyz, q = torch.zeros(10, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="non-decreasing"):
        O.furthestsampling(xyz, i32(6, 4, 10), i32(1, 2, 4))
    with pytest.raises(ValueError, match="non-decreasing"):
        O.furthestsampling(xyz, i32(4, 10), i32(3, 2))
    with pytest.raises(ValueError, match="10 rows"):
        O.furthestsampling(xyz, i32(4, 9), i32(2, 4))
    with pytest.raises(ValueError, match="segments"):
        O.furthestsampling(xyz, i32(4, 10), i32(4))
    with pytest.raises(ValueError, match="asks for 5 samples of 4 points"):
        O.furthestsampling(xyz, i32(4, 10), i32(5, 6))
    with pytest.raises(ValueError, match="non-decreasing"):
        O.ballquery(0.1, 4, xyz, q, i32(7, 3, 10), i32(2, 4))
    with pytest.raises(ValueError, match="10 rows"):
        O.ballquery(0.1, 4, xyz, q, i32(4, 11), i32(2, 4))
    with pytest.raises(ValueError, match="4 rows"):
        O.ballquery(0.1, 4, xyz, q, i32(4, 10), i32(2, 5))
    # valid offsets on CPU tensors: the package's refusal to compute on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        O.furthestsampling(xyz, i32(4, 10), i32(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        O.ballquery(0.1, 4, xyz, q, i32(4, 10), i32(2, 4))
