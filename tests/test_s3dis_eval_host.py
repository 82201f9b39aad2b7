"""Host side of S3DIS validation / whole-room testing: the numpy restatements of tests/s3dis_eval_ref.py -- which the GPU
tests use where the reference leaves a bit unspecified (the xy-centre's torch.mean) -- pinned to what the reference's own code
returned (tests/golden/s3dis_eval.npz, tests/tools/gen_golden_s3dis_eval.py), and the fixture's own claims."""
import math

import numpy as np
import pytest

import s3dis_eval_ref as ref
from conftest import load_golden

BATCH = 3  # the `batch` of tests/test_gpu_s3dis_eval.py


@pytest.fixture(scope="module")
def g():
    return load_golden("s3dis_eval")


def _room(g, tag):
    room = ref.fixture_room(g, tag)
    cdata = ref.fixture_cdata(room)
    return room, cdata, cdata[:, :3] - cdata[:, :3].min(0), cdata[:, 3:6]


def _sub_clouds(g, tag):
    """every recorded sub-cloud: (name, mode, coord, colour, idx, recorded rows, columns of the sub-cloud they are, centre)"""
    room, cdata, shifted, colour = _room(g, tag)
    parts, pick = room["parts"].astype(np.int64), room["pick"].astype(np.int64)
    for i in range(len(parts)):
        yield f"rows/{i}", "test", shifted, colour, parts[i], room[f"rows/{i}"], pick, room["centre"][i]
        if f"full/{i}" in room:
            yield f"full/{i}", "test", shifted, colour, parts[i], room[f"full/{i}"], slice(None), room["centre"][i]
    yield "nn", "test", shifted, colour, room["nn/part"].astype(np.int64), room["nn/rows"], pick, room["nn/centre"]
    c32 = cdata.astype(np.float32)
    yield ("val", "val", c32[:, :3] - c32[:, :3].min(0), np.ascontiguousarray(c32[:, 3:6]), room["val/idx_unique"].astype(np.int64),
           room["val/full"], slice(None), room["val/centre"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_the_reference_run(g, tag):
    """both routes bit for bit, given the centre the reference's torch.mean returned"""
    rows = g["meta"]["rows"]
    seen = 0
    for name, mode, coord, colour, idx, rec, cols, centre in _sub_clouds(g, tag):
        pos, x, heights, inp = ref.fixture_rows(rec, rows)
        got = ref.sub_cloud(coord, colour, idx, mode, centre=centre)
        for a, b, what in zip(got, (pos, x, heights), ("pos", "x", "heights")):
            assert a.dtype == b.dtype and np.array_equal(a[cols], b), (name, what)
        assert np.array_equal(ref.assemble(*got[:3])[:, cols], inp), name
        seen += 1
    room = ref.fixture_room(g, tag)
    assert seen == len(room["parts"]) + len(g["meta"]["full"][tag]) + 2
    cdata = ref.fixture_cdata(room)
    assert np.array_equal(room["label_u8"][room["val/idx_unique"]], room["val/y"])
    raw = cdata.astype(np.float32)[room["val/idx_unique"], 3:6]
    assert (raw.max() > 1) == (tag == "a")  # the / 255 branch taken (a) and not taken (b)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_rooms_meet_their_shape_conditions(g, tag):
    room, cdata, shifted, _ = _room(g, tag)
    assert cdata.dtype == (np.float64 if tag == "a" else np.float32) and 5000 < len(cdata) < 7000
    assert g["meta"]["voxel_size"] == ref.VOXEL == 0.06
    for k, v in ref.make_raw_room(tag).items():  # the stored rooms are the generator's
        assert np.array_equal(room[k], v), k
    if tag == "a":  # float64 for a reason: the coordinates are no float32 numbers
        assert (cdata[:, :3].astype(np.float32) != cdata[:, :3]).mean() > 0.5
    count = room["count"].astype(np.int64)
    P = int(count.max())
    assert room["parts"].shape == (P, len(count)) and count.sum() == len(cdata)
    assert P >= 5 and (count == 1).any() and (P % count != 0).any() and P % BATCH != 0
    perm, start = ref.fixture_perm(room)
    idx_sort = room["idx_sort"].astype(np.int64)
    for i in range(P):
        assert np.array_equal(idx_sort[start[perm[i]] + i % count[perm[i]]], room["parts"][i])
    # the voxels are those of a stable sort; only the order inside a voxel is the reference's own
    s_sort, voxel_idx, st, ct = ref.stable_tables(shifted)
    assert np.array_equal(ct, count) and np.array_equal(voxel_idx, room["voxel_idx"]) and np.array_equal(st, start)
    # nearest neighbour: the representatives, the inverse permutation and the expansion
    rnd, nperm = room["nn/rnd"].astype(np.int64), room["nn/perm"].astype(np.int64)
    assert np.array_equal(room["nn/part"], idx_sort[start[:-1] + rnd % count][nperm])
    assert np.array_equal(room["nn/where"], np.argsort(nperm)) and (rnd >= count).any()
    voxel_of = np.empty(len(cdata), np.int64)
    voxel_of[idx_sort] = room["voxel_idx"]
    assert np.array_equal(room["nn/expand"], room["nn/where"][voxel_of])
    # the val item's picks
    v_sort, v_count = room["val/idx_sort"].astype(np.int64), room["val/count"].astype(np.int64)
    v_start = np.cumsum(np.insert(v_count, 0, 0))[:-1]
    assert np.array_equal(room["val/idx_unique"], v_sort[v_start + room["val/rnd"] % v_count])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_centres_are_clear_of_rounding_boundaries(g, tag):
    """For every recorded sub-cloud the exact column mean is further than 2**-30 (relative) from the nearest float32 rounding
    boundary, so that a fixed-order fp64 sum (relative error below n * 2**-53 < 2**-40 here) rounds as the exact mean does;
    and torch.mean's own centre lies within the recorded number of ulp of it."""
    worst, ulp = np.inf, 0
    for name, mode, coord, colour, idx, rec, cols, centre in _sub_clouds(g, tag):
        if name.startswith("full/"):
            continue
        q = coord[idx]
        if mode == "test":
            q = q - q.min(0)
        q = q.astype(np.float32)
        exact = ref.exact_centre(q)
        for c in range(3):
            m = math.fsum(q[:, c].tolist()) / len(q)
            f = exact[c]
            lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
            edge = min(abs((float(lo) + float(f)) / 2 - m), abs((float(hi) + float(f)) / 2 - m)) / abs(m)
            assert edge > 2.0 ** -30, (name, c, edge)
            worst = min(worst, edge)
        assert np.array_equal(ref.sub_cloud(coord, colour, idx, mode)[3], exact)
        ulp = max(ulp, ref.ulp_distance(centre, exact))
    print(f"{tag}: nearest rounding boundary {worst:.3e} relative; torch.mean within {ulp} ulp of the exactly rounded mean")
    assert ulp <= g["meta"]["centre_ulp"] <= 2 and g["meta"]["centre_edge"] > 2.0 ** -30
