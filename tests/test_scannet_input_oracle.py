"""The numpy restatement of ScanNet's training input (tests/scannet_input_ref.py) against what the reference's own
ScanNet.__getitem__ and transforms returned for the same raw rooms and the same random draws
(tests/golden/scannet_input.npz, recorded by tests/tools/gen_golden_scannet.py).  CPU only."""
import numpy as np
import pytest

import scannet_input_ref as ref
from conftest import load_golden

CASES = ("a", "b")


def _case(g, tag):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}


@pytest.fixture(scope="module")
def golden():
    return load_golden("scannet_input")


def test_fixture_covers_the_branches(golden):
    a, b = _case(golden, "a"), _case(golden, "b")
    assert a["contrast_u"] < 0.2 and a["mirror_u"][0] <= 0.2 and a["drop_u"] >= 0.2
    assert len(a["count"]) >= int(a["voxel_max"]) and len(a["crop_idx"]) == int(a["voxel_max"])
    assert b["contrast_u"] >= 0.2 and b["drop_u"] < 0.2 and len(b["count"]) < int(b["voxel_max"]) and len(b["pad"]) > 0
    for c in (a, b):
        assert c["t_pos"].dtype == np.float64 and c["pos"].shape == (int(c["voxel_max"]), 3) and np.any(c["label"] == -100)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(golden, tag):
    c = _case(golden, tag)
    pos, x = ref.transform_room(c["coord"], c["feat"], c["R"], c["scale"][0], c["mirror_u"], c["contrast_u"], c["blend"],
                                c["drop_u"])
    np.testing.assert_array_equal(pos, c["t_pos"])
    np.testing.assert_array_equal(x, c["t_x"])
    vm = int(c["voxel_max"])
    init = int(c["init_idx"]) if c["init_idx"] >= 0 else None
    got = ref.crop_room(pos, x, c["label"], 0.02, vm, False, c["rnd"], init, c["pad"], c["perm"])
    np.testing.assert_array_equal(got["key"], c["key"])
    np.testing.assert_array_equal(got["count"], c["count"])
    np.testing.assert_array_equal(c["key"][got["idx_unique"]], c["key"][c["idx_unique"]])  # same voxel for every pick
    # the reference's sorts are unstable: follow its picks and crop order for the quantities that depend on them
    same = ref.crop_room(pos, x, c["label"], 0.02, vm, False, c["rnd"], init, c["pad"], c["perm"], pick=c["idx_unique"],
                         crop=c["crop_idx"] if init is not None else None)
    if init is not None:
        np.testing.assert_array_equal(same["d2"], c["d2"])
        assert set(np.argsort(same["d2"], kind="stable")[:vm].tolist()) == set(c["crop_idx"].tolist()) or \
            np.sum(c["d2"] == c["d2"][c["crop_idx"][-1]]) > 1
    for k in ("pos", "x", "y", "heights"):
        np.testing.assert_array_equal(same[k], c[k])


def test_cos_sin_rotation_is_within_a_few_ulp_of_expm(golden):
    for tag in CASES:
        c = _case(golden, tag)
        R = ref.rotation(float(c["angle"]))
        assert np.max(np.abs(R - c["R"])) <= 16 * np.finfo(np.float64).eps
