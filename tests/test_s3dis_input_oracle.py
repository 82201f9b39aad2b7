"""The numpy restatement of one S3DIS training item (tests/s3dis_input_ref.py) against what the reference's own
S3DIS.__getitem__ and training transforms returned for the same raw rooms and the same random draws
(tests/golden/s3dis_input.npz, recorded by tests/tools/gen_golden_s3dis_input.py).  CPU only."""
import numpy as np
import pytest

import s3dis_input_ref as ref
from conftest import load_golden

CASES = ("a", "b")


def _case(g, tag):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}


def _draws(c):
    d = {k: c[k] for k in ("rnd", "pad", "perm", "blend", "scale_u", "theta", "noise")}
    d["init_idx"] = int(c["init_idx"])
    d["contrast"], d["drop"] = bool(c["contrast_u"] < 0.2), bool(c["drop_u"] < 0.2)
    return d


@pytest.fixture(scope="module")
def golden():
    return load_golden("s3dis_input")


def test_fixture_covers_the_branches(golden):
    a, b = _case(golden, "a"), _case(golden, "b")
    assert a["contrast_u"] < 0.2 and a["drop_u"] >= 0.2 and b["contrast_u"] >= 0.2 and b["drop_u"] < 0.2
    assert len(a["count"]) >= int(a["voxel_max"]) and len(a["crop_idx"]) == int(a["voxel_max"]) and a["init_idx"] >= 0
    assert len(b["count"]) < int(b["voxel_max"]) and len(b["pad"]) == int(b["voxel_max"]) - len(b["count"])
    for c in (a, b):
        assert c["cdata"].dtype == np.float64 and c["cdata"].shape[1] == 7 and np.abs(c["cdata"][:, :3]).min() > 0.2
        assert c["count"].max() > 1 and c["pos"].shape == (int(c["voxel_max"]), 3) and c["heights"].shape == (int(c["voxel_max"]), 1)
        assert not np.array_equal(c["cdata"][:, :3], c["cdata"][:, :3].astype(np.float32))  # the float32 cast rounds


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(golden, tag):
    c = _case(golden, tag)
    vm = int(c["voxel_max"])
    d = _draws(c)
    got = ref.train_item(c["cdata"], d, voxel_max=vm)
    np.testing.assert_array_equal(got["key"], c["key"])
    np.testing.assert_array_equal(got["count"], c["count"])
    np.testing.assert_array_equal(c["key"][got["idx_unique"]], c["key"][c["idx_unique"]])  # same voxel for every pick
    # the reference's sorts are unstable: follow its picks and crop order for the quantities that depend on them
    cropped = len(c["count"]) >= vm
    same = ref.train_item(c["cdata"], d, voxel_max=vm, idx_unique=c["idx_unique"], crop_idx=c["crop_idx"] if cropped else None)
    if cropped:
        np.testing.assert_array_equal(same["d2"], c["d2"])
        assert same["d2"].dtype == np.float32
        stable = np.argsort(same["d2"], kind="stable")[:vm]
        np.testing.assert_array_equal(c["d2"][stable], c["d2"][c["crop_idx"]])  # the same distances in the same order
    for k in ("pos0", "y", "heights"):
        np.testing.assert_array_equal(same[k], c[k])
    assert same["y"].dtype == np.int64 and same["pos0"].dtype == same["heights"].dtype == np.float32
    np.testing.assert_array_equal(same["heights"], same["pos0"][:, 2:3])
    # the transformed tensors, at the bounds of the chain's own fixture (tests/test_oracle_augment.py)
    np.testing.assert_allclose(same["pos"], c["pos"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(same["x"], c["x"], rtol=0, atol=2e-5)
