"""What test_gpu_csr_groups.py relies on, asserted on the CPU with numpy (no GPU): the lists of csr_group_cases.build() put
several lists of every kind into one lane group of the reverse-list collapse (csrc/csr.hip), across cloud boundaries and
around empty lists, at every `per` and kernel of the table.  These are conditions on the inputs, not measurements."""
import numpy as np
import pytest

import csr_group_cases as CG

# tag -> (B, n, C, per): the sizes follow from csr_pts_per_group()'s thresholds (n may move by a few points, per may not)
TABLE = {
    "c64-per3": (2, 64, 3), "c128-per5": (3, 128, 5), "c32-per6": (2, 32, 6), "c16-per6": (3, 16, 6), "c8-per4": (2, 8, 4),
    "c32-per16": (2, 32, 16), "c32-per17": (2, 32, 17), "c16-per17": (2, 16, 17), "c8-per17": (2, 8, 17),
}


def test_the_table_is_complete():
    assert [c.tag for c in CG.CASES] == list(TABLE)
    for c in CG.CASES:
        assert (c.B, c.C, c.per) == TABLE[c.tag] and 128 <= c.M <= 256
    assert [c.tag for c in CG.CASES if c.relu_off] == ["c64-per3", "c32-per6"]
    assert [c.tag for c in CG.CASES if c.position_major] == ["c64-per3", "c32-per6"]


def test_plan_restates_the_rule_at_known_shapes():
    """the workload's two layers, as the kernel's own comments state them, and per == 1 below 4096 * groups points"""
    assert CG.plan(8, 24000, 32)[:2] == (8, 6)
    assert CG.plan(8, 6000, 64)[:2] == (4, 3)
    assert CG.plan(3, 1500, 64) == (4, 1, 1125)
    assert CG.plan(2, 6000, 32) == (8, 1, 1500)
    assert CG.plan(2, 16384, 32)[1] == 1 and CG.plan(2, 16385, 32)[1] == 2


@pytest.mark.parametrize("case", CG.CASES, ids=lambda c: c.tag)
def test_the_lists_of_every_case(case):
    B, n, C, M = case.B, case.n, case.C, case.M
    groups, per, parts = CG.plan(B, n, C)
    idx, dp = CG.build(B, n, C, M, seed=0)
    d = CG.describe(idx, B, n, C)
    G, deg = B * n, d["deg"]
    print(f"{case.tag}: per {per}, parts {parts}, {len(d['multi'])} groups with two or more lists, {len(d['interior'])} with an "
          f"empty list inside, longest list {d['longest']}, lengths {d['lengths'].tolist()}")
    # 1. the route
    assert (per, parts) == (case.per, case.parts) and n % per != 0
    assert case.kernel.startswith(CG.kernel(B, n, C, True)) and CG.kernel(B, n, C, False) == f"gather<{min(C, 64)}>"
    # 2. every cloud boundary lies inside a lane group that has edges of both clouds
    assert len(d["straddle"]) == B - 1
    for bound, (below, above) in d["straddle_sides"].items():
        assert bound % per != 0 and below >= 1 and above >= 1, (bound, below, above)
    # 3. / 4. groups that walk from list to list, and over an empty one
    assert len(d["multi"]) >= 30
    if per >= 3:
        assert len(d["interior"]) >= 5
        assert np.isin(d["interior"], d["multi"]).all()
    # 5. the list lengths around the chunks of eight, inside such groups
    for want in (0, 1, 8, 9, 16, 17):
        assert want in d["lengths"], want
    assert d["lengths"].max() > 32
    # 6. ragged end: the last workgroup is not full and none of its points has an edge; the one before it has some
    assert G % (groups * per) != 0 and d["last_wg"] < G
    assert deg[d["last_wg"]:].sum() == 0
    assert deg[d["pts_last2"]].max() > 0
    tail = G - d["last_wg"]  # lane groups of the last workgroup: full ones, possibly a short one, possibly some without a point
    print(f"    last workgroup: {tail} points = {tail // per} full groups + {tail % per} points, {groups - -(-tail // per)} groups without")
    # 7. / 8.
    assert d["longest"] <= CG.LONGEST
    assert idx.dtype == np.int32 and idx.shape == (B, M, 32) and idx.min() >= 0 and idx.max() < n
    assert dp.dtype == np.float32 and dp.shape == (B, 3, M, 32) and np.abs(dp).max() <= 1.0
    # rows as a ball query pads them: j distinct targets in front, then repeats of slot 0; every fifth row has no such shape
    for b in range(B):
        for m in range(M):
            row = idx[b, m]
            if m % CG.UNIFORM_EVERY == 0:
                continue
            j = len(set(row.tolist()))
            assert 1 <= j <= 8 and len(set(row[:j].tolist())) == j and (row[j:] == row[0]).all()
    # the same call gives the same lists
    again, dp2 = CG.build(B, n, C, M, seed=0)
    assert np.array_equal(idx, again) and np.array_equal(dp, dp2)
