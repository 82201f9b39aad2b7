"""What test_gpu_geometry_edges.py relies on, asserted on the CPU with the oracle alone (no GPU): the clouds of
geometry_clouds.py are what their names say, and no query of an untied k-NN case has two equal distances among its k+1
nearest.  A tied query is handed to the heap replay (csrc/knn.hip, knn_exact_list_kernel), which is right whatever the grid
kernel did; only an untied query's stored list is the grid kernel's own."""
import numpy as np
import pytest
import torch

import geometry_clouds as G

CASES = G.knn_cases()
GRID_CASES = sorted(name for name, c in CASES.items() if c.grid)


def tied_rows(c):
    """queries with two equal distances among their k+1 nearest (placeholders of a segment with fewer points do not
    count), from the reference's own distance expression -- as test_gpu_knn_groups.tie_share"""
    from oracle import pointops_ref as K
    q = c.queries
    m = q.shape[0]
    iw = torch.zeros(m, c.k + 1, dtype=torch.int32)
    dw = torch.zeros(m, c.k + 1)
    K.knnquery_cuda(m, c.k + 1, torch.from_numpy(c.xyz), torch.from_numpy(q), torch.tensor(c.off, dtype=torch.int32),
                    torch.tensor(c.qoff, dtype=torch.int32), iw, dw)
    d = dw.numpy()
    return ((d[:, 1:] == d[:, :-1]) & (d[:, 1:] < 1e10)).any(axis=1)


@pytest.mark.parametrize("name", GRID_CASES)
def test_tie_share_of_every_grid_case(name):
    """exactly 0 over the rows of the untied kinds; `point` ties every query; `clusters` and `outlier` are recorded only
    (they are there for the grid build, the shell expansion and the hand-over to the replay).  The k = 100 cases take
    the all-pairs heap, which is the reference's own scan (and k + 1 = 101 is beyond what the reference's heap holds)."""
    c = CASES[name]
    tied = tied_rows(c)
    assert tied.shape == c.untied_rows.shape
    share = float(tied[c.untied_rows].mean()) if c.untied_rows.any() else None
    print(f"{name}: tied share {float(tied.mean()):.4f} of all rows, {share} of the rows that must not tie")
    if share is not None:
        assert share == 0.0, f"{int(tied[c.untied_rows].sum())} tied queries"
    if "-point-" in name:
        assert tied.all()
    if name.startswith("ragged-"):
        first = c.off[0]
        assert tied[:first].all() and not c.untied_rows[:first].any() and c.untied_rows[first:].all()


def test_every_untied_kind_has_its_grid_cases():
    for kind in G.UNTIED:
        for n in G.SELF_N:
            for k in G.SELF_K_GROUP + (G.SELF_K_WAVE,):
                c = CASES[f"self-{kind}-{n}-{k}"]
                assert c.grid and c.untied_rows.all() and c.xyz.shape == (n, 3) and c.xyz.dtype == np.float32
    for kind in G.KINDS:
        for n in G.SELF_N:
            assert not CASES[f"self-{kind}-{n}-{G.SELF_K_HEAP}"].grid


@pytest.mark.parametrize("kind", G.KINDS)
def test_clouds_are_what_they_say(kind):
    n = 2049
    p = G.cloud(kind, 3, n)
    assert p.shape == (n, 3) and p.dtype == np.float32 and p.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(p, G.cloud(kind, 3, n))  # seeded
    ext = p.max(0) - p.min(0)
    lo = p.min(0) - G.offset_of(kind)
    if kind in ("far", "outlier", "clusters"):
        assert (ext > 0).all()
    if kind in ("far", "far_plane"):
        assert (lo >= 0).all() and (lo < 2).all() and (np.abs(p).min(0) >= 512).all()
    if kind in ("plane_z", "far_plane"):
        assert ext[2] == 0 and (ext[:2] > 1.9).all() and p[0, 2] == np.float32(0.75 + G.offset_of(kind)[2])
    if kind == "plane_x":
        assert ext[0] == 0 and (ext[1:] > 1.9).all() and p[0, 0] == np.float32(-0.5)
    if kind == "line":
        assert ext[0] > 1.9 and ext[1] == 0 and ext[2] == 0 and p[0, 1] == 1 and p[0, 2] == -3
    if kind == "point":
        assert (p == np.array(G.POINT, dtype=np.float32)).all()
    if kind == "clusters":
        a, b = p[:n // 2], p[n // 2:]
        assert (a >= 0).all() and (a < 0.0101).all() and (b >= 100).all() and (b < 100.0101).all()
        assert abs(len(a) - len(b)) <= 1


def test_outside_queries_lie_outside_the_support_box():
    for kind in G.APART_KINDS:
        c = CASES[f"apart-{kind}"]
        lo, hi = c.xyz.min(0), c.xyz.max(0)
        if kind == "outlier":  # its box reaches the remote rows: take the main cloud's
            lo, hi = c.xyz[:-G.OUTLIER_ROWS].min(0), c.xyz[:-G.OUTLIER_ROWS].max(0)
        outside = ((c.q < lo) | (c.q > hi)).any(axis=1)
        assert outside.mean() >= 0.5, outside.mean()
    q = G.outside_queries(7, 4000)
    assert q.dtype == np.float32 and (q >= -1).all() and (q <= 3).all()
    assert 0.8 < ((q < 0) | (q >= 2)).any(axis=1).mean() < 0.95  # 7/8
    sup = G.cloud("far", 2, 100)
    s = G.superset_queries(sup, 7, 300, G.offset_of("far"))
    np.testing.assert_array_equal(s[:100], sup)
    np.testing.assert_array_equal(s[100:], G.outside_queries(7, 200, G.offset_of("far")))


@pytest.mark.parametrize("seed,n", sorted({(G.SELF_SEED["outlier"], n) for n in G.SELF_N}
                                          | {(G.APART_SEED["outlier"][0], 6000), (G.REUSE_SEED["outlier"], 8192)}))
def test_outlier_rows_have_exactly_four_neighbours_within_distance_one(seed, n):
    """so k = 4 (the row itself and three of them) ends next door and k > 5 has to cross the gap"""
    p = G.cloud("outlier", seed, n).astype(np.float64)
    for row in p[n - G.OUTLIER_ROWS:]:
        d = np.sqrt(((p - row) ** 2).sum(1))
        assert int((d <= 1.0).sum()) == 1 + 4  # itself and the other four
    main = p[:n - G.OUTLIER_ROWS]
    assert (main >= 0).all() and (main < 2).all()
