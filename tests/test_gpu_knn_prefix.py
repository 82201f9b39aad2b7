"""ops.knn_prefix (csrc/knn.hip amc3d_knn_prefix): the kr nearest support points of queries that are themselves support
points, read off the rows of a finished 24-column self search.  Indices and squared distances must carry the bits of the
search (amc3d_knnquery) and of the oracle's restatement of the reference's heap; the number of queries that were searched
after all (no unique support point, a tie through column kr, an unfilled slot) is read back and asserted, so that no case
can pass on the search alone -- or on the prefix alone where the search is what the case is about."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K0 = 24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from amcontrast3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cloud():
    """synthetic.make_batch(2, 2048) as one cloud of 4096 points: no row has a tie among its first 25 distances"""
    from amcontrast3d_amd import synthetic
    return np.ascontiguousarray(synthetic.make_batch(2, 2048)["pos"].reshape(-1, 3))


def lattice():
    g = np.arange(12, dtype=np.float32) * np.float32(0.04)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def run(dev, xyz, q, off, qoff, kr):
    """-> number of searched queries, after comparing knn_prefix with the search and with the oracle"""
    from amcontrast3d_amd import ops
    from oracle import pointops_ref as K
    xyz_c, q_c = torch.from_numpy(np.ascontiguousarray(xyz)), torch.from_numpy(np.ascontiguousarray(q))
    off_c, qoff_c = torch.tensor(off, dtype=torch.int32), torch.tensor(qoff, dtype=torch.int32)
    x, y, o, qo = xyz_c.to(dev), q_c.to(dev), off_c.to(dev), qoff_c.to(dev)
    m = y.shape[0]
    with ops.knn_grid_reuse():  # where the self search goes through the grid, the prefix pass reuses it
        rows_idx, rows_d2 = ops.knnquery_squared(K0, x, x, o, o)
        idx, d2, count = ops.knn_prefix(kr, x, y, o, qo, rows_idx, rows_d2)
        count = int(count.item())
    want_idx, want_d2 = ops.knnquery_squared(kr, x, y, o, qo)
    assert torch.equal(idx, want_idx)
    assert torch.equal(d2, want_d2)
    iw = torch.zeros(m, kr, dtype=torch.int32)
    dw = torch.zeros(m, kr)
    K.knnquery_cuda(m, kr, xyz_c, q_c, off_c, qoff_c, iw, dw)
    np.testing.assert_array_equal(idx.cpu().numpy(), iw.numpy())
    np.testing.assert_array_equal(d2.cpu().numpy(), dw.numpy())
    assert count == searched_by_rule(xyz, q, off, qoff, kr, rows_d2.cpu().numpy()), count
    return count


def searched_by_rule(xyz, q, off, qoff, kr, rows_d2):
    """the queries the rule sends to the search, from the self search's distances: no single support point of the query's
    segment has its coordinates, or that point's row does not ascend strictly through column kr, or column kr is unfilled"""
    n = 0
    for i, pt in enumerate(q):
        s = int(np.searchsorted(qoff, i, side="right"))
        lo, hi = (off[s - 1] if s else 0), off[s]
        same = np.flatnonzero((xyz[lo:hi] == pt).all(1))
        row = rows_d2[lo + same[0]] if len(same) == 1 else None
        n += not (row is not None and (row[:kr] < row[1:kr + 1]).all() and row[kr] < 1e10)
    return n


@pytest.mark.parametrize("kr,step", [(4, 4), (16, 16)])
def test_random_cloud_takes_the_prefix(dev, cloud, kr, step):
    q = cloud[::step]
    searched = run(dev, cloud, q, [len(cloud)], [len(q)], kr)
    assert searched <= len(q) // 100, searched


@pytest.mark.parametrize("kr,step", [(4, 4), (16, 16)])
def test_lattice_is_searched(dev, kr, step):
    """12 x 12 x 12 points of edge 0.04: 12 of the 1728 rows are free of ties through column 4"""
    xyz = lattice()
    q = xyz[::step]
    searched = run(dev, xyz, q, [len(xyz)], [len(q)], kr)
    assert searched >= len(q) - 12, searched


@pytest.mark.parametrize("kr", [4, 16])
def test_coincident_points_are_searched(dev, cloud, kr):
    pick = np.arange(32) * 97 + 5
    xyz = np.concatenate([cloud, cloud[pick]])
    assert run(dev, xyz, cloud[pick], [len(xyz)], [32], kr) == 32
    q = np.concatenate([cloud[pick], cloud[::8]])  # among other queries
    searched = run(dev, xyz, q, [len(xyz)], [len(q)], kr)
    assert 32 <= searched < len(q), searched  # (and the neighbours of a doubled point, whose rows hold a tie)


def test_tie_at_the_cut_is_searched(dev, cloud):
    """a query whose 4th and 5th nearest (itself included) are equally far: columns 3 and 4 of its row"""
    c = np.float32(50.0)

    def with_cluster(last):
        pts = np.array([[0, 0, 0], [0.125, 0, 0], [0, 0.25, 0], [0.5, 0, 0], last, [0, 0, 2], [0, 3, 0]], dtype=np.float32) + c
        return np.concatenate([cloud, pts]), pts[:1]

    xyz, q = with_cluster([-0.5, 0, 0])
    assert run(dev, xyz, q, [len(xyz)], [1], 4) == 1
    xyz, q = with_cluster([-0.75, 0, 0])  # the same without the tie
    assert run(dev, xyz, q, [len(xyz)], [1], 4) == 0


@pytest.mark.parametrize("kr,short,searched_short", [(4, 20, False), (16, 20, False), (16, 10, True)])
def test_short_segment(dev, cloud, kr, short, searched_short):
    """a segment with fewer points than the rows have columns: its rows end in 1e10 slots; with no more than kr points the
    slot in column kr is one of them and the segment's queries are searched"""
    off = [short, len(cloud)]
    q = np.concatenate([cloud[:short:3], cloud[short::16]])
    nq0 = len(cloud[:short:3])
    searched = run(dev, cloud, q, off, [nq0, len(q)], kr)
    if searched_short:
        assert nq0 <= searched <= nq0 + len(q) // 100, searched
    else:
        assert searched <= len(q) // 100, searched


@pytest.mark.parametrize("kr", [4, 16])
def test_two_segments(dev, cloud, kr):
    cut = 1500
    q = np.concatenate([cloud[1:cut:5], cloud[cut::7]])
    nq0 = len(cloud[1:cut:5])
    searched = run(dev, cloud, q, [cut, len(cloud)], [nq0, len(q)], kr)
    assert searched <= len(q) // 100, searched
    # a point of the other segment as a query of this one: not a support point of ITS segment
    q = np.concatenate([cloud[cut:cut + 3], cloud[0:3]])
    assert run(dev, cloud, q, [cut, len(cloud)], [3, 6], kr) == 6


@pytest.mark.parametrize("kr", [4, 16])
def test_foreign_queries_are_searched(dev, cloud, kr):
    from amcontrast3d_amd import synthetic
    q = np.ascontiguousarray(synthetic.make_batch(1, 200, first_id=7)["pos"].reshape(-1, 3))
    assert run(dev, cloud, q, [len(cloud)], [len(q)], kr) == len(q)


def test_label_votes_take_the_route_inside_the_plan(dev, cloud, monkeypatch):
    """ops.knn_of_support_points: prefixes after a self search of the same tensors inside knn_grid_reuse, the search
    otherwise (other tensors, no block, kr beyond the rows)"""
    from amcontrast3d_amd import ops
    x = torch.from_numpy(cloud).to(dev)
    o = torch.tensor([len(cloud)], dtype=torch.int32, device=dev)
    y = x[::4].contiguous()
    qo = torch.tensor([y.shape[0]], dtype=torch.int32, device=dev)
    calls = []
    real = ops.knn_prefix
    monkeypatch.setattr(ops, "knn_prefix", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    want4, want64 = ops.knnquery_squared(4, x, y, o, qo)[0], ops.knnquery_squared(64, x, y, o, qo)[0]
    assert torch.equal(ops.knn_of_support_points(4, x, y, o, qo), want4) and calls == []  # no block
    with ops.knn_grid_reuse():
        assert torch.equal(ops.knn_of_support_points(4, x, y, o, qo), want4) and calls == []  # no self search yet
        ops.knnquery_squared(K0, x, x, o, o)
        assert torch.equal(ops.knn_of_support_points(4, x, y, o, qo), want4) and calls == [4]
        assert torch.equal(ops.knn_of_support_points(64, x, y, o, qo), want64) and calls == [4]  # more than the rows hold
        assert torch.equal(ops.knn_of_support_points(4, x.clone(), y, o, qo), want4) and calls == [4]  # another tensor
