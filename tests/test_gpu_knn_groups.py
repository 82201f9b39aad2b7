"""The grid k-NN search with several queries per wavefront (`kg_query_group_kernel`, nsample <= 32) against the
oracle's restatement of the reference's heap: indices AND squared distances to the bit, at the smallest shapes that
still take the grid path (n * m >= 2^22, n >= 256).

A query with equal distances among its k+1 nearest is handed to the heap replay, which would also be right if the new
kernel were wrong.  So for the `uniform` and `room` clouds the test first asserts, in numpy on the oracle's own k+1
distances, that NO query has such a tie: there every compared list is the group kernel's own.  `lattice` (every query
tied) and `dup` (coincident points) cover the two tie flags and the hand-over instead.  (Random float32 clouds do tie
now and then -- one query in 2049 with some seeds -- so the seeds below are ones for which the share is exactly 0.)"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_ops import clouds

pytestmark = pytest.mark.gpu

KINDS = ["uniform", "room", "lattice", "dup"]
UNTIED = ("uniform", "room")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    assert lib.amc3d_knnquery_uses_grid(2048, 32, 2048, 1) == 1 and lib.amc3d_knnquery_uses_grid(700, 16, 6000, 3) == 1
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def cloud(seed, n, kind):
    t = torch.from_numpy(np.ascontiguousarray(clouds(seed, 1, n, kind)[0]))
    return t


def oracle(k, xyz, q, off, qoff):
    from oracle import pointops_ref as K
    m = q.shape[0]
    iw = torch.zeros(m, k, dtype=torch.int32)
    dw = torch.zeros(m, k)
    K.knnquery_cuda(m, k, xyz, q, off, qoff, iw, dw)
    return iw.numpy(), dw.numpy()


def tie_share(k, xyz, q, off, qoff):
    """share of the queries with two equal distances among their k+1 nearest (placeholders of a segment with fewer
    points do not count), from the reference's own distance expression"""
    _, d = oracle(k + 1, xyz, q, off, qoff)
    real = d[:, 1:] < 1e10
    return float(((d[:, 1:] == d[:, :-1]) & real).any(axis=1).mean())


def check(dev, k, xyz, q, off, qoff, kind):
    from amcontrast3d_amd import compat
    same = q is xyz
    off_t, qoff_t = torch.tensor(off, dtype=torch.int32), torch.tensor(qoff, dtype=torch.int32)
    if kind in UNTIED:
        assert tie_share(k, xyz, q, off_t, qoff_t) == 0.0
    iw, dw = oracle(k, xyz, q, off_t, qoff_t)
    m = q.shape[0]
    gx = xyz.to(dev)
    gq = gx if same else q.to(dev)          # the same tensors: the kernel's self-search order
    go = off_t.to(dev)
    gqo = go if same else qoff_t.to(dev)
    ig = torch.full((m, k), -7, dtype=torch.int32, device=dev)
    dg = torch.full((m, k), -7.0, device=dev)
    compat.knnquery_cuda(m, k, gx, gq, go, gqo, ig, dg)
    np.testing.assert_array_equal(dg.cpu().numpy(), dw)
    np.testing.assert_array_equal(ig.cpu().numpy(), iw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 4, 16, 25, 32])
@pytest.mark.parametrize("n", [2048, 2049])
def test_self_search(dev, n, k, kind):
    """2049: the last wavefront holds one query, its other group must store nothing"""
    xyz = cloud(9, n, kind)
    check(dev, k, xyz, xyz, [n], [n], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [33, 64])
def test_wave_per_query_kernel_above_32(dev, k, kind):
    xyz = cloud(15, 2048, kind)
    check(dev, k, xyz, xyz, [2048], [2048], kind)


@pytest.mark.parametrize("kind", KINDS)
def test_queries_apart_from_support(dev, kind):
    check(dev, 16, cloud(9, 6000, kind), cloud(10, 700, kind), [6000], [700], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,off", [(25, [1300, 2049]), (25, [700, 710, 2049]), (16, [10, 1033, 2049])])
def test_ragged_segments_self(dev, k, off, kind):
    """a segment of 10 points with k = 25 (and k = 16): placeholders (1e10, segment start) fill the tail"""
    xyz = cloud(15, 2049, kind)
    check(dev, k, xyz, xyz, off, off, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,off,qoff", [(25, [2500, 6000], [1, 700]), (25, [2500, 2510, 6000], [300, 305, 700])])
def test_ragged_segments_apart(dev, k, off, qoff, kind):
    check(dev, k, cloud(9, 6000, kind), cloud(10, 700, kind), off, qoff, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_grid_reuse_k25_then_4_then_16(dev, kind):
    """the loss's pattern: the self search builds the grid (cell edge calibrated for k = 25), the votes' searches at
    k = 4 and k = 16 reuse it"""
    from amcontrast3d_amd import ops
    n = 8192
    xyz = cloud(12, n, kind)
    gx = xyz.to(dev)
    go = torch.tensor([n], dtype=torch.int32, device=dev)
    calls = [(25, xyz, gx, go), (4, xyz[::4].contiguous(), None, None), (16, xyz[::16].contiguous(), None, None)]
    got = []
    with ops.knn_grid_reuse():
        for k, q, gq, gqo in calls:
            if gq is None:
                gq = q.to(dev)
                gqo = torch.tensor([q.shape[0]], dtype=torch.int32, device=dev)
            idx, d2 = ops.knnquery_squared(k, gx, gq, go, gqo)
            got.append((idx.cpu().numpy(), d2.cpu().numpy()))
    off = torch.tensor([n], dtype=torch.int32)
    for (k, q, _, _), (idx, d2) in zip(calls, got):
        qoff = torch.tensor([q.shape[0]], dtype=torch.int32)
        if kind in UNTIED:
            assert tie_share(k, xyz, q, off, qoff) == 0.0
        iw, dw = oracle(k, xyz, q, off, qoff)
        np.testing.assert_array_equal(d2, dw)
        np.testing.assert_array_equal(idx, iw)
