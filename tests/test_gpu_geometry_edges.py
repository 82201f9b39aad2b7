"""The geometry searches -- k-NN, ball query and 3-NN on the calibrated cell grid of csrc/knn.hip, FPS with its Morton sort and
box pruning -- against the oracle's C restatement of the reference's brute-force scans, to the bit, on the clouds of
geometry_clouds.py: far from the origin, planar, collinear, coincident, two distant clusters, a cloud with five remote
rows, and queries outside the support's box.  They reach what the clouds of test_gpu_ops.py cannot: the fallback cell
size h = emax, the cell-budget loop, grids one cell thin, shell expansion over many empty rings, the stopping margin
against the coordinate quantum at |x| ~ 1000-2000, clamped query cells, and fps_kernel_large.

Every case asserts the route it is about (amc3d_knnquery_uses_grid, amc3d_grid_search_pays, the n brackets of
amc3d_furthest_point_sampling).  That no query of an untied k-NN case has equal distances among its k+1 nearest -- such a
query goes to the heap replay, which would hide a wrong grid kernel -- is asserted on the CPU by
test_geometry_clouds_host.py over the same `knn_cases()`.

Largest shell radius R a `for (int R = 1;; ++R)` loop can need: `whole` ends it once the block covers the grid, i.e. at
R <= max(nx, ny, nz) - 1, and the cell budget caps the grid at max(8 n, 4096) cells.  `point`: one cell, R = 1.  Self
searches on `line` and the planes: a few hundred cells along an axis but even density, the stopping rule ends at R <= 3.
`outlier` / `clusters`: the budget loop leaves cbrt(8 n) cells per axis (25 at n = 2048, 36 at 6000, 40 at 8192; 16 for the
3-NN grids over 256 points), which bounds R for the rows that cross the gap.  Outside queries over small cells (the mixed
k-NN case, 3-NN at (1, 2304, 2048)) cross up to 1.75 units: ~20 rings in 3-D, ~60 over a plane, and over `line` -- 2 units
from every outside query -- until the block is the whole grid, a few hundred cheap rings of one row each."""
import functools

import numpy as np
import pytest
import torch

import geometry_clouds as G

pytestmark = pytest.mark.gpu

CASES = G.knn_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from amcontrast3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def lib():
    from amcontrast3d_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------- k-NN
@functools.lru_cache(maxsize=None)
def knn_oracle(name):
    from oracle import pointops_ref as K
    c = CASES[name]
    q = c.queries
    m = q.shape[0]
    iw = torch.zeros(m, c.k, dtype=torch.int32)
    dw = torch.zeros(m, c.k)
    K.knnquery_cuda(m, c.k, torch.from_numpy(c.xyz), torch.from_numpy(q), torch.tensor(c.off, dtype=torch.int32),
                    torch.tensor(c.qoff, dtype=torch.int32), iw, dw)
    return iw.numpy(), dw.numpy()


def knn_check(dev, name):
    from amcontrast3d_amd import compat
    c = CASES[name]
    m, n = c.queries.shape[0], c.xyz.shape[0]
    assert lib().amc3d_knnquery_uses_grid(m, c.k, n, len(c.off)) == (1 if c.grid else 0)
    iw, dw = knn_oracle(name)
    gx = torch.from_numpy(c.xyz).to(dev)
    go = torch.tensor(c.off, dtype=torch.int32, device=dev)
    same = c.q is None
    gq = gx if same else torch.from_numpy(c.q).to(dev)  # the same tensors: the kernel's self-search order
    gqo = go if same else torch.tensor(c.qoff, dtype=torch.int32, device=dev)
    ig = torch.full((m, c.k), -7, dtype=torch.int32, device=dev)
    dg = torch.full((m, c.k), -7.0, device=dev)
    compat.knnquery_cuda(m, c.k, gx, gq, go, gqo, ig, dg)
    np.testing.assert_array_equal(dg.cpu().numpy(), dw)
    np.testing.assert_array_equal(ig.cpu().numpy(), iw)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("k", G.SELF_K_GROUP)
@pytest.mark.parametrize("n", G.SELF_N)
def test_knn_self_group_kernel(dev, n, k, kind):
    knn_check(dev, f"self-{kind}-{n}-{k}")


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("n", G.SELF_N)
def test_knn_self_wave_per_query_kernel(dev, n, kind):
    knn_check(dev, f"self-{kind}-{n}-{G.SELF_K_WAVE}")


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("n", G.SELF_N)
def test_knn_self_heap_k100(dev, n, kind):
    """k > 64: the all-pairs heap, no grid (asserted in knn_check)"""
    knn_check(dev, f"self-{kind}-{n}-{G.SELF_K_HEAP}")


@pytest.mark.parametrize("kind", G.APART_KINDS)
def test_knn_queries_outside_the_support_box(dev, kind):
    """about 7/8 of the 700 queries lie outside the box of the 6000 support points: their cells are clamped"""
    knn_check(dev, f"apart-{kind}")


@pytest.mark.parametrize("kind", G.APART_KINDS)
def test_knn_support_rows_and_outside_queries_mixed(dev, kind):
    """cells as small as a self search's, and 100 queries that cross many empty rings from a clamped cell"""
    knn_check(dev, f"mixed-{kind}")


@pytest.mark.parametrize("first", [300, 10])
def test_knn_ragged_with_a_coincident_segment(dev, first):
    c = CASES[f"ragged-{first}"]
    knn_check(dev, c.name)
    iw, dw = knn_oracle(c.name)
    if first < c.k:  # the oracle's rows of the short segment end in placeholders: the case is what it claims to be
        assert (dw[:first, first:] == np.float32(1e10)).all() and (iw[:first, first:] == 0).all()


@pytest.mark.parametrize("kind", G.REUSE_KINDS)
def test_knn_grid_reuse_k25_then_4_then_16(dev, kind):
    from amcontrast3d_amd import ops
    cases = G.reuse_cases(kind)
    n = cases[0].xyz.shape[0]
    gx = torch.from_numpy(cases[0].xyz).to(dev)
    go = torch.tensor([n], dtype=torch.int32, device=dev)
    got = []
    with ops.knn_grid_reuse():
        for c in cases:
            m = c.queries.shape[0]
            assert lib().amc3d_knnquery_uses_grid(m, c.k, n, 1) == 1
            gq, gqo = (gx, go) if c.q is None else (torch.from_numpy(c.q).to(dev),
                                                    torch.tensor([m], dtype=torch.int32, device=dev))
            idx, d2 = ops.knnquery_squared(c.k, gx, gq, go, gqo)
            got.append((idx.cpu().numpy(), d2.cpu().numpy()))
    for c, (idx, d2) in zip(cases, got):
        iw, dw = knn_oracle(c.name)
        np.testing.assert_array_equal(d2, dw)
        np.testing.assert_array_equal(idx, iw)


# ------------------------------------------------------------------------------------------------------- ball query
BALL_SHAPES = [(1, 2048, 1024, True), (2, 2048, 1024, True), (2, 1000, 250, False)]  # B, N, M, grid route
BALL_NSAMPLE = (1, 32, 64)


def ball_radii(kind):
    """most queries get between 1 and nsample hits; everything in range (except across the gap of `clusters`); nothing
    but coincident points"""
    return (0.002 if kind == "clusters" else 0.25, 10.0, 1e-6)


@functools.lru_cache(maxsize=None)
def ball_inputs(kind, B, N, M, outside):
    xyz = np.stack([G.cloud(kind, 11 + b, N) for b in range(B)])
    if outside:
        q = np.stack([G.outside_queries(31 + b, M, G.offset_of(kind)) for b in range(B)])
    else:
        pick = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:M].numpy()
        q = np.ascontiguousarray(xyz[:, pick])
    return torch.from_numpy(xyz), torch.from_numpy(q)


@pytest.mark.parametrize("outside", [False, True], ids=["subset", "outside"])
@pytest.mark.parametrize("B,N,M,grid", BALL_SHAPES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_ball_query(dev, kind, B, N, M, grid, outside):
    from amcontrast3d_amd import ops
    from oracle import pointops_ref as K
    assert lib().amc3d_grid_search_pays(B, N, M) == (1 if grid else 0)
    assert int(lib().amc3d_grid_search_workspace_bytes(B, N, M)) > 0
    xyz, q = ball_inputs(kind, B, N, M, outside)
    gx, gq = xyz.to(dev), q.to(dev)
    for r in ball_radii(kind):
        for ns in BALL_NSAMPLE:  # all <= 64: none leaves the grid route
            want = K.ball_query(r, ns, xyz, q).numpy()
            got = ops.ball_query(r, ns, gx, gq).cpu().numpy()
            np.testing.assert_array_equal(got, want, err_msg=f"radius {r} nsample {ns}")
            if kind == "point" and not outside:  # every query hits all N points
                assert (got == np.arange(ns, dtype=np.int32)).all()


# ------------------------------------------------------------------------------------------------------------ 3-NN
# B, n unknown, m known, grid route.  In the first two shapes most unknown points are outside rows, so the cell size --
# calibrated on 64 sampled queries -- comes out as wide as the cloud; in (1, 2304, 2048) eight of nine unknown points are
# known ones, the cells are as small as the known points' spacing, and the 256 outside rows expand ring by ring from a
# clamped cell (for `point` the sampled distance is 0: h = emax, and the outside rows' cell coordinate saturates)
NN3_SHAPES = [(1, 8192, 256, True), (2, 2048, 1024, True), (1, 2304, 2048, True), (1, 517, 3, False)]


def nn3_check(dev, B, n, m, grid, known, unknown):
    from amcontrast3d_amd import compat
    from oracle import pointops_ref as K
    assert lib().amc3d_grid_search_pays(B, m, n) == (1 if grid else 0)  # the support is `known`
    unknown, known = torch.from_numpy(unknown), torch.from_numpy(known)
    d2w = torch.empty(B, n, 3)
    iw = torch.empty(B, n, 3, dtype=torch.int32)
    K.three_nn_wrapper(B, n, m, unknown, known, d2w, iw)
    d2g = torch.full((B, n, 3), -7.0, device=dev)
    ig = torch.full((B, n, 3), -7, dtype=torch.int32, device=dev)
    compat.three_nn_wrapper(B, n, m, unknown.to(dev), known.to(dev), d2g, ig)
    np.testing.assert_array_equal(ig.cpu().numpy(), iw.numpy())
    np.testing.assert_array_equal(d2g.cpu().numpy(), d2w.numpy())  # squared distances: bit-exact (inf included)
    return d2w.numpy()


@pytest.mark.parametrize("B,n,m,grid", NN3_SHAPES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_three_nn_superset_queries(dev, kind, B, n, m, grid):
    """FeaturePropagation: the unknown points are the known ones plus points outside their box"""
    known = np.stack([G.cloud(kind, 4 + b, m) for b in range(B)])
    unknown = np.stack([G.superset_queries(known[b], 41 + b, n, G.offset_of(kind)) for b in range(B)])
    nn3_check(dev, B, n, m, grid, known, unknown)


@pytest.mark.parametrize("rows", [4, 3, 2])
def test_three_nn_reaches_across_the_gap(dev, rows):
    """4, 3 and 2 remote rows among 256 known points: the queries at those rows find 3, 2 or 1 neighbour besides
    themselves nearby and must cross ~48 units of empty cells for the rest"""
    B, n, m = 1, 8192, 256
    known = G.cloud("outlier", 4, m, outlier_rows=rows)[None]
    unknown = G.superset_queries(known[0], 41, n)[None]
    d2 = nn3_check(dev, B, n, m, True, known, unknown)
    far_rows = d2[0, m - rows:m]
    assert (far_rows[:, :min(rows, 3)] < 1.0).all()
    if rows < 3:
        assert (far_rows[:, rows:] > 48.0 ** 2).all()  # the third neighbour is in the main cloud


# -------------------------------------------------------------------------------------------------------------- FPS
# one n per launch of amc3d_furthest_point_sampling (csrc/fps.hip): fps_kernel<1,1> n <= 64, <2,1> <= 512, <3,1> <= 1536,
# <6,3> <= 3072, <12,3> <= 6144, <24,3> <= 12288, <48,6> <= 24576 (13000 and the bracket's last size); fps_kernel_l2 up to
# FPS_L2_MAX = 262144 (its first and last size); fps_kernel_large above
FPS_REGISTER_N = (64, 300, 600, 1600, 3100, 7000, 13000, 24576)
FPS_L2_N = (24577, 262144)
FPS_LARGE_N = 262145
FPS_KINDS = ("far", "plane_x", "line", "point", "clusters")


def fps_check(dev, xyz, m):
    from amcontrast3d_amd import ops
    from oracle import pointops_ref as K
    xyz = torch.from_numpy(xyz)
    want = K.furthest_point_sample(xyz, m)
    got = ops.furthest_point_sample(xyz.to(dev), m)
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    return want.numpy()


@pytest.mark.parametrize("kind", FPS_KINDS)
@pytest.mark.parametrize("n", FPS_REGISTER_N + FPS_L2_N[:1])
def test_fps_degenerate_clouds(dev, n, kind):
    """`point`: every iteration is a total tie (the slow path all the way, every pick is index 0); `clusters` ties
    nothing but leaves all Morton cells but two empty; `plane_x` / `line` have axes of zero extent"""
    want = fps_check(dev, G.cloud(kind, 5, n)[None], min(n, 96))
    if kind == "point":
        assert (want == 0).all()


@pytest.mark.parametrize("n", [FPS_L2_N[1], FPS_LARGE_N])
def test_fps_last_l2_size_and_large_kernel(dev, n):
    """262144 = FPS_L2_MAX is fps_kernel_l2's last size, 262145 the first of fps_kernel_large"""
    assert FPS_L2_N[1] == 16 * 32 * 512 and FPS_LARGE_N == FPS_L2_N[1] + 1
    fps_check(dev, G.cloud("far", 5, n)[None], 16)


def test_fps_batch_of_mixed_kinds(dev):
    fps_check(dev, np.stack([G.cloud(kind, 5, 3100) for kind in ("far", "point", "plane_x")]), 96)
