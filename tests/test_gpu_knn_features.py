"""ops.knn_features (csrc/knn_feat.hip: fp32-MFMA distance tiles, selection on chip) against the fp64 restatement of
knn_features_ref.py.

Lattice inputs (integers in [-3, 3]): every product, sum and root is exact in fp32 and ties abound, so the indices must equal
the stable sort on (d2, index) for every query and the distances its roots to the last bit.

Gaussian inputs: the kernel's d2 carries fp32 rounding, bounded by the derived band tol_ij = 2 (C + 3) 2^-24 (|q_i|^2 +
|s_j|^2) (knn_features_ref.band).  A search that orders by computed distances can only confuse two points whose exact
distances lie within the sum of their two bands; that is what is asserted, for every query.  Queries whose exact first k + 1
distances are pairwise more than two bands apart must return the exact list, and at least 85 % of the queries are of that
kind.

Shapes: N = 300 (four full support tiles of 64 and one of 44), M = 77 (three wavefronts of 32 queries, the last with 13),
C from below one MFMA k-step (1) over odd tails (3, 5, 33) to several 32-channel chunks (64, 130), k up to the list's 100
(the second 64 entries of a lane's list), M = 300 for more than one workgroup per cloud."""
import functools

import numpy as np
import pytest
import torch

import knn_features_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def ops():
    from amcontrast3d_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def lattice(C, N, M, seed=5):
    g = torch.Generator().manual_seed(seed + C)
    sup = torch.randint(-3, 4, (2, N, C), generator=g).float()
    qry = torch.randint(-3, 4, (2, M, C), generator=g).float()
    return sup, qry


@functools.lru_cache(maxsize=None)
def gaussian(C, N, M, seed=11):
    g = torch.Generator().manual_seed(seed + C)
    return torch.randn(2, N, C, generator=g), torch.randn(2, M, C, generator=g)


@functools.lru_cache(maxsize=None)
def exact(kind, C, N, M, k, farthest):
    sup, qry = (lattice if kind == "lattice" else gaussian)(C, N, M)
    return R.exact_lists(qry, sup, k, farthest)


def ieee_root(d2):
    """the correctly rounded fp32 root of exact fp32 values (np.sqrt; torch.sqrt on the CPU is 1 ulp off now and then)"""
    return torch.from_numpy(np.sqrt(d2.float().numpy()))


def search(dev, k, sup, qry=None, **kw):
    gs = sup.to(dev)
    gq = None if qry is None else qry.to(dev)
    dist, idx = ops().knn_features(k, gs, gq, dist="bmk", **kw)
    torch.cuda.synchronize()
    return dist.cpu(), idx.cpu().long()


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("k", [1, 9, 100])
@pytest.mark.parametrize("C", [2, 16])
def test_lattice_lists_equal_the_stable_sort(dev, C, k, farthest):
    sup, qry = lattice(C, 300, 77)
    want_idx, want_d2, _ = exact("lattice", C, 300, 77, k, farthest)
    dist, idx = search(dev, k, sup, qry, farthest=farthest)
    assert torch.equal(idx, want_idx)
    assert torch.equal(dist, ieee_root(want_d2))


@pytest.mark.parametrize("farthest", [False, True])
def test_lattice_self_search_with_duplicated_rows(dev, farthest):
    sup = lattice(16, 300, 77)[0].clone()
    sup[:, 150:] = sup[:, :150]  # every row twice: the pair (0, own index) and (0, the twin) are told apart by index alone
    want_idx, want_d2, _ = R.exact_lists(sup, sup, 9, farthest)
    dist, idx = search(dev, 9, sup, None, farthest=farthest)
    assert torch.equal(idx, want_idx)
    assert torch.equal(dist, ieee_root(want_d2))
    if not farthest:
        assert torch.equal(idx[:, :150, 0], torch.arange(150).expand(2, -1)) and bool((dist[:, :, :2] == 0).all())


GAUSS = ([(C, 77, 9, False) for C in (1, 3, 5, 16, 33, 64, 130)]
         + [(16, 77, 100, False), (16, 300, 40, False), (5, 77, 9, True), (64, 77, 9, True)])


@pytest.mark.parametrize("C,M,k,farthest", GAUSS)
def test_gaussian_lists_within_the_rounding_band(dev, C, M, k, farthest):
    N = 300
    sup, qry = gaussian(C, N, M)
    want_idx, want_d2, d2 = exact("gaussian", C, N, M, k, farthest)
    tol = R.band(qry, sup)
    dist, idx = search(dev, k, sup, qry, farthest=farthest)
    sign = -1.0 if farthest else 1.0

    got_d2 = torch.gather(d2, -1, idx)          # exact distances of the returned points
    got_tol = torch.gather(tol, -1, idx)
    reported = dist.double() ** 2
    err = ((reported - got_d2).abs() / got_tol).max()
    print(f"C={C} k={k} farthest={farthest}: reported d2 off by at most {float(err):.3f} of the band")
    assert bool(((reported - got_d2).abs() <= got_tol).all())

    # a returned point j and a point x of the exact list that it displaced satisfy d2(j) - tol_j <= d2(x) + tol_x
    kth = want_d2[..., -1:]
    tol_list = torch.gather(tol, -1, want_idx).amax(-1, keepdim=True)
    assert bool((sign * (got_d2 - kth) <= got_tol + tol_list).all())
    # a missing point j was displaced by a returned point y outside the exact list: d2(y) - tol_y <= d2(j) + tol_j
    tol_ret = got_tol.amax(-1, keepdim=True)
    present = torch.zeros_like(d2, dtype=torch.bool).scatter_(-1, idx, True)
    must = sign * (d2 - kth) < -(tol + tol_ret)
    assert bool((present | ~must).all())
    assert bool((idx.sort(-1).values.diff(dim=-1) > 0).all()) if k > 1 else True  # no point twice

    # the reported order: distances never decrease (farthest: never increase)
    assert bool((sign * dist.diff(dim=-1) >= 0).all()) if k > 1 else True

    # well-separated queries: the exact first k + 1 distances pairwise more than two bands apart -> the exact list
    kk = min(k + 1, N)
    first_idx, first_d2, _ = exact("gaussian", C, N, M, kk, farthest)
    first_tol = torch.gather(tol, -1, first_idx)
    gaps = sign * first_d2.diff(dim=-1)
    clear = (gaps > 2 * torch.maximum(first_tol[..., 1:], first_tol[..., :-1])).all(-1) if kk > 1 else torch.ones(2, M, dtype=torch.bool)
    share = float(clear.double().mean())
    print(f"well-separated queries: {share:.3f}")
    assert share >= 0.85
    assert torch.equal(idx[clear], want_idx[clear])


def test_every_point_returned_when_k_is_n(dev):
    sup, qry = gaussian(5, 20, 7)
    dist, idx = search(dev, 20, sup, qry)
    assert torch.equal(idx.sort(-1).values, torch.arange(20).expand(2, 7, -1))
    assert torch.equal(idx, exact("gaussian", 5, 20, 7, 20, False)[0])


def test_single_point(dev):
    x = torch.randn(1, 1, 4)
    dist, idx = search(dev, 1, x)
    assert idx.tolist() == [[[0]]] and dist.tolist() == [[[0.0]]]


@pytest.mark.parametrize("B,M", [(1, 77), (2, 1), (1, 1)])
def test_one_cloud_one_query(dev, B, M):
    sup, qry = gaussian(16, 300, 77)
    sup, qry = sup[:B].contiguous(), qry[:B, :M].contiguous()
    full = search(dev, 9, *gaussian(16, 300, 77))
    got = search(dev, 9, sup, qry)
    assert torch.equal(got[1], full[1][:B, :M]) and torch.equal(got[0], full[0][:B, :M])


def test_dilation_picks_every_third_column(dev):
    sup, qry = gaussian(16, 300, 77)
    dist, idx = search(dev, 27, sup, qry)
    ddist, didx = search(dev, 9, sup, qry, dilation=3)
    assert didx.shape == (2, 77, 9)
    for j in range(9):
        assert torch.equal(didx[:, :, j], idx[:, :, 3 * j]) and torch.equal(ddist[:, :, j], dist[:, :, 3 * j])


def test_bkm_distances_are_the_transpose(dev):
    sup, qry = gaussian(16, 300, 77)
    gs, gq = sup.to(dev), qry.to(dev)
    d_bmk, i_bmk = ops().knn_features(9, gs, gq, dist="bmk")
    d_bkm, i_bkm = ops().knn_features(9, gs, gq, dist="bkm")
    assert d_bkm.shape == (2, 9, 77) and torch.equal(d_bkm.transpose(1, 2), d_bmk) and torch.equal(i_bmk, i_bkm)
    assert ops().knn_features(9, gs, gq)[0] is None


@pytest.mark.parametrize("C", [5, 64])
def test_channel_major_reads_in_place(dev, C):
    sup, qry = gaussian(C, 300, 77)
    want = search(dev, 9, sup, qry)
    got = search(dev, 9, sup.transpose(1, 2).contiguous(), qry.transpose(1, 2).contiguous(), channel_major=True)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


def test_self_search_is_the_search_of_a_copy_and_sees_itself_at_zero(dev):
    sup = gaussian(33, 300, 77)[0].to(dev)
    d_self, i_self = ops().knn_features(9, sup, dist="bmk")
    d_same, i_same = ops().knn_features(9, sup, sup, dist="bmk")
    d_copy, i_copy = ops().knn_features(9, sup, sup.clone(), dist="bmk")
    assert torch.equal(i_self, i_copy) and torch.equal(d_self, d_copy) and torch.equal(i_same, i_copy)
    assert torch.equal(i_self[:, :, 0].cpu().long(), torch.arange(300).expand(2, -1))
    assert bool((d_self[:, :, 0] == 0).all())


def test_two_calls_give_the_same_bits(dev):
    sup, qry = gaussian(64, 300, 77)
    a, b = search(dev, 40, sup, qry), search(dev, 40, sup, qry)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bad_arguments_raise(dev):
    sup = gaussian(16, 300, 77)[0]
    gs = sup.to(dev)
    with pytest.raises(RuntimeError, match="k \\* dilation must be in 1..100"):
        ops().knn_features(101, gs)
    with pytest.raises(RuntimeError, match="k \\* dilation must be in 1..100"):
        ops().knn_features(0, gs)
    with pytest.raises(RuntimeError, match="k \\* dilation must be in 1..100"):
        ops().knn_features(26, gs, dilation=4)
    with pytest.raises(RuntimeError, match="out of range for 20 support points"):
        ops().knn_features(21, gs[:, :20].contiguous())
    with pytest.raises(RuntimeError, match="expected \\(B,N,C\\)"):
        ops().knn_features(3, gs, gs[:, :, :5].contiguous())
    with pytest.raises(ValueError):
        ops().knn_features(3, gs, dist="kbm")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops().knn_features(3, sup)


def test_workspace_does_not_grow_with_the_support(dev):
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    small = lib.amc3d_knn_features_workspace_bytes(8, 1000, 1000, 64, 20)
    assert small > 0 and small == lib.amc3d_knn_features_workspace_bytes(8, 100000, 1000, 64, 20)
    assert lib.amc3d_knn_features_workspace_bytes(8, 1 << 29, 1000, 64, 20) == 0
