"""ops.knn_batch (amc3d_knn_batch: the grid search of amc3d_knnquery over uniform segments + one epilogue kernel) against
the oracle's restatement of the reference's pointops k-NN, made cloud-local: indices to the bit, tie order included,
at the smallest shapes at which each path can go wrong --

  2 x 2048 self-search      the grid path, two queries per wavefront up to 32 columns, a wavefront per query above
  2 x 2049                  the last wavefront holds one query
  2 x 6000 / 700            queries apart from the support
  2 x 300 / 77, 64 / 7      the all-pairs heap kernel; the epilogue's last workgroup is partly filled
  m = 1, k = n = 64

For `uniform` and `room` the test first asserts on the oracle's own k+1 distances that no query is tied (the rule of
test_gpu_knn_groups.py), so every compared list is the search kernel's own; `lattice` and `dup` cover the ties.  The
euclidean distances are the IEEE root of the oracle's squared ones: within 1 ulp of np.sqrt, equality expected."""
import functools

import numpy as np
import pytest
import torch

import knn_group_ref as R
from test_gpu_ops import clouds

pytestmark = pytest.mark.gpu

KINDS = ["uniform", "room", "lattice", "dup"]
UNTIED = ("uniform", "room")
# untied kinds: seeds without two equal distances among the 97 nearest of any query, at every shape below (room: seeds 1-11
# each have a tied query at 2 x 2048 or 6000 / 700)
SEEDS = {"uniform": 1, "room": 12, "lattice": 9, "dup": 9}
SHAPES = [(2048, None), (2049, None), (6000, 700), (300, 77), (64, 7), (300, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    assert lib.amc3d_knnquery_uses_grid(2 * 2048, 32, 2 * 2048, 2) == 1 and lib.amc3d_knnquery_uses_grid(2 * 700, 36, 2 * 6000, 2) == 1
    assert lib.amc3d_knnquery_uses_grid(2 * 77, 9, 2 * 300, 2) == 0 and lib.amc3d_knnquery_uses_grid(2 * 2048, 96, 2 * 2048, 2) == 0
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def pair(kind, n, m):
    """(support, queries) on the CPU; m None: the self-search, one tensor"""
    sup = torch.from_numpy(np.ascontiguousarray(clouds(SEEDS[kind], 2, n, kind)))
    return sup, (sup if m is None else torch.from_numpy(np.ascontiguousarray(clouds(SEEDS[kind] + 1, 2, m, kind))))


@functools.lru_cache(maxsize=None)
def oracle(kind, n, m, columns):
    sup, qry = pair(kind, n, m)
    if kind in UNTIED:
        assert bool(R.oracle_untied(columns, qry, sup).all()), "choose another seed: a query is tied"
    return R.oracle_knn(columns, qry, sup)


def on_gpu(dev, kind, n, m):
    sup, qry = pair(kind, n, m)
    gs = sup.to(dev)
    return gs, (gs if qry is sup else qry.to(dev))  # the self-search is called with one tensor for both arguments


def check(dev, kind, n, m, k, dilation=1):
    from amcontrast3d_amd import ops
    want_idx, want_d2 = oracle(kind, n, m, k * dilation)
    want_idx, want_d = want_idx[..., ::dilation].numpy(), np.sqrt(want_d2[..., ::dilation].numpy())
    gs, gq = on_gpu(dev, kind, n, m)
    none, idx = ops.knn_batch(k, gs, gq, dilation=dilation)
    assert none is None and idx.dtype == torch.int32 and idx.shape == want_idx.shape
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    d_bmk, idx1 = ops.knn_batch(k, gs, gq, dilation=dilation, dist="bmk")
    d_bkm, idx2 = ops.knn_batch(k, gs, gq, dilation=dilation, dist="bkm")
    assert torch.equal(idx1, idx) and torch.equal(idx2, idx)
    assert d_bmk.shape == want_d.shape and d_bkm.shape == (want_d.shape[0], want_d.shape[2], want_d.shape[1])
    assert torch.equal(d_bkm, d_bmk.transpose(1, 2))
    ulp = R.ulp_diff(d_bmk.cpu().numpy(), want_d)
    print(f"largest distance difference: {ulp} ulp")
    assert ulp <= 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 9, 16, 32])
@pytest.mark.parametrize("n,m", SHAPES)
def test_indices_and_distances(dev, n, m, k, kind):
    check(dev, kind, n, m, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,dilation", [(9, 2), (9, 4), (16, 6)])
@pytest.mark.parametrize("n,m", [(2048, None), (6000, 700), (300, 77)])
def test_dilated_columns(dev, n, m, k, dilation, kind):
    """36 columns and above: the wavefront-per-query kernel; 96: above the grid's 64, the heap kernel"""
    check(dev, kind, n, m, k, dilation)


@pytest.mark.parametrize("kind", KINDS)
def test_k_equals_n(dev, kind):
    check(dev, kind, 64, 7, 64)
    check(dev, kind, 64, None, 64)


def test_k_above_n_raises_on_both_routes(dev):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import ops
    from openpoints.models.layers import KNN
    gs, gq = on_gpu(dev, "uniform", 64, 7)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.knn_batch(65, gs, gq)
    with pytest.raises(RuntimeError, match="out of range"):
        KNN(65)(gq, gs)
    with pytest.raises(RuntimeError, match="out of range"):
        KNN(65)(gq.cpu(), gs.cpu())
    with pytest.raises(RuntimeError):
        ops.knn_batch(9, gs.cpu(), gq.cpu())  # the operator itself has no CPU route


def test_same_bits_twice_and_in_deterministic_mode(dev):
    from amcontrast3d_amd import ops
    gs, gq = on_gpu(dev, "room", 6000, 700)
    first = ops.knn_batch(9, gs, gq, dilation=4, dist="bkm")
    idx = first[1]
    dp = ops.knn_group_dp(idx, gq, gs, True, True)
    with ops.deterministic_mode():
        again = ops.knn_batch(9, gs, gq, dilation=4, dist="bkm")
        dp2 = ops.knn_group_dp(idx, gq, gs, True, True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and torch.equal(dp, dp2)
    third = ops.knn_batch(9, gs, gq, dilation=4, dist="bkm")
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])
    assert torch.equal(dp, ops.knn_group_dp(idx, gq, gs, True, True))


@pytest.mark.parametrize("n,m", [(2048, None), (300, 77)])
def test_replays_from_a_graph(dev, n, m):
    """new coordinates copied into the static inputs: the replay searches those"""
    from amcontrast3d_amd import ops
    sup_a, qry_a = pair("uniform", n, m)
    sup_b, qry_b = pair("room", n, m)
    gs = sup_a.to(dev).clone()
    gq = gs if m is None else qry_a.to(dev).clone()

    def step():
        d, idx = ops.knn_batch(16, gs, gq, dist="bkm")
        return d, idx, ops.knn_group_dp(idx, gq, gs, True, True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d, idx, dp = step()
    for sup, qry, kind in ((sup_b, qry_b, "room"), (sup_a, qry_a, "uniform")):
        gs.copy_(sup)
        if m is not None:
            gq.copy_(qry)
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_d2 = oracle(kind, n, m, 16)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_idx.numpy())
        assert R.ulp_diff(d.cpu().numpy(), np.sqrt(want_d2.numpy()).transpose(0, 2, 1)) <= 1
        want_dp, _ = R.knn_group_forward(want_idx, qry, sup, None, True, True)
        assert R.ulp_diff(dp.cpu().numpy(), want_dp.numpy()) <= 2


def test_grid_reuse_gives_the_same_lists(dev):
    from amcontrast3d_amd import ops
    gs, _ = on_gpu(dev, "room", 2048, None)
    sup, _ = pair("room", 2048, None)
    with ops.knn_grid_reuse():
        a = ops.knn_batch(16, gs)[1]
        b = ops.knn_batch(9, gs, dilation=4)[1]  # reuses the grid of the search above
        c = ops.knn_batch(16, gs, gs.clone())[1]  # equal coordinates in another tensor: not the self-search
    np.testing.assert_array_equal(a.cpu().numpy(), oracle("room", 2048, None, 16)[0].numpy())
    np.testing.assert_array_equal(b.cpu().numpy(), oracle("room", 2048, None, 36)[0][..., ::4].numpy())
    np.testing.assert_array_equal(c.cpu().numpy(), R.oracle_knn(16, sup.clone(), sup)[0].numpy())


def _capped(got, cpu, exact):
    """the index comparison of test_knn_group_host.py: only queries whose CPU list is the exact one, at most 1 % left out"""
    ok = (cpu.long() == exact).all(-1)
    assert 1.0 - float(ok.float().mean()) <= 0.01
    np.testing.assert_array_equal(got.cpu().long()[ok].numpy(), cpu.long()[ok].numpy())


def test_other_inputs_take_the_composition(dev, monkeypatch):
    """k * dilation = 120, farthest=True and width-5 inputs: cdist + topk on the device, equal to the CPU route"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import ops
    from openpoints.models.layers import knn, group
    monkeypatch.setattr(ops, "knn_batch", lambda *a, **k: pytest.fail("the kernel route was taken"))
    sup, qry = pair("uniform", 300, 77)
    gs, gq = sup.to(dev), qry.to(dev)
    for mod in (knn, group):
        _capped(mod.DilatedKNN(20, 6)(gs), mod.DilatedKNN(20, 6)(sup), R.exact_knn(120, sup, sup)[0][..., ::6])
    v, i = knn.KNN(9, farthest=True)(gq, gs)
    cv, ci = knn.KNN(9, farthest=True)(qry, sup)
    far = torch.sort(((qry.double()[:, :, None] - sup.double()[:, None]) ** 2).sum(-1), dim=2, descending=True, stable=True).indices[..., :9]
    _capped(i, ci, far)
    np.testing.assert_allclose(v.cpu().numpy(), cv.numpy(), rtol=0, atol=1e-5)
    g = torch.Generator().manual_seed(4)
    s5, q5 = torch.rand(2, 300, 5, generator=g), torch.rand(2, 77, 5, generator=g)
    _capped(knn.knn_point(9, q5.to(dev), s5.to(dev))[1], knn.knn_point(9, q5, s5)[1], R.exact_knn(9, q5, s5)[0])
    _capped(group.KNN(9)(s5.to(dev), q5.to(dev))[1], group.KNN(9)(s5, q5)[1], R.exact_knn(9, q5, s5)[0])
    _capped(knn.KNN(9)(gq.double(), gs.double())[1], knn.KNN(9)(qry.double(), sup.double())[1], R.exact_knn(9, qry, sup)[0])


def test_modules_take_the_kernel_route(dev):
    """shapes, dtypes and layouts of the modules on the device, against the oracle"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import timing
    from openpoints.models.layers import knn, group
    gs, gq = on_gpu(dev, "uniform", 300, 77)
    want_idx, want_d2 = oracle("uniform", 300, 77, 9)
    want_d = np.sqrt(want_d2.numpy())
    with timing.count_calls() as calls:
        v, i = knn.knn_point(9, gq, gs)
        assert i.dtype == torch.int64 and v.shape == (2, 77, 9)
        np.testing.assert_array_equal(i.cpu().numpy(), want_idx.numpy())
        v, i = knn.KNN(9)(gq, gs)
        assert i.dtype == torch.int32 and R.ulp_diff(v.cpu().numpy(), want_d) <= 1
        v, i = group.KNN(9)(gs, gq)
        assert v.shape == (2, 9, 77) and i.shape == (2, 77, 9) and i.dtype == torch.int32
        assert R.ulp_diff(v.cpu().numpy(), want_d.transpose(0, 2, 1)) <= 1
        np.testing.assert_array_equal(i.cpu().numpy(), want_idx.numpy())
        self18 = oracle("uniform", 300, None, 18)[0]
        for mod in (knn, group):
            np.testing.assert_array_equal(mod.DilatedKNN(9, 2)(gs).cpu().numpy(), self18[..., ::2].numpy())
            sto = mod.DilatedKNN(9, 2, stochastic=True, epsilon=1.0).train()
            torch.manual_seed(5)
            got = sto(gs)
            torch.manual_seed(5)
            torch.rand(1)
            cols = torch.randperm(18)[:9]
            np.testing.assert_array_equal(got.cpu().numpy(), self18[..., cols].numpy())
        assert dict(calls).get("knn_batch", 0) == 7, dict(calls)


@pytest.mark.parametrize("n,m,k", [(2048, None, 16), (6000, 700, 9), (300, 77, 32)])
def test_far_from_the_origin(dev, n, m, k):
    """a uniform cloud shifted by +100 on every axis: the kernel route's lists are the exact fp64 lists for every query
    whose distances are distinct (the direct differences are exact there; cdist's matmul form is not)"""
    from amcontrast3d_amd import ops
    sup, qry = pair("uniform", n, m)
    sup = (sup + 100.0).contiguous()
    qry = sup if m is None else (qry + 100.0).contiguous()
    exact, untied = R.exact_knn(k, qry, sup)
    sel = untied & R.oracle_untied(k, qry, sup)
    gs = sup.to(dev)
    idx = ops.knn_batch(k, gs, gs if m is None else qry.to(dev))[1].cpu().long()
    differ = int((idx != exact).any(-1)[sel].sum())
    print(f"{differ} of {int(sel.sum())} untied queries differ from the exact lists ({int((~sel).sum())} tied)")
    assert differ == 0 and float(sel.float().mean()) >= 0.9
