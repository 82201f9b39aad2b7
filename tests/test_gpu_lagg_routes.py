"""Convolve-before-gather aggregation (csrc/lagg.hip) on every launch route and every neighbourhood size class, against the fp64
torch evaluation of tests/test_gpu_lagg.py with its tolerances.

 * the max-pool kernel with 8, 4 and 2 centroids per wave (cpw): the prefetch of the next centroid's idx / dp, the wave-uniform
   break inside a wave's centroids, waves that own no centroid of the last tile, the LDS image of 4 * cpw centroids.  The shapes
   of the other dedicated tests all end at cpw = 1;
 * the backward scatter with one tile per workgroup at exactly 8192 workgroups and with LAGG_TILES = 4 above, atomic and
   reverse-list form, with more than 1024 partial records for the finalize kernel;
 * K below, between and above the rows one load instruction gathers (64 / LPR), K = 1 and K = 64;
 * the first-maximum rule exactly: a padded ball query repeats its first neighbour, the copies have bit-identical inputs and hence
   bit-identical values in any arithmetic, so a later copy may never be the pick;
 * channels that ReLU kills everywhere: exact zeros in every output and gradient;
 * eval mode: a centroid's bits do not depend on which other centroids share the launch.

Every case asserts its route through amc3d_local_aggregation_pool_centroids / amc3d_local_aggregation_partial_counts before it
compares anything: should the thresholds move, the case fails as "no longer selects this route" instead of testing another one.

Where ReLU is on, the upstream gradient is zeroed at the elements whose fp64 pre-activation at the kernel's pick is within 1e-5 of
zero (two correct fp32 evaluations disagree on the mask there and a whole gradient term flips); at most 1e-4 of the elements."""
import contextlib
import ctypes

import pytest
import torch

from test_gpu_lagg import _case, _reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAGG_MT, LAGG_TILES, LAGG_CT = 32, 4, 128  # csrc/lagg.hip
FINALIZE_PASS = 1024                       # records one pass of the finalize kernels' unrolled loop consumes


def _ops():
    from amcontrast3d_amd import _lib, ops
    return ops, _lib, _lib.load()


def _cdiv(a, b):
    return -(-a // b)


def _route(B, C, N, M, K):
    """(centroids per wave of the max-pool launch, partial records of the backward scatter), as the library reports them"""
    ops, _lib, lib = _ops()
    c = (ctypes.c_int * 4)()
    _lib.check(lib.amc3d_local_aggregation_partial_counts(B, C, N, M, K, c), "partial counts")
    return int(lib.amc3d_local_aggregation_pool_centroids(B, C, M)), int(c[1])


def _assert_route(B, C, N, M, K, cpw, tiles):
    got_cpw, records = _route(B, C, N, M, K)
    assert got_cpw == cpw, f"(B={B}, C={C}, M={M}) no longer selects cpw = {cpw} but {got_cpw}"
    want = B * _cdiv(_cdiv(M, LAGG_MT), tiles)
    assert records == want, f"(B={B}, C={C}, M={M}) no longer scatters {tiles} tile(s) per workgroup: {records} records, not {want}"
    return records


def _first_copy(idx, dp):
    """(B,M,K): the smallest k' whose idx[b,m,k'] and dp[b,:,m,k'] equal those at k bit for bit"""
    K = idx.shape[-1]
    eq = idx.unsqueeze(-1) == idx.unsqueeze(-2)
    bits = dp.contiguous().view(torch.int32)
    for j in range(3):
        eq &= bits[:, j].unsqueeze(-1) == bits[:, j].unsqueeze(-2)
    kk = torch.arange(K, device=idx.device)
    return torch.where(eq, kk, K).amin(-1), eq[:, :, 0, 1:].any(-1)


def _preactivation_at(idx, dp, f, w, gamma, beta, arg, eps=1e-5):
    """fp64: bn(conv([dp ; f[idx]])) before the ReLU, at `arg`"""
    B, Cin, N = f.shape
    with torch.no_grad():
        fj = f.double().gather(2, idx.reshape(B, 1, -1).expand(-1, Cin, -1).long()).reshape(B, Cin, idx.shape[1], idx.shape[2])
        y = torch.nn.functional.conv2d(torch.cat([dp.double(), fj], 1), w.double())
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        ystar = y.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)
        del y
        return (ystar - mean[None, :, None]) / torch.sqrt(var[None, :, None] + eps) * gamma.double()[None, :, None] + beta.double()[None, :, None]


def _check(B, Cin, C, N, M, K, relu, radius, cpw, tiles=1, seed=None, dead=None, dup_floor=None):
    """forward and both backward forms of one shape against the fp64 reference; -> the measured figures"""
    ops, _lib, lib = _ops()
    records = _assert_route(B, C, N, M, K, cpw, tiles)
    p, idx, dp, f, w, gamma, beta, go = _case(B, Cin, C, N, M, K, 11 + C + K if seed is None else seed, relu, radius=radius)
    if dead is not None:  # channels that the ReLU kills at every position
        gamma[dead] = torch.where(gamma[dead] < 0, -0.1, 0.1)
        beta[dead] = -10.0
    live = torch.ones(C, dtype=torch.bool, device=DEV)
    if dead is not None:
        live[dead] = False
    first, row_repeats_k0 = _first_copy(idx, dp)
    mom = ops.group_moments(idx, dp, N)
    indeg = torch.zeros(B, N, device=DEV).scatter_add_(1, idx.reshape(B, -1).long(), torch.ones(B, M * K, device=DEV))
    fig = {"shape": (B, Cin, C, N, M, K, relu), "cpw": cpw, "scatter_records": records, "tiles": tiles,
           "padded_rows": float(row_repeats_k0.double().mean()), "nobodys_neighbour": float((indeg == 0).double().mean())}
    ref = None
    for det in (False, True):  # the atomic and the reverse-list backward
        bn = torch.nn.BatchNorm2d(C).to(DEV)
        fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
        log = {}
        ops.pool_log(log)
        try:
            with (ops.deterministic_mode() if det else contextlib.nullcontext()):
                pooled = ops.LocalAggregationFused.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, relu, bn)
        finally:
            ops.pool_log(None)
        arg = log[0]
        if ref is None:
            arg0 = arg
            fig["zeroed"] = 0.0
            if relu:
                near = _preactivation_at(idx, dp, f, w, gamma, beta, arg).abs() < 1e-5
                fig["zeroed"] = float(near.double().mean())
                assert fig["zeroed"] <= 1e-4, fig
                go = torch.where(near, torch.zeros_like(go), go)
            ref = _reference(idx, dp, f, w, gamma, beta, go, relu, arg)
            # first index among equals, exactly: no earlier bit-identical copy of the picked neighbour
            picked_first = first.unsqueeze(1).expand(B, C, M, K).gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)
            later = int((picked_first != arg.long()).sum())
            qualifies = (ref["own_arg"] == 0) & row_repeats_k0.unsqueeze(1)  # the fp64 maximum is the repeated first neighbour
            fig["dup_share"] = float(qualifies.double().mean())
            if dup_floor is not None:
                assert fig["dup_share"] >= dup_floor, fig
            assert later == 0, f"{later} picks have an earlier bit-identical copy in their row"
        assert torch.equal(arg, arg0)
        pooled.backward(go)
        tol = lambda r: 2e-5 * max(1.0, float(r.abs().max()))  # noqa: E731
        errs = {"pooled": (float((pooled.detach().double() - ref["pooled"]).abs().max()), tol(ref["pooled"])),
                "pick": (float((ref["pooled"] - ref["own_max"]).abs().max()), tol(ref["own_max"])),
                "mean": (float((bn.running_mean.double() - 0.1 * ref["mean"]).abs().max()), 1e-5),
                "var": (float((bn.running_var.double() - (0.9 + 0.1 * ref["var_u"])).abs().max()),
                        1e-5 * max(1.0, float(ref["var_u"].max())))}
        for name, got, want in (("df", fr.grad, ref["df"]), ("dw", wr.grad, ref["dw"]), ("dgamma", gr.grad, ref["dgamma"]),
                                ("dbeta", br.grad, ref["dbeta"])):
            errs[name] = (float((got.double() - want).abs().max()), 5e-5 * max(1.0, float(want.abs().max())))
        fig["lists" if det else "atomic"] = errs
        print("lagg route", "lists" if det else "atomic", {k: v for k, v in fig.items() if k not in ("lists", "atomic")},
              {k: "%.3g / %.3g" % v for k, v in errs.items()})
        for name, (err, bound) in errs.items():
            assert err <= bound, (det, name, err, bound)
        assert int(bn.num_batches_tracked) == 1
        if dead is not None:
            assert relu
            assert float(ref["own_max"][:, dead].abs().max()) == 0.0  # the reference agrees that they are dead
            assert float(pooled[:, dead].abs().max()) == 0.0 and int(arg[:, dead].max()) == 0
            assert float(gr.grad[dead].abs().max()) == 0.0 and float(br.grad[dead].abs().max()) == 0.0
            assert float(wr.grad[dead].abs().max()) == 0.0
            if not bool(live.any()):
                assert float(fr.grad.abs().max()) == 0.0
    return fig


# ---- A: the max-pool kernel's routes ---------------------------------------------------------------------------------------
POOL_CASES = [
    # B, Cin, C, N, M, K, relu, cpw
    (8, 8, 8, 4109, 4109, 32, True, 8),      # 129 tiles of 32; the last holds 13: wave 0 full, wave 1 has 5 of 8, waves 2-3 none
    (8, 8, 8, 4109, 4109, 20, True, 8),      # the generic K loop
    (4, 16, 256, 4101, 4101, 8, True, 8),    # two channel chunks, 32 lanes per row
    (8, 8, 8, 2051, 2051, 32, False, 4),     # the last tile of 16 holds 3
    (8, 8, 16, 1027, 1027, 32, True, 2),     # the last tile of 8 holds 3: two in wave 0, one in wave 1
    (8, 8, 32, 16436, 4109, 32, True, 8),    # strided SetAbstraction
    (8, 8, 8, 4109, 4109, 64, True, 8),      # every lane holds a neighbour
    (8, 8, 128, 4109, 4109, 20, True, 8),    # two rows per load instruction, K a multiple of it
]


@pytest.mark.parametrize("B,Cin,C,N,M,K,relu,cpw", POOL_CASES)
def test_pool_routes(B, Cin, C, N, M, K, relu, cpw):
    fig = _check(B, Cin, C, N, M, K, relu, 0.1, cpw)
    assert 0.0 < fig["padded_rows"]  # some balls hold fewer than K points
    if M < N:
        assert fig["nobodys_neighbour"] > 0.05  # in-degree 0


# ---- B: the backward scatter's routes ---------------------------------------------------------------------------------------
SCATTER_CASES = [
    # B, Cin, C, N, M, K, relu, tiles, records
    (8, 8, 8, 32768, 32768, 8, True, 1, 8192),       # exactly 8192 workgroups of one tile
    (8, 8, 8, 32811, 32811, 8, True, 4, 8 * 257),    # 1026 tiles per cloud: the last workgroup takes 2, its last tile 11 centroids
    (8, 8, 16, 32811, 32811, 4, False, 4, 8 * 257),
]


@pytest.mark.parametrize("B,Cin,C,N,M,K,relu,tiles,records", SCATTER_CASES)
def test_scatter_routes(B, Cin, C, N, M, K, relu, tiles, records):
    assert (B * _cdiv(M, LAGG_MT) * _cdiv(C, LAGG_CT) <= 8192) == (tiles == 1)
    fig = _check(B, Cin, C, N, M, K, relu, 0.05, 8, tiles=tiles)
    assert fig["scatter_records"] == records and records > FINALIZE_PASS


# ---- C: every neighbourhood size class ---------------------------------------------------------------------------------------
CK = [(8, 1), (8, 31), (8, 33), (8, 64), (16, 3), (16, 17), (32, 7), (32, 20), (64, 5), (64, 63), (128, 1), (128, 3), (128, 64),
      (256, 24)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("C,K", CK)
def test_neighbourhood_sizes(C, K, strided, relu):
    ops, _lib, lib = _ops()
    assert lib.amc3d_local_aggregation_supported(C, K) == 1
    N = 811
    M = N // 4 if strided else N
    _check(2, min(C, 32), C, N, M, K, relu, 0.2, 1)


# ---- D: the first-maximum rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,N,radius,cpw", [(2, 8, 1100, 0.06, 1), (2, 32, 1100, 0.06, 1), (2, 128, 1100, 0.06, 1),
                                              (8, 8, 4109, 0.04, 8)])
def test_a_later_copy_of_the_first_neighbour_never_wins(B, C, N, radius, cpw):
    """balls of a handful of points, padded to 32 with repeats of the first: wherever fp64 says the first neighbour is the
    maximum, its copies tie with it bit for bit in every slot of the cross-lane reduction"""
    fig = _check(B, 8, C, N, N, 32, True, radius, cpw, seed=3 + C, dup_floor=0.05)
    assert fig["padded_rows"] > 0.5


# ---- E: channels that the ReLU kills ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,N,radius,cpw,dead", [(2, 32, 811, 0.2, 1, slice(0, None, 3)), (2, 8, 811, 0.2, 1, slice(None)),
                                                   (8, 8, 4109, 0.1, 8, slice(0, None, 3)), (8, 8, 4109, 0.1, 8, slice(None))])
def test_dead_channels_are_exactly_zero(B, C, N, radius, cpw, dead):
    _check(B, 8, C, N, N, 32, True, radius, cpw, seed=17 + C, dead=dead)


# ---- F: eval mode, the same bits on every route -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 20])
def test_eval_bits_do_not_depend_on_the_route(K):
    ops, _lib, lib = _ops()
    B, Cin, C, N = 8, 8, 8, 4109
    p, idx, dp, f, w, gamma, beta, _ = _case(B, Cin, C, N, N, K, 23 + K, True, radius=0.1)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5); bn.weight.copy_(gamma); bn.bias.copy_(beta)
    bn.eval()
    assert _route(B, C, N, N, K)[0] == 8
    whole = ops.local_aggregation_eval(f, dp, idx, w, bn, True)
    fj = ops.grouping_operation(f, idx)
    want = torch.relu(bn(torch.nn.functional.conv2d(torch.cat([dp, fj], 1), w))).max(-1).values
    assert float((whole - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    for M, cpw in ((2051, 4), (1027, 2), (100, 1)):
        assert _route(B, C, N, M, K)[0] == cpw, f"(B={B}, C={C}, M={M}) no longer selects cpw = {cpw}"
        part = ops.local_aggregation_eval(f, dp[:, :, :M], idx[:, :M], w, bn, True)
        assert torch.equal(part, whole[:, :, :M]), (M, cpw)
