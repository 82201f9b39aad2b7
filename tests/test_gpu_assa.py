"""The separable aggregation kernels of csrc/assa.hip against their NumPy restatement (tests/assa_ref.py).

The C entries are called directly on NaN-filled outputs, so an element a kernel skips shows.  Forward and the reverse-list
backward promise an arithmetic and an order: compared bit for bit.  The default backward adds with float atomics in any
order: compared with the fp64 twin, element by element, under

    |got - exact| <= 2 * (cnt + 4) * U * sum|terms|,    U = 2^-24, cnt = the in-degree of the support point:

an edge's term costs three product roundings, two adds and the scale (6 relative errors of U on at most its |products|,
the "+ 4" beyond the (cnt + 1) of the sum itself, whose cnt adds act on partial sums no larger than sum|terms|), doubled for
the higher-order terms as in tests/test_gpu_interp_grad_lds.py.  A support point nobody gathers has sum|terms| = 0: exactly 0.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import assa_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
RED = {"mean": 0, "sum": 1, "max": 2}
KS, CS, MS, NS = (1, 5, 16, 32), (1, 3, 12, 43, 64, 130), (1, 77, 300), (5, 300)
KINDS = ("random", "equal", "perm", "ball")


def _ops():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import _lib, ops
    return ops, _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _idx(kind, rng, B, M, K, N):
    if kind == "random":
        return rng.integers(0, N, (B, M, K)).astype(np.int32)
    if kind == "equal":  # one support point gathers everything: in-degree M*K, all others 0
        return np.full((B, M, K), N // 2, np.int32)
    if kind == "perm":   # the positions run through a permutation of the support points: in-degrees differ by at most one
        return np.stack([rng.permutation(N)[np.arange(M * K) % N].reshape(M, K) for _ in range(B)]).astype(np.int32)
    return R.ball_like_idx(rng, B, M, K, N)


def _inputs(seed, B, C, N, M, K, kind):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((B, C, N)).astype(np.float32)
    dp = rng.uniform(-1, 1, (B, 3, M, K)).astype(np.float32)
    idx = _idx(kind, rng, B, M, K, N)
    if kind == "ball":  # a padded row repeats its first hit: dp repeats with it, exact ties under max
        same = idx == idx[:, :, :1]
        dp = np.where(same[:, None], dp[:, :, :, :1], dp)
    g = rng.standard_normal((B, 3 * C, M)).astype(np.float32)
    return f, idx, dp, g


def _forward(lib, _lib, f, idx, dp, reduction):
    """the C entry on NaN-filled outputs -> out (B,3C,M), arg (B,M,3C) uint8 or None, as numpy"""
    B, C, N = f.shape
    _, M, K = idx.shape
    f_pm = torch.from_numpy(np.ascontiguousarray(f.transpose(0, 2, 1))).to(DEV)
    ti, td = torch.from_numpy(idx).to(DEV), torch.from_numpy(dp).to(DEV)
    out = torch.full((B, 3 * C, M), float("nan"), device=DEV)
    arg = torch.full((B, M, 3 * C), 255, dtype=torch.uint8, device=DEV) if reduction == "max" else None
    _lib.check(lib.amc3d_assa_aggregate_forward(B, C, N, M, K, RED[reduction], _p(f_pm), _p(ti), _p(td), _p(out), _p(arg), _stream()),
               "assa_aggregate_forward")
    return out.cpu().numpy(), (arg.cpu().numpy() if arg is not None else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("reduction", list(RED))
@pytest.mark.parametrize("K", KS)
def test_forward_bits(K, reduction):
    ops, _lib, lib = _ops()
    B = 2
    for n, (C, M, N, kind) in enumerate(itertools.product(CS, MS, NS, KINDS)):
        f, idx, dp, _ = _inputs(100 * K + n, B, C, N, M, K, kind)
        got, arg = _forward(lib, _lib, f, idx, dp, reduction)
        want, warg = R.forward(f, idx, dp, reduction)
        case = (K, C, M, N, kind, reduction)
        assert not np.isnan(got).any(), case
        assert np.array_equal(_bits(got), _bits(want)), (case, float(np.abs(got - want).max()))
        if reduction == "max":
            stored = arg.reshape(B, M, 3 * C).transpose(0, 2, 1)  # rows -> (B,3C,M)
            assert np.array_equal(stored.astype(np.int64), warg), case
            if kind == "ball":
                first = idx == idx[:, :, :1]  # positions that repeat the first hit: the stored k is never a later copy
                k_is_copy = np.take_along_axis(np.broadcast_to(first[:, None], (B, 3 * C, M, K)), stored[..., None].astype(np.int64), 3)[..., 0]
                assert (stored[k_is_copy] == 0).all(), case


def test_max_propagates_nan():
    """torch.max's rule, which the reference's reduction follows: a NaN product wins from its k on (the first NaN is the
    one stored), so a diverging run shows in the output; every other element keeps its bits"""
    ops, _lib, lib = _ops()
    B, C, N, M, K = 2, 43, 300, 77, 16
    f, idx, dp, _ = _inputs(9, B, C, N, M, K, "ball")
    f[0, 5, idx[0, 10, 3]] = np.nan      # one channel of one support point
    f[1, :, idx[1, 20, 0]] = np.nan      # a whole row, met first at k = 0
    dp[1, 2, 30, 7] = np.nan             # one coordinate of one edge
    got, arg = _forward(lib, _lib, f, idx, dp, "max")
    want, warg = R.forward(f, idx, dp, "max")
    nan = np.isnan(want)
    assert nan.any() and not nan.all() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    assert np.array_equal(arg.reshape(B, M, 3 * C).transpose(0, 2, 1).astype(np.int64), warg)
    t = torch.from_numpy
    fj = torch.gather(t(f), 2, t(idx).long().reshape(B, 1, -1).expand(-1, C, -1)).reshape(B, C, M, K)
    ref = (fj.unsqueeze(1) * t(dp).unsqueeze(2)).reshape(B, 3 * C, M, K).max(-1)[0].numpy()  # the reference's expression
    assert np.array_equal(np.isnan(ref), nan)


# shapes of the backward tests: every C (16- / 32- / 64-lane groups, channel chunks and tails), every K, every idx kind, one
# query, five support points, several workgroups of queries and of support points
BACKWARD_CASES = [(1, 1, 1, 5, "equal"), (5, 3, 77, 5, "random"), (16, 12, 77, 300, "ball"), (32, 43, 300, 300, "ball"),
                  (16, 64, 77, 300, "perm"), (5, 130, 300, 300, "random"), (32, 130, 1, 300, "perm"), (1, 43, 300, 5, "equal"),
                  (16, 3, 300, 300, "equal"), (5, 12, 1, 5, "ball"), (3, 16, 20, 300, "perm")]


def _backward(lib, _lib, ops, g, idx, dp, arg_pm, reduction, N, lists):
    B, C3, M = g.shape
    C, K = C3 // 3, idx.shape[-1]
    g_pm = torch.from_numpy(np.ascontiguousarray(g.transpose(0, 2, 1))).to(DEV)
    ti, td = torch.from_numpy(idx).to(DEV), torch.from_numpy(dp).to(DEV)
    ta = torch.from_numpy(arg_pm).to(DEV) if arg_pm is not None else None
    df = torch.full((B, N, C), float("nan"), device=DEV)
    if lists:
        start, edge = ops.group_csr(ti, N)
        _lib.check(lib.amc3d_assa_aggregate_backward_csr(B, C, N, M, K, RED[reduction], _p(g_pm), _p(td), _p(ta), _p(start), _p(edge),
                                                         _p(df), _stream()), "assa_aggregate_backward_csr")
    else:
        _lib.check(lib.amc3d_assa_aggregate_backward(B, C, N, M, K, RED[reduction], _p(g_pm), _p(ti), _p(td), _p(ta), _p(df), _stream()),
                   "assa_aggregate_backward")
    return df.cpu().numpy().transpose(0, 2, 1)


@pytest.mark.parametrize("reduction", list(RED))
@pytest.mark.parametrize("case", BACKWARD_CASES, ids=lambda c: "K%d-C%d-M%d-N%d-%s" % c)
def test_backward_bits_over_reverse_lists(case, reduction):
    ops, _lib, lib = _ops()
    K, C, M, N, kind = case
    f, idx, dp, g = _inputs(7 + K + C, 2, C, N, M, K, kind)
    arg_pm = None
    warg = None
    if reduction == "max":
        _, arg_pm = _forward(lib, _lib, f, idx, dp, reduction)
        warg = R.forward(f, idx, dp, reduction)[1]
    got = _backward(lib, _lib, ops, g, idx, dp, arg_pm, reduction, N, lists=True)
    want = R.backward(g, idx, dp, warg, reduction, N)
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(want)), float(np.abs(got - want).max())
    unreferenced = np.ones((2, N), bool)
    for b in range(2):
        unreferenced[b, np.unique(idx[b])] = False
    if kind == "equal" or M * K < N:
        assert unreferenced.any()
    assert (_bits(got.transpose(0, 2, 1)[unreferenced]) == 0).all(), "exactly +0.0 where nobody gathers"


@pytest.mark.parametrize("reduction", list(RED))
@pytest.mark.parametrize("case", BACKWARD_CASES, ids=lambda c: "K%d-C%d-M%d-N%d-%s" % c)
def test_backward_atomics_within_the_rounding_bound(case, reduction):
    ops, _lib, lib = _ops()
    K, C, M, N, kind = case
    f, idx, dp, g = _inputs(7 + K + C, 2, C, N, M, K, kind)
    arg_pm = warg = None
    if reduction == "max":
        _, arg_pm = _forward(lib, _lib, f, idx, dp, reduction)
        warg = R.forward(f, idx, dp, reduction)[1]
    got = _backward(lib, _lib, ops, g, idx, dp, arg_pm, reduction, N, lists=False)
    exact, mag, cnt = R.backward(g, idx, dp, warg, reduction, N, np.float64, magnitudes=True)
    assert not np.isnan(got).any()
    bound = 2 * (cnt[:, None, :] + 4) * U * mag
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{case} {reduction}: worst error / bound = {worst:.3f}, in-degrees {int(cnt.min())}..{int(cnt.max())}")
    assert (err <= bound).all()
    if kind == "equal":
        assert int(cnt.max()) == M * K and int(cnt.min()) == (0 if N > 1 else M * K)
    assert (_bits(got.transpose(0, 2, 1)[cnt == 0]) == 0).all()


def test_autograd_wiring():
    ops, _lib, lib = _ops()
    B, C, N, M, K = 2, 12, 300, 77, 16
    f, idx, dp, g = _inputs(3, B, C, N, M, K, "ball")
    tf, ti, td, tg = (torch.from_numpy(a).to(DEV) for a in (f, idx, dp, g))
    for reduction in RED:
        x = tf.clone().requires_grad_(True)
        d = td.clone().requires_grad_(True)
        with ops.deterministic_mode():
            out = ops.SeparableAggregation.apply(x, ti, d, reduction)
            out.backward(tg)
        want, warg = R.forward(f, idx, dp, reduction)
        assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(want))
        assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(R.backward(g, idx, dp, warg, reduction, N)))
        assert d.grad is None, "dp is geometry: no gradient"
        # default mode: whichever route the dispatch takes, within the atomic route's bound
        y = tf.clone().requires_grad_(True)
        ops.separable_aggregation(y, ti, td, reduction).backward(tg)
        exact, mag, cnt = R.backward(g, idx, dp, warg, reduction, N, np.float64, magnitudes=True)
        assert (np.abs(y.grad.cpu().numpy().astype(np.float64) - exact) <= 2 * (cnt[:, None, :] + 4) * U * mag).all()
        # bf16 autocast: the inputs are cast to fp32, the result is the fp32 call on the same (bf16-representable) values
        fb, db = tf.bfloat16(), td.bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cast = ops.separable_aggregation(fb, ti, db, reduction)
        assert cast.dtype == torch.float32
        assert torch.equal(cast, ops.separable_aggregation(fb.float(), ti, db.float(), reduction))
        # a non-contiguous view is copied, not misread
        wide = torch.from_numpy(np.ascontiguousarray(np.repeat(f, 2, axis=2))).to(DEV)
        assert torch.equal(ops.separable_aggregation(wide[:, :, ::2], ti, td, reduction), out.detach())
    # lists handed over in default mode change nothing: the default backward scatters and stays inside its bound
    z = tf.clone().requires_grad_(True)
    ops.separable_aggregation(z, ti, td, "mean", ops.group_csr(ti, N)).backward(tg)
    exact, mag, cnt = R.backward(g, idx, dp, None, "mean", N, np.float64, magnitudes=True)
    assert (np.abs(z.grad.cpu().numpy().astype(np.float64) - exact) <= 2 * (cnt[:, None, :] + 4) * U * mag).all()
    with pytest.raises(RuntimeError, match="int32"):
        ops.separable_aggregation(tf, ti.long(), td)
    with pytest.raises(RuntimeError, match="float32"):
        ops.separable_aggregation(tf.double(), ti, td)
    with pytest.raises(NotImplementedError):
        ops.separable_aggregation(tf, ti, td, "median")


@pytest.mark.parametrize("reduction", list(RED))
def test_capture_replays_the_eager_bits(reduction):
    """forward + backward captured on one stream (deterministic mode, the plan's reverse lists) replay to the eager bits"""
    ops, _lib, lib = _ops()
    B, C, N, M, K = 2, 43, 300, 77, 16
    f, idx, dp, g = _inputs(5, B, C, N, M, K, "ball")
    ti, td, sg = (torch.from_numpy(a).to(DEV) for a in (idx, dp, g))
    csr = ops.group_csr(ti, N)  # as ASSA.plan hands them over in deterministic mode

    def step(leaf):
        out = ops.separable_aggregation(leaf, ti, td, reduction, csr)
        return out, torch.autograd.grad(out, leaf, sg)[0]
    with ops.deterministic_mode():
        eager = step(torch.from_numpy(f).to(DEV).requires_grad_(True))
        # a fresh leaf for the captured part, as in tests/test_gpu_refine.py: the eager backward above ran on the default
        # stream, and autograd would synchronise a leaf it has seen there with that stream inside the capture
        sf = torch.from_numpy(f).to(DEV).requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step(sf)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, grad = step(sf)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(grad, eager[1])


def test_no_tensor_of_neighbourhood_size():
    """forward + backward at B=2, C=64, N=4096, M=1024, K=32 stay below a quarter of the reference's (B,3C,M,K) tensor above
    the inputs, in both backward routes"""
    ops, _lib, lib = _ops()
    B, C, N, M, K = 2, 64, 4096, 1024, 32
    gen = torch.Generator().manual_seed(0)
    f = torch.randn(B, C, N, generator=gen).to(DEV).requires_grad_(True)
    idx = torch.randint(0, N, (B, M, K), generator=gen, dtype=torch.int32).to(DEV)
    dp = torch.rand(B, 3, M, K, generator=gen).to(DEV)
    g = torch.randn(B, 3 * C, M, generator=gen).to(DEV)
    limit = B * 3 * C * M * K * 4 // 4
    for det in (False, True):
        for reduction in RED:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with ops.deterministic_mode(det):
                out = ops.separable_aggregation(f, idx, dp, reduction)
                (grad,) = torch.autograd.grad(out, f, g)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            print(f"deterministic={det} {reduction}: peak {peak / 2**20:.1f} MiB above the inputs, limit {limit / 2**20:.1f} MiB")
            assert peak < limit
            del out, grad
