"""The offset-layout pointops kernels (csrc/pointops.hip) and their Python layers on the MI355X.

Searches, forwards and row-local gradients are held bit for bit against the NumPy restatement
(tests/pointops_offset_ref.py; furthest sampling also against the oracle's dense kernel per segment).  The four scatter
gradients: in deterministic mode bit for bit against the restatement's sequential sum; in the default mode (float atomics,
any order) against fp64 under the bound tests/test_gpu_interp_grad_lds.py derives,

    |got - exact| <= 2 * (cnt + 1) * U * sum|terms|,     U = 2^-24, cnt = the in-degree of the target.

Against the fixtures recorded from the reference's pointops.py: indices and values produced by kernels alone are exact
(scatter gradients: exact in deterministic mode, the bound above in the default mode); where torch elementwise operators
on the device enter -- interpolation's weights, normalize_dp -- the bound is (k + 6) * U * sum|terms| per element: the
roundings of sqrt, + 1e-8, reciprocal, two adds of the norm, the division, and k products and adds (normalize_dp: the
element itself is the one term and k = 3, the three squares under the root; torch divides by a host scalar through its
reciprocal, one rounding more than the division and inside the same allowance).
"""
import ctypes

import numpy as np
import pytest
import torch

import pointops_offset_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SEG, QSEG = [1, 2, 65, 300, 7], [1, 1, 20, 75, 3]
eq = np.testing.assert_array_equal


def _mods():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import _lib, compat, offset_ops, ops
    return ops, offset_ops, compat, _lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call(name, *args):
    _, _, _, _lib = _mods()
    args = [_p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
    _lib.check(getattr(_lib.load(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def nan_like(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def ridx(seed, rows, ns, n_targets, how="random"):
    rng = np.random.default_rng(seed)
    if how == "random":
        return rng.integers(0, n_targets, size=(rows, ns)).astype(np.int32)
    if how == "equal":  # one target of in-degree rows * ns
        return np.full((rows, ns), n_targets // 2, np.int32)
    assert how == "perm" and n_targets >= rows * ns  # in-degree 1
    return rng.permutation(n_targets)[:rows * ns].reshape(rows, ns).astype(np.int32)


# shapes: (support segment counts, query segment counts).  The shared ragged shape crosses a wavefront and a 256-thread
# boundary, holds a one-point segment and no end on a multiple of 64; one segment of 2500 spans three LDS tiles and many
# blocks; the third makes one block's queries straddle segments whose union spans three tiles.
SHAPES = {"ragged": (SEG, QSEG), "one2500": ([2500], [600]), "straddle": ([1500, 1200, 3], [10, 9, 3])}


def cloud_and_queries(kind, counts, qcounts, off_support):
    xyz = np.concatenate([R.cloud(9 + i, c, kind) for i, c in enumerate(counts)])
    rng = np.random.default_rng(3)
    if off_support:
        q = np.concatenate([R.cloud(40 + i, c, kind) + np.float32(0.37) for i, c in enumerate(qcounts)])
    else:
        q = np.concatenate([xyz[a:b][rng.permutation(b - a)[:c]] for (a, b), c in zip(R.segments(R.ends(counts)), qcounts)])
    return xyz, np.ascontiguousarray(q)


# ----------------------------------------------------------------------------------------------- ball query
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind,radius,nsample", [
    ("uniform", 0.3, 16), ("lattice", 0.25, 16), ("lattice", 0.25, 1), ("lattice", 0.25, 70), ("dup", 10.0, 70), ("dup", 10.0, 1),
    ("uniform", 10.0, 16), ("uniform", 1e-6, 16), ("uniform", 1e-6, 1), ("dup", 0.1, 16)])
def test_ballquery_equals_restatement(shape, kind, radius, nsample):
    _, O, _, _ = _mods()
    counts, qcounts = SHAPES[shape]
    xyz, q = cloud_and_queries(kind, counts, qcounts, off_support=radius < 1e-3)
    off, noff = R.ends(counts), R.ends(qcounts)
    want = R.ballquery(radius, nsample, xyz, q, off, noff)
    got = host(O.ballquery(radius, nsample, dv(xyz), dv(q), dv(off), dv(noff)))
    eq(got, want)
    if radius < 1e-3:
        assert not got.any()  # whole rows of zeros: global row 0, not the segment's start


def test_ballquery_with_empty_segments_and_self_queries():
    _, O, _, _ = _mods()
    counts, qcounts = [5, 0, 70, 0, 9], [5, 0, 70, 0, 9]  # empty segments on both sides, new_xyz = None
    xyz = np.concatenate([R.cloud(2 + i, c, "uniform") for i, c in enumerate(counts) if c])
    off = R.ends(counts)
    got = host(O.ballquery(0.5, 8, dv(xyz), None, dv(off), dv(off)))
    eq(got, R.ballquery(0.5, 8, xyz, xyz, off, off))


# ----------------------------------------------------------------------------------------- furthest sampling
def fps_samples(counts, rule):
    return [c if (s + rule) % 3 == 0 else max(1, c // 3) if (s + rule) % 3 == 1 else 1 for s, c in enumerate(counts)]


@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("kind", ["lattice", "dup", "room"])
@pytest.mark.parametrize("counts", [[40, 300, 7], [2500, 130, 1], SEG, [2500]], ids=lambda c: "-".join(map(str, c)))
def test_fps_equals_oracle_per_segment(counts, kind, rule):
    from oracle import pointops_ref as K
    _, O, _, _ = _mods()
    xyz = np.concatenate([R.cloud(5 + i, c, kind) for i, c in enumerate(counts)])
    picks = fps_samples(counts, rule)
    if len(counts) == 1:
        picks = [(2500, 700, 1)[rule]]
    off, noff = R.ends(counts), R.ends(picks)
    n, m = xyz.shape[0], int(noff[-1])
    tmp, idx = torch.full((n,), 1e10, device=DEV), torch.full((m,), -1, dtype=torch.int32, device=DEV)
    call("amc3d_pointops_furthestsampling", len(counts), max(counts), n, dv(xyz), dv(off), dv(noff), tmp, idx)
    want_idx, want_tmp = R.furthestsampling(xyz, off, noff)
    for (a, b), (ma, mb) in zip(R.segments(off), R.segments(noff)):
        dense = K.furthest_point_sample(torch.from_numpy(xyz[a:b])[None], mb - ma)[0].numpy() + a
        eq(host(idx)[ma:mb], dense)
    eq(host(idx), want_idx)
    eq(host(tmp), want_tmp)
    eq(host(O.furthestsampling(dv(xyz), dv(off), dv(noff))), want_idx)  # the Python layer (dense route where segments are equal)


@pytest.mark.parametrize("big,n_max", [(4096, 4096), (4097, 4097), (8192, 8192), (8193, 8193), (12288, 12288), (12289, 12289),
                                       (5000, 100)])
def test_fps_register_budgets_and_zero_sample_segment(big, n_max):
    """n_max picks the kernel variant (4, 8 or 12 points per thread in registers); a segment beyond the variant's budget
    -- longer than 12288, or longer than an understated n_max promised -- keeps its minima in tmp.  Each threshold from
    both sides.  A segment without samples writes nothing."""
    from oracle import pointops_ref as K
    counts, picks = [big, 50, 30], [24, 0, 30]
    xyz = np.concatenate([R.cloud(15 + i, c, "dup") for i, c in enumerate(counts)])
    off, noff = R.ends(counts), R.ends(picks)
    tmp, idx = torch.full((xyz.shape[0],), 1e10, device=DEV), torch.full((54,), -7, dtype=torch.int32, device=DEV)
    call("amc3d_pointops_furthestsampling", 3, n_max, xyz.shape[0], dv(xyz), dv(off), dv(noff), tmp, idx)
    want_idx, want_tmp = R.furthestsampling(xyz, off, noff)
    eq(host(idx), want_idx)
    eq(host(tmp), want_tmp)
    eq(host(idx)[:24], K.furthest_point_sample(torch.from_numpy(xyz[:big])[None], 24)[0].numpy())
    eq(host(tmp)[big:big + 50], np.full(50, 1e10, np.float32))


def test_fps_equal_segments_take_the_dense_route_and_agree_with_the_ragged_kernel():
    from oracle import pointops_ref as K
    _, O, _, _ = _mods()
    xyz = np.concatenate([R.cloud(60 + i, 512, "lattice") for i in range(3)])
    off, noff = R.ends([512] * 3), R.ends([128] * 3)
    got = host(O.furthestsampling(dv(xyz), dv(off), dv(noff)))
    tmp, idx = torch.full((1536,), 1e10, device=DEV), torch.empty(384, dtype=torch.int32, device=DEV)
    call("amc3d_pointops_furthestsampling", 3, 512, 1536, dv(xyz), dv(off), dv(noff), tmp, idx)
    eq(got, host(idx))
    dense = K.furthest_point_sample(torch.from_numpy(xyz.reshape(3, 512, 3)), 128).numpy() + np.arange(3)[:, None] * 512
    eq(got, dense.reshape(-1))


# ------------------------------------------------------------------------------------------------- forwards
ROWS = {"ragged": (375, 100), "one2500": (2500, 600)}  # (n source rows, m query rows)
CS = [1, 3, 5, 32, 48]
NSS = [1, 5, 16]


@pytest.mark.parametrize("shape", list(ROWS))
@pytest.mark.parametrize("nsample", NSS)
@pytest.mark.parametrize("c", CS)
def test_grouping_and_subtraction_forward(shape, c, nsample):
    n, m = ROWS[shape]
    x, x2 = rnd(1, n, c), rnd(2, n, c)
    gi, si = ridx(3, m, nsample, n), ridx(4, n, nsample, n)
    out = nan_like(m, nsample, c)
    call("amc3d_pointops_grouping_forward", m, nsample, c, n, dv(x), dv(gi), out)
    eq(host(out), R.grouping_forward(x, gi))
    out = nan_like(n, nsample, c)
    call("amc3d_pointops_subtraction_forward", n, nsample, c, dv(x), dv(x2), dv(si), out)
    eq(host(out), R.subtraction_forward(x, x2, si))


@pytest.mark.parametrize("shape", list(ROWS))
@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("c", CS)
def test_interpolation_forward_both_accumulate_forms(shape, c, k):
    n, m = ROWS[shape]
    x, w, idx = rnd(1, m, c), np.abs(rnd(2, n, k)), ridx(3, n, k, m)
    out = nan_like(n, c)  # overwrite form into NaN
    call("amc3d_pointops_interpolation_forward", n, c, k, m, 0, dv(x), dv(idx), dv(w), out)
    eq(host(out), R.interpolation_forward(x, idx, w))
    pattern = rnd(4, n, c)  # accumulate form into a pattern
    out = dv(pattern)
    call("amc3d_pointops_interpolation_forward", n, c, k, m, 1, dv(x), dv(idx), dv(w), out)
    eq(host(out), R.interpolation_forward(x, idx, w, out=pattern))


@pytest.mark.parametrize("shape", list(ROWS))
@pytest.mark.parametrize("nsample", NSS)
@pytest.mark.parametrize("c", CS)
def test_aggregation_forward_and_row_local_gradients(shape, c, nsample):
    n, _ = ROWS[shape]
    for w_c in sorted({1, 8, c}):
        x, pos, w, idx = rnd(1, n, c), rnd(2, n, nsample, c), rnd(3, n, nsample, w_c), ridx(4, n, nsample, n)
        out = nan_like(n, c)
        call("amc3d_pointops_aggregation_forward", n, nsample, c, w_c, 0, dv(x), dv(pos), dv(w), dv(idx), out)
        eq(host(out), R.aggregation_forward(x, pos, w, idx))
        pattern = rnd(5, n, c)
        out = dv(pattern)
        call("amc3d_pointops_aggregation_forward", n, nsample, c, w_c, 1, dv(x), dv(pos), dv(w), dv(idx), out)
        eq(host(out), R.aggregation_forward(x, pos, w, idx, out=pattern))
        # grad_position and grad_weight are written (NaN-filled buffers), without atomics: exact; grad_input skipped (NULL)
        go = rnd(6, n, c)
        gp, gw = nan_like(n, nsample, c), nan_like(n, nsample, w_c)
        call("amc3d_pointops_aggregation_backward", n, nsample, c, w_c, dv(x), dv(pos), dv(w), dv(idx), dv(go), None, gp, gw)
        _, want_gp, want_gw = R.aggregation_backward(x, pos, w, idx, go)
        eq(host(gp), want_gp)
        eq(host(gw), want_gw)
    # subtraction's grad_input1: the sequential sum over j, written
    up = rnd(7, n, nsample, c)
    g1 = nan_like(n, c)
    call("amc3d_pointops_subtraction_backward", n, nsample, c, dv(ridx(4, n, nsample, n)), dv(up), g1, None)
    eq(host(g1), R.subtraction_backward(up, ridx(4, n, nsample, n))[0])


# ------------------------------------------------------------------------------------------ scatter gradients
def scatter_case(op, how, shape, c, ns):
    """-> (run(default) -> got, run_csr(out) -> None, sequential want, (exact, mag, deg)) through the C ABI"""
    ops, _, _, _ = _mods()
    n, m = ROWS[shape]
    if op == "grouping":
        rows, nt = m, (m * ns if how == "perm" else n)
        idx, g = ridx(1, rows, ns, nt, how), rnd(2, rows, ns, c)
        want, exact = R.grouping_backward(g, idx, nt), R.grouping_backward_exact(g, idx, nt)
        default = lambda out: call("amc3d_pointops_grouping_backward", rows, ns, c, nt, dv(g), dv(idx), out)  # noqa: E731
        kind, per, w_c, w = 0, 1, 1, None
    elif op == "interpolation":
        rows, nt = n, (n * ns if how == "perm" else m)
        idx, g, w = ridx(1, rows, ns, nt, how), rnd(2, rows, c), np.abs(rnd(3, rows, ns))
        want, exact = R.interpolation_backward(g, idx, w, nt), R.interpolation_backward_exact(g, idx, w, nt)
        default = lambda out: call("amc3d_pointops_interpolation_backward", rows, c, ns, nt, dv(g), dv(idx), dv(w), out)  # noqa: E731
        kind, per, w_c = 1, ns, 1
    elif op == "subtraction":
        rows, nt = n, (n * ns if how == "perm" else n)
        idx, g = ridx(1, rows, ns, nt, how), rnd(2, rows, ns, c)
        want, exact = R.subtraction_backward(g, idx, nt)[1], R.subtraction_backward_exact(g, idx, nt)
        default = lambda out: call("amc3d_pointops_subtraction_backward", rows, ns, c, dv(idx), dv(g), nan_like(rows, c), out)  # noqa: E731
        kind, per, w_c, w = 2, 1, 1, None
    else:
        rows, nt, w_c = n, (n * ns if how == "perm" else n), (8 if c > 8 else 1)
        idx, g, w = ridx(1, rows, ns, nt, how), rnd(2, rows, c), rnd(3, rows, ns, w_c)
        x, pos = rnd(4, nt, c), rnd(5, rows, ns, c)
        want, exact = R.aggregation_backward(x, pos, w, idx, g)[0], R.aggregation_backward_exact(x, w, idx, g)
        default = lambda out: call("amc3d_pointops_aggregation_backward", rows, ns, c, w_c, dv(x), dv(pos), dv(w), dv(idx), dv(g), out,  # noqa: E731
                                   nan_like(rows, ns, c), nan_like(rows, ns, w_c))
        kind, per = 3, ns
    d_idx = dv(idx)
    rev_start, rev_edge = ops.group_csr(d_idx.view(1, rows, ns), nt)

    def csr(out):
        call("amc3d_pointops_scatter_csr", kind, nt, c, per, w_c, dv(g), None if w is None else dv(w), rev_start, rev_edge, out)

    return default, csr, want, exact, nt


OPS4 = ["grouping", "interpolation", "subtraction", "aggregation"]


@pytest.mark.parametrize("shape", list(ROWS))
@pytest.mark.parametrize("how", ["random", "equal", "perm"])
@pytest.mark.parametrize("op", OPS4)
def test_scatter_gradients_default_mode_within_the_any_order_bound(op, how, shape):
    for c, ns in ((3, 5), (48, 16), (32, 1)):
        default, _, _, (exact, mag, deg), nt = scatter_case(op, how, shape, c, ns)
        out = torch.zeros(nt, c, device=DEV)
        default(out)
        err, bound = np.abs(host(out).astype(np.float64) - exact), 2 * (deg + 1) * U * mag
        print(f"{op} {how} {shape} c={c} ns={ns}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
        assert (host(out)[deg[:, 0] == 0] == 0).all()


@pytest.mark.parametrize("shape", list(ROWS))
@pytest.mark.parametrize("how", ["random", "equal", "perm"])
@pytest.mark.parametrize("op", OPS4)
def test_scatter_gradients_deterministic_mode_is_the_sequential_sum(op, how, shape):
    for c, ns in ((3, 5), (48, 16), (32, 1)):
        _, csr, want, (_, _, deg), nt = scatter_case(op, how, shape, c, ns)
        a, b = nan_like(nt, c), nan_like(nt, c)  # every element is written
        csr(a)
        csr(b)
        eq(host(a), want)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # the same bits on a second run
        unnamed = host(a.view(torch.int32))[deg[:, 0] == 0]
        assert (unnamed == 0).all()  # exactly +0.0, sign bit clear
        if how == "equal":
            assert (deg[:, 0] == 0).sum() == nt - 1 and unnamed.shape[0] == nt - 1


def test_python_layer_honours_the_mode_recorded_in_forward():
    ops, O, _, _ = _mods()
    n, m, c, ns = 375, 100, 5, 16
    x, idx, up = rnd(1, n, c), ridx(2, m, ns, n), rnd(3, m, ns, c)
    leaf = dv(x).requires_grad_(True)
    with ops.deterministic_mode():
        out = O.grouping(leaf, dv(idx))
    out.backward(dv(up))  # outside the block: ctx.det decides
    eq(host(leaf.grad), R.grouping_backward(up, idx, n))
    a, b = dv(x).requires_grad_(True), dv(rnd(4, n, c)).requires_grad_(True)
    sidx, sup = ridx(5, n, ns, n), rnd(6, n, ns, c)
    with ops.deterministic_mode():
        O.subtraction(a, b, dv(sidx)).backward(dv(sup))
    g1, g2 = R.subtraction_backward(sup, sidx)
    eq(host(a.grad), g1)
    eq(host(b.grad), g2)
    pos, w, go = rnd(7, n, ns, c), rnd(8, n, ns, 1), rnd(9, n, c)
    leaves = [dv(t).requires_grad_(True) for t in (x, pos, w)]
    with ops.deterministic_mode():
        O.aggregation(*leaves, dv(sidx)).backward(dv(go))
    for t, want in zip(leaves, R.aggregation_backward(x, pos, w, sidx, go)):
        eq(host(t.grad), want)


# --------------------------------------------------------------------------- the Python layer against the fixtures
@pytest.fixture(scope="module")
def fix():
    return load_golden("pointops_offset")


def close(got, want, k, mag=None):
    mag = np.abs(want).astype(np.float64) if mag is None else mag
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"  max err / ((k+6) U sum|terms|) = {np.max(err / np.maximum((k + 6) * U * mag, 1e-300)):.3f}")
    assert (err <= (k + 6) * U * mag).all()


def scatter_close(got, idx, terms, want_seq, det):
    if det:
        eq(got, want_seq)
        return
    exact, mag, deg = R._scatter_exact(want_seq.shape[0], want_seq.shape[1], idx, terms)
    assert (np.abs(got.astype(np.float64) - exact) <= 2 * (deg + 1) * U * mag).all()


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_public_functions_against_the_recorded_reference(fix, det):
    ops, _, _, _ = _mods()
    from openpoints.cpp.pointops.functions import pointops as P
    meta = fix["meta"]
    ns, k, radius = meta["nsample"], meta["k"], meta["radius"]
    xyz, new_xyz, offset, new_offset = dv(fix["xyz"]), dv(fix["new_xyz"]), dv(fix["offset"]), dv(fix["new_offset"])
    n = xyz.shape[0]

    def run(key, fn, leaves):
        leaves = [dv(fix[name]).requires_grad_(True) for name in leaves]
        with ops.deterministic_mode(det):
            res = fn(*leaves)
        res = res if isinstance(res, tuple) else (res,)
        pairs = [(r, dv(fix[f"{key}/up{i}"])) for i, r in enumerate(res) if r.requires_grad]
        torch.autograd.backward([r for r, _ in pairs], [u for _, u in pairs])
        return [host(r) for r in res], [host(t.grad) for t in leaves]

    fps = P.furthestsampling(xyz, offset, new_offset)
    eq(host(fps), fix["furthestsampling/idx"])
    knn, dist = P.knnquery(ns, xyz, new_xyz, offset, new_offset)
    eq(host(knn), fix["knnquery/idx"])
    ball = P.ballquery(radius, ns, xyz, new_xyz, offset, new_offset)
    eq(host(ball), fix["ballquery/idx"])
    nbrs = {"knn": fix["knnquery/idx"], "knnquery": fix["knnquery/idx"], "ballquery": fix["ballquery/idx"]}

    outs, grads = run("grouping", lambda f: P.grouping(f, ball), ["feat"])
    eq(outs[0], fix["grouping/out0"])
    scatter_close(grads[0], nbrs["ballquery"], fix["grouping/up0"], fix["grouping/grad0"], det)

    for method, rad in (("knn", None), ("knnquery", radius), ("ballquery", radius)):
        for norm in (False, True):
            key = f"querygroup/{method}/{int(norm)}"
            outs, grads = run(key, lambda f: P.querygroup(ns, xyz, new_xyz, f, offset, new_offset, radius=rad,
                                                          query_method=method, normalize_dp=norm), ["feat"])
            if norm:
                close(outs[0], fix[key + "/out0"], 3)
            else:
                eq(outs[0], fix[key + "/out0"])
            eq(outs[1], fix[key + "/out1"])
            scatter_close(grads[0], nbrs[method], fix[key + "/up1"], fix[key + "/grad0"], det)
    outs, grads = run("querygroup_xyz", lambda x, f: P.querygroup(ns, x, new_xyz, f, offset, new_offset), ["xyz", "feat"])
    eq(outs[0], fix["querygroup_xyz/out0"])
    scatter_close(grads[0], nbrs["knn"], fix["querygroup_xyz/up0"], fix["querygroup_xyz/grad0"], det)
    scatter_close(grads[1], nbrs["knn"], fix["querygroup_xyz/up1"], fix["querygroup_xyz/grad1"], det)

    for use_xyz in (True, False):
        key = f"queryandgroup/{int(use_xyz)}"
        outs, grads = run(key, lambda f: P.queryandgroup(ns, xyz, new_xyz, f, None, offset, new_offset, use_xyz=use_xyz), ["feat"])
        eq(outs[0], fix[key + "/out0"])
        up = fix[key + "/up0"]
        scatter_close(grads[0], nbrs["knn"], up[..., 3:] if use_xyz else up, fix[key + "/grad0"], det)
    outs, grads = run("queryandgroup_idx", lambda f: P.queryandgroup(ns, xyz, new_xyz, f, ball, offset, new_offset), ["feat"])
    eq(outs[0], fix["queryandgroup_idx/out0"])
    scatter_close(grads[0], nbrs["ballquery"], fix["queryandgroup_idx/up0"][..., 3:], fix["queryandgroup_idx/grad0"], det)

    sidx = dv(fix["self_idx"])
    eq(host(P.knnquery(ns, xyz, xyz, offset, offset)[0]), fix["self_idx"])
    outs, grads = run("subtraction", lambda a, b: P.subtraction(a, b, sidx), ["feat", "feat2"])
    eq(outs[0], fix["subtraction/out0"])
    eq(grads[0], fix["subtraction/grad0"])
    scatter_close(grads[1], fix["self_idx"], -fix["subtraction/up0"], fix["subtraction/grad1"], det)

    outs, grads = run("aggregation", lambda f, p, w: P.aggregation(f, p, w, sidx), ["feat", "position", "weight"])
    eq(outs[0], fix["aggregation/out0"])
    eq(grads[1], fix["aggregation/grad1"])
    eq(grads[2], fix["aggregation/grad2"])
    scatter_close(grads[0], fix["self_idx"], fix["aggregation/grad1"], fix["aggregation/grad0"], det)

    # interpolation: torch forms the weights on the device
    up_idx, feat_m = fix["interpolation/idx"].astype(np.int64), fix["feat_m"]
    d = torch.from_numpy(fix["interpolation/dist"])
    w = 1.0 / (d + 1e-8)
    w = (w / w.sum(1, keepdim=True)).numpy().astype(np.float64)
    mag_out = (np.abs(feat_m.astype(np.float64))[up_idx] * w[:, :, None]).sum(1)
    for name, fn in (("interpolation", lambda f: P.interpolation(new_xyz, xyz, f, new_offset, offset, k=k)),
                     ("interpolation2", lambda f: P.interpolation2(new_xyz, xyz, f, new_offset, offset, k))):
        outs, grads = run(name, fn, ["feat_m"])
        close(outs[0], fix[name + "/out0"], k, mag_out)
        mag_grad = np.zeros_like(feat_m, dtype=np.float64)
        np.add.at(mag_grad, up_idx.reshape(-1), (np.abs(fix[name + "/up0"].astype(np.float64))[:, None, :] * w[:, :, None]).reshape(-1, feat_m.shape[1]))
        close(grads[0], fix[name + "/grad0"], k, mag_grad)
    eq(host(P.knnquery(k, new_xyz, xyz, new_offset, offset)[0]), fix["interpolation/idx"])


# ----------------------------------------------------------------------------------------- compat, errors, capture
def test_each_new_compat_entry_point_against_the_restatement():
    _, _, compat, _ = _mods()
    C = compat.pointops_cuda
    counts, qcounts = SEG, QSEG
    xyz, q = cloud_and_queries("uniform", counts, qcounts, False)
    off, noff = R.ends(counts), R.ends(qcounts)
    n, m, c, ns, w_c, k = 375, 100, 5, 16, 1, 3

    tmp, idx = torch.full((n,), 1e10, device=DEV), torch.zeros(m, dtype=torch.int32, device=DEV)
    C.furthestsampling_cuda(5, torch.tensor(300), dv(xyz), dv(off), dv(noff), tmp, idx)
    eq(host(idx), R.furthestsampling(xyz, off, noff)[0])
    bidx = torch.zeros(m, ns, dtype=torch.int32, device=DEV)
    C.ballquery_cuda(m, 0.3, ns, dv(xyz), dv(q), dv(off), dv(noff), bidx)
    eq(host(bidx), R.ballquery(0.3, ns, xyz, q, off, noff))

    # distinct targets below: the atomics have one adder per address, so the sums are exact
    x, gi, up = rnd(1, n, c), ridx(2, m, 3, n, "perm"), rnd(3, m, 3, c)
    out = nan_like(m, 3, c)
    C.grouping_forward_cuda(m, 3, c, dv(x), dv(gi), out)
    eq(host(out), R.grouping_forward(x, gi))
    pattern = rnd(4, n, c)
    gin = dv(pattern)
    C.grouping_backward_cuda(m, 3, c, dv(up), dv(gi), gin)
    eq(host(gin), pattern + R.grouping_backward(up, gi, n))

    xm, w, ii = rnd(5, m, c), np.abs(rnd(6, n, k)), ridx(7, n, k, m)
    out = dv(pattern)
    C.interpolation_forward_cuda(n, c, k, dv(xm), dv(ii), dv(w), out)  # the reference's += into the caller's buffer
    eq(host(out), R.interpolation_forward(xm, ii, w, out=pattern))
    pi = ridx(7, 30, k, m, "perm")
    g, pw = rnd(8, 30, c), np.abs(rnd(9, 30, k))
    gin = torch.zeros(m, c, device=DEV)
    C.interpolation_backward_cuda(30, c, k, dv(g), dv(pi), dv(pw), gin)
    eq(host(gin), R.interpolation_backward(g, pi, pw, m))

    x2, si = rnd(10, n, c), ridx(11, n, ns, n)
    out = nan_like(n, ns, c)
    C.subtraction_forward_cuda(n, ns, c, dv(x), dv(x2), dv(si), out)
    eq(host(out), R.subtraction_forward(x, x2, si))
    p1 = ridx(12, n, 1, n, "perm")
    sup = rnd(13, n, 1, c)
    g1, g2 = nan_like(n, c), torch.zeros(n, c, device=DEV)
    C.subtraction_backward_cuda(n, 1, c, dv(p1), dv(sup), g1, g2)
    w1, w2 = R.subtraction_backward(sup, p1)
    eq(host(g1), w1)
    eq(host(g2), w2)

    pos, wt = rnd(14, n, ns, c), rnd(15, n, ns, w_c)
    out = dv(pattern)
    C.aggregation_forward_cuda(n, ns, c, w_c, dv(x), dv(pos), dv(wt), dv(si), out)
    eq(host(out), R.aggregation_forward(x, pos, wt, si, out=pattern))
    pos1, wt1, go = rnd(16, n, 1, c), rnd(17, n, 1, w_c), rnd(18, n, c)
    gi_, gp, gw = torch.zeros(n, c, device=DEV), nan_like(n, 1, c), nan_like(n, 1, w_c)
    C.aggregation_backward_cuda(n, 1, c, w_c, dv(x), dv(pos1), dv(wt1), dv(p1), dv(go), gi_, gp, gw)
    for got, want in zip((gi_, gp, gw), R.aggregation_backward(x, pos1, wt1, p1, go)):
        eq(host(got), want)


def test_cpu_tensors_raise_the_no_cpu_fallback_error():
    _, O, compat, _ = _mods()
    x, idx = torch.zeros(10, 4), torch.zeros(6, 3, dtype=torch.int32)
    off, noff = torch.tensor([4, 10], dtype=torch.int32), torch.tensor([2, 6], dtype=torch.int32)
    for fn in (lambda: O.grouping(x, idx), lambda: O.subtraction(x, x, torch.zeros(10, 3, dtype=torch.int32)),
               lambda: O.aggregation(x, torch.zeros(10, 3, 4), torch.zeros(10, 3, 2), torch.zeros(10, 3, dtype=torch.int32)),
               lambda: O.interpolation2(torch.zeros(10, 3), torch.zeros(6, 3), x, off, noff),
               lambda: O.furthestsampling(torch.zeros(10, 3), off, noff),
               lambda: O.ballquery(0.1, 3, torch.zeros(10, 3), torch.zeros(6, 3), off, noff),
               lambda: compat.pointops_cuda.grouping_forward_cuda(6, 3, 4, x, idx, torch.zeros(6, 3, 4))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_grouping_and_aggregation_capture_and_replay():
    """forward and backward of both on one stream inside torch.cuda.graph (no parallel branches), replayed twice with
    refreshed inputs; the index sets are permutations, so the atomic scatters have one adder per address and replays
    equal eager bit for bit"""
    _, O, _, _ = _mods()
    n, c, ns, w_c = 375, 32, 5, 8
    idx = dv(ridx(1, n, ns, n * ns, "perm"))
    static = {"x": torch.zeros(n * ns, c, device=DEV), "pos": torch.zeros(n, ns, c, device=DEV), "w": torch.zeros(n, ns, w_c, device=DEV),
              "up_g": torch.zeros(n, ns, c, device=DEV), "up_a": torch.zeros(n, c, device=DEV)}

    def step(t):
        x, pos, w = (t[k].detach().requires_grad_(True) for k in ("x", "pos", "w"))
        g = O.grouping(x, idx)
        a = O.aggregation(x, pos, w, idx)
        grads = torch.autograd.grad([g, a], [x, pos, w], [t["up_g"], t["up_a"]])
        return (g.detach(), a.detach()) + tuple(grads)

    def fill(seed):
        return {k: dv(rnd(seed + i, *v.shape)) for i, (k, v) in enumerate(static.items())}

    for k, v in fill(100).items():
        static[k].copy_(v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(static)
    for seed in (200, 300):
        fresh = fill(seed)
        for k, v in fresh.items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, step(fresh)):
            assert torch.equal(got, want)
