"""three_interpolate's backward summed in LDS (three_interpolate_grad_lds_kernel): every case against an fp64 evaluation of
the same sum, element by element, under the bound tests/test_gpu_deterministic.py uses for the atomic route,

    |got - exact| <= 2 * (cnt + 1) * U * sum|terms|,     U = 2^-24, cnt = the in-degree of the target,

which holds for ANY summation order: cnt products rounded once each (relative error U) and at most cnt adds, each with
relative error U on a partial sum no larger than sum|terms|; (cnt + 1) * U * sum|terms| to first order, doubled for the
higher-order terms.  In accumulate form the old value of the output is one more term of the sum: cnt + 1 terms, so
2 * (cnt + 2) * U * (sum|terms| + |old|).  Every case asserts the route it takes through amc3d_three_interpolate_grad_route.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
LDS_MAX_M = 16384  # 128 KiB of fp64 slab: the largest m whose single-channel slab is on the route


def _ops():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import _lib, ops
    return ops, _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _route(lib, b, c, n, m):
    cg, threads = ctypes.c_int(-1), ctypes.c_int(-1)
    r = lib.amc3d_three_interpolate_grad_route(b, c, n, m, ctypes.byref(cg), ctypes.byref(threads))
    return r, cg.value, threads.value


def _case(b, c, m, n, seed, idx=None, zero_weights=False):
    g = torch.Generator().manual_seed(seed)
    if idx is None:
        idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32)
    w = torch.rand(b, n, 3, generator=g) + 0.05
    w = w / w.sum(2, keepdim=True)
    if zero_weights:
        w[:, ::2, 1] = 0.0
        w[:, 1::3, :] = 0.0
    go = torch.randn(b, c, n, generator=g)
    return go.to(DEV), idx.to(DEV).contiguous(), w.to(DEV).contiguous()


def _exact(go, idx, w, m):
    """fp64 sum, sum of |terms| and in-degree per target"""
    b, c, n = go.shape
    terms = (go.double().unsqueeze(-1) * w.double().unsqueeze(1)).reshape(b, c, -1)  # (b, c, n*3)
    flat = idx.reshape(b, -1).long()
    want = torch.zeros(b, c, m, dtype=torch.float64, device=DEV)
    sabs = torch.zeros(b, c, m, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(b, m, dtype=torch.float64, device=DEV)
    for bs in range(b):
        want[bs].index_add_(1, flat[bs], terms[bs])
        sabs[bs].index_add_(1, flat[bs], terms[bs].abs())
        cnt[bs].index_add_(0, flat[bs], torch.ones_like(flat[bs], dtype=torch.float64))
    return want, sabs, cnt.unsqueeze(1)


def _check(go, idx, w, m, route=2, cg=None, threads=None):
    """overwrite entry into NaN and accumulate entry into a pattern, both against fp64; returns the overwrite result"""
    ops, _lib, lib = _ops()
    b, c, n = go.shape
    r, got_cg, got_threads = _route(lib, b, c, n, m)
    assert r == route, (r, got_cg, got_threads)
    if cg is not None:
        assert got_cg == cg, got_cg
    if threads is not None:
        assert got_threads == threads, got_threads
    want, sabs, cnt = _exact(go, idx, w, m)
    named = (cnt > 0).expand(b, c, m)

    out = None
    if route == 2:
        out = torch.full((b, c, m), float("nan"), device=DEV)
        _lib.check(lib.amc3d_three_interpolate_grad_write(b, c, n, m, _p(go), _p(idx), _p(w), _p(out), _stream()), "write")
        assert not torch.isnan(out).any()
        err = (out.double() - want).abs()
        print(f"overwrite: max err {float(err.max()):.3e}, max err/bound {float((err / (2 * (cnt + 1) * U * sabs).clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= 2 * (cnt + 1) * U * sabs).all())
        z = out[~named]
        assert torch.equal(z, torch.zeros_like(z)) and not torch.signbit(z).any()  # unnamed known points: exactly +0.0

    old = (torch.arange(b * c * m, device=DEV, dtype=torch.float32).reshape(b, c, m) % 13 - 6.5) * 0.375
    acc = old.clone()
    work = torch.empty(b * c * m, device=DEV)
    _lib.check(lib.amc3d_three_interpolate_grad(b, c, n, m, _p(go), _p(idx), _p(w), _p(acc), _p(work), work.numel() * 4, _stream()), "grad")
    err = (acc.double() - (want + old.double())).abs()
    assert bool((err <= 2 * (cnt + 2) * U * (sabs + old.double().abs())).all())
    assert torch.equal(acc[~named], old[~named])  # unnamed known points: unchanged
    return out


@pytest.mark.parametrize("b,c,m,n", [(2, 12, 40, 160), (2, 7, 40, 333)])
def test_channels_and_points_that_fill_no_group_and_no_block(b, c, m, n):
    go, idx, w = _case(b, c, m, n, 1)
    _check(go, idx, w, m, route=2 if c >= 8 else 0)


@pytest.mark.parametrize("c", [8, 9])
def test_the_smallest_channel_counts_on_the_route(c):
    go, idx, w = _case(2, c, 50, 200, 2)
    _check(go, idx, w, 50, cg=1, threads=256)
    assert _route(_ops()[2], 2, 7, 200, 50)[0] == 0


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("same", ["within a point", "every point"])
def test_same_address_adds_within_one_instruction_and_across_waves(m, same):
    b, c, n = 2, 10, 700
    g = torch.Generator().manual_seed(m)
    if same == "within a point":
        idx = torch.randint(0, m, (b, n, 1), generator=g, dtype=torch.int32).expand(b, n, 3).contiguous()
    else:
        idx = torch.full((b, n, 3), m - 1, dtype=torch.int32)
    go, idx, w = _case(b, c, m, n, 3, idx)
    _check(go, idx, w, m)


def test_known_points_that_nobody_names():
    b, c, m, n = 2, 16, 200, 50  # at most 150 of the 200 known points are named
    go, idx, w = _case(b, c, m, n, 4)
    out = _check(go, idx, w, m)
    assert int((out == 0).all(1).sum()) >= b * 50


@pytest.mark.parametrize("b,n", [(2, 63), (2, 1), (1, 1), (1, 130)])
def test_fewer_points_than_a_wave_and_one_cloud(b, n):
    go, idx, w = _case(b, 24, 17, n, 5)
    _check(go, idx, w, 17)


def test_weights_with_exact_zeros():
    go, idx, w = _case(2, 12, 30, 400, 6, zero_weights=True)
    _check(go, idx, w, 30)


def test_the_largest_m_on_the_route_and_the_first_beyond_it():
    go, idx, w = _case(1, 8, LDS_MAX_M, 300, 7)
    _check(go, idx, w, LDS_MAX_M, route=2, cg=1)
    go, idx, w = _case(1, 8, LDS_MAX_M + 1, 300, 7)
    _check(go, idx, w, LDS_MAX_M + 1, route=1, cg=0, threads=0)  # the point-major atomics, as before


# b * ceil(c / cg) >= 256 workgroups decides cg below the cap of 16 and what fits; c = 1030: a last group of 2 channels
@pytest.mark.parametrize("b,c,m,n,cg", [(4, 1024, 3, 70, 16), (2, 1024, 5, 70, 8), (1, 1030, 5, 130, 4), (1, 512, 9, 70, 2),
                                        (1, 300, 40, 70, 1), (2, 300, 5000, 300, 2)])
def test_every_channel_group_the_dispatch_can_choose(b, c, m, n, cg):
    go, idx, w = _case(b, c, m, n, 8)
    _check(go, idx, w, m, cg=cg)


@pytest.mark.parametrize("n,threads", [(1023, 256), (1024, 512), (8191, 512), (8192, 1024)])
def test_every_workgroup_size(n, threads):
    go, idx, w = _case(1, 8, 300, n, 9)
    _check(go, idx, w, 300, threads=threads)


@pytest.mark.parametrize("cg,threads,c,n", [(3, 512, 10, 100), (5, 1024, 12, 3000), (16, 256, 8, 129), (2, 1024, 9, 100)])
def test_the_explicit_entry_at_configurations_the_dispatch_does_not_choose(cg, threads, c, n):
    ops, _lib, lib = _ops()
    b, m = 2, 37
    go, idx, w = _case(b, c, m, n, 10)
    want, sabs, cnt = _exact(go, idx, w, m)
    out = torch.full((b, c, m), float("nan"), device=DEV)
    _lib.check(lib.amc3d_three_interpolate_grad_lds(b, c, n, m, cg, threads, 0, _p(go), _p(idx), _p(w), _p(out), _stream()), "lds")
    assert bool(((out.double() - want).abs() <= 2 * (cnt + 1) * U * sabs).all())
    assert lib.amc3d_three_interpolate_grad_lds(b, c, n, m, cg, 384, 0, _p(go), _p(idx), _p(w), _p(out), _stream()) != 0
    assert lib.amc3d_three_interpolate_grad_lds(b, c, n, 40961, 1, 256, 0, _p(go), _p(idx), _p(w), _p(out), _stream()) != 0


def test_the_overwrite_entry_refuses_a_shape_of_another_route():
    ops, _lib, lib = _ops()
    go, idx, w = _case(1, 7, 10, 20, 11)
    out = torch.zeros(1, 7, 10, device=DEV)
    assert lib.amc3d_three_interpolate_grad_write(1, 7, 20, 10, _p(go), _p(idx), _p(w), _p(out), _stream()) != 0


def test_backward_through_ops_with_and_without_a_base():
    ops, _lib, lib = _ops()
    from amcontrast3d_amd import timing
    ops.set_deterministic(False)
    b, c, m, n = 2, 12, 40, 160
    go, idx, w = _case(b, c, m, n, 12)
    assert _route(lib, b, c, n, m)[0] == 2
    want, sabs, cnt = _exact(go, idx, w, m)
    f = torch.randn(b, c, m, device=DEV, requires_grad=True)
    base = torch.randn(b, c, n, device=DEV, requires_grad=True)
    y1 = ops.three_interpolate(f, idx, w)
    y2 = ops.three_interpolate_add(f, idx, w, base)
    with timing.count_calls() as calls:
        g1, = torch.autograd.grad(y1, f, go)
        g2, gb = torch.autograd.grad(y2, (f, base), go)
    assert calls["three_interpolate_grad"] == 2 and calls["three_interpolate_grad_csr"] == 0
    for g in (g1, g2):
        assert bool(((g.double() - want).abs() <= 2 * (cnt + 1) * U * sabs).all())
    assert torch.equal(gb, go)  # the gradient to base passes through untouched
