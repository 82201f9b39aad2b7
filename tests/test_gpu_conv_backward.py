"""Backward of the 1x1 convolutions (csrc/pwconv.hip, csrc/gemm.hip) in the forms the training step uses them: dx written
as position-major rows for the reverse-list gather of GroupedConvBN, weights and weight gradients addressed as column blocks
of a wider matrix, repeated and captured calls.  torch's conv in fp64 is the arbiter, with the bound of test_gpu_pwconv.py:
err <= max(4 x the error of torch's own fp32 conv, 2e-6 x scale), for y, dx, dw and db."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B, Cin, Cout, spatial, bias, dx requested, dx as position-major rows
CASES = {
    1: (2, 4, 32, (1000,), False, False, False),     # dx not requested (the stem)
    2: (2, 32, 13, (777,), True, True, False),       # bias; P % 4 != 0; ragged Cout
    3: (1, 1, 1, (5,), True, True, False),
    4: (3, 96, 32, (200,), False, True, False),      # two k-chunks; a workgroup's tile run crosses cloud boundaries
    5: (2, 64, 64, (129,), False, True, False),      # deep family; one position past a tile
    6: (2, 96, 200, (1000,), False, True, False),    # ragged channel counts
    7: (2, 64, 128, (300, 32), False, True, True),   # rows from the tiled GEMM, K split over workgroups
    8: (1, 128, 256, (100, 32), False, True, True),
    9: (3, 32, 64, (23, 32), False, True, True),     # rows from the streaming kernel
    # the routes SA2 and SA3 of PointNeXt-S take at full size (enough tiles that nothing is split), and rows whose width is
    # no multiple of 4 (4-byte stores)
    10: (2, 64, 128, (384, 32), False, True, True),  # streaming kernel, two 32-channel accumulators per wave
    11: (2, 128, 256, (384, 32), False, True, True),  # tiled GEMM, one pass over K
    12: (2, 35, 64, (23, 32), False, True, True),
}


def _inputs(case, seed=0):
    B, Cin, Cout, spatial, bias, _, _ = CASES[case]
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + 7919 * seed)
    x = torch.randn(B, Cin, *spatial, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, *([1] * len(spatial)), generator=g) * 0.1).to(DEV)
    bvec = torch.randn(Cout, generator=g).to(DEV) if bias else None
    go = torch.randn(B, Cout, *spatial, generator=g).to(DEV)
    return x, w, bvec, go


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(fp64 results, fp32 results of torch's conv) as (y, dx, dw, db), computed once per case and left unchanged"""
    x, w, bvec, go = _inputs(case)
    conv = F.conv1d if x.dim() == 3 else F.conv2d

    def ref(dtype):
        xr, wr = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
        br = bvec.to(dtype).requires_grad_(True) if bvec is not None else None
        y = conv(xr, wr, br)
        y.backward(go.to(dtype))
        return y.detach(), xr.grad, wr.grad, (br.grad if br is not None else None)

    return ref(torch.float64), ref(torch.float32)


def _run(case, inputs=None, rows=None):
    """one forward + backward through ops.pointwise_conv -> (y, dx, dw, db); absent gradients are None"""
    from amcontrast3d_amd import ops
    _, _, _, _, bias, need_x, pm = CASES[case]
    x, w, bvec, go = inputs if inputs is not None else _inputs(case)
    xg = x.detach().requires_grad_(need_x)
    wg = w.detach().requires_grad_(True)
    bg = bvec.detach().requires_grad_(True) if bias else None
    y = ops.pointwise_conv(xg, wg, bg, False, pm if rows is None else rows)
    wanted = [t for t in (xg if need_x else None, wg, bg) if t is not None]
    grads = list(torch.autograd.grad(y, wanted, go))
    dx = grads.pop(0) if need_x else None
    dw = grads.pop(0)
    db = grads.pop(0) if bias else None
    return y.detach(), dx, dw, db


def _check_against_fp64(case, got):
    r64, r32 = _reference(case)
    for a, b64, b32, what in zip(got, r64, r32, ("y", "dx", "dw", "db")):
        if a is None:
            assert what in ("dx", "db"), what
            continue
        assert a.shape == b64.shape, what
        err = float((a.double() - b64).abs().max())
        err_torch = float((b32.double() - b64).abs().max())
        scale = max(1.0, float(b64.abs().max()))
        print(f"case {case} {what}: err {err:.3e} torch fp32 {err_torch:.3e} scale {scale:.3e}")
        assert err <= max(4 * err_torch, 2e-6 * scale), (what, err, err_torch, scale)


def _is_rows(dx):
    """dx (B,C,*spatial) is a view of a contiguous (B,*spatial,C) buffer"""
    return dx.permute(0, *range(2, dx.dim()), 1).is_contiguous()


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv_backward_matches_fp64(case):
    got = _run(case)
    need_x, pm = CASES[case][5], CASES[case][6]
    assert (got[1] is not None) == need_x
    if pm:
        assert _is_rows(got[1]), got[1].stride()
    _check_against_fp64(case, got)


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c][6]])
def test_position_major_dx_is_the_channel_major_dx(case):
    """the accumulators are the same, only the store differs: bit-equal values, and nothing else of the call changes"""
    rows, plain = _run(case, rows=True), _run(case, rows=False)
    assert _is_rows(rows[1]) and plain[1].is_contiguous()
    assert torch.equal(rows[1], plain[1])
    assert torch.equal(rows[0], plain[0]) and torch.equal(rows[2], plain[2])
    # as GroupedConvBN.backward recognises it
    assert rows[1].dim() == 4 and rows[1].permute(0, 2, 3, 1).is_contiguous()


def test_library_gemm_conv_position_major_dx():
    """the three-GEMM route of the short deep layers (SA4): dx = dy^T . W as rows, a different library product than the
    channel-major one -- held to the fp64 bound, not to bit-equality"""
    from amcontrast3d_amd import ops
    x, w, _, go = _inputs(8)
    out = []
    for rows in (True, False):
        xg, wg = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
        y = ops.library_gemm_conv(xg, wg, rows)
        dx, dw = torch.autograd.grad(y, (xg, wg), go)
        out.append((y.detach(), dx, dw, None))
    assert _is_rows(out[0][1]) and out[0][1].permute(0, 2, 3, 1).is_contiguous() and out[1][1].is_contiguous()
    _check_against_fp64(8, out[0])
    _check_against_fp64(8, out[1])


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# rows, c1, c2, B, P: weight (rows, c1 + c2); the blocks [0, c1) and [c1, c1 + c2) are used where they lie
STRIDED = [
    (32, 3, 32, 2, 777),     # [W_dp | W_f]: the block starts at column 3 (not 16-byte aligned), odd row stride
    (32, 32, 64, 2, 1000),   # [W_skip | W_up] split at 32
    (128, 64, 64, 2, 640),   # both sides >= 64 channels: the tiled GEMM and the streaming weight-gradient kernel
]


@pytest.mark.parametrize("rows,c1,c2,B,P", STRIDED)
def test_strided_weight_blocks(rows, c1, c2, B, P):
    """forward, dx and a dw written into the wide matrix equal the computation on contiguous copies bit for bit, and the
    columns a call does not own keep their sentinel"""
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + c1)
    wide = (torch.randn(rows, c1 + c2, generator=g) * 0.1).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    SENTINEL = -12345.5
    for lo, cin in ((0, c1), (c1, c2)):
        if cin == 3:
            continue  # the dp columns belong to the neighbourhood kernels
        x = torch.randn(B, cin, P, generator=g).to(DEV)
        dy = torch.randn(B, rows, P, generator=g).to(DEV)
        block = wide[:, lo:lo + cin]
        copy = block.contiguous()
        wsf = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(B, cin, rows, P, 0))
        wb = int(lib.amc3d_pointwise_conv_workspace_bytes(B, cin, rows, P))
        work = torch.empty(max(wsf, wb, 4), dtype=torch.uint8, device=DEV)
        y0, y1 = torch.empty(B, rows, P, device=DEV), torch.empty(B, rows, P, device=DEV)
        _lib.check(lib.amc3d_pointwise_conv_forward_ws(B, cin, rows, P, _vp(x), _vp(copy), None, _vp(y0), _vp(work), wsf, stream), "fwd")
        _lib.check(lib.amc3d_pointwise_conv_forward_strided(B, cin, rows, P, _vp(x), _vp(block), c1 + c2, None, _vp(y1), _vp(work),
                                                            wsf, stream), "fwd strided")
        assert torch.equal(y0, y1)
        dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
        dw0 = torch.empty(rows, cin, device=DEV)
        dwide = torch.full((rows, c1 + c2), SENTINEL, device=DEV)
        _lib.check(lib.amc3d_pointwise_conv_backward(B, cin, rows, P, _vp(x), _vp(copy), _vp(dy), _vp(dx0), _vp(dw0), _vp(work), wb,
                                                     stream), "bwd")
        _lib.check(lib.amc3d_pointwise_conv_backward_strided(B, cin, rows, P, _vp(x), _vp(block), c1 + c2, _vp(dy), _vp(dx1), 0,
                                                             _vp(dwide[:, lo:]), c1 + c2, _vp(work), wb, stream), "bwd strided")
        assert torch.equal(dx0, dx1)
        assert torch.equal(dwide[:, lo:lo + cin], dw0)
        other = torch.cat((dwide[:, :lo], dwide[:, lo + cin:]), 1)
        assert bool((other == SENTINEL).all())


def test_split_weight_views_feed_the_convs():
    """ops.split_weight hands out the two column blocks without a copy; the conv on such a view and its gradients equal
    those on a contiguous copy bit for bit, and the gradient of the whole weight is the two halves side by side"""
    from amcontrast3d_amd import ops
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(32, 96, 1, generator=g) * 0.1).to(DEV).requires_grad_(True)
    f1, f2 = torch.randn(2, 32, 1000, generator=g).to(DEV), torch.randn(2, 64, 1000, generator=g).to(DEV)
    go = torch.randn(2, 32, 1000, generator=g).to(DEV)
    w1, w2 = ops.split_weight(w, 32)
    assert w1.data_ptr() == w.data_ptr() and w2.data_ptr() == w.data_ptr() + 4 * 32 and w2.stride(0) == 96
    y = ops.pointwise_conv(f1, w1.reshape(32, 32, 1)) + ops.pointwise_conv(f2, w2.reshape(32, 64, 1))
    y.backward(go)
    c1 = w.detach()[:, :32].clone().requires_grad_(True)
    c2 = w.detach()[:, 32:].clone().requires_grad_(True)
    yc = ops.pointwise_conv(f1, c1) + ops.pointwise_conv(f2, c2)
    yc.backward(go)
    assert torch.equal(y, yc)
    assert torch.equal(w.grad, torch.cat((c1.grad, c2.grad), 1))


@pytest.mark.parametrize("case", [2, 4, 5])
def test_repeated_backward_is_bit_equal(case):
    runs = [_run(case) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(runs[0][2], r[2])
        if runs[0][3] is not None:
            assert torch.equal(runs[0][3], r[3])


@pytest.mark.parametrize("case", [4, 7])
def test_captured_backward_replays_bit_equal(case):
    """forward + backward captured on a side stream, replayed with the inputs overwritten in between: every replay equals the
    eager result on the same inputs (no state survives a call)"""
    sets = [_inputs(case, seed) for seed in (1, 2)]
    eager = [_run(case, s) for s in sets]
    static = [t.clone() if t is not None else None for t in _inputs(case, 3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(case, static)  # allocations and one-time attributes before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _run(case, static)
    for inputs, want in list(zip(sets, eager)) + [(sets[0], eager[0])]:
        for dst, src in zip(static, inputs):
            if dst is not None:
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b)


def _layer_case(Cin, C, seed):
    from amcontrast3d_amd import ops
    B, N, M, K = 2, 512, 128, 32
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, N, 3, generator=g).to(DEV)
    q = p[:, :M].contiguous()
    idx = ops.ball_query(0.35, K, p, q)
    dp = ((ops.grouping_operation(p.transpose(1, 2).contiguous(), idx) - q.transpose(1, 2).unsqueeze(-1)) / 0.35).contiguous()
    f = torch.randn(B, Cin, N, generator=g).to(DEV)
    w = (torch.randn(C, Cin + 3, 1, 1, generator=g) * 0.3).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    return B, N, M, K, idx, dp, f, w, gamma, beta, g


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("layer", ["local_aggregation", "grouped_conv_bn", "grouped_conv_bn_csr"])
def test_neighbourhood_layers_use_the_weight_in_place(layer, C, monkeypatch):
    """LocalAggregationFused and GroupedConvBN read [W_dp | W_f] where it lies and write both gradient blocks into one matrix:
    output and every gradient equal, bit for bit, the layer composed from amc3d_split_columns / amc3d_join_columns"""
    from amcontrast3d_amd import ops
    B, N, M, K, idx, dp, f, w, gamma, beta, g = _layer_case(C, C, 100 + C)
    mom = ops.group_moments(idx, dp, N)
    csr = None
    if layer == "grouped_conv_bn_csr":
        start, edge = ops.group_csr(idx, N)
        csr = (start, edge, ops.group_csr_dp(idx, dp, edge))
    go = torch.randn((B, C, M) if layer == "local_aggregation" else (B, C, M, K), generator=g).to(DEV)

    def run():
        fr, wr, gr, br = (t.clone().requires_grad_(True) for t in (f, w, gamma, beta))
        if layer == "local_aggregation":
            out = ops.LocalAggregationFused.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, None)
        else:
            out = ops.GroupedConvBN.apply(fr, dp, idx, mom, wr, gr, br, 1e-5, True, None, csr)
        out.backward(go)
        return out.detach(), fr.grad, wr.grad, gr.grad, br.grad

    in_place = run()
    blocks, grads = ops._dp_f_blocks, ops._dp_f_grad
    calls = []
    monkeypatch.setattr(ops, "_dp_f_blocks", lambda w2, bf16: (calls.append("split"), blocks(w2, True))[1])
    monkeypatch.setattr(ops, "_dp_f_grad", lambda C_, Cin_, dev, bf16: (calls.append("join"), grads(C_, Cin_, dev, True))[1])
    composed = run()
    assert calls == ["split", "join"]
    for name, a, b in zip(("out", "df", "dw", "dgamma", "dbeta"), in_place, composed):
        if layer != "grouped_conv_bn_csr" and name != "out":
            # without reverse lists the backward of both layers scatters with float atomics: two runs of one form agree
            # only to rounding, so the two forms can do no better (the reverse-list form, which training uses, is exact)
            assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max())), name
        else:
            assert torch.equal(a, b), name
