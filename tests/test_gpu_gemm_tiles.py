"""The tile family of gm_gemm_kernel (csrc/gemm.hip): every tile gives the bits of the 128 x 128 one.

amc3d_gemm_probe runs one product (forward, backward-data, generic weight gradient) with a forced tile; the cases sit on the
edges of the tiles -- fewer rows or columns than a tile, one more than a tile, positions that are no multiple of 4 (scalar
loads), a K tail chunk and a single chunk -- in the channel-major and the rows forms, with a strided unaligned weight view
(w + 3, ldw = cin + 3) and with the split-K branch.  All cases run once (module fixture); each test reads one list of findings.

The fp64 bound: an output element is a length-K chain of fp32 fused multiply-adds (split-K: shorter chains and their sum), whose
forward error is at most K * u * sum_k |a_k b_k| to first order with u = 2^-24; K counts every summed product (b * P for the
weight gradient).  One tile is held to it, the others inherit it by being bit-equal.
"""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -7.25
GUARD = 256
MS = (64, 72, 128, 130, 200)
PS = (1, 31, 63, 65, 129, 200)
KS = (16, 17, 40, 64, 136)
BS = (1, 3)
NTILES = 3
FORWARD, BACKWARD_DATA, WGRAD = 0, 1, 2


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def div_up(a, b):
    return (a + b - 1) // b


def deep(cin, cout):
    return cin >= 64 and cout >= 64


def wgrad_partials_bytes(b, cin, cout, P):
    """b * splits * cout * cin floats, splits as gemm_wgrad_splits (csrc/gemm.hip) counts them"""
    if P % 4 == 0 and P >= 128:
        tiles = div_up(cout, 128) * div_up(cin, 64 if cin <= 64 else 128)
        s = max(1, min(512 // (tiles * b), max(P // 128, 1)))
        per = div_up(div_up(P, s), 32) * 32
    else:
        tiles = div_up(cout, 128) * div_up(cin, 128)
        s = max(1, min(1024 // (tiles * b), max(P // 64, 1)))
        per = div_up(div_up(P, s), 16) * 16
    return 4 * b * div_up(P, per) * cout * cin


class Guarded:
    """n floats between two runs of GUARD sentinels; `offset` floats shift the payload off its 16-byte alignment"""

    def __init__(self, n, dev, offset=0):
        self.buf = torch.full((GUARD + offset + n + GUARD,), SENT, device=dev)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.view = self.buf[self.lo:self.hi]

    def dirty(self):
        """0-d bool tensor on the device: a guard float changed"""
        return (self.buf[:self.lo] != SENT).any() | (self.buf[self.hi:] != SENT).any()


class Run:
    def __init__(self, lib, dev):
        self.lib, self.dev = lib, dev
        self.gen = torch.Generator(device="cpu").manual_seed(7)
        self.tile_diff, self.public_diff, self.rows_diff, self.bound, self.status = [], [], [], [], []
        self.guard_dirty = torch.zeros((), dtype=torch.bool, device=dev)
        self.guard_cases = []
        self.ncases = self.npublic = 0

    def rand(self, *shape):
        return torch.randn(*shape, generator=self.gen).to(self.dev)

    def call(self, what, status):
        if status != 0:
            self.status.append((what, status))

    def probe(self, tile, product, b, cin, cout, P, ldw, pm, src, w, nout, ws_bytes, offset=0):
        out, ws = Guarded(nout, self.dev, offset), Guarded(div_up(ws_bytes, 4), self.dev)
        self.call(("probe", tile, product, b, cin, cout, P, pm),
                  self.lib.amc3d_gemm_probe(tile, product, b, cin, cout, P, ldw, pm, _p(src), _p(w), _p(out.view),
                                            _p(ws.view) if ws_bytes else None, ws_bytes, _s()))
        self.guard_dirty |= out.dirty() | ws.dirty()
        return out.view

    def weight(self, cout, cin, strided):
        """(cout, cin) weight: dense, or the feature block of a [W_dp | W_f] matrix: w + 3, ldw = cin + 3, never 16-byte aligned"""
        if not strided:
            w = self.rand(cout, cin)
            return w, w, cin
        base = self.rand(cout * (cin + 3) + 4)
        view = base[3:]
        return view, torch.as_strided(base, (cout, cin), (cin + 3, 1), 3), cin + 3

    def conv_case(self, product, b, M, P, K, strided, offsets=(0,)):
        lib = self.lib
        cin, cout = (K, M) if product == FORWARD else (M, K)
        wptr, wdense, ldw = self.weight(cout, cin, strided)
        src = self.rand(b, K, P)
        if product == FORWARD:
            wsb = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, 0))
        else:
            wsb = int(lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P)) if deep(cin, cout) else 0
        case = (("forward", "backward-data")[product], b, M, P, K, "strided" if strided else "dense")
        self.ncases += 1
        cm = [self.probe(t, product, b, cin, cout, P, ldw, 0, src, wptr, b * M * P, wsb).view(b, M, P) for t in range(NTILES)]
        for t in range(1, NTILES):
            if not torch.equal(cm[t], cm[0]):
                self.tile_diff.append(case + ("channel-major", t))
        for off in offsets:  # rows: 16-byte stores (M % 4 == 0, aligned) or 4-byte stores (M = 130, or the base moved by 4 bytes)
            rows = [self.probe(t, product, b, cin, cout, P, ldw, 1, src, wptr, b * M * P, wsb, off).view(b, P, M) for t in range(NTILES)]
            for t in range(1, NTILES):
                if not torch.equal(rows[t], rows[0]):
                    self.tile_diff.append(case + ("rows+%d" % off, t))
            if not torch.equal(rows[0].transpose(1, 2), cm[0]):
                self.rows_diff.append(case + (off,))
        # the public entries, where their routing reaches this kernel (deep layers; backward-data: these cases are all "short")
        if deep(cin, cout):
            self.npublic += 1
            y, ypm, ws = Guarded(b * M * P, self.dev), Guarded(b * M * P, self.dev), Guarded(div_up(wsb, 4), self.dev)
            wsp = _p(ws.view) if wsb else None
            if product == FORWARD:
                if strided:
                    self.call(case, lib.amc3d_pointwise_conv_forward_strided(b, cin, cout, P, _p(src), _p(wptr), ldw, None, _p(y.view),
                                                                             wsp, wsb, _s()))
                else:
                    self.call(case, lib.amc3d_pointwise_conv_forward_ws(b, cin, cout, P, _p(src), _p(wptr), None, _p(y.view), wsp, wsb,
                                                                        _s()))
                self.call(case, lib.amc3d_pointwise_conv_forward_rows(b, cin, cout, P, _p(src), _p(wptr), ldw, _p(ypm.view), wsp, wsb,
                                                                      _s()))
            else:
                if strided:
                    self.call(case, lib.amc3d_pointwise_conv_backward_strided(b, cin, cout, P, None, _p(wptr), ldw, _p(src), _p(y.view), 0,
                                                                              None, cin, wsp, wsb, _s()))
                else:
                    self.call(case, lib.amc3d_pointwise_conv_backward(b, cin, cout, P, None, _p(wptr), _p(src), _p(y.view), None, wsp,
                                                                      wsb, _s()))
                self.call(case, lib.amc3d_pointwise_conv_backward_strided(b, cin, cout, P, None, _p(wptr), ldw, _p(src), _p(ypm.view), 1,
                                                                          None, cin, wsp, wsb, _s()))
            self.guard_dirty |= y.dirty() | ypm.dirty() | ws.dirty()
            if not torch.equal(y.view.view(b, M, P), cm[0]):
                self.public_diff.append(case + ("channel-major",))
            if not torch.equal(ypm.view.view(b, P, M), rows[0]):
                self.public_diff.append(case + ("rows",))
        # fp64 on the CPU against the smallest tile
        a64 = wdense.double().cpu() if product == FORWARD else wdense.double().cpu().t()
        s64 = src.double().cpu()
        ref, mag = torch.matmul(a64, s64), torch.matmul(a64.abs(), s64.abs())
        err = (cm[NTILES - 1].double().cpu() - ref).abs()
        over = err - K * 2.0 ** -24 * mag
        if float(over.max()) > 0:
            self.bound.append(case + (float(err.max()), float(over.max())))

    def wgrad_case(self, b, cout, cin, P):
        lib = self.lib
        dy, x = self.rand(b, cout, P), self.rand(b, cin, P)
        wsb = wgrad_partials_bytes(b, cin, cout, P)
        if deep(cin, cout):
            wsb = max(wsb, int(lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P)))
        case = ("weight-grad", b, cout, cin, P)
        self.ncases += 1
        dw = [self.probe(t, WGRAD, b, cin, cout, P, cin, 0, dy, x, cout * cin, wsb).view(cout, cin) for t in range(NTILES)]
        for t in range(1, NTILES):
            if not torch.equal(dw[t], dw[0]):
                self.tile_diff.append(case + (t,))
        if deep(cin, cout) and not (P % 4 == 0 and P >= 128):  # the public entry's generic branch
            self.npublic += 1
            out, ws = Guarded(cout * cin, self.dev), Guarded(div_up(wsb, 4), self.dev)
            self.call(case, lib.amc3d_pointwise_conv_backward(b, cin, cout, P, _p(x), None, _p(dy), None, _p(out.view), _p(ws.view), wsb,
                                                              _s()))
            self.guard_dirty |= out.dirty() | ws.dirty()
            if not torch.equal(out.view.view(cout, cin), dw[0]):
                self.public_diff.append(case)
        d64, x64 = dy.double().cpu(), x.double().cpu()
        ref = torch.einsum("bmp,bnp->mn", d64, x64)
        mag = torch.einsum("bmp,bnp->mn", d64.abs(), x64.abs())
        err = (dw[NTILES - 1].double().cpu() - ref).abs()
        over = err - b * P * 2.0 ** -24 * mag
        if float(over.max()) > 0:
            self.bound.append(case + (float(err.max()), float(over.max())))


@pytest.fixture(scope="module")
def run():
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    r = Run(lib, dev)
    with torch.cuda.device(dev):
        for b, M, P, K in itertools.product(BS, MS, PS, KS):
            strided = b == 3  # the [W_dp | W_f] view: vec_a == 0
            offsets = (0, 1) if K == 40 else (0,)  # K = 40: the rows once more with the output base moved by 4 bytes
            r.conv_case(FORWARD, b, M, P, K, strided, offsets)
            r.conv_case(BACKWARD_DATA, b, M, P, K, strided, offsets)
            r.wgrad_case(b, M, P, K)  # cout = M, cin from the column sizes, positions from the K sizes
        # the split-K branch: 256 x 256 channels on 2 x 94 positions, partials in a workspace of exactly *_workspace_bytes
        assert int(lib.amc3d_pointwise_conv_forward_workspace_bytes(2, 256, 256, 94, 0)) == 4 * 2 * 4 * 256 * 94
        assert int(lib.amc3d_pointwise_conv_workspace_bytes(2, 256, 256, 94)) == 4 * 2 * 4 * 256 * 94
        for strided in (False, True):
            r.conv_case(FORWARD, 2, 256, 94, 256, strided, (0, 1))
            r.conv_case(BACKWARD_DATA, 2, 256, 94, 256, strided, (0, 1))
        r.wgrad_case(2, 256, 256, 94)
        torch.cuda.synchronize()
    return r


def test_cases_ran(run):
    assert not run.status, run.status[:5]
    assert run.ncases == 3 * len(BS) * len(MS) * len(PS) * len(KS) + 5
    assert run.npublic > 100  # the deep ones also went through the public entries


def test_every_tile_gives_the_bits_of_128x128(run):
    assert not run.tile_diff, (len(run.tile_diff), run.tile_diff[:8])
    assert not run.rows_diff, (len(run.rows_diff), run.rows_diff[:8])  # rows == channel-major transposed


def test_probe_128x128_equals_the_public_entries(run):
    assert not run.public_diff, (len(run.public_diff), run.public_diff[:8])


def test_fp64_bound(run):
    """|err| <= K * 2^-24 * (|A| . |B|) per element, smallest tile against fp64 matmul on the CPU"""
    assert not run.bound, (len(run.bound), run.bound[:8])


def test_memory_around_output_and_workspace_is_untouched(run):
    """256 sentinel floats before and after every output and every workspace of every case above -- among them P = 1, M = 64
    with tile 128 x 128 and M = 130 with tile 64 x 64 -- are unchanged"""
    assert not bool(run.guard_dirty)


def test_rule_is_a_function_of_its_arguments_and_holds_under_capture():
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    args = list(itertools.product((64, 130, 256, 512), (1, 94, 1500, 6000, 24000), (1, 8), (1, 4)))
    first = [lib.amc3d_gemm_tile_for(*a) for a in args]
    assert first == [lib.amc3d_gemm_tile_for(*a) for a in args]
    assert all(0 <= t < NTILES for t in first)
    assert lib.amc3d_gemm_tile_for(0, 5, 1, 1) == -1
    # a forward whose launch takes the 64 x 64 tile: eager, then captured and replayed twice
    b, cin, cout, P = 1, 64, 64, 200
    assert lib.amc3d_gemm_tile_for(cout, P, b, 1) == 2
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(b, cin, P, generator=g).to(dev), torch.randn(cout, cin, generator=g).to(dev)
    eager, y = torch.empty(b, cout, P, device=dev), torch.zeros(b, cout, P, device=dev)
    with torch.cuda.device(dev):
        assert lib.amc3d_pointwise_conv_forward_ws(b, cin, cout, P, _p(x), _p(w), None, _p(eager), None, 0, _s()) == 0
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                captured_choice = lib.amc3d_gemm_tile_for(cout, P, b, 1)
                assert lib.amc3d_pointwise_conv_forward_ws(b, cin, cout, P, _p(x), _p(w), None, _p(y), None, 0, _s()) == 0
        assert captured_choice == 2
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
    probe = torch.empty(b, cout, P, device=dev)
    assert lib.amc3d_gemm_probe(0, FORWARD, b, cin, cout, P, cin, 0, _p(x), _p(w), _p(probe), None, 0, _s()) == 0
    assert torch.equal(probe, eager)


@pytest.mark.parametrize("b,P", [(0, 8), (2, 0)])
def test_empty_call_returns_zero_and_writes_nothing(b, P):
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    out = torch.full((4096,), SENT, device=dev)
    a, w = torch.ones(4096, device=dev), torch.ones(4096, device=dev)
    for product in (FORWARD, BACKWARD_DATA, WGRAD):
        for tile in range(NTILES):
            assert lib.amc3d_gemm_probe(tile, product, b, 16, 16, P, 16, 0, _p(a), _p(w), _p(out), _p(a), 4096 * 4, _s()) == 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
