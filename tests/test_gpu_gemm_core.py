"""The K walk of gm_gemm_kernel (csrc/gemm.hip): every k counted once on every edge of a stage, and the order of the sum.

A stage of the walk is 32 k deep, consumed as two chunks of 16; a K range (all of K, or one split of it) may begin and end in the
middle of a stage.  The cases sit on those edges: K-side channel counts around 64 / 80 / 96, 136 (split in two ranges of 80
and 56: kper is an odd multiple of 16) and 200 (three ranges of 80 / 80 / 40), weight-gradient positions around 16 / 32 / 48
and 200, rows 64 / 72 / 130, one and three clouds, positions that are no multiple of 4 (scalar loads), the unaligned strided weight
view (w + 3, ldw = cin + 3) with three clouds, the channel-major output and the rows with 16-byte and with 4-byte stores.
amc3d_gemm_probe forces every tile; the public entries take the rule's choice.

1. Integers in [-8, 8] as fp32: every partial sum stays below 2^24 (at most 64 * 600), so every order of the sum gives the same
   exact result, and the outputs must equal torch.matmul in fp64 on the CPU.
2. Uniform [-1, 1) operands from numpy.random.default_rng(1000 + case index): the outputs must have the bits that the kernel
   had before the rework, recorded in tests/golden/gemm_core_parent.npz by tools/record_gemm_golden.py from a library built
   from the parent commit (never from the code under test): a SHA-256 of the output bytes and the first 64 values per output.
   The contract behind it: an output element is an fp32 fmaf chain from 0 over its K range in chunks of 16 ascending, inside a
   chunk in the order 0, 8, 1, 9, ..., 7, 15; split ranges are chains of their own, summed afterwards in a fixed order.

All cases run once (module fixture); each test reads one list of findings.  256 sentinel floats lie before and after every
output and every workspace.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_core_parent.npz")
SENT = -7.25
GUARD = 256
NTILES = 3
FORWARD, BACKWARD_DATA, WGRAD = 0, 1, 2
KS = (64, 65, 79, 80, 81, 95, 96, 97, 136)          # channels on the K side of the conv products (N of the weight gradient)
PS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 200)   # positions: N of the conv products, K of the weight gradient
MS = (64, 72, 130)
BS = (1, 3)


def cases():
    """(product, b, M, P, K-side channels, strided), as tools/record_gemm_golden.py lists them"""
    out, i = [], 0
    for K in KS:
        for M in MS:
            for b in BS:
                for product in (FORWARD, BACKWARD_DATA):
                    out.append((product, b, M, PS[i % len(PS)], K, int(b == 3)))
                    i += 1
    for P in PS:
        for M in MS:
            for b in BS:
                out.append((WGRAD, b, M, P, KS[i % len(KS)], 0))
                i += 1
    for product in (FORWARD, BACKWARD_DATA):
        out += [(product, 2, 256, 94, 256, 0), (product, 2, 256, 94, 256, 1), (product, 1, 130, 33, 200, 0)]
    return out


def operands(case, seed, integers):
    product, b, M, P, K, _ = case
    rng = np.random.default_rng(seed)
    if integers:
        u = lambda *s: rng.integers(-8, 9, size=s).astype(np.float32)  # noqa: E731
    else:
        u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)  # noqa: E731
    if product == WGRAD:
        return u(b, M, P), u(b, K, P)          # dy (b, cout, P), x (b, cin, P)
    cin, cout = (K, M) if product == FORWARD else (M, K)
    return u(cout, cin), u(b, K, P)            # w, x or dy


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def div_up(a, b):
    return (a + b - 1) // b


def short_splits(b, M, N, K):
    """gemm_short_splits of csrc/gemm.hip"""
    tiles = div_up(M, 128) * div_up(N, 128) * b
    if tiles >= 192 or K < 128:
        return 1
    s = min(512 // tiles, 8, K // 64)
    return 1 if s < 2 else s


def wgrad_splits(b, cin, cout, P):
    """gemm_wgrad_splits of csrc/gemm.hip: (splits, kper)"""
    if P % 4 == 0 and P >= 128:
        tiles = div_up(cout, 128) * div_up(cin, 64 if cin <= 64 else 128)
        s = max(1, min(512 // (tiles * b), max(P // 128, 1)))
        per = div_up(div_up(P, s), 32) * 32
    else:
        tiles = div_up(cout, 128) * div_up(cin, 128)
        s = max(1, min(1024 // (tiles * b), max(P // 64, 1)))
        per = div_up(div_up(P, s), 16) * 16
    return div_up(P, per), per


class Guarded:
    """n floats between two runs of GUARD sentinels; `offset` floats shift the payload off its 16-byte alignment"""

    def __init__(self, n, dev, offset=0):
        self.buf = torch.full((GUARD + offset + n + GUARD,), SENT, device=dev)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.view = self.buf[self.lo:self.hi]

    def dirty(self):
        return (self.buf[:self.lo] != SENT).any() | (self.buf[self.hi:] != SENT).any()


class Run:
    def __init__(self, lib, dev, golden):
        self.lib, self.dev = lib, dev
        self.sha = dict(zip(golden["names"].tolist(), golden["sha256"].tolist()))
        self.head = dict(zip(golden["names"].tolist(), golden["head"]))
        self.status, self.exact_diff, self.order_diff, self.public_diff = [], [], [], []
        self.tile_diff = torch.zeros((), dtype=torch.bool, device=dev)   # some tile != the 128 x 128 one, some rows != transposed
        self.guard_dirty = torch.zeros((), dtype=torch.bool, device=dev)
        self.odd_kper_ranges = self.npublic = self.noutputs = 0

    def call(self, what, status):
        if status != 0:
            self.status.append((what, status))

    def probe(self, tile, product, b, cin, cout, P, ldw, pm, src, other, nout, wsb, offset=0):
        out, ws = Guarded(nout, self.dev, offset), Guarded(div_up(wsb, 4), self.dev)
        self.call(("probe", tile, product, b, cin, cout, P, pm),
                  self.lib.amc3d_gemm_probe(tile, product, b, cin, cout, P, ldw, pm, _p(src), _p(other), _p(out.view),
                                            _p(ws.view) if wsb else None, wsb, _s()))
        self.guard_dirty |= out.dirty() | ws.dirty()
        return out.view

    def tiles(self, *args, **kw):
        """the output of the 128 x 128 tile; the other tiles must equal it"""
        outs = [self.probe(t, *args, **kw) for t in range(NTILES)]
        for o in outs[1:]:
            self.tile_diff |= (o != outs[0]).any()
        self.noutputs += NTILES
        return outs[0]

    def case(self, i, case, integers):
        lib, dev = self.lib, self.dev
        product, b, M, P, K, strided = case
        first_h, second_h = operands(case, 1000 + i, integers)
        first, second = torch.from_numpy(first_h).to(dev), torch.from_numpy(second_h).to(dev)
        found = {}
        if product == WGRAD:
            cout, cin = M, K
            wsb = int(lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P))
            splits, kper = wgrad_splits(b, cin, cout, P)
            assert wsb >= 4 * b * splits * cout * cin
            found["0"] = self.tiles(WGRAD, b, cin, cout, P, cin, 0, first, second, cout * cin, wsb)
            if not (P % 4 == 0 and P >= 128):  # the public entry's generic branch
                self.npublic += 1
                out, ws = Guarded(cout * cin, dev), Guarded(div_up(wsb, 4), dev)
                self.call(case, lib.amc3d_pointwise_conv_backward(b, cin, cout, P, _p(second), None, _p(first), None, _p(out.view),
                                                                  _p(ws.view), wsb, _s()))
                self.guard_dirty |= out.dirty() | ws.dirty()
                found["public 0"] = out.view
            ref = torch.einsum("bmp,bnp->mn", torch.from_numpy(first_h).double(), torch.from_numpy(second_h).double()) if integers else None
        else:
            cin, cout = (K, M) if product == FORWARD else (M, K)
            ldw = cin + 3 * strided
            wptr = first
            if strided:  # the feature block of a [W_dp | W_f] matrix: never 16-byte aligned
                base = torch.zeros(cout * ldw + 4, device=dev)
                torch.as_strided(base, (cout, cin), (ldw, 1), 3).copy_(first)
                wptr = base[3:]
            wsb = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, 0) if product == FORWARD
                      else lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P))
            splits = short_splits(b, M, P, K)
            assert (wsb >= 4 * b * splits * M * P) if splits > 1 else True
            kper = K if splits == 1 else div_up(div_up(K, splits), 16) * 16
            n = b * M * P
            cm = found["0"] = self.tiles(product, b, cin, cout, P, ldw, 0, second, wptr, n, wsb)
            rows = found["1"] = self.tiles(product, b, cin, cout, P, ldw, 1, second, wptr, n, wsb)            # 16-byte stores if M % 4 == 0
            rows4 = self.tiles(product, b, cin, cout, P, ldw, 1, second, wptr, n, wsb, offset=1)               # 4-byte stores
            self.tile_diff |= (rows != rows4).any() | (rows.view(b, P, M).transpose(1, 2) != cm.view(b, M, P)).any()
            self.npublic += 1
            y, ypm, ws = Guarded(n, dev), Guarded(n, dev), Guarded(div_up(wsb, 4), dev)
            wsp = _p(ws.view) if wsb else None
            if product == FORWARD:
                self.call(case, lib.amc3d_pointwise_conv_forward_strided(b, cin, cout, P, _p(second), _p(wptr), ldw, None, _p(y.view), wsp,
                                                                         wsb, _s()))
                self.call(case, lib.amc3d_pointwise_conv_forward_rows(b, cin, cout, P, _p(second), _p(wptr), ldw, _p(ypm.view), wsp, wsb,
                                                                      _s()))
            else:
                for pm, o in ((0, y), (1, ypm)):
                    self.call(case, lib.amc3d_pointwise_conv_backward_strided(b, cin, cout, P, None, _p(wptr), ldw, _p(second), _p(o.view),
                                                                              pm, None, cin, wsp, wsb, _s()))
            self.guard_dirty |= y.dirty() | ypm.dirty() | ws.dirty()
            found["public 0"], found["public 1"] = y.view, ypm.view
            if integers:
                w64 = torch.from_numpy(first_h).double()
                ref = torch.matmul(w64 if product == FORWARD else w64.t(), torch.from_numpy(second_h).double())
        if splits > 1 and (kper // 16) % 2 == 1:
            self.odd_kper_ranges += 1
        for name, t in found.items():
            pm = name[-1]
            host = t.cpu()
            if integers:
                want = ref if pm == "0" or product == WGRAD else ref.transpose(1, 2).contiguous()
                if not torch.equal(host.double().view(want.shape), want):
                    self.exact_diff.append((i, case, name, float((host.double().view(want.shape) - want).abs().max())))
            else:
                key, raw = f"{i}:{pm}", host.numpy()
                if hashlib.sha256(raw.tobytes()).hexdigest() != self.sha[key] or raw[:64].tobytes() != self.head[key].tobytes():
                    (self.public_diff if name.startswith("public") else self.order_diff).append(
                        (i, case, name, raw[:4].tolist(), self.head[key][:4].tolist()))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def run(golden):
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    r = Run(lib, dev, golden)
    with torch.cuda.device(dev):
        for integers in (True, False):
            for i, case in enumerate(cases()):
                r.case(i, case, integers)
        torch.cuda.synchronize()
    return r


def test_fixture_lists_these_cases(golden):
    assert golden["cases"].tolist() == [list(c) for c in cases()]
    assert len(golden["sha256"]) == len(golden["names"]) == len(golden["head"])


def test_cases_ran(run):
    assert not run.status, run.status[:5]
    assert run.npublic > 2 * 150
    assert run.odd_kper_ranges == 2 * 14  # K ranges that begin and end in the middle of a 32-k stage, integers and uniform


def test_integer_operands_are_summed_exactly(run):
    """every k counted once: torch.equal to fp64 matmul on the CPU, every tile, every product, probe and public entries"""
    assert not run.exact_diff, (len(run.exact_diff), run.exact_diff[:6])
    assert not bool(run.tile_diff)  # every tile the bits of 128 x 128; rows == channel-major transposed, 16- and 4-byte stores


def test_order_of_the_sum_is_the_parents(run):
    """bit-equal to the fixture recorded from the parent commit's library"""
    assert not run.order_diff, (len(run.order_diff), run.order_diff[:6])


def test_public_entries_give_the_parents_bits(run):
    assert not run.public_diff, (len(run.public_diff), run.public_diff[:6])


def test_memory_around_outputs_and_workspaces_is_untouched(run):
    assert not bool(run.guard_dirty)
