"""Point operators on MI355X: torch.autograd front-ends over the C-ABI (include/amc3d.h).

These mirror, name for name, the reference's Python wrappers of its CUDA
extensions (argument meaning, dtypes, shapes, contiguity asserts, outputs):

    ball_query, grouping_operation, gather_operation   openpoints/models/layers/group.py:76-203
    furthest_point_sample                               openpoints/models/layers/subsample.py:76-106
    three_nn, three_interpolate, three_interpolation    openpoints/models/layers/upsampling.py:11-102
    knnquery                                            openpoints/cpp/pointops/functions/pointops.py:32-56

PyTorch is only plumbing here (device memory, the current HIP stream, autograd
bookkeeping); every operator runs a hand-written gfx950 kernel.  CPU tensors are
rejected: there is no fallback path.
"""
import ctypes
from types import SimpleNamespace

import torch
from torch.autograd import Function

from . import _lib, timing


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


_dedicated = []  # (handle, ExternalStream): kept alive for the life of the process


def _destroy_dedicated():
    if not _dedicated:
        return
    try:
        torch.cuda.synchronize()
        for handle, _ in _dedicated:
            _lib.load().amc3d_stream_destroy(handle)
    finally:
        _dedicated.clear()


def dedicated_stream(device=None, first_cu=0, n_cus=0):
    """A torch stream with a hardware queue of its own (amc3d_stream_create_dedicated): for the FPS launches of a
    pipelined loop, which otherwise stall whichever stream shares their queue for milliseconds.  n_cus > 0 restricts
    the stream's kernels to the CUs [first_cu, first_cu + n_cus) of the mask."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    handle = ctypes.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amc3d_stream_create_masked(ctypes.byref(handle), int(first_cu), int(n_cus)),
                   "stream_create_masked")
    s = torch.cuda.ExternalStream(handle.value, device=dev)
    if not _dedicated:
        import atexit
        atexit.register(_destroy_dedicated)
    _dedicated.append((handle, s))
    return s


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("amcontrast3d_amd operators run on the GPU only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)


_deterministic = False


def deterministic():
    """True while deterministic mode is on: no kernel that adds floats with atomics is launched, so a train step on one GPU
    is a pure function of its inputs (same bits on every run).  An operator then takes an atomic-free route -- the
    reverse-list gathers of csrc/csr.hip and the *_csr entries, this library's fixed-order GEMMs instead of the BLAS
    library -- or raises RuntimeError("<op>: no deterministic route ..."); it never falls back silently.  Integer and
    fixed-point atomics are independent of their order and stay.  Off by default; the default routes do not change."""
    return _deterministic


def set_deterministic(flag):
    """switch deterministic mode on or off for the whole process"""
    global _deterministic
    _deterministic = bool(flag)


class deterministic_mode:
    """with deterministic_mode(flag=True): the mode set for the block, the previous state restored on leaving it.  Autograd
    runs backward outside the block of forward: every Function records the mode it was built under (ctx.det) and its
    backward honours that record, not the mode at the time backward runs."""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = deterministic()
        set_deterministic(self.flag)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


def _no_route(op, why):
    return RuntimeError(f"{op}: no deterministic route ({why}); see amcontrast3d_amd.ops.deterministic")


def mixed_precision():
    """True inside torch.autocast('cuda', dtype=torch.bfloat16): the pointwise convolutions then run in bf16 compute /
    fp32 accumulate (csrc/gemm_bf16.hip) while every tensor stays fp32 in memory (main_AA.py:389-394 use_amp)"""
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


def _pw_forward(lib, bf16, B, Cin, Cout, P, x, w2, bias, y, what="pointwise_conv_forward"):
    """y = w2 . x (+ bias) through the fp32 or bf16-compute kernels; the fp32 short deep layers get scratch for their
    split-K partial products (amc3d_pointwise_conv_forward_ws)"""
    bptr = _ptr(bias) if bias is not None else None
    if not bf16 and _ld(w2) != Cin:  # a column block of a wider matrix, used where it lies
        wsf = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(B, Cin, Cout, P, int(bias is not None)))
        work = torch.empty(wsf, dtype=torch.uint8, device=x.device) if wsf else None
        _lib.check(lib.amc3d_pointwise_conv_forward_strided(B, Cin, Cout, P, _ptr(x), _ptr(w2), _ld(w2), bptr, _ptr(y),
                                                            _ptr(work) if wsf else None, wsf, _stream(x)), what)
        return
    if not bf16:
        wsf = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(B, Cin, Cout, P, int(bias is not None)))
        if wsf:
            work = torch.empty(wsf, dtype=torch.uint8, device=x.device)
            _lib.check(lib.amc3d_pointwise_conv_forward_ws(B, Cin, Cout, P, _ptr(x), _ptr(w2), bptr, _ptr(y), _ptr(work), wsf,
                                                           _stream(x)), what)
            return
    _lib.check(_pw(lib, bf16)[0](B, Cin, Cout, P, _ptr(x), _ptr(w2), bptr, _ptr(y), _stream(x)), what)


def _pw_forward_rows(lib, B, Cin, Cout, P, x, w2, y_pm, what="pointwise_conv_forward"):
    """y_pm (B,P,Cout) = (w2 . x) as position-major rows, fp32, no bias: the conv of a neighbourhood layer on its source
    points, stored the way the layer gathers it (the same bits as _pw_forward's output, transposed)"""
    wsf = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(B, Cin, Cout, P, 0))
    work = torch.empty(wsf, dtype=torch.uint8, device=x.device) if wsf else None
    _lib.check(lib.amc3d_pointwise_conv_forward_rows(B, Cin, Cout, P, _ptr(x), _ptr(w2), _ld(w2), _ptr(y_pm),
                                                     _ptr(work) if wsf else None, wsf, _stream(x)), what)


def _ld(w2):
    """row stride of a (rows, cols) weight view with unit column stride (one row: no stride to speak of)"""
    return w2.stride(0) if w2.shape[0] > 1 else w2.shape[1]


def _weight_rows(w2, bf16):
    """w2 (Cout,Cin) as the kernels take it: rows at a stride >= Cin with unit column stride (a column block of a wider
    matrix stays a view; the bf16-compute kernels take contiguous weights only)"""
    if not bf16 and w2.dim() == 2 and w2.stride(1) == 1 and _ld(w2) >= w2.shape[1]:
        return w2
    return w2.contiguous()


def _pw(lib, bf16):
    """(forward, workspace_bytes, backward) entry points of the pointwise conv in the requested arithmetic"""
    if bf16:
        return (lib.amc3d_pointwise_conv_forward_bf16, lib.amc3d_pointwise_conv_workspace_bytes_bf16,
                lib.amc3d_pointwise_conv_backward_bf16)
    return lib.amc3d_pointwise_conv_forward, lib.amc3d_pointwise_conv_workspace_bytes, lib.amc3d_pointwise_conv_backward


def _need_dtype(dtype, **named):
    """The C-ABI takes raw pointers: a float64 / bf16 coordinate or an int64 index would be reinterpreted silently.
    The reference's pybind layer throws on data_ptr<float>() / data_ptr<int>() of another dtype (ball_query.cpp:29-38);
    so does this."""
    for name, t in named.items():
        if t is not None and t.dtype != dtype:
            raise RuntimeError(f"expected {name} to be {dtype}, got {t.dtype}")


# tests only: {sequence number of the max-pool in forward order: arg-max (B,C,M) uint8} while a dict is installed
# (pool_log(d)); the oracle then routes its max-pool gradients through the same elements (tests/test_gpu_fullsize.py)
_pool_log = None
_pool_seq = 0


def pool_log(d):
    """install (dict) or remove (None) the arg-max log; resets the forward-order counter"""
    global _pool_log, _pool_seq
    _pool_log, _pool_seq = d, 0


def _next_pool_seq():
    global _pool_seq
    _pool_seq += 1
    return _pool_seq - 1


def _grid_ws(b, n_support, m_queries, device):
    """caller-owned scratch of the grid searches (ball query, 3-NN); the library falls back to the all-pairs
    kernels by itself where a grid does not pay (small clouds)"""
    wb = int(_lib.load().amc3d_grid_search_workspace_bytes(b, n_support, m_queries))
    return torch.empty(max(wb, 4), dtype=torch.uint8, device=device), wb


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """xyz (B,N,3) support, new_xyz (B,npoint,3) centres -> idx (B,npoint,nsample) int32"""
        assert new_xyz.is_contiguous()
        assert xyz.is_contiguous()
        _need_gpu(xyz, new_xyz)
        _need_dtype(torch.float32, xyz=xyz, new_xyz=new_xyz)
        B, N, _ = xyz.size()
        npoint = new_xyz.size(1)
        idx = torch.empty(B, npoint, nsample, dtype=torch.int32, device=xyz.device)
        work, wb = _grid_ws(B, N, npoint, xyz.device)
        with torch.cuda.device(xyz.device), timing.span("ball_query", (B * N + B * npoint) * 12 + idx.numel() * 4):
            _lib.check(_lib.load().amc3d_ball_query(B, N, npoint, float(radius), int(nsample), _ptr(new_xyz),
                                                    _ptr(xyz), _ptr(idx), _ptr(work), wb, _stream(xyz)), "ball_query")
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


ball_query = BallQuery.apply


class GroupingOperation(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, features, idx):
        """features (B,C,N), idx (B,npoint,nsample) int32 -> (B,C,npoint,nsample)"""
        assert features.is_contiguous()
        assert idx.is_contiguous()
        _need_gpu(features, idx)
        _need_dtype(torch.float32, features=features)
        _need_dtype(torch.int32, idx=idx)
        B, nfeatures, nsample = idx.size()
        _, C, N = features.size()
        output = torch.empty(B, C, nfeatures, nsample, dtype=torch.float32, device=features.device)
        with torch.cuda.device(features.device), timing.span("group_points", features.numel() * 4 + idx.numel() * 4 + output.numel() * 4):
            _lib.check(_lib.load().amc3d_group_points(B, C, N, nfeatures, nsample, _ptr(features), _ptr(idx),
                                                      _ptr(output), _stream(features)), "group_points")
        ctx.for_backwards = (idx, N)
        ctx.det = deterministic()
        return output

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        idx, N = ctx.for_backwards
        if ctx.det:
            raise _no_route("group_points_grad", "the scatter adds floats with atomics; the fused layers gather over reverse lists")
        B, C, npoint, nsample = grad_out.size()
        grad_features = torch.zeros(B, C, N, dtype=torch.float32, device=grad_out.device)
        grad_out_data = grad_out.detach().contiguous()
        with torch.cuda.device(grad_out.device), timing.span("group_points_grad", grad_out_data.numel() * 4 + idx.numel() * 4 + grad_features.numel() * 4):
            work = torch.empty(B * C * N, dtype=torch.float32, device=grad_out.device)
            _lib.check(_lib.load().amc3d_group_points_grad(B, C, N, npoint, nsample, _ptr(grad_out_data), _ptr(idx),
                                                           _ptr(grad_features), _ptr(work), work.numel() * 4,
                                                           _stream(grad_out)), "group_points_grad")
        return grad_features, None


grouping_operation = GroupingOperation.apply


class GatherOperation(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, features, idx):
        """features (B,C,N), idx (B,npoint) int32 -> (B,C,npoint)"""
        assert features.is_contiguous()
        assert idx.is_contiguous()
        _need_gpu(features, idx)
        _need_dtype(torch.float32, features=features)
        _need_dtype(torch.int32, idx=idx)
        B, npoint = idx.size()
        _, C, N = features.size()
        output = torch.empty(B, C, npoint, dtype=torch.float32, device=features.device)
        with torch.cuda.device(features.device), timing.span("gather_points", features.numel() * 4 + idx.numel() * 4 + output.numel() * 4):
            _lib.check(_lib.load().amc3d_gather_points(B, C, N, npoint, _ptr(features), _ptr(idx), _ptr(output),
                                                       _stream(features)), "gather_points")
        ctx.for_backwards = (idx, C, N)
        ctx.det = deterministic()
        return output

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        idx, C, N = ctx.for_backwards
        B, npoint = idx.size()
        if ctx.det and not torch.cuda.is_current_stream_capturing() and int(index_duplicates(idx, N)):
            # one atomic per address is deterministic (furthest-point picks are unique); several are not
            raise _no_route("gather_points_grad", "idx repeats an index")
        grad_features = torch.zeros(B, C, N, dtype=torch.float32, device=grad_out.device)
        grad_out_data = grad_out.detach().contiguous()
        with torch.cuda.device(grad_out.device), timing.span("gather_points_grad", grad_out_data.numel() * 4 + idx.numel() * 4 + grad_features.numel() * 4):
            _lib.check(_lib.load().amc3d_gather_points_grad(B, C, N, npoint, _ptr(grad_out_data), _ptr(idx),
                                                            _ptr(grad_features), _stream(grad_out)), "gather_points_grad")
        return grad_features, None


gather_operation = GatherOperation.apply


class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz (B,N,3) -> (B,npoint) int32, first index 0"""
        assert xyz.is_contiguous()
        _need_gpu(xyz)
        _need_dtype(torch.float32, xyz=xyz)
        B, N, _ = xyz.size()
        output = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
        # the reference's (B,N) scratch of running minima (filled with 1e10) lives in registers (N <= 24576) or in
        # the workspace (N <= 262144); only larger clouds need the buffer itself
        temp = None
        if N > 262144:
            temp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
        lib = _lib.load()
        wb = int(lib.amc3d_fps_workspace_bytes(B, N))
        with torch.cuda.device(xyz.device), timing.span("furthest_point_sampling", B * N * 12 + B * int(npoint) * 4):
            work = torch.empty(max(wb, 4), dtype=torch.uint8, device=xyz.device)
            _lib.check(_lib.load().amc3d_furthest_point_sampling(B, N, int(npoint), _ptr(xyz),
                                                                 _ptr(temp) if temp is not None else None,
                                                                 _ptr(output), _ptr(work), wb,
                                                                 _stream(xyz)), "furthest_point_sampling")
        ctx.mark_non_differentiable(output)
        return output

    @staticmethod
    def backward(xyz, a=None):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown (B,N,3), known (B,M,3) -> dist (B,N,3) (euclidean, not squared), idx (B,N,3) int32"""
        assert unknown.is_contiguous()
        assert known.is_contiguous()
        _need_gpu(unknown, known)
        _need_dtype(torch.float32, unknown=unknown, known=known)
        B, N, _ = unknown.size()
        m = known.size(1)
        dist2 = torch.empty(B, N, 3, dtype=torch.float32, device=unknown.device)
        idx = torch.empty(B, N, 3, dtype=torch.int32, device=unknown.device)
        work, wb = _grid_ws(B, m, N, unknown.device)
        with torch.cuda.device(unknown.device), timing.span("three_nn", (B * N + B * m) * 12 + B * N * 24):
            _lib.check(_lib.load().amc3d_three_nn(B, N, m, _ptr(unknown), _ptr(known), _ptr(dist2), _ptr(idx),
                                                  _ptr(work), wb, _stream(unknown)), "three_nn")
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, features, idx, weight, csr=None):
        """features (B,C,M), idx (B,n,3) int32, weight (B,n,3) -> (B,C,n).  csr: group_csr(idx, M) of the geometry plan, or
        None (deterministic mode then builds the lists in backward)"""
        assert features.is_contiguous()
        assert idx.is_contiguous()
        assert weight.is_contiguous()
        _need_gpu(features, idx, weight)
        _need_dtype(torch.float32, features=features, weight=weight)
        _need_dtype(torch.int32, idx=idx)
        B, c, m = features.size()
        n = idx.size(1)
        ctx.three_interpolate_for_backward = (idx, weight, m)
        ctx.det, ctx.csr = deterministic(), csr
        output = torch.empty(B, c, n, dtype=torch.float32, device=features.device)
        with torch.cuda.device(features.device), timing.span("three_interpolate", features.numel() * 4 + idx.numel() * 8 + output.numel() * 4):
            _lib.check(_lib.load().amc3d_three_interpolate(B, c, m, n, _ptr(features), _ptr(idx), _ptr(weight),
                                                           _ptr(output), _stream(features)), "three_interpolate")
        return output

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        idx, weight, m = ctx.three_interpolate_for_backward
        B, c, n = grad_out.size()
        if ctx.det:
            return _three_interpolate_grad_csr(grad_out.detach().contiguous(), idx, weight, m, ctx.csr), None, None, None
        return _three_interpolate_grad(grad_out.detach().contiguous(), idx, weight, m), None, None, None


def _three_interpolate_grad(grad_out, idx, weight, m):
    """grad of three_interpolate, default mode: summed in LDS and written whole where the shape takes that route, else
    global float atomics into a zeroed output through a point-major workspace"""
    B, c, n = grad_out.size()
    lib = _lib.load()
    lds = lib.amc3d_three_interpolate_grad_route(B, c, n, m, None, None) == 2
    grad_features = (torch.empty if lds else torch.zeros)(B, c, m, dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device), timing.span("three_interpolate_grad", grad_out.numel() * 4 + idx.numel() * 8 + grad_features.numel() * 4):
        if lds:
            _lib.check(lib.amc3d_three_interpolate_grad_write(B, c, n, m, _ptr(grad_out), _ptr(idx), _ptr(weight),
                                                              _ptr(grad_features), _stream(grad_out)), "three_interpolate_grad")
        else:
            work = torch.empty(B * c * m, dtype=torch.float32, device=grad_out.device)
            _lib.check(lib.amc3d_three_interpolate_grad(B, c, n, m, _ptr(grad_out), _ptr(idx), _ptr(weight), _ptr(grad_features),
                                                        _ptr(work), work.numel() * 4, _stream(grad_out)), "three_interpolate_grad")
    return grad_features


def _three_interpolate_grad_csr(grad_out, idx, weight, m, csr):
    """grad of three_interpolate without atomics: a gather over the reverse lists of idx (built here unless the plan has them)"""
    B, c, n = grad_out.size()
    if csr is None:
        csr = group_csr(idx, m)
    grad_features = torch.empty(B, c, m, dtype=torch.float32, device=grad_out.device)  # written whole
    with torch.cuda.device(grad_out.device), timing.span("three_interpolate_grad_csr", grad_out.numel() * 4 + idx.numel() * 12 + grad_features.numel() * 4):
        _lib.check(_lib.load().amc3d_three_interpolate_grad_csr(B, c, n, m, _ptr(grad_out), _ptr(idx), _ptr(weight), _ptr(csr[0]),
                                                                _ptr(csr[1]), _ptr(grad_features), _stream(grad_out)),
                   "three_interpolate_grad_csr")
    return grad_features


three_interpolate = ThreeInterpolate.apply


class ThreeInterpolateAdd(Function):
    """base (B,C,n) + three_interpolate(features (B,C,m), idx, weight): the interpolated branch of a FeaturePropogation
    conv added onto the skip branch in the interpolation kernel itself (no (B,C1+C2,n) concatenation is ever built)"""

    @staticmethod
    def forward(ctx, features, idx, weight, base, csr=None):
        _need_gpu(features, idx, weight, base)
        _need_dtype(torch.float32, features=features, weight=weight, base=base)
        _need_dtype(torch.int32, idx=idx)
        features, idx, weight, base = features.contiguous(), idx.contiguous(), weight.contiguous(), base.contiguous()
        B, c, m = features.size()
        n = idx.size(1)
        assert base.shape == (B, c, n)
        ctx.save_for_backward(idx, weight)
        ctx.m = m
        ctx.det, ctx.csr = deterministic(), csr
        output = torch.empty(B, c, n, dtype=torch.float32, device=features.device)
        with torch.cuda.device(features.device), timing.span("three_interpolate", features.numel() * 4 + idx.numel() * 8 + output.numel() * 8):
            _lib.check(_lib.load().amc3d_three_interpolate_add(B, c, m, n, _ptr(features), _ptr(idx), _ptr(weight), _ptr(base),
                                                               _ptr(output), _stream(features)), "three_interpolate_add")
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        m = ctx.m
        B, c, n = grad_out.size()
        grad_out_data = grad_out.detach().contiguous()
        if ctx.det:
            return _three_interpolate_grad_csr(grad_out_data, idx, weight, m, ctx.csr), None, None, grad_out, None
        return _three_interpolate_grad(grad_out_data, idx, weight, m), None, None, grad_out, None


three_interpolate_add = ThreeInterpolateAdd.apply


def three_interpolation(unknown_xyz, known_xyz, know_feat):
    """Inverse-distance 3-NN interpolation (upsampling.py:92-102)."""
    dist, idx = three_nn(unknown_xyz, known_xyz)
    dist_recip = 1.0 / (dist + 1e-8)
    norm = torch.sum(dist_recip, dim=2, keepdim=True)
    weight = dist_recip / norm
    return three_interpolate(know_feat, idx, weight)


_grid_cache = None  # {(support ptr, n, offset ptr, segments, stream): workspace} while knn_grid_reuse() is active
#                    and {("rows", support ptr, ...): (idx, dist2)} of a self search over that grid (knn_of_support_points)


class knn_grid_reuse:
    """with knn_grid_reuse(): k-NN searches over the same support tensor (same storage, same offsets) reuse the
    cell grid the first of them built -- the caller guarantees the support is not modified inside the block."""

    def __enter__(self):
        global _grid_cache
        self.prev = _grid_cache
        if _grid_cache is None:  # re-entrant: an enclosing block's grids stay visible
            _grid_cache = {}
        return self

    def __exit__(self, *exc):
        global _grid_cache
        _grid_cache = self.prev
        return False


class KNNQuery(Function):
    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz, offset, new_offset):
        """xyz (n,3), new_xyz (m,3), offset/new_offset (b) int32 cumulative ends
        -> idx (m,nsample) int32, dist (m,nsample) (euclidean)"""
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.is_contiguous() and new_xyz.is_contiguous()
        _need_gpu(xyz, new_xyz, offset, new_offset)
        _need_dtype(torch.float32, xyz=xyz, new_xyz=new_xyz)
        _need_dtype(torch.int32, offset=offset, new_offset=new_offset)
        nsample = int(nsample)
        n, m, nb = xyz.shape[0], new_xyz.shape[0], offset.shape[0]
        idx = torch.empty(m, nsample, dtype=torch.int32, device=xyz.device)
        dist2 = torch.empty(m, nsample, dtype=torch.float32, device=xyz.device)
        lib = _lib.load()
        wbytes = int(lib.amc3d_knnquery_workspace_bytes(n, m, nsample, nb))
        offset, new_offset = offset.contiguous(), new_offset.contiguous()
        # inside `with knn_grid_reuse():` searches over the same support set share one cell grid
        key = (xyz.data_ptr(), n, offset.data_ptr(), nb, _stream(xyz).value)
        cached = _grid_cache.get(key) if _grid_cache is not None else None
        gridded = bool(lib.amc3d_knnquery_uses_grid(m, nsample, n, nb))  # else: all-pairs kernel, no grid in `work`
        reuse = gridded and cached is not None and cached.numel() >= wbytes
        work = cached if reuse else torch.empty(wbytes, dtype=torch.uint8, device=xyz.device)
        if _grid_cache is not None and gridded and not reuse:
            _grid_cache[key] = work
        with torch.cuda.device(xyz.device), timing.span("knnquery", (n + m) * 12 + m * nsample * 8):
            _lib.check(lib.amc3d_knnquery(m, nsample, n, nb, _ptr(xyz), _ptr(new_xyz), _ptr(offset),
                                          _ptr(new_offset), _ptr(idx), _ptr(dist2), _ptr(work), work.numel(),
                                          int(reuse), _stream(xyz)), "knnquery")
        if _grid_cache is not None and gridded and m == n and new_xyz.data_ptr() == xyz.data_ptr() and new_offset.data_ptr() == offset.data_ptr():
            _grid_cache[("rows",) + key] = (idx, dist2)  # a finished self search: knn_of_support_points() reads prefixes of it
        ctx.mark_non_differentiable(idx)
        if _knn_squared:  # knnquery_squared(): the plan code wants no root (one elementwise launch per search on the geometry queue)
            return idx, dist2
        return idx, torch.sqrt(dist2)

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None


knnquery = KNNQuery.apply
_knn_squared = False


def knnquery_squared(nsample, xyz, new_xyz, offset, new_offset):
    """knnquery that leaves the distances SQUARED, as the kernel (and the reference's knnquery_cuda) produces them: the
    reference's wrapper takes the root in a separate elementwise op (pointops.py:55), which the loss's plan never looks at"""
    global _knn_squared
    prev, _knn_squared = _knn_squared, True
    try:
        return KNNQuery.apply(nsample, xyz, new_xyz, offset, new_offset)
    finally:
        _knn_squared = prev


KNN_PREFIX_MAX = 31  # amc3d_knn_prefix: kr + 1 columns of a row in 32 lanes


@torch.no_grad()
def knn_prefix(kr, xyz, new_xyz, offset, new_offset, rows_idx, rows_d2, work=None, want_dist=True):
    """knnquery_squared(kr, xyz, new_xyz, offset, new_offset) read off the rows (n, k0) of a finished self search of the
    support, knnquery_squared(k0, xyz, xyz, offset, offset) with k0 > kr: a query that is a support point (equal
    coordinates, exactly one such point in its segment) and whose row ascends strictly through column kr takes the row's
    first kr columns; every other query is searched (csrc/knn.hip amc3d_knn_prefix).  Same bits as the search.
    work: the workspace that holds the support's cell grid; None: the one an enclosing knn_grid_reuse() block keeps for this
    support, else a grid is built.
    -> (idx (m,kr) int32, dist2 (m,kr) or None, count: int32 tensor (1), how many queries were searched)"""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and rows_idx.is_contiguous() and rows_d2.is_contiguous()
    _need_gpu(xyz, new_xyz, offset, new_offset, rows_idx, rows_d2)
    _need_dtype(torch.float32, xyz=xyz, new_xyz=new_xyz, rows_d2=rows_d2)
    _need_dtype(torch.int32, offset=offset, new_offset=new_offset, rows_idx=rows_idx)
    kr = int(kr)
    n, m, nb = xyz.shape[0], new_xyz.shape[0], offset.shape[0]
    k0 = rows_idx.shape[1]
    if rows_idx.shape != (n, k0) or rows_d2.shape != (n, k0) or not 0 < kr < k0 or kr > KNN_PREFIX_MAX:
        raise RuntimeError(f"knn_prefix: rows {tuple(rows_idx.shape)} / {tuple(rows_d2.shape)} for {n} support points, kr = {kr}")
    lib = _lib.load()
    wbytes = int(lib.amc3d_knnquery_workspace_bytes(n, m, kr, nb))
    offset, new_offset = offset.contiguous(), new_offset.contiguous()
    if work is None and _grid_cache is not None:
        kept = _grid_cache.get((xyz.data_ptr(), n, offset.data_ptr(), nb, _stream(xyz).value))
        work = kept if kept is not None and kept.numel() >= wbytes else None
    reuse = work is not None
    if reuse and work.numel() < wbytes:
        raise RuntimeError("knn_prefix: the kept workspace is too small for these queries")
    if not reuse:
        work = torch.empty(wbytes, dtype=torch.uint8, device=xyz.device)
    idx = torch.empty(m, kr, dtype=torch.int32, device=xyz.device)
    dist2 = torch.empty(m, kr, dtype=torch.float32, device=xyz.device) if want_dist else None
    with torch.cuda.device(xyz.device), timing.span("knn_prefix", m * (12 + (kr + 1) * 4 + kr * (12 if want_dist else 8))):
        _lib.check(lib.amc3d_knn_prefix(m, kr, n, nb, _ptr(xyz), _ptr(new_xyz), _ptr(offset), _ptr(new_offset), k0,
                                        rows_idx.stride(0), _ptr(rows_idx), _ptr(rows_d2), _ptr(idx),
                                        _ptr(dist2) if want_dist else None, _ptr(work), work.numel(), int(reuse),
                                        _stream(xyz)), "knn_prefix")
    count = work[_lib.KNN_FALLBACK_COUNT_OFFSET:_lib.KNN_FALLBACK_COUNT_OFFSET + 4].view(torch.int32)
    return idx, dist2, count


def knn_of_support_points(kr, xyz, new_xyz, offset, new_offset):
    """The indices of knnquery(kr, xyz, new_xyz, offset, new_offset) for queries that are (mostly) points of the support,
    as the loss's label votes are: inside `with knn_grid_reuse():`, after a self search of the same support tensor and
    offsets with more than kr columns, they are prefixes of its rows (knn_prefix); otherwise the search runs."""
    key = (xyz.data_ptr(), xyz.shape[0], offset.data_ptr(), offset.shape[0], _stream(xyz).value)
    rows = _grid_cache.get(("rows",) + key) if _grid_cache is not None and offset.is_contiguous() else None
    work = _grid_cache.get(key) if rows is not None else None
    if (work is not None and kr <= KNN_PREFIX_MAX and kr < rows[0].shape[1] and offset.shape[0] <= 64 and new_xyz.dtype == torch.float32
            and work.numel() >= int(_lib.load().amc3d_knnquery_workspace_bytes(xyz.shape[0], new_xyz.shape[0], kr, offset.shape[0]))):
        return knn_prefix(kr, xyz, new_xyz, offset, new_offset, rows[0], rows[1], work=work, want_dist=False)[0]
    return knnquery_squared(kr, xyz, new_xyz, offset, new_offset)[0]


KNN_BATCH_MAX = 100  # the search's heap (amc3d_knnquery: nsample <= 100)
_KNN_DIST_LAYOUT = {"bmk": 0, "bkm": 1}  # AMC_KNN_DIST_BMK / AMC_KNN_DIST_BKM


@torch.no_grad()
def knn_batch(k, support, query=None, dilation=1, dist=None):
    """support (B,N,3), query (B,M,3) (None: the support itself) -> (dist or None, idx): idx (B,M,k) int32 cloud-local,
    column j the (j*dilation)-th of the k*dilation nearest support points, in amc3d_knnquery's order; dist the euclidean
    distances of those columns as (B,M,k) ('bmk') or (B,k,M) ('bkm').  Coordinates carry no gradient."""
    if query is None:
        query = support
    assert support.is_contiguous() and query.is_contiguous()
    _need_gpu(support, query)
    _need_dtype(torch.float32, support=support, query=query)
    if support.dim() != 3 or query.dim() != 3 or support.shape[2] != 3 or query.shape[2] != 3 or support.shape[0] != query.shape[0]:
        raise RuntimeError(f"knn_batch: expected (B,N,3) and (B,M,3), got {tuple(support.shape)} and {tuple(query.shape)}")
    k, dilation = int(k), int(dilation)
    ksearch = k * dilation
    B, N, _ = support.shape
    M = query.shape[1]
    if k <= 0 or dilation <= 0 or ksearch > KNN_BATCH_MAX:
        raise RuntimeError(f"knn_batch: k * dilation must be in 1..{KNN_BATCH_MAX}, got {k} * {dilation}")
    if ksearch > N:
        raise RuntimeError(f"knn_batch: k * dilation = {ksearch} out of range for {N} support points")
    if dist is not None and dist not in _KNN_DIST_LAYOUT:
        raise ValueError(f"knn_batch: dist must be None, 'bmk' or 'bkm', got {dist!r}")
    dev = support.device
    idx = torch.empty(B, M, k, dtype=torch.int32, device=dev)
    out = None if dist is None else torch.empty((B, M, k) if dist == "bmk" else (B, k, M), dtype=torch.float32, device=dev)
    if B == 0 or M == 0:
        return out, idx
    lib = _lib.load()
    wbytes = int(lib.amc3d_knn_batch_workspace_bytes(B, N, M, ksearch))
    if wbytes == 0:
        raise RuntimeError("knn_batch: sizes out of range for 32-bit indices")
    # inside `with knn_grid_reuse():` searches over the same support share one cell grid (KNNQuery's key; the uniform
    # segment ends live in the workspace, so the points per cloud stand in for the offset tensor)
    key = (support.data_ptr(), B * N, ("uniform", N), B, _stream(support).value)
    cached = _grid_cache.get(key) if _grid_cache is not None else None
    gridded = bool(lib.amc3d_knnquery_uses_grid(B * M, ksearch, B * N, B))
    reuse = gridded and cached is not None and cached.numel() >= wbytes
    work = cached if reuse else torch.empty(wbytes, dtype=torch.uint8, device=dev)
    if _grid_cache is not None and gridded and not reuse:
        _grid_cache[key] = work
    same = query.data_ptr() == support.data_ptr() and M == N
    with torch.cuda.device(dev), timing.span("knn_batch", B * (N + M) * 12 + idx.numel() * (4 if out is None else 8),
                                             moved=B * (N + M) * 12 + B * M * ksearch * 16 + idx.numel() * 8):
        _lib.check(lib.amc3d_knn_batch(B, N, M, ksearch, dilation, _ptr(support), _ptr(support if same else query), _ptr(idx),
                                       _ptr(out) if out is not None else None, _KNN_DIST_LAYOUT.get(dist, 0), _ptr(work),
                                       work.numel(), int(reuse), _stream(support)), "knn_batch")
    return out, idx


@torch.no_grad()
def knn_features(k, support, query=None, dilation=1, farthest=False, dist=None, channel_major=False):
    """k-NN in feature space (csrc/knn_feat.hip): support (B,N,C), query (B,M,C) (None: the support itself) -- with
    `channel_major` (B,C,N) and (B,C,M), read in place -- -> (dist or None, idx): idx (B,M,k) int32 cloud-local, column j the
    (j*dilation)-th of the k*dilation nearest (`farthest`: farthest) support rows, ascending in (d2, index) (descending d2,
    ascending index), d2 = (|q|^2 + |s|^2) - 2 q.s in fp32 with every sum an fmaf chain over ascending channels; dist the
    euclidean distances of those columns as (B,M,k) ('bmk') or (B,k,M) ('bkm').  No (B,M,N) matrix exists.  Features carry no
    gradient through the search."""
    if query is None:
        query = support
    assert support.is_contiguous() and query.is_contiguous()
    _need_gpu(support, query)
    _need_dtype(torch.float32, support=support, query=query)
    ca, ra = (1, 2) if channel_major else (2, 1)
    if support.dim() != 3 or query.dim() != 3 or support.shape[ca] != query.shape[ca] or support.shape[0] != query.shape[0] \
            or support.shape[ca] < 1:
        want = "(B,C,N) and (B,C,M)" if channel_major else "(B,N,C) and (B,M,C)"
        raise RuntimeError(f"knn_features: expected {want}, got {tuple(support.shape)} and {tuple(query.shape)}")
    k, dilation = int(k), int(dilation)
    ksearch = k * dilation
    B, N, M, C = support.shape[0], support.shape[ra], query.shape[ra], support.shape[ca]
    if k <= 0 or dilation <= 0 or ksearch > KNN_BATCH_MAX:
        raise RuntimeError(f"knn_features: k * dilation must be in 1..{KNN_BATCH_MAX}, got {k} * {dilation}")
    if ksearch > N:
        raise RuntimeError(f"knn_features: k * dilation = {ksearch} out of range for {N} support points")
    if dist is not None and dist not in _KNN_DIST_LAYOUT:
        raise ValueError(f"knn_features: dist must be None, 'bmk' or 'bkm', got {dist!r}")
    dev = support.device
    idx = torch.empty(B, M, k, dtype=torch.int32, device=dev)
    out = None if dist is None else torch.empty((B, M, k) if dist == "bmk" else (B, k, M), dtype=torch.float32, device=dev)
    if B == 0 or M == 0:
        return out, idx
    lib = _lib.load()
    wbytes = int(lib.amc3d_knn_features_workspace_bytes(B, N, M, C, ksearch))
    if wbytes == 0:
        raise RuntimeError("knn_features: sizes out of range for 32-bit indices")
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    s_strides, q_strides = ((1, N), (1, M)) if channel_major else ((C, 1), (C, 1))
    with torch.cuda.device(dev), timing.span("knn_features", B * (N + M) * C * 4 + idx.numel() * (4 if out is None else 8),
                                             2.0 * B * N * M * C):
        _lib.check(lib.amc3d_knn_features(B, N, M, C, ksearch, dilation, int(bool(farthest)), _ptr(support), *s_strides,
                                          _ptr(query), *q_strides, _ptr(idx), _ptr(out) if out is not None else None,
                                          _KNN_DIST_LAYOUT.get(dist, 0), _ptr(work), work.numel(), _stream(support)),
                   "knn_features")
    return out, idx


@torch.no_grad()
def knn_group_dp(idx, query, support, relative=True, normalize=False):
    """idx (B,M,K) int32 cloud-local, query (B,M,3), support (B,N,3) -> dp (B,3,M,K) = support[idx] (- query if relative);
    normalize: every cloud divided by its largest sqrt((x*x + y*y) + z*z) over (M,K), taken after the subtraction
    (KNNGroup, group.py:310-315).  Coordinates carry no gradient.  There is no grid here, so nothing of
    knn_grid_reuse() applies."""
    assert idx.is_contiguous() and query.is_contiguous() and support.is_contiguous()
    _need_gpu(idx, query, support)
    _need_dtype(torch.float32, query=query, support=support)
    _need_dtype(torch.int32, idx=idx)
    B, M, K = idx.shape
    N = support.shape[1]
    if support.shape != (B, N, 3) or query.shape != (B, M, 3):
        raise RuntimeError(f"knn_group_dp: idx {tuple(idx.shape)}, query {tuple(query.shape)}, support {tuple(support.shape)}")
    dev = support.device
    dp = torch.empty(B, 3, M, K, dtype=torch.float32, device=dev)
    cloud_max = torch.empty(B, dtype=torch.float32, device=dev) if normalize else None
    with torch.cuda.device(dev), timing.span("knn_group_dp", idx.numel() * (4 + 12 + 12) + B * M * 12,
                                             moved=idx.numel() * (4 + 12 + 12 + (24 if normalize else 0)) + B * M * 12):
        _lib.check(_lib.load().amc3d_knn_group_dp(B, N, M, K, _ptr(support), _ptr(query), _ptr(idx), int(bool(relative)),
                                                  int(bool(normalize)), _ptr(dp), _ptr(cloud_max) if normalize else None,
                                                  _stream(support)), "knn_group_dp")
    return dp


# ----------------------------------------------------------------------------------------------
# adaptive-margin contrastive loss (no native counterpart in the reference: it runs these as
# torch ops + a Python loop -- AMContrast3D/MarginContrast.py, AEF/ambiguity.py, AEF/utils.py)
# ----------------------------------------------------------------------------------------------
def _nbr_view(neighbor_idx):
    """(pointer to first used column, k, row stride) of an int32 index that may be a column slice
    idx[:, 1:] of a contiguous (m, K) tensor -- no copy (the reference calls .contiguous())."""
    assert neighbor_idx.dtype == torch.int32 and neighbor_idx.dim() == 2
    if neighbor_idx.stride(1) != 1:
        neighbor_idx = neighbor_idx.contiguous()
    return _ptr(neighbor_idx), neighbor_idx.shape[1], neighbor_idx.stride(0), neighbor_idx


def vote_labels(labels0, neighbor_idx, num_classes):
    """labels0 (n0) int32 classes of the full-resolution points, neighbor_idx (m,kr) int32 -> (m) int32:
    arg-max of the mean one-hot label over the kr neighbours (AEF/utils.py:29-41)."""
    _need_gpu(labels0, neighbor_idx)
    assert labels0.dtype == torch.int32 and neighbor_idx.dtype == torch.int32 and neighbor_idx.is_contiguous()
    m, kr = neighbor_idx.shape
    out = torch.empty(m, dtype=torch.int32, device=labels0.device)
    with torch.cuda.device(labels0.device), timing.span("vote_labels", m * kr * 8 + m * 4):
        _lib.check(_lib.load().amc3d_vote_labels(m, kr, int(num_classes), _ptr(labels0), _ptr(neighbor_idx), _ptr(out),
                                                 _stream(labels0)), "vote_labels")
    return out


def posmask_from_labels(labels, neighbor_idx):
    """labels (m) int32, neighbor_idx (m,k) int32 (may be idx[:, 1:]) -> (m,k) bool"""
    _need_gpu(labels, neighbor_idx)
    nptr, k, stride, keep = _nbr_view(neighbor_idx)
    m = labels.shape[0]
    out = torch.empty(m, k, dtype=torch.bool, device=labels.device)
    with torch.cuda.device(labels.device), timing.span("posmask", m * k * 9 + m * 4):
        _lib.check(_lib.load().amc3d_posmask(m, k, stride, _ptr(labels), nptr, _ptr(out), _stream(labels)), "posmask")
    return out


_CCTYPE = {"Method1": 1, "Method2": 2, "Method3": 3}


def loss_rows_supported(p, labels, neighbor_idx):
    """fp32 coordinates on the GPU and at most 64 neighbours: posmask_and_ambiguity takes the stage"""
    return (p.is_cuda and p.dtype == torch.float32 and labels.dtype == torch.int32 and neighbor_idx.dtype == torch.int32
            and bool(_lib.load().amc3d_loss_rows_supported(neighbor_idx.shape[1])))


def posmask_and_ambiguity(labels, p, neighbor_idx, cctype, beta, stats=False):
    """posmask_from_labels(labels, neighbor_idx) and ambiguity(p, posmask, neighbor_idx, cctype, beta) in one pass over the
    neighbour rows (csrc/loss.hip amc3d_loss_rows): the same bits.  -> (posmask (m,k) bool, a (m) fp32); stats: also the
    workspace's (max n+ (1) int32, n+ (m) int32, d+ (m), d- (m))."""
    _need_gpu(labels, p, neighbor_idx)
    _need_dtype(torch.float32, p=p)
    _need_dtype(torch.int32, labels=labels)
    assert p.is_contiguous() and labels.is_contiguous()
    nptr, k, stride, keep = _nbr_view(neighbor_idx)
    m = p.shape[0]
    lib = _lib.load()
    wbytes = int(lib.amc3d_ambiguity_workspace_bytes(m))
    work = torch.empty(wbytes, dtype=torch.uint8, device=p.device)
    posmask = torch.empty(m, k, dtype=torch.bool, device=p.device)
    a = torch.empty(m, dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device), timing.span("loss_rows", m * (12 + 4 + 4) + m * k * (4 + 1), moved=m * 20 + m * k * (4 + 1 + 4 + 12)):
        _lib.check(lib.amc3d_loss_rows(m, k, stride, _CCTYPE[cctype], float(beta), _ptr(labels), _ptr(p), nptr, _ptr(posmask),
                                       _ptr(a), _ptr(work), wbytes, _stream(p)), "loss_rows")
    if not stats:
        return posmask, a
    return posmask, a, (work[:4].view(torch.int32), work[64:64 + 4 * m].view(torch.int32),
                        work[64 + 4 * m:64 + 8 * m].view(torch.float32), work[64 + 8 * m:64 + 12 * m].view(torch.float32))


def ambiguity(p, posmask, neighbor_idx, cctype, beta):
    """p (m,3), posmask (m,k) bool, neighbor_idx (m,k) int32 -> a (m) fp32 (AEF/ambiguity.py:11-71)"""
    _need_gpu(p, posmask, neighbor_idx)
    assert p.is_contiguous() and posmask.is_contiguous() and posmask.dtype == torch.bool
    nptr, k, stride, keep = _nbr_view(neighbor_idx)
    m = p.shape[0]
    lib = _lib.load()
    wbytes = int(lib.amc3d_ambiguity_workspace_bytes(m))
    work = torch.empty(wbytes, dtype=torch.uint8, device=p.device)
    a = torch.empty(m, dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device), timing.span("ambiguity", m * (12 + 4) + m * k * (4 + 1), moved=m * (12 + 4) + m * k * (4 + 1 + 12)):
        _lib.check(lib.amc3d_ambiguity(m, k, stride, _CCTYPE[cctype], float(beta), _ptr(p), _ptr(posmask), nptr,
                                       _ptr(a), _ptr(work), wbytes, _stream(p)), "ambiguity")
    return a


def select_anchors(a):
    """a (m) fp32 -> int32 list of the anchors with 0 < a <= 1 (MarginContrast.py:250-252), ascending:
    [0] = count, [1..count] = ids (the tail of the tensor is scratch).  Part of a stage's plan: it depends on
    coordinates and labels only."""
    _need_gpu(a)
    _need_dtype(torch.float32, a=a)
    assert a.is_contiguous() and a.dim() == 1
    m = a.shape[0]
    lib = _lib.load()
    n = int(lib.amc3d_select_anchors_ints(m))
    sel = torch.empty(n, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device), timing.span("select_anchors", m * 12):
        _lib.check(lib.amc3d_select_anchors(m, _ptr(a), _ptr(sel), n, _stream(a)), "select_anchors")
    return sel


def contrast_csr(neighbor_idx, anchors):
    """Reverse lists of a loss stage's k-NN edges: neighbor_idx (m,k) int32 (may be idx[:, 1:]), anchors =
    select_anchors(a) -> int32 [rev_start (m+1) | rev_edge (m*k)]: for every row n the positions i*k + j, ascending, of the
    selected anchors i whose j-th neighbour is n.  Part of a stage's plan; ContrastStage's backward gathers along it
    instead of scattering with float atomics."""
    _need_gpu(neighbor_idx, anchors)
    _need_dtype(torch.int32, anchors=anchors)
    nptr, k, stride, keep = _nbr_view(neighbor_idx)
    m = neighbor_idx.shape[0]
    lib = _lib.load()
    rev = torch.empty(m + 1 + m * k, dtype=torch.int32, device=anchors.device)
    wbytes = int(lib.amc3d_contrast_csr_workspace_bytes(m))
    work = torch.empty(wbytes, dtype=torch.uint8, device=anchors.device)
    with torch.cuda.device(anchors.device), timing.span("contrast_csr", m * k * 12):
        _lib.check(lib.amc3d_contrast_csr(m, k, stride, nptr, _ptr(anchors), _ptr(rev), _ptr(work), wbytes,
                                          _stream(anchors)), "contrast_csr")
    return rev


def contrast_mutual(neighbor_idx, a, dist2=None):
    """The mutual-edge structure of a loss stage's k-NN graph (csrc/csr.hip amc3d_contrast_mutual): neighbor_idx (m,k) int32
    (may be idx[:, 1:]), a (m) the stage's ambiguities -> (mutual (m,k) uint8, rev int32 [rev_start (m+1) | rev_edge (m*k)]).
    mutual[i,s] = 1 iff i is in the list of its s-th neighbour; rev lists, per row, the NON-mutual edges of the anchors with
    0 < a <= 1 that point at it.  Coordinates and labels only: part of a stage's plan; ContrastStage's backward then
    gathers every gradient row (no float atomics).  dist2: the squared distances knnquery returned with neighbor_idx (the
    same view of them) when the lists are the self-search of the stage's cloud -- membership then follows from one distance
    comparison per edge; None scans the neighbours' lists (any lists).
    Precondition of the backward that uses this plan: the stage's posmask is SYMMETRIC on mutual edges (posmask[i, s] ==
    posmask[x, j] when x = nidx[i, s] and nidx[x, j] = i), as every label-derived mask is (posmask_from_labels) -- the
    receiving row reads the mask of an incoming mutual edge from its own list."""
    _need_gpu(neighbor_idx, a)
    _need_dtype(torch.float32, a=a)
    nptr, k, stride, keep = _nbr_view(neighbor_idx)
    m = neighbor_idx.shape[0]
    lib = _lib.load()
    dptr = None
    if dist2 is not None:
        _need_dtype(torch.float32, dist2=dist2)
        assert dist2.shape == neighbor_idx.shape and dist2.stride() == neighbor_idx.stride() and dist2.device == a.device
        dptr = _ptr(dist2)
    mutual = torch.empty(m, k, dtype=torch.uint8, device=a.device)
    rev = torch.empty(m + 1 + m * k, dtype=torch.int32, device=a.device)
    wbytes = int(lib.amc3d_contrast_mutual_workspace_bytes(m))
    work = torch.empty(wbytes, dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device), timing.span("contrast_mutual", m * k * 9 + m * 8, moved=m * k * (13 if dist2 is not None else 5 + 4 * k)):
        _lib.check(lib.amc3d_contrast_mutual(m, k, stride, nptr, dptr, _ptr(a), _ptr(mutual), _ptr(rev), _ptr(work), wbytes,
                                             _stream(a)), "contrast_mutual")
    return mutual, rev


def _contrast_inputs(f, m, neighbor_idx, posmask, a, anchors=None, rev=None, mutual=None, name="features"):
    """What every contrast entry point requires of the inputs they share, before any launch: f the contiguous fp32
    embeddings of m points (rows (m, C), or channel-major (B, C, n) with m = B * n), posmask (m, k) bool, a (m) fp32, both
    contiguous (the library reads them through raw pointers), and the plan tensors as select_anchors / contrast_csr /
    contrast_mutual return them.  -> _nbr_view(neighbor_idx)"""
    _need_gpu(f, neighbor_idx, posmask, a, *(t for t in (anchors, rev, mutual) if t is not None))
    _need_dtype(torch.float32, **{name: f}, a=a)
    _need_dtype(torch.int32, anchors=anchors, rev=rev)
    _need_dtype(torch.uint8, mutual=mutual)
    view = _nbr_view(neighbor_idx)
    k, dev = view[1], f.device
    assert neighbor_idx.shape[0] == m and posmask.dtype == torch.bool and posmask.is_contiguous() and posmask.shape == (m, k)
    assert a.shape == (m,) and a.is_contiguous()
    if anchors is not None:
        assert anchors.is_contiguous() and anchors.numel() >= m + 1 and anchors.device == dev
    if rev is not None:
        assert anchors is not None and rev.is_contiguous() and rev.numel() == m + 1 + m * k and rev.device == dev
    if mutual is not None:  # rev then holds the non-mutual edges only (contrast_mutual)
        assert rev is not None and mutual.is_contiguous() and mutual.shape == (m, k) and mutual.device == dev
    return view


def _contrast_buffers(m, C, k, dev, unit, per_slot):
    """norm (m), unit (m, C: the rows f_i / |f_i| the row-gather kernels read, forward and mutual-edge backward; None where
    `unit` is false), sim (m, k: the cosines) or, per_slot false, stats (m, 2: the two sums of exponentials per anchor --
    the positives', the negatives' -- the backward's records need when the cosines are not stored), loss_pt (m), mean_cnt (2)"""
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    return e(m), (e(m, C) if unit else None), e(m, k if per_slot else 2), e(m), e(2)


def _contrast_grad_out(grad_out):
    """the upstream gradient of the scalar loss as the one-element fp32 tensor the library reads"""
    return grad_out.detach().to(torch.float32).reshape(1).contiguous()


def _contrast_backward_route(C, aligned, det, has_rev, has_mutual, has_unit, csr_supported, rows_supported):
    """'mutual' (gather over mutual edges), 'rows' (gather over the reverse lists of all edges) or 'atomic' (float atomics).
    The gathers need 16-byte aligned rows f (a misaligned f also left the forward without unit rows); default mode keeps the
    atomic form at the widths without a power-of-two row kernel (the wide one is unmeasured there)."""
    if has_mutual and has_unit and aligned:
        return "mutual"
    if has_rev and aligned and (csr_supported(C) or (det and rows_supported(C))):
        return "rows"
    return "atomic"


def _contrast_route_and_lists(op, ctx, f, nbr, a, anchors, rev, mutual=None, unit=None):
    """-> (route, anchors, rev) of a backward over rows f.  Deterministic mode has no atomic route: where the stage's plan
    has no reverse lists of all edges (none, or contrast_mutual's, which hold the non-mutual edges only) it builds them
    here, and raises for rows the gathers cannot read (misaligned, or no multiple of 4, or above 512 channels)."""
    lib = _lib.load()
    C, aligned, all_edges = f.shape[1], f.data_ptr() % 16 == 0, rev is not None and mutual is None
    route = _contrast_backward_route(C, aligned, ctx.det, all_edges, mutual is not None, unit is not None,
                                     lib.amc3d_contrast_backward_csr_supported, lib.amc3d_contrast_backward_rows_supported)
    if route == "mutual" or not ctx.det:
        return route, anchors, rev
    if not aligned:
        raise _no_route(op, "the reverse-list backward needs 16-byte aligned rows")
    if not lib.amc3d_contrast_backward_rows_supported(C):
        raise _no_route(op, f"the reverse-list backward does not cover {C} channels")
    if not all_edges:
        anchors = select_anchors(a) if anchors is None else anchors
        rev = contrast_csr(nbr, anchors)
    return "rows", anchors, rev


def _opt(t):
    return _ptr(t) if t is not None else None


class ContrastStage(Function):
    """Stage loss of ContrastHead.point_contrast_margin (MarginContrast.py:250-257): mean over the
    anchors with 0 < a <= 1 of the margin soft-NN loss on cosine similarities.  anchors: select_anchors(a) of
    the same a, or None (every anchor is then visited and tested).  With `mutual` (the plan of contrast_mutual) the backward
    gathers over mutual edges and needs posmask symmetric on them (equal classes: posmask_from_labels); without it, or with
    rev = contrast_csr(...) alone, any mask is differentiated correctly."""

    @staticmethod
    def forward(ctx, features, neighbor_idx, posmask, a, mu, nu, temperature, anchors=None, rev=None, mutual=None):
        f = features.contiguous()
        m, C = f.shape
        nptr, k, stride, keep = _contrast_inputs(f, m, neighbor_idx, posmask, a, anchors, rev, mutual)
        lib = _lib.load()
        norm, unit, sim, loss_pt, mean_cnt = _contrast_buffers(m, C, k, f.device, lib.amc3d_contrast_backward_csr_supported(C), True)
        with torch.cuda.device(f.device), timing.span("contrast_forward", m * C * 4 + m * k * 9 + m * 12, moved=m * C * 4 * (3 + k) + m * k * 9 + m * 12):
            _lib.check(lib.amc3d_contrast_forward(m, C, k, stride, _ptr(f), nptr, _ptr(posmask), _ptr(a), _opt(anchors),
                                                  float(mu), float(nu), float(temperature), _ptr(norm), _opt(unit),
                                                  _ptr(sim), None, _ptr(loss_pt), _ptr(mean_cnt), _stream(f)),
                       "contrast_forward")
        ctx.save_for_backward(f, norm, keep, posmask, a, sim, mean_cnt, anchors, rev, mutual, unit)
        ctx.args = (float(mu), float(nu), float(temperature), k, stride)
        ctx.det = deterministic()
        return mean_cnt[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        f, norm, nbr, posmask, a, sim, mean_cnt, anchors, rev, mutual, unit = ctx.saved_tensors
        mu, nu, temperature, k, stride = ctx.args
        m, C = f.shape
        g = _contrast_grad_out(grad_out)
        nptr = _ptr(nbr)  # data_ptr includes the offset of an idx[:, 1:] view: the first used column
        lib = _lib.load()
        route, anchors, rev = _contrast_route_and_lists("contrast_backward", ctx, f, nbr, a, anchors, rev, mutual, unit)
        if route == "mutual":
            grad_f = torch.empty_like(f)  # every row is written
            wb = int(lib.amc3d_contrast_backward_mutual_workspace_bytes(m))
            work = torch.empty(wb, dtype=torch.uint8, device=f.device)
            with torch.cuda.device(f.device), timing.span("contrast_backward", m * C * 8 + m * k * 10 + m * 8,
                                                          moved=m * C * 4 * (2 + k) + m * k * 42 + m * 40):
                _lib.check(lib.amc3d_contrast_backward_mutual(m, C, k, stride, _ptr(unit), _ptr(norm), nptr, _ptr(posmask), _ptr(a),
                                                              _ptr(mutual), _ptr(rev), mu, nu, temperature, _ptr(sim), None,
                                                              _ptr(mean_cnt), _ptr(g), _ptr(work), wb, _ptr(grad_f), _stream(f)),
                           "contrast_backward_mutual")
        elif route == "rows":
            grad_f = torch.empty_like(f)  # every row is written
            gco = torch.empty(m * k, dtype=torch.float32, device=f.device)
            with torch.cuda.device(f.device), timing.span("contrast_backward_csr", m * C * 8 + m * k * 17, moved=m * C * 4 * (2 + 2 * k) + m * k * 17):
                _lib.check(lib.amc3d_contrast_backward_csr(m, C, k, stride, _ptr(f), _ptr(norm), nptr, _ptr(posmask),
                                                           _ptr(a), _ptr(anchors), _ptr(rev), mu, nu, temperature,
                                                           _ptr(sim), _ptr(mean_cnt), _ptr(g), _ptr(gco), _ptr(grad_f),
                                                           _stream(f)), "contrast_backward_csr")
        else:
            grad_f = torch.zeros_like(f)
            with torch.cuda.device(f.device), timing.span("contrast_backward", m * C * 8 + m * k * 9 + m * 8, moved=m * C * 4 * (1 + 2 * k) + m * k * 9):
                _lib.check(lib.amc3d_contrast_backward(m, C, k, stride, _ptr(f), _ptr(norm), nptr, _ptr(posmask), _ptr(a),
                                                       _opt(anchors), mu, nu, temperature, _ptr(sim), _ptr(mean_cnt),
                                                       _ptr(g), _ptr(grad_f), _stream(f)), "contrast_backward")
        return (grad_f,) + (None,) * 9


contrast_stage = ContrastStage.apply


_MARGIN_MODE = {"constant": 0, "adaptive": 1, "learned": 2}
_SUPERVISED_CL = {"Method1": 1, "Method2": 2}


def contrast_form(margin, db, supervisedCL, temperature):
    """The config's own values (ambiguity_args.margin / db / supervisedCL / temperature) -> (margin_mode, db, method,
    has_temperature, temperature) of include/amc3d.h.  Any db other than '-m' / '+m' means no shift, as the reference's
    `else` (MarginContrast.py:144-145); an unknown margin or supervisedCL leaves the reference without a value and is an error."""
    if margin not in _MARGIN_MODE:
        raise ValueError(f"ambiguity_args.margin must be one of {sorted(_MARGIN_MODE)} (got {margin!r})")
    if supervisedCL not in _SUPERVISED_CL:
        raise ValueError(f"ambiguity_args.supervisedCL must be one of {sorted(_SUPERVISED_CL)} (got {supervisedCL!r})")
    return (_MARGIN_MODE[margin], {"-m": 1, "+m": 2}.get(db, 0), _SUPERVISED_CL[supervisedCL],
            0 if temperature is None else 1, 1.0 if temperature is None else float(temperature))


def contrast_form_is_default(margin, db, supervisedCL, temperature):
    """the one form ContrastStage / ContrastStageChannelMajor evaluate"""
    return margin == "adaptive" and db == "-m" and supervisedCL == "Method1" and temperature is not None


def contrast_variant_forward(features, neighbor_idx, posmask, a, form, mu, nu, anchors=None):
    """Forward of ContrastStageVariant as its buffers: form = contrast_form(...) -> dict with f, norm, unit (None where the
    width has no row kernels), sim (m,k: the cosines of the visited anchors, the bits contrast_stage's forward stores),
    loss_pt (m: the per-anchor loss of the selected anchors; the rest of it is not written when `anchors` is given),
    mean_cnt (2: stage loss, number of selected anchors), nbr (the index tensor the pointers refer to), k, stride."""
    f = features.contiguous()
    m, C = f.shape
    nptr, k, stride, keep = _contrast_inputs(f, m, neighbor_idx, posmask, a, anchors)
    lib = _lib.load()
    norm, unit, sim, loss_pt, mean_cnt = _contrast_buffers(m, C, k, f.device, lib.amc3d_contrast_backward_csr_supported(C), True)
    mode, dbv, method, has_t, T = form
    with torch.cuda.device(f.device), timing.span("contrast_variant_forward", m * C * 4 + m * k * 13 + m * 12,
                                             moved=m * C * 4 * (3 + k) + m * k * 13 + m * 12):
        _lib.check(lib.amc3d_contrast_variant_forward(m, C, k, stride, _ptr(f), nptr, _ptr(posmask), _ptr(a), _opt(anchors),
                                                      mode, dbv, method, has_t, float(mu), float(nu), T, _ptr(norm),
                                                      _opt(unit), _ptr(sim), _ptr(loss_pt), _ptr(mean_cnt), _stream(f)),
                   "contrast_variant_forward")
    return {"f": f, "norm": norm, "unit": unit, "sim": sim, "loss_pt": loss_pt, "mean_cnt": mean_cnt, "nbr": keep, "k": k,
            "stride": stride}


class ContrastStageVariant(Function):
    """ContrastStage for every form of contrast_softnn_margin (MarginContrast.py:117-174): margin 'constant' / 'adaptive' /
    'learned', db '-m' / '+m' / anything else (no shift), supervisedCL 'Method1' / 'Method2', temperature a number or None --
    the config's own values.  anchors: select_anchors(a) or None.  rev: contrast_csr(neighbor_idx, anchors), the reverse lists
    of ALL edges of the selected anchors (never contrast_mutual's, which hold the non-mutual edges only); with it and a width
    of the row kernels (16/32/64/128/256; in deterministic mode every multiple of 4 up to 512, lists built where rev is None)
    the backward gathers every gradient row, otherwise it scatters with float atomics."""

    @staticmethod
    def forward(ctx, features, neighbor_idx, posmask, a, margin, db, supervisedCL, mu, nu, temperature, anchors=None, rev=None):
        form = contrast_form(margin, db, supervisedCL, temperature)
        f = features.contiguous()
        _contrast_inputs(f, f.shape[0], neighbor_idx, posmask, a, anchors, rev)  # (rev: the forward itself does not take it)
        b = contrast_variant_forward(f, neighbor_idx, posmask, a, form, mu, nu, anchors)
        ctx.save_for_backward(b["f"], b["norm"], b["nbr"], posmask, a, b["sim"], b["mean_cnt"], anchors, rev)
        ctx.args = (form, float(mu), float(nu), b["k"], b["stride"])
        ctx.det = deterministic()
        return b["mean_cnt"][0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        f, norm, nbr, posmask, a, sim, mean_cnt, anchors, rev = ctx.saved_tensors
        (mode, dbv, method, has_t, T), mu, nu, k, stride = ctx.args
        m, C = f.shape
        g = _contrast_grad_out(grad_out)
        lib = _lib.load()
        route, anchors, rev = _contrast_route_and_lists("contrast_variant_backward", ctx, f, nbr, a, anchors, rev)
        gather = route == "rows"
        grad_f = torch.empty_like(f) if gather else torch.zeros_like(f)  # (the gather writes every row)
        gco = torch.empty(m * k, dtype=torch.float32, device=f.device)
        name = "contrast_variant_backward_csr" if gather else "contrast_variant_backward"
        with torch.cuda.device(f.device), timing.span(name, m * C * 8 + m * k * 17, moved=m * C * 4 * (2 + 2 * k) + m * k * 17):
            _lib.check(lib.amc3d_contrast_variant_backward(m, C, k, stride, _ptr(f), _ptr(norm), _ptr(nbr), _ptr(posmask), _ptr(a),
                                                           _opt(anchors), _ptr(rev) if gather else None, mode, dbv, method, has_t,
                                                           mu, nu, T, _ptr(sim), _ptr(mean_cnt), _ptr(g), _ptr(gco), _ptr(grad_f),
                                                           _stream(f)), name)
        return (grad_f,) + (None,) * 11


def contrast_stage_variant(features, neighbor_idx, posmask, a, margin, db, supervisedCL, mu, nu, temperature, anchors=None,
                           rev=None):
    return ContrastStageVariant.apply(features, neighbor_idx, posmask, a, margin, db, supervisedCL, mu, nu, temperature,
                                      anchors, rev)


class ContrastStageChannelMajor(Function):
    """contrast_stage on the decoder's channel-major embeddings f_cm (B, C, n) -- what the reference flattens into (B*n, C) rows
    first (pointnext_AA.py:518-519).  The point-major copy of f is never made: the forward writes the unit rows f_i / |f_i|
    through an LDS tile, the mutual-edge backward reads only those; its gradient rows go back through one tiled transpose.
    Needs the mutual-edge plan (anchors, rev, mutual) and C in {16, 32, 64, 128, 256}: contrast_stage_supported_cm() -- and,
    with that plan, a posmask that is symmetric on mutual edges (label-derived: posmask_from_labels; see contrast_mutual).
    The cosines are not stored (the backward recomputes the ones it needs from the unit rows it fetches anyway)."""

    @staticmethod
    def forward(ctx, f_cm, neighbor_idx, posmask, a, mu, nu, temperature, anchors, rev, mutual):
        assert anchors is not None and rev is not None and mutual is not None
        f_cm = f_cm.contiguous()
        B, C, n = f_cm.shape
        m = B * n
        nptr, k, stride, keep = _contrast_inputs(f_cm, m, neighbor_idx, posmask, a, anchors, rev, mutual, "f_cm")
        norm, unit, stats, loss_pt, mean_cnt = _contrast_buffers(m, C, k, f_cm.device, True, False)
        with torch.cuda.device(f_cm.device), timing.span("contrast_forward", m * C * 4 + m * k * 5 + m * 20, moved=m * C * 4 * (2 + k) + m * k * 5 + m * 20):
            _lib.check(_lib.load().amc3d_contrast_forward_cm(B, C, n, k, stride, _ptr(f_cm), nptr, _ptr(posmask), _ptr(a), _ptr(anchors),
                                                             float(mu), float(nu), float(temperature), _ptr(norm), _ptr(unit),
                                                             None, _ptr(stats), _ptr(loss_pt), _ptr(mean_cnt), _stream(f_cm)),
                       "contrast_forward_cm")
        ctx.save_for_backward(norm, keep, posmask, a, stats, mean_cnt, rev, mutual, unit)
        ctx.args = (float(mu), float(nu), float(temperature), k, stride, B, C, n)
        return mean_cnt[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        norm, nbr, posmask, a, stats, mean_cnt, rev, mutual, unit = ctx.saved_tensors
        mu, nu, temperature, k, stride, B, C, n = ctx.args
        m = B * n
        g = _contrast_grad_out(grad_out)
        lib = _lib.load()
        grad_rows = torch.empty_like(unit)  # every row is written
        grad_cm = torch.empty(B, C, n, dtype=torch.float32, device=unit.device)
        wb = int(lib.amc3d_contrast_backward_mutual_workspace_bytes(m))
        work = torch.empty(wb, dtype=torch.uint8, device=unit.device)
        with torch.cuda.device(unit.device), timing.span("contrast_backward", m * C * 8 + m * k * 10 + m * 8,
                                                         moved=m * C * 4 * (4 + k) + m * k * 42 + m * 40):
            _lib.check(lib.amc3d_contrast_backward_mutual(m, C, k, stride, _ptr(unit), _ptr(norm), _ptr(nbr), _ptr(posmask), _ptr(a),
                                                          _ptr(mutual), _ptr(rev), mu, nu, temperature, None, _ptr(stats),
                                                          _ptr(mean_cnt), _ptr(g), _ptr(work), wb, _ptr(grad_rows), _stream(unit)),
                       "contrast_backward_mutual")
            # (B, n, C) -> (B, C, n)
            _lib.check(lib.amc3d_transpose_cn(B, n, C, _ptr(grad_rows), _ptr(grad_cm), _stream(unit)), "transpose_cn")
        return (grad_cm,) + (None,) * 9


def contrast_stage_supported_cm(f_cm, anchors, rev, mutual):
    return (torch.is_tensor(f_cm) and f_cm.is_cuda and f_cm.dtype == torch.float32 and f_cm.dim() == 3 and anchors is not None
            and rev is not None and mutual is not None and bool(_lib.load().amc3d_contrast_backward_csr_supported(int(f_cm.shape[1]))))


contrast_stage_cm = ContrastStageChannelMajor.apply

_STAGE_TENSORS = 7  # per stage: f_cm, neighbor_idx, posmask, a, anchors, rev, mutual


def _contrast_stage_descs(stages):
    """-> the AmcContrastStage array of include/amc3d.h over `stages`, dicts of sizes (ints) and tensors (pointers)"""
    descs = (_lib.ContrastStageDesc * len(stages))()
    for d, st in zip(descs, stages):
        for name, v in st.items():
            setattr(d, name, _ptr(v) if torch.is_tensor(v) else v)
    return descs


class ContrastStagesChannelMajor(Function):
    """Every stage of the loss in one call: what contrast_stage_cm computes per stage, their sum in the order of
    ContrastHead.forward and the loss weight, in three launches forward and two backward for ALL stages
    (amc3d_contrast_stages_forward_cm / _backward_cm).  apply(mu, nu, temperature, scale, f_cm_0, neighbor_idx_0, posmask_0,
    a_0, anchors_0, rev_0, mutual_0, f_cm_1, ...) -> (total, means): total = scale * (((l_0 + l_1) + l_2) + ...) rounded as the
    per-stage route rounds it, means (stages, 2) = each stage's {loss, number of selected anchors}, without a gradient.
    The backward writes each stage's gradient channel-major, (B, C, n), straight from the gather: no row-major gradient, no
    transpose.  Every stage must satisfy contrast_stage_supported_cm()."""

    @staticmethod
    def forward(ctx, mu, nu, temperature, scale, *tensors):
        assert tensors and len(tensors) % _STAGE_TENSORS == 0
        lib, dev = _lib.load(), tensors[0].device
        nst = len(tensors) // _STAGE_TENSORS
        if nst > _lib.CONTRAST_MAX_STAGES:
            raise ValueError(f"contrast_stages_cm: at most {_lib.CONTRAST_MAX_STAGES} stages per call (got {nst})")
        means = torch.empty(nst, 2, dtype=torch.float32, device=dev)
        total = torch.empty((), dtype=torch.float32, device=dev)
        stages, keep, nbytes, moved = [], [], 0, 0
        for s in range(nst):
            f_cm, neighbor_idx, posmask, a, anchors, rev, mutual = tensors[s * _STAGE_TENSORS:(s + 1) * _STAGE_TENSORS]
            assert anchors is not None and rev is not None and mutual is not None and f_cm.dim() == 3 and f_cm.device == dev
            f_cm = f_cm.contiguous()
            B, C, n = f_cm.shape
            m = B * n
            nptr, k, stride, nbr = _contrast_inputs(f_cm, m, neighbor_idx, posmask, a, anchors, rev, mutual, "f_cm")
            norm, unit, stats, loss_pt, _ = _contrast_buffers(m, C, k, dev, True, False)
            stages.append(dict(b=B, C=C, n=n, k=k, nbr_stride=stride, f_cm=f_cm, nbr=nptr, posmask=posmask, a=a, sel=anchors,
                               mutual=mutual, rev=rev, norm=norm, unit=unit, stats=stats, loss_pt=loss_pt, mean_cnt=means[s]))
            keep += [nbr, posmask, a, rev, mutual, norm, unit, stats]
            nbytes += m * C * 4 + m * k * 5 + m * 20
            moved += m * C * 4 * (2 + k) + m * k * 5 + m * 20
        with torch.cuda.device(dev), timing.span("contrast_forward", nbytes, moved=moved):
            _lib.check(lib.amc3d_contrast_stages_forward_cm(nst, _contrast_stage_descs(stages), float(mu), float(nu),
                                                            float(temperature), float(scale), _ptr(total), _stream(total)),
                       "contrast_stages_forward_cm")
        timing.note("contrast_forward", nst - 1)  # (count_calls: one per stage)
        timing.note("contrast_stages_forward")
        ctx.save_for_backward(means, *keep)
        ctx.args = (float(mu), float(nu), float(temperature), float(scale),
                    [{key: st[key] for key in ("b", "C", "n", "k", "nbr_stride")} for st in stages])
        ctx.mark_non_differentiable(means)
        ctx.set_materialize_grads(False)
        return total, means

    @staticmethod
    def backward(ctx, grad_total, _grad_means):
        mu, nu, temperature, scale, sizes = ctx.args
        nst = len(sizes)
        if grad_total is None:
            return (None,) * (4 + nst * _STAGE_TENSORS)
        means, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        lib, dev = _lib.load(), means.device
        g = _contrast_grad_out(grad_total)
        stages, grads, nbytes, moved = [], [], 0, 0
        for s, sz in enumerate(sizes):
            nbr, posmask, a, rev, mutual, norm, unit, stats = saved[s * 8:(s + 1) * 8]
            m, C, k = sz["b"] * sz["n"], sz["C"], sz["k"]
            grad_cm = torch.empty(sz["b"], C, sz["n"], dtype=torch.float32, device=dev)  # every element is written
            stages.append(dict(sz, nbr=nbr, posmask=posmask, a=a, mutual=mutual, rev=rev, norm=norm, unit=unit, stats=stats,
                               mean_cnt=means[s], grad_cm=grad_cm))
            grads += [grad_cm] + [None] * (_STAGE_TENSORS - 1)
            nbytes += m * C * 8 + m * k * 10 + m * 8
            moved += m * C * 4 * (2 + k) + m * k * 42 + m * 40
        descs = _contrast_stage_descs(stages)
        wb = int(lib.amc3d_contrast_stages_backward_cm_workspace_bytes(nst, descs))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev), timing.span("contrast_backward", nbytes, moved=moved):
            _lib.check(lib.amc3d_contrast_stages_backward_cm(nst, descs, mu, nu, temperature, scale, _ptr(g), _ptr(work), wb,
                                                             _stream(means)), "contrast_stages_backward_cm")
        timing.note("contrast_backward", nst - 1)
        timing.note("contrast_stages_backward")
        return (None,) * 4 + tuple(grads)


def contrast_stages_cm(stages, mu, nu, temperature, scale=1.0):
    """stages: one (f_cm, neighbor_idx, posmask, a, anchors, rev, mutual) per stage -> (total, means) of
    ContrastStagesChannelMajor"""
    return ContrastStagesChannelMajor.apply(mu, nu, temperature, scale, *(t for st in stages for t in st))


# ----------------------------------------------------------------------------------------------
# training-mode BatchNorm fused with ReLU / neighbourhood max-pool (csrc/bn.hip)
# ----------------------------------------------------------------------------------------------
def _bn_ws(C, dev, extra=0):
    n = int(_lib.load().amc3d_bn_workspace_bytes(C)) + extra
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def _bn_running_args(bn):
    """(momentum, running_mean ptr, running_var ptr, num_batches_tracked ptr) of an nn.BatchNorm module whose
    buffers the fused forward updates in place, or (0, None, None, None)"""
    if bn is None or not bn.track_running_stats or bn.running_mean is None:
        return 0.0, None, None, None
    assert bn.running_mean.dtype == torch.float32 and bn.num_batches_tracked.dtype == torch.int64
    mom = -1.0 if bn.momentum is None else float(bn.momentum)
    return mom, _ptr(bn.running_mean), _ptr(bn.running_var), _ptr(bn.num_batches_tracked)


def _bn_stat_bufs(C, dev):
    """mean, invstd and unbiased variance of C channels, for a kernel to fill"""
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    return mean, torch.empty_like(mean), torch.empty_like(mean)


def _bn_begin(x, bn):
    """What every fused forward starts from: x contiguous, its shape as (B, C, L), the statistics buffers, the workspace
    (tensor, bytes) and the running-buffer arguments of `bn`."""
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    return x, (B, C, x.numel() // (B * C)), _bn_stat_bufs(C, x.device), _bn_ws(C, x.device), _bn_running_args(bn)


def _bn_finish(ctx, y, mean, var_u, *saved):
    """The forward's bookkeeping: returns (y, batch mean, unbiased batch variance), the statistics without gradients."""
    ctx.save_for_backward(*saved)
    ctx.mark_non_differentiable(mean, var_u)
    ctx.set_materialize_grads(False)  # no zero tensors for the statistics' (absent) gradients
    return y, mean, var_u


def _bn_backward_begin(x, dy, gamma, beta):
    """(B, C, L), dy contiguous, the dx / dgamma / dbeta to fill and the workspace (tensor, bytes) of a fused backward."""
    B, C = x.shape[0], x.shape[1]
    return ((B, C, x.numel() // (B * C)), dy.contiguous(), torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta),
            _bn_ws(C, x.device, extra=C * 8))


class BatchNormAct(Function):
    """y = [relu](batch_norm(x)) with batch statistics; x (B, C, *) contiguous fp32.  `bn`: the nn.BatchNorm module
    whose running buffers are updated in the same launch (None: no update).
    Returns (y, batch mean, unbiased batch variance)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, bn=None):
        _need_gpu(x, gamma, beta)
        x, (B, C, L), (mean, invstd, var_u), (work, wb), (mom, rm, rv, nbt) = _bn_begin(x, bn)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device), timing.span("bn_act_forward", x.numel() * 8, moved=x.numel() * 12):
            _lib.check(_lib.load().amc3d_bn_forward(B, C, L, 0, int(bool(relu)), float(eps), mom, _ptr(x), _ptr(gamma),
                                                    _ptr(beta), _ptr(y), None, _ptr(mean), _ptr(invstd), _ptr(var_u), rm, rv,
                                                    nbt, _ptr(work), wb, _stream(x)), "bn_forward")
        ctx.relu = bool(relu)
        return _bn_finish(ctx, y, mean, var_u, x, gamma, beta, mean, invstd)

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        (B, C, L), dy, dx, dgamma, dbeta, (work, wb) = _bn_backward_begin(x, dy, gamma, beta)
        with torch.cuda.device(x.device), timing.span("bn_act_backward", x.numel() * 12, moved=x.numel() * 20):
            _lib.check(_lib.load().amc3d_bn_backward(B, C, L, 1, int(ctx.relu), _ptr(x), _ptr(dy), None, _ptr(mean),
                                                     _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(dx), _ptr(dgamma),
                                                     _ptr(dbeta), _ptr(work), wb, _stream(x)), "bn_backward")
        return dx, dgamma, dbeta, None, None, None


class BatchNormResidualAct(Function):
    """y = relu(batch_norm(x) + res) with batch statistics: the tail of an InvResMLP block (pointnext_AA.py:296-307: the
    last Conv1d -> BatchNorm1d of pwconv, `f += identity`, `self.act(f)`) in the two launches of a plain BatchNorm layer;
    backward: dres = dy * (y > 0) and the BatchNorm backward of that, two launches.  Returns (y, mean, unbiased variance)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, bn=None):
        _need_gpu(x, res, gamma, beta)
        _need_dtype(torch.float32, x=x, res=res, gamma=gamma, beta=beta)
        x, (B, C, L), (mean, invstd, var_u), (work, wb), (mom, rm, rv, nbt) = _bn_begin(x, bn)
        res = res.contiguous()
        assert x.shape == res.shape
        y = torch.empty_like(x)
        with torch.cuda.device(x.device), timing.span("bn_residual_forward", x.numel() * 12, moved=x.numel() * 16):
            _lib.check(_lib.load().amc3d_bn_residual_forward(B, C, L, float(eps), mom, _ptr(x), _ptr(res), _ptr(gamma), _ptr(beta),
                                                             _ptr(y), _ptr(mean), _ptr(invstd), _ptr(var_u), rm, rv, nbt,
                                                             _ptr(work), wb, _stream(x)), "bn_residual_forward")
        return _bn_finish(ctx, y, mean, var_u, x, y, gamma, beta, mean, invstd)

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        x, y, gamma, beta, mean, invstd = ctx.saved_tensors
        (B, C, L), dy, dx, dgamma, dbeta, (work, wb) = _bn_backward_begin(x, dy, gamma, beta)
        dres = torch.empty_like(x)
        with torch.cuda.device(x.device), timing.span("bn_residual_backward", x.numel() * 20, moved=x.numel() * 28):
            _lib.check(_lib.load().amc3d_bn_residual_backward(B, C, L, _ptr(x), _ptr(y), _ptr(dy), _ptr(mean), _ptr(invstd),
                                                              _ptr(gamma), _ptr(beta), _ptr(dx), _ptr(dres), _ptr(dgamma),
                                                              _ptr(dbeta), _ptr(work), wb, _stream(x)), "bn_residual_backward")
        return dx, dres, dgamma, dbeta, None, None


class BatchNormSigmoid(Function):
    """y = sigmoid(batch_norm(x)) with batch statistics: nn.BatchNorm1d -> nn.Sigmoid of the APM towers of AMContrast3D++
    (openpoints/AMContrast3D/APM/concatenation.py:20-60) in the two launches of a plain BatchNorm layer; backward from the saved
    output (dy * y (1 - y), then BatchNorm backward), two launches.  Returns (y, mean, unbiased variance)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, bn=None):
        _need_gpu(x, gamma, beta)
        _need_dtype(torch.float32, x=x, gamma=gamma, beta=beta)
        x, (B, C, L), (mean, invstd, var_u), (work, wb), (mom, rm, rv, nbt) = _bn_begin(x, bn)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device), timing.span("bn_sigmoid_forward", x.numel() * 8, moved=x.numel() * 12):
            _lib.check(_lib.load().amc3d_bn_sigmoid_forward(B, C, L, float(eps), mom, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y),
                                                            _ptr(mean), _ptr(invstd), _ptr(var_u), rm, rv, nbt, _ptr(work), wb,
                                                            _stream(x)), "bn_sigmoid_forward")
        return _bn_finish(ctx, y, mean, var_u, x, y, gamma, beta, mean, invstd)

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        x, y, gamma, beta, mean, invstd = ctx.saved_tensors
        (B, C, L), dy, dx, dgamma, dbeta, (work, wb) = _bn_backward_begin(x, dy, gamma, beta)
        with torch.cuda.device(x.device), timing.span("bn_sigmoid_backward", x.numel() * 16, moved=x.numel() * 24):
            _lib.check(_lib.load().amc3d_bn_sigmoid_backward(B, C, L, _ptr(x), _ptr(y), _ptr(dy), _ptr(mean), _ptr(invstd),
                                                             _ptr(gamma), _ptr(beta), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                                             _ptr(work), wb, _stream(x)), "bn_sigmoid_backward")
        return dx, dgamma, dbeta, None, None


@torch.no_grad()
def bn_update_running(bn, mean, var_unbiased):
    """nn.BatchNorm's training-mode buffer update (num_batches_tracked, running_mean, running_var) in one launch."""
    _need_gpu(mean, var_unbiased, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    mom = -1.0 if bn.momentum is None else float(bn.momentum)
    _lib.check(_lib.load().amc3d_bn_update_running(mean.numel(), mom, _ptr(mean), _ptr(var_unbiased),
                                                   _ptr(bn.running_mean), _ptr(bn.running_var),
                                                   _ptr(bn.num_batches_tracked), _stream(mean)), "bn_update_running")


class BatchNormMax(Function):
    """y (B,C,M) = max over the K neighbours of [relu](batch_norm(x (B,C,M,K))) with batch statistics.
    Returns (y, batch mean, unbiased batch variance); the (B,C,M,K) normalised tensor is never written."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, bn=None):
        _need_gpu(x, gamma, beta)
        x, (B, C, L), (mean, invstd, var_u), (work, wb), (mom, rm, rv, nbt) = _bn_begin(x, bn)
        _, _, M, K = x.shape
        y = torch.empty(B, C, M, dtype=torch.float32, device=x.device)
        arg = torch.empty(B, C, M, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device), timing.span("bn_max_forward", x.numel() * 4 + y.numel() * 5, moved=x.numel() * 8 + y.numel() * 5):
            _lib.check(_lib.load().amc3d_bn_forward(B, C, L, K, int(bool(relu)), float(eps), mom, _ptr(x), _ptr(gamma),
                                                    _ptr(beta), _ptr(y), _ptr(arg), _ptr(mean), _ptr(invstd), _ptr(var_u), rm, rv,
                                                    nbt, _ptr(work), wb, _stream(x)), "bn_forward")
        ctx.relu = bool(relu)
        if _pool_log is not None:
            _pool_log[_next_pool_seq()] = arg
        return _bn_finish(ctx, y, mean, var_u, x, gamma, beta, mean, invstd, arg)

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        x, gamma, beta, mean, invstd, arg = ctx.saved_tensors
        (B, C, L), dy, dx, dgamma, dbeta, (work, wb) = _bn_backward_begin(x, dy, gamma, beta)
        with torch.cuda.device(x.device), timing.span("bn_max_backward", x.numel() * 4 + dy.numel() * 9, moved=x.numel() * 8 + dy.numel() * 5):
            _lib.check(_lib.load().amc3d_bn_backward(B, C, L, x.shape[-1], int(ctx.relu), _ptr(x), _ptr(dy), _ptr(arg),
                                                     _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(dx),
                                                     _ptr(dgamma), _ptr(dbeta), _ptr(work), wb, _stream(x)),
                       "bn_backward")
        return dx, dgamma, dbeta, None, None, None


@torch.no_grad()
def bn_eval(x, bn, relu, pool=False):
    """Inference-mode BatchNorm (running statistics) [+ReLU] [+max over the last, neighbour, dimension] in one pass:
    the whole-room evaluation loop of the reference (examples/segmentation/main_AA.py:431-802) runs the same blocks with
    model.eval().  y = ((x - running_mean) * rsqrt(running_var + eps)) * weight + bias, no gradient."""
    _need_gpu(x, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        if pool:
            M, K = x.shape[-2], x.shape[-1]
            y = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
            arg = torch.empty(x.shape[:-1], dtype=torch.uint8, device=x.device)
            _lib.check(lib.amc3d_bn_max(B, C, M, K, int(bool(relu)), _ptr(x), _ptr(bn.running_mean), _ptr(invstd),
                                        _ptr(bn.weight), _ptr(bn.bias), _ptr(y), _ptr(arg), _stream(x)), "bn_max")
            return y
        L = x.numel() // (B * C)
        y = torch.empty_like(x)
        _lib.check(lib.amc3d_bn_act(B, C, L, int(bool(relu)), _ptr(x), _ptr(bn.running_mean), _ptr(invstd),
                                    _ptr(bn.weight), _ptr(bn.bias), _ptr(y), _stream(x)), "bn_act")
        return y


class SyncBatchNormFused(Function):
    """BatchNormAct (pool=False) / BatchNormMax (pool=True) with statistics over every rank of `group`:
    torch.nn.SyncBatchNorm's arithmetic (torch/nn/modules/_functions.py; the reference converts all BN layers to it
    when world_size > 1, examples/segmentation/main_AA.py:146-148) on the fused kernels.  Per layer one all-reduce of
    2C+1 doubles forward ({sum x, sum x^2} per channel and the element count) and one of 2C doubles backward
    ({sum dq, sum dq*xhat}); parameter gradients stay rank-local, as torch's do.  Counts stay on the device, so ranks
    may hold different numbers of points and the whole sequence can be captured in a graph."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, pool, bn, group):
        import torch.distributed as dist
        _need_gpu(x, gamma, beta)
        x = x.contiguous()
        B, C = x.shape[0], x.shape[1]
        L = x.numel() // (B * C)
        K = x.shape[-1] if pool else 0
        dev = x.device
        lib = _lib.load()
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        sums[2 * C:].fill_(float(B * L))
        work, wb = _bn_ws(C, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.amc3d_bn_sums(B, C, L, _ptr(x), _ptr(sums), _ptr(work), wb, _stream(x)), "bn_sums")
        from . import graphs
        graphs.collective(lambda: dist.all_reduce(sums, group=group))  # eager, between two captured segments (graphs.py)
        mean, invstd, var_u = _bn_stat_bufs(C, dev)
        if pool:
            y = torch.empty(x.shape[:-1], dtype=torch.float32, device=dev)
            arg = torch.empty(x.shape[:-1], dtype=torch.uint8, device=dev)
        else:
            y, arg = torch.empty_like(x), None
        mom, rm, rv, nbt = _bn_running_args(bn)
        with torch.cuda.device(dev):
            _lib.check(lib.amc3d_bn_forward_synced(B, C, L, K, int(bool(relu)), float(eps), mom, _ptr(x), _ptr(sums),
                                                   _ptr(gamma), _ptr(beta), _ptr(y), None if arg is None else _ptr(arg),
                                                   _ptr(mean), _ptr(invstd), _ptr(var_u), rm, rv, nbt, _stream(x)),
                       "bn_forward_synced")
        ctx.relu, ctx.pool, ctx.group = bool(relu), bool(pool), group
        return _bn_finish(ctx, y, mean, var_u, x, gamma, beta, mean, invstd, sums, *([arg] if pool else []))

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        import torch.distributed as dist
        x, gamma, beta, mean, invstd, sums = ctx.saved_tensors[:6]
        arg = ctx.saved_tensors[6] if ctx.pool else None
        B, C = x.shape[0], x.shape[1]
        L = x.numel() // (B * C)
        K = x.shape[-1] if ctx.pool else 1
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(beta)
        dsums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
        work, wb = _bn_ws(C, x.device)
        lib = _lib.load()
        aptr = None if arg is None else _ptr(arg)
        with torch.cuda.device(x.device):
            _lib.check(lib.amc3d_bn_backward_sums(B, C, L, K, int(ctx.relu), _ptr(x), _ptr(dy), aptr, _ptr(mean),
                                                  _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(dsums), _ptr(dgamma),
                                                  _ptr(dbeta), _ptr(work), wb, _stream(x)), "bn_backward_sums")
        from . import graphs
        group = ctx.group
        graphs.collective(lambda: dist.all_reduce(dsums, group=group))
        with torch.cuda.device(x.device):
            _lib.check(lib.amc3d_bn_backward_synced(B, C, L, K, int(ctx.relu), _ptr(x), _ptr(dy), aptr, _ptr(mean),
                                                    _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(dsums),
                                                    ctypes.c_void_p(sums.data_ptr() + 16 * C), _ptr(dx), _stream(x)),
                       "bn_backward_synced")
        return dx, dgamma, dbeta, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# grouped 1x1 convolution fused with its gather, fp32 MFMA (csrc/gcc.hip)
# ----------------------------------------------------------------------------------------------
def grouped_conv_supported(cin, cout):
    return bool(_lib.load().amc3d_grouped_conv_supported(int(cin), int(cout)))


class GroupedConv(Function):
    """y (B,Cout,M,K) = W . [dp ; features[:, :, idx]] -- grouping_operation + torch.cat + nn.Conv2d 1x1 of the
    reference (group.py:244-255,323-325; pointnext_AA.py:164-166) without the (B,C+3,M,K) tensor.
    features (B,C,N) fp32, dp (B,3,M,K), idx (B,M,K) int32, weight (Cout,C+3,1,1)."""

    @staticmethod
    def forward(ctx, features, dp, idx, weight):
        _need_gpu(features, dp, idx, weight)
        features, dp, idx = features.contiguous(), dp.contiguous(), idx.contiguous()
        B, C, N = features.shape
        _, M, K = idx.shape
        Cout = weight.shape[0]
        assert weight.shape[1] == C + 3 and idx.dtype == torch.int32
        dev = features.device
        f_pm = torch.empty(B, N, C, dtype=torch.float32, device=dev)
        y = torch.empty(B, Cout, M, K, dtype=torch.float32, device=dev)
        w2 = weight.reshape(Cout, C + 3).contiguous()
        lib = _lib.load()
        flops = 2.0 * B * M * K * (C + 3) * Cout
        with torch.cuda.device(dev), timing.span("grouped_conv_forward", B * M * K * (4 * C + 16 + 4 * Cout), flops):
            _lib.check(lib.amc3d_transpose_cn(B, C, N, _ptr(features), _ptr(f_pm), _stream(features)), "transpose_cn")
            _lib.check(lib.amc3d_grouped_conv_forward(B, C, Cout, N, M, K, _ptr(f_pm), _ptr(dp), _ptr(idx), _ptr(w2),
                                                      _ptr(y), _stream(features)), "grouped_conv_forward")
        ctx.save_for_backward(f_pm, dp, idx, w2)
        ctx.wshape = tuple(weight.shape)
        ctx.det = deterministic()
        return y

    @staticmethod
    def backward(ctx, dy):
        f_pm, dp, idx, w2 = ctx.saved_tensors
        if ctx.det:
            raise _no_route("grouped_conv_backward", "its backward-data product scatters with float atomics; "
                            "GroupedConvBN / LocalAggregationFused gather over reverse lists")
        B, N, C = f_pm.shape
        _, M, K = idx.shape
        Cout = w2.shape[0]
        dy = dy.contiguous()
        dev = dy.device
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        df_pm = torch.zeros(B, N, C, dtype=torch.float32, device=dev) if need_f else None
        dw = torch.empty(Cout, C + 3, dtype=torch.float32, device=dev) if need_w else None
        lib = _lib.load()
        wb = int(lib.amc3d_grouped_conv_workspace_bytes(B, C, Cout, M, K))
        work = torch.empty(max(wb, 4), dtype=torch.uint8, device=dev)
        flops = 2.0 * B * M * K * Cout * ((C if need_f else 0) + (C + 3 if need_w else 0))
        with torch.cuda.device(dev), timing.span("grouped_conv_backward", B * M * K * (8 * C + 16 + 8 * Cout), flops):
            _lib.check(lib.amc3d_grouped_conv_backward(B, C, Cout, N, M, K, _ptr(f_pm), _ptr(dp), _ptr(idx), _ptr(w2),
                                                       _ptr(dy), _ptr(df_pm) if need_f else None,
                                                       _ptr(dw) if need_w else None, _ptr(work), wb, _stream(dy)),
                       "grouped_conv_backward")
        df = df_pm.transpose(1, 2).contiguous() if need_f else None
        return df, None, None, (dw.view(ctx.wshape) if need_w else None)


grouped_conv = GroupedConv.apply


class PointMajorRows(Function):
    """(B,C,n) channel-major features -> (B*n, C) rows: torch.flatten(f.transpose(1, 2), 0, 1), the per-stage embedding
    the contrastive loss reads (pointnext_AA.py:459-460, 518-519), as ONE coalesced LDS-tiled transpose each way.  torch
    makes the copy with a strided elementwise kernel and, in backward, adds the strided gradient view into the
    channel-major gradient with another one (0.7 GB of scattered traffic per step, measured)."""

    @staticmethod
    def forward(ctx, f):
        _need_gpu(f)
        _need_dtype(torch.float32, f=f)
        f = f.contiguous()
        B, C, n = f.shape
        out = torch.empty(B * n, C, dtype=torch.float32, device=f.device)
        with torch.cuda.device(f.device), timing.span("transpose_rows", f.numel() * 8):
            _lib.check(_lib.load().amc3d_transpose_cn(B, C, n, _ptr(f), _ptr(out), _stream(f)), "transpose_cn")
        ctx.shape = (B, C, n)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, n = ctx.shape
        g = g.contiguous()
        out = torch.empty(B, C, n, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device), timing.span("transpose_rows", g.numel() * 8):
            # (B, n, C) -> (B, C, n): the same kernel with the roles of the two axes exchanged
            _lib.check(_lib.load().amc3d_transpose_cn(B, n, C, _ptr(g), _ptr(out), _stream(g)), "transpose_cn")
        return out


def point_major_rows(f):
    """(B,C,n) -> (B*n,C); the fused transpose on fp32 GPU tensors, torch's flatten(transpose) otherwise"""
    if f.is_cuda and f.dtype == torch.float32 and f.dim() == 3:
        return PointMajorRows.apply(f)
    return torch.flatten(f.transpose(1, 2), start_dim=0, end_dim=1)


# ----------------------------------------------------------------------------------------------
# single grouped conv + BatchNorm [+ReLU] + max over the neighbours, convolved before the gather (csrc/lagg.hip)
# ----------------------------------------------------------------------------------------------
def local_aggregation_supported(cout, nsample):
    return bool(_lib.load().amc3d_local_aggregation_supported(int(cout), int(nsample)))


@torch.no_grad()
def group_moments(idx, dp, n_support):
    """Geometry moments of a neighbourhood query -- idx (B,M,K) int32 into n_support points, dp (B,3,M,K) -- that the
    convolve-before-gather layers need for their BatchNorm statistics and backward (in-degree and dp sum per support point,
    global dp moments): coordinates only, so part of the geometry plan.  -> opaque uint8 buffer."""
    _need_gpu(idx, dp)
    _need_dtype(torch.int32, idx=idx)
    _need_dtype(torch.float32, dp=dp)
    idx, dp = idx.contiguous(), dp.contiguous()
    B, M, K = idx.shape
    lib = _lib.load()
    nb = int(lib.amc3d_group_moments_bytes(B, int(n_support)))
    out = torch.empty(nb, dtype=torch.uint8, device=idx.device)
    with torch.cuda.device(idx.device), timing.span("group_moments", idx.numel() * 16 + nb):
        _lib.check(lib.amc3d_group_moments(B, int(n_support), M, K, _ptr(idx), _ptr(dp), _ptr(out), nb, _stream(idx)),
                   "group_moments")
    return out


@torch.no_grad()
def group_csr(idx, n_support):
    """Reverse adjacency of a neighbourhood query idx (B,M,K) into n_support points: (rev_start (B*n+1), rev_edge (B*M*K))
    int32 -- for every source point the positions that gathered it, in ascending position order (csrc/csr.hip).
    Coordinates only: part of the geometry plan.  The backward passes that used float atomics gather over these lists."""
    _need_gpu(idx)
    _need_dtype(torch.int32, idx=idx)
    idx = idx.contiguous()
    B, M, K = idx.shape
    n = int(n_support)
    dev = idx.device
    lib = _lib.load()
    rev_start = torch.empty(B * n + 1, dtype=torch.int32, device=dev)
    rev_edge = torch.empty(B * M * K, dtype=torch.int32, device=dev)
    wb = int(lib.amc3d_group_csr_workspace_bytes(B, M, K))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), timing.span("group_csr", idx.numel() * 12 + B * n * 4):
        _lib.check(lib.amc3d_group_csr(B, n, M, K, _ptr(idx), _ptr(rev_start), _ptr(rev_edge), _ptr(work), wb, _stream(idx)),
                   "group_csr")
    return rev_start, rev_edge


@torch.no_grad()
@torch.no_grad()
def group_csr_dp(idx, dp, rev_edge):
    """(dp, position) of every edge of group_csr's lists in list order, (B*M*K, 4) fp32 (the position as int32 bits in the
    fourth float): the stream the gathering backward of GroupedConvBN reads instead of an edge id + three scattered floats"""
    _need_gpu(idx, dp, rev_edge)
    _need_dtype(torch.float32, dp=dp)
    _need_dtype(torch.int32, rev_edge=rev_edge)
    B, M, K = idx.shape
    dp = dp.contiguous()
    assert dp.numel() == B * 3 * M * K and rev_edge.numel() == B * M * K and rev_edge.is_contiguous()
    out = torch.empty(B * M * K, 4, dtype=torch.float32, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().amc3d_group_csr_dp(B, M, K, _ptr(rev_edge), _ptr(dp), _ptr(out), _stream(idx)), "group_csr_dp")
    return out


def group_moments_csr(idx, dp, n_support, csr):
    """group_moments from the reverse lists: exact in-degree, dp sums in list order, no scattered atomics"""
    _need_gpu(idx, dp)
    dp = dp.contiguous()
    B, M, K = idx.shape
    lib = _lib.load()
    nb = int(lib.amc3d_group_moments_bytes(B, int(n_support)))
    out = torch.empty(nb, dtype=torch.uint8, device=idx.device)
    with torch.cuda.device(idx.device), timing.span("group_moments", idx.numel() * 16 + nb):
        _lib.check(lib.amc3d_group_moments_csr(B, int(n_support), M, K, _ptr(csr[0]), _ptr(csr[1]), _ptr(dp), _ptr(out), nb,
                                               _stream(idx)), "group_moments_csr")
    return out


def _sync(group, buf):
    """all-reduce of a statistics buffer between the two phases of a layer: eager, between captured graph segments"""
    import torch.distributed as dist
    from . import graphs
    graphs.collective(lambda: dist.all_reduce(buf, group=group))


def _dp_f_blocks(w2, bf16):
    """(W_dp, its row stride, W_f) of a neighbourhood layer's weight w2 = [W_dp | W_f] (C, 3 + Cin): the two column blocks
    where they lie (the kernels take a row stride); contiguous copies for the bf16-compute conv, which takes no stride"""
    if bf16:
        w_dp, w_f = _split_columns(w2, 3)
        return w_dp, 3, w_f
    return w2, w2.shape[1], w2[:, 3:]


def _dp_f_grad(C, Cin, dev, bf16):
    """(dW or None, dW_dp, its row stride, dW_f, its row stride): the two gradient blocks inside one (C, 3 + Cin) matrix -- the
    layer kernel writes columns 0-2, the conv's backward columns 3 onwards -- or apart (bf16: joined afterwards)"""
    if bf16:
        return (None, torch.empty(C, 3, dtype=torch.float32, device=dev), 3,
                torch.empty(C, Cin, dtype=torch.float32, device=dev), Cin)
    dw = torch.empty(C, Cin + 3, dtype=torch.float32, device=dev)
    return dw, dw, Cin + 3, dw[:, 3:], Cin + 3


def _pw_backward_blocks(lib, bf16, B, Cin, C, N, f, w_f, dg_cm, df, dw_f, lddw, work2, wb2):
    """backward of the conv on the source points: the weight a column block of the layer's weight, its gradient one of dW"""
    if bf16:
        _lib.check(lib.amc3d_pointwise_conv_backward_bf16(B, Cin, C, N, _ptr(f), _ptr(w_f), _ptr(dg_cm),
                                                          _ptr(df) if df is not None else None, _ptr(dw_f), _ptr(work2), wb2,
                                                          _stream(f)), "pointwise_conv_backward")
        return
    _lib.check(lib.amc3d_pointwise_conv_backward_strided(B, Cin, C, N, _ptr(f), _ptr(w_f), _ld(w_f), _ptr(dg_cm),
                                                         _ptr(df) if df is not None else None, 0, _ptr(dw_f), lddw,
                                                         _ptr(work2), wb2, _stream(f)), "pointwise_conv_backward")


def _lagg_begin(ctx, f, dp, idx, moments, weight, gamma, beta, eps, relu, bn, csr):
    """What both neighbourhood layers' forwards start from: the checked inputs, the weight's two blocks, G's buffers, the
    statistics buffers, the workspace and the arguments of the layer's C call around its outputs: *s.head, outputs, *s.tail(phase)"""
    _need_gpu(f, dp, idx, moments, weight, gamma, beta)
    _need_dtype(torch.float32, f=f, dp=dp, weight=weight)
    _need_dtype(torch.int32, idx=idx)
    s = SimpleNamespace(f=f.contiguous(), dp=dp.contiguous(), idx=idx.contiguous(), lib=_lib.load())
    B, Cin, N = f.shape
    _, M, K = idx.shape
    C = weight.shape[0]
    assert weight.numel() == C * (Cin + 3)
    s.shape, dev = (B, Cin, C, N, M, K), f.device
    # deterministic mode: the backward gathers over the reverse lists of idx (csr = (rev_start, rev_edge[, group_csr_dp's
    # stream]) of ops.group_csr from the plan, or built in backward) instead of scattering with float atomics
    ctx.det, ctx.csr = deterministic(), csr
    ctx.bf16 = mixed_precision() and min(Cin, C) >= 64 and B * N >= 4096  # the conv on the source points on the bf16 MFMA
    w2 = weight.detach().reshape(C, Cin + 3).contiguous()
    s.w_dp, ctx.ldw, s.w_f = _dp_f_blocks(w2, ctx.bf16)
    # fp32: the conv writes G as the rows the layer gathers; the bf16-compute conv writes it channel-major and the layer turns it
    s.g_cm = torch.empty(B, C, N, dtype=torch.float32, device=dev) if ctx.bf16 else None
    s.g_pm = torch.empty(B, N, C, dtype=torch.float32, device=dev)
    s.mean, s.invstd, s.var_u = mean, invstd, var_u = _bn_stat_bufs(C, dev)
    s.gd = gd = torch.empty(C, 3, dtype=torch.float64, device=dev)
    s.sums = sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    wb = int(s.lib.amc3d_local_aggregation_workspace_bytes(B, C, N, M))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    mom, rm, rv, nbt = _bn_running_args(bn)
    s.head = (B, C, N, M, K, 1, int(bool(relu)), float(eps), mom, _ptr(s.g_cm) if ctx.bf16 else None, _ptr(s.idx), _ptr(s.dp),
              _ptr(s.w_dp), ctx.ldw, _ptr(moments), _ptr(gamma), _ptr(beta), _ptr(s.g_pm))
    # (the closure names no `s`: in a cycle with it every buffer here would outlive the call until the garbage collector runs)
    s.tail = lambda phase: (_ptr(mean), _ptr(invstd), _ptr(var_u), _ptr(gd), rm, rv, nbt, phase, _ptr(sums), _ptr(work), wb,
                            _stream(f))
    return s


def _lagg_finish(ctx, s, name, nbytes, moved, call, moments, weight, gamma, beta, relu, bn, group, *saved):
    """The forward itself -- the conv on the source points, then call(phase) under the span `name`: phase 0, or 1 and 2 around
    the all-reduce over `group` -- and its bookkeeping; `saved` follows the twelve tensors both layers keep."""
    B, Cin, C, N, M, K = s.shape
    with torch.cuda.device(s.f.device):
        with timing.span("pointwise_conv_forward", 4 * B * N * (Cin + C), 2.0 * B * N * Cin * C):
            if s.g_cm is None:
                _pw_forward_rows(s.lib, B, Cin, C, N, s.f, s.w_f, s.g_pm)
            else:
                _pw_forward(s.lib, True, B, Cin, C, N, s.f, s.w_f, None, s.g_cm)
        with timing.span(name, nbytes, moved=moved):
            if group is None:
                call(0)
            else:
                call(1)
                _sync(group, s.sums)
                call(2)
    if bn is not None and bn.track_running_stats and bn.running_mean is not None and bn.momentum is None:
        bn_update_running(bn, s.mean, s.var_u)  # cumulative average: its own launch
    ctx.save_for_backward(s.f, s.w_f, s.w_dp, s.g_pm, s.idx, s.dp, moments, gamma, beta, s.mean, s.invstd, s.gd, *saved)
    ctx.relu, ctx.wshape, ctx.group = bool(relu), tuple(weight.shape), group
    ctx.shape = s.shape


def _lagg_backward_begin(ctx, lists_given, lists_bytes):
    """What both backwards start from: the gradients to fill, the reverse lists (deterministic mode builds those the plan did not
    give; `lists_given`: a layer that gathers over given lists in any mode), the workspaces (`lists_bytes(lib, B, C, N, M, K)`:
    the layer's with lists) and the arguments of the layer's C call: *s.dims, ..., *s.lists, ..., *s.mid, *s.tail(phase)"""
    saved = ctx.saved_tensors
    f, w_f, w_dp, g_pm, idx, dp, moments, gamma, beta, mean, invstd, gd = saved[:12]
    sums = saved[-1]
    B, Cin, C, N, M, K = ctx.shape
    dev = f.device
    s = SimpleNamespace(saved=saved, f=f, w_f=w_f, g_pm=g_pm, idx=idx, lib=_lib.load())
    s.dg_cm = dg_cm = torch.empty(B, C, N, dtype=torch.float32, device=dev)
    s.dw, s.dw_dp, lddw, s.dw_f, s.lddw_f = _dp_f_grad(C, Cin, dev, ctx.bf16)
    dw_dp = s.dw_dp
    s.dgamma, s.dbeta = dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    s.dsums = dsums = torch.empty(2 * C, dtype=torch.float64, device=dev)
    count = ctypes.c_void_p(sums.data_ptr() + 16 * C)
    s.csr = ctx.csr if ctx.det or lists_given else None
    if s.csr is None and ctx.det:
        s.csr = group_csr(idx, N)
    wb = int(lists_bytes(s.lib, B, C, N, M, K) if s.csr is not None else s.lib.amc3d_local_aggregation_workspace_bytes(B, C, N, M))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    s.need_f = ctx.needs_input_grad[0]
    s.df = torch.empty_like(f) if s.need_f else None
    _, pw_wbytes, _ = _pw(s.lib, ctx.bf16)
    s.wb2 = int(pw_wbytes(B, Cin, C, N))
    s.work2 = torch.empty(max(s.wb2, 4), dtype=torch.uint8, device=dev)
    s.dims = (B, C, N, M, K, int(ctx.relu))
    s.lists = (_ptr(s.csr[0]), _ptr(s.csr[1])) if s.csr is not None else (None, None)
    s.mid = (_ptr(dp), _ptr(w_dp), ctx.ldw, _ptr(moments), _ptr(gd), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta))
    # (as in _lagg_begin, no `s` in the closure: autograd takes dgamma / dbeta as .grad only while nothing else holds them, and
    # copies them otherwise)
    s.tail = lambda phase: (_ptr(dg_cm), _ptr(dw_dp), lddw, _ptr(dgamma), _ptr(dbeta), phase, _ptr(dsums), count, _ptr(work), wb,
                            _stream(f))
    return s


def _lagg_backward_finish(ctx, s, name, nbytes, moved, call):
    """The backward itself -- call(phase) under the span `name`, then the conv's backward on the source points -- and the
    gradients of either layer's twelve inputs."""
    B, Cin, C, N, M, K = ctx.shape
    need_f = s.need_f
    with torch.cuda.device(s.f.device):
        with timing.span(name, nbytes, moved=moved):
            if ctx.group is None:
                call(0)
            else:
                call(1)
                _sync(ctx.group, s.dsums)
                call(2)
        with timing.span("pointwise_conv_backward", 4 * B * N * (Cin + C + Cin * int(need_f)),
                         2.0 * B * N * Cin * C * (1 + int(need_f)), moved=4 * B * N * (Cin + C) * (1 + int(need_f))):
            _pw_backward_blocks(s.lib, ctx.bf16, B, Cin, C, N, s.f, s.w_f, s.dg_cm, s.df, s.dw_f, s.lddw_f, s.work2, s.wb2)
    dw = (_join_columns(s.dw_dp, s.dw_f) if s.dw is None else s.dw).view(ctx.wshape)
    return s.df, None, None, None, dw, s.dgamma, s.dbeta, None, None, None, None, None


class LocalAggregationFused(Function):
    """pooled (B,C,M) = max_k [relu](bn(conv1x1([dp ; f[idx]]))) -- grouping_operation + cat + Conv2d + BatchNorm2d (batch
    statistics) [+ ReLU] + max of LocalAggregation / single-layer SetAbstraction (pointnext_AA.py:57-63, 139-170) -- with
    the conv applied to the N source points BEFORE the gather:  W.[dp ; f[idx]] = (W_f.f)[idx] + W_dp.dp.
    f (B,Cin,N) fp32, dp (B,3,M,K), idx (B,M,K) int32, moments = group_moments(idx, dp, N), weight (C,Cin+3,1,1),
    `bn`: the nn.BatchNorm2d whose running buffers are updated (None: no update); `group`: a process group over which the
    statistics are taken (nn.SyncBatchNorm semantics: one all-reduce of 2C+1 doubles forward, 2C backward), or None."""

    @staticmethod
    def forward(ctx, f, dp, idx, moments, weight, gamma, beta, eps, relu, bn=None, group=None, csr=None):
        s = _lagg_begin(ctx, f, dp, idx, moments, weight, gamma, beta, eps, relu, bn, csr)
        B, Cin, C, N, M, K = s.shape
        pooled = torch.empty(B, C, M, dtype=torch.float32, device=f.device)
        ystar = torch.empty_like(pooled)
        arg = torch.empty(B, C, M, dtype=torch.uint8, device=f.device)

        def call(phase):
            _lib.check(s.lib.amc3d_local_aggregation_forward(*s.head, _ptr(pooled), _ptr(arg), _ptr(ystar), *s.tail(phase)),
                       "local_aggregation_forward")

        # algorithmic bytes: G read (statistics) + the gathered rows, idx, dp + the pooled outputs; a channel-major G is
        # read once more and written as rows
        _lagg_finish(ctx, s, "local_aggregation_forward", 4 * B * N * C + 16 * B * M * K + 5 * B * M * C,
                     (4 if s.g_cm is None else 12) * B * N * C + B * M * K * (4 * C + 16) + 9 * B * M * C, call,
                     moments, weight, gamma, beta, relu, bn, group, ystar, arg, s.sums)
        if _pool_log is not None:
            _pool_log[_next_pool_seq()] = arg
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        s = _lagg_backward_begin(ctx, False, lambda lib, B, C, N, M, K: lib.amc3d_local_aggregation_csr_workspace_bytes(B, C, N, M))
        ystar, arg = s.saved[12:14]
        B, Cin, C, N, M, K = ctx.shape
        dpooled = dpooled.contiguous()
        name = "local_aggregation_backward_csr" if s.csr is not None else "local_aggregation_backward"

        def call(phase):
            _lib.check(s.lib.amc3d_local_aggregation_backward(
                *s.dims, _ptr(dpooled), _ptr(ystar), _ptr(arg), _ptr(s.g_pm), _ptr(s.idx), *s.mid, *s.lists, *s.tail(phase)), name)

        return _lagg_backward_finish(
            ctx, s, name, 5 * B * M * C + 8 * B * N * C + 16 * B * M * K,
            (17 + (10 + 5 * K if s.csr is not None else 0)) * B * M * C + 12 * B * N * C + 16 * B * M * K, call)


class GroupedConvBN(Function):
    """x1 (B,C,M,32) = [relu](bn(conv1x1([dp ; f[idx]]))) -- the FIRST block of a multi-layer SetAbstraction MLP
    (PointNeXt-S: sa_layers = 2; pointnext_AA.py:104-127, 164-166) convolved before the gather like LocalAggregationFused,
    but with the activation materialised for the blocks that follow.  Backward: one pass over dx1 (csrc/lagg.hip
    lagg_collapse_kernel, or csrc/csr.hip over reverse edge lists when `csr` is given) instead of BatchNorm-backward
    statistics + apply + the conv's two backward products.  `group`: statistics over a process group (SyncBatchNorm)."""

    @staticmethod
    def forward(ctx, f, dp, idx, moments, weight, gamma, beta, eps, relu, bn=None, csr=None, group=None):
        s = _lagg_begin(ctx, f, dp, idx, moments, weight, gamma, beta, eps, relu, bn, csr)
        B, Cin, C, N, M, K = s.shape
        x1 = torch.empty(B, C, M, K, dtype=torch.float32, device=f.device)

        def call(phase):
            _lib.check(s.lib.amc3d_grouped_conv_bn_forward(*s.head, _ptr(x1), *s.tail(phase)), "grouped_conv_bn_forward")

        _lagg_finish(ctx, s, "grouped_conv_bn_forward", 4 * B * N * C + B * M * K * (4 * C + 16),
                     (4 if s.g_cm is None else 12) * B * N * C + B * M * K * (8 * C + 16), call,
                     moments, weight, gamma, beta, relu, bn, group, s.sums)
        return x1

    @staticmethod
    def backward(ctx, dx1):
        # without lists (no plan, not deterministic mode) the backward scatters with float atomics
        s = _lagg_backward_begin(ctx, True, lambda lib, B, C, N, M, K: lib.amc3d_grouped_conv_bn_csr_workspace_bytes(B, C, N, M, K))
        B, Cin, C, N, M, K = ctx.shape
        # SATailActivated hands the gradient over as position-major rows (a (B,C,M,K) view of a (B,M,K,C) buffer): the
        # gather along the reverse lists reads those directly; any other layout is made channel-major and transposed
        dx1_pm = s.csr is not None and dx1.dim() == 4 and dx1.permute(0, 2, 3, 1).is_contiguous() and C > 1
        if not dx1_pm:
            dx1 = dx1.contiguous()
        rev_dp = _ptr(s.csr[2]) if s.csr is not None and len(s.csr) > 2 and s.csr[2] is not None else None

        def call(phase):
            _lib.check(s.lib.amc3d_grouped_conv_bn_backward(
                *s.dims, _ptr(dx1), int(dx1_pm), _ptr(s.g_pm), _ptr(s.idx), *s.lists, rev_dp, *s.mid, *s.tail(phase)),
                "grouped_conv_bn_backward")

        return _lagg_backward_finish(ctx, s, "grouped_conv_bn_backward", B * M * K * (8 * C + 16) + 4 * B * N * C,
                                     B * M * K * (8 * C + 16) + 12 * B * N * C, call)


def _lagg_eval_begin(f, dp, idx, weight, bn, relu):
    """Either layer in inference mode (running statistics): runs the conv on the source points and returns (B, C, M, K) and
    the arguments of the layer's C call before and after its outputs"""
    f, dp, idx = f.contiguous(), dp.contiguous(), idx.contiguous()
    B, Cin, N = f.shape
    _, M, K = idx.shape
    C = weight.shape[0]
    lib = _lib.load()
    w2 = weight.detach().reshape(C, Cin + 3).contiguous()
    w_dp, ldw, w_f = _dp_f_blocks(w2, False)
    g_pm = torch.empty(B, N, C, dtype=torch.float32, device=f.device)
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    with torch.cuda.device(f.device):
        _pw_forward_rows(lib, B, Cin, C, N, f, w_f, g_pm)
    # `keep`: what the pointers point into, for the caller to hold until its launch
    keep = (f, dp, idx, w2, g_pm, invstd)
    head = (B, C, N, M, K, 0, int(bool(relu)), float(bn.eps), 0.0, None, _ptr(idx), _ptr(dp), _ptr(w_dp), ldw, None,
            _ptr(bn.weight), _ptr(bn.bias), _ptr(g_pm))
    tail = (_ptr(bn.running_mean), _ptr(invstd), None, None, None, None, None, 0, None, None, 0, _stream(f))
    return (B, C, M, K), head, tail, keep


@torch.no_grad()
def grouped_conv_bn_eval(f, dp, idx, weight, bn, relu):
    """GroupedConvBN in inference mode (running statistics), no gradient -> x1 (B,C,M,32)"""
    (B, C, M, K), head, tail, _keep = _lagg_eval_begin(f, dp, idx, weight, bn, relu)
    x1 = torch.empty(B, C, M, K, dtype=torch.float32, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().amc3d_grouped_conv_bn_forward(*head, _ptr(x1), *tail), "grouped_conv_bn_forward")
    return x1


def grouped_conv_bn_supported(cout, nsample):
    return bool(_lib.load().amc3d_grouped_conv_bn_supported(int(cout), int(nsample)))


@torch.no_grad()
def local_aggregation_eval(f, dp, idx, weight, bn, relu):
    """the same layer in inference mode (running statistics), no gradient"""
    (B, C, M, K), head, tail, _keep = _lagg_eval_begin(f, dp, idx, weight, bn, relu)
    pooled = torch.empty(B, C, M, dtype=torch.float32, device=f.device)
    ystar = torch.empty_like(pooled)
    arg = torch.empty(B, C, M, dtype=torch.uint8, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().amc3d_local_aggregation_forward(*head, _ptr(pooled), _ptr(arg), _ptr(ystar), *tail),
                   "local_aggregation_forward")
    return pooled


class PointwiseConv(Function):
    """y = conv1x1(x, weight, bias): nn.Conv1d / nn.Conv2d with kernel size 1 (models/layers/conv.py:8-21) on the
    fp32 MFMA kernels of csrc/pwconv.hip.  x (B,Cin,*spatial) fp32, weight (Cout,Cin,1[,1]), bias (Cout) or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, bf16=False, dx_position_major=False):
        _need_gpu(x, weight)
        _need_dtype(torch.float32, x=x, weight=weight, bias=bias)
        x = x.contiguous()
        B, Cin = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        Cout = weight.shape[0]
        assert weight.numel() == Cout * Cin, "pointwise_conv needs a 1x1 kernel"
        w2 = _weight_rows(weight.reshape(Cout, Cin), bf16)
        y = torch.empty((B, Cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        lib = _lib.load()
        with torch.cuda.device(x.device), timing.span("pointwise_conv_forward", 4 * B * P * (Cin + Cout),
                                                      2.0 * B * P * Cin * Cout):
            _pw_forward(lib, bf16, B, Cin, Cout, P, x, w2, bias.contiguous() if bias is not None else None, y)
        ctx.save_for_backward(x, w2)
        ctx.wshape = tuple(weight.shape)
        ctx.has_bias = bias is not None
        ctx.bf16 = bool(bf16)
        # dx as position-major rows (B,*spatial,Cin), returned as the permuted (B,Cin,*spatial) view: what the reverse-list
        # gather of GroupedConvBN.backward reads directly (fp32 kernels only)
        ctx.dx_pm = bool(dx_position_major) and not ctx.bf16 and Cin > 1
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        B, Cin = x.shape[0], x.shape[1]
        P = x[0, 0].numel()
        Cout = w2.shape[0]
        dy = dy.contiguous()
        dev = dy.device
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = torch.empty_like(x) if need_x else None
        if need_x and ctx.dx_pm:
            dx = torch.empty((B,) + tuple(x.shape[2:]) + (Cin,), dtype=torch.float32, device=dev)
        dw = torch.empty(Cout, Cin, dtype=torch.float32, device=dev) if need_w else None
        _, wbytes, bwd = _pw(_lib.load(), ctx.bf16)
        wb = int(wbytes(B, Cin, Cout, P))  # weight-gradient partials and / or the split-K partials of dx
        work = torch.empty(max(wb, 4), dtype=torch.uint8, device=dev)
        flops = 2.0 * B * P * Cin * Cout * (int(need_x) + int(need_w))
        with torch.cuda.device(dev), timing.span("pointwise_conv_backward",
                                                 4 * B * P * (Cout + Cin * int(need_x) + Cin * int(need_w)), flops,
                                                 moved=4 * B * P * ((Cin + Cout) * int(need_x) + (Cin + Cout) * int(need_w))):
            if ctx.dx_pm or _ld(w2) != Cin:
                _lib.check(_lib.load().amc3d_pointwise_conv_backward_strided(
                    B, Cin, Cout, P, _ptr(x), _ptr(w2), _ld(w2), _ptr(dy), _ptr(dx) if need_x else None, int(ctx.dx_pm),
                    _ptr(dw) if need_w else None, Cin, _ptr(work), wb, _stream(dy)), "pointwise_conv_backward")
            else:
                _lib.check(bwd(B, Cin, Cout, P, _ptr(x), _ptr(w2), _ptr(dy), _ptr(dx) if need_x else None,
                               _ptr(dw) if need_w else None, _ptr(work), wb, _stream(dy)), "pointwise_conv_backward")
        if need_x and ctx.dx_pm:
            dx = dx.permute(0, dx.dim() - 1, *range(1, dx.dim() - 1))
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(Cout, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.load().amc3d_bias_grad(B, Cout, P, _ptr(dy), _ptr(db), _stream(dy)), "bias_grad")
        return dx, (dw.view(ctx.wshape) if need_w else None), db, None, None


def pointwise_conv(x, weight, bias=None, bf16=False, dx_position_major=False):
    return PointwiseConv.apply(x, weight, bias, bf16, dx_position_major)


class PointwiseConvCloudTerm(Function):
    """y[b,:,p] = weight . x[b,:,p] + cloud_term[b,:]: a bias-free 1x1 convolution plus one Cout-vector per cloud, broadcast
    along its points (amc3d_pointwise_conv_cloud_term_forward).  x (B,Cin,P) fp32, weight (Cout,Cin[,1]) -- a column block
    of a wider matrix stays a view --, cloud_term (B,Cout).  The part-segmentation decoders' class-conditioned channels are
    constant along a cloud: cloud_term = e @ W_cls.T stands for their share of the conv, and its gradient, the per-cloud
    sums of dy (amc3d_cloud_term_grad), carries dW_cls and de through autograd on that small matmul.  dx and dweight are
    PointwiseConv's.  Never the BLAS or convolution library; no float atomics in either direction."""

    @staticmethod
    def forward(ctx, x, weight, cloud_term):
        _need_gpu(x, weight, cloud_term)
        _need_dtype(torch.float32, x=x, weight=weight, cloud_term=cloud_term)
        x = x.contiguous()
        assert x.dim() == 3, "pointwise_conv_cloud_term takes (B, Cin, P) features"
        B, Cin, P = x.shape
        Cout = weight.shape[0]
        assert weight.numel() == Cout * Cin, "pointwise_conv_cloud_term needs a 1x1 kernel"
        assert tuple(cloud_term.shape) == (B, Cout), "cloud_term is (B, Cout)"
        w2 = _weight_rows(weight.reshape(Cout, Cin), False)
        c = cloud_term.contiguous()
        y = torch.empty(B, Cout, P, dtype=torch.float32, device=x.device)
        lib = _lib.load()
        wsf = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(B, Cin, Cout, P, 0))
        work = torch.empty(wsf, dtype=torch.uint8, device=x.device) if wsf else None
        with torch.cuda.device(x.device), timing.span("pointwise_conv_cloud_term_forward", 4 * B * P * (Cin + Cout),
                                                      2.0 * B * P * Cin * Cout):
            _lib.check(lib.amc3d_pointwise_conv_cloud_term_forward(B, Cin, Cout, P, _ptr(x), _ptr(w2), _ld(w2), _ptr(c), _ptr(y),
                                                                   _ptr(work) if wsf else None, wsf, _stream(x)),
                       "pointwise_conv_cloud_term_forward")
        ctx.save_for_backward(x, w2)
        ctx.wshape = tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        B, Cin, P = x.shape
        Cout = w2.shape[0]
        dy = dy.contiguous()
        dev = dy.device
        need_x, need_w, need_c = ctx.needs_input_grad
        lib = _lib.load()
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty(Cout, Cin, dtype=torch.float32, device=dev) if need_w else None
        dc = torch.empty(B, Cout, dtype=torch.float32, device=dev) if need_c else None
        with torch.cuda.device(dev):
            # the backward products put the cloud on the grid's z axis: more than 65535 clouds go in runs of 65535, their
            # weight gradients added in run order (a fixed order)
            run = 65535
            for b0 in range(0, B if (need_x or need_w) else 0, run):
                nb = min(run, B - b0)
                dw_run = dw if b0 == 0 or not need_w else torch.empty_like(dw)
                wb = int(lib.amc3d_pointwise_conv_workspace_bytes(nb, Cin, Cout, P))
                work = torch.empty(max(wb, 4), dtype=torch.uint8, device=dev)
                _lib.check(lib.amc3d_pointwise_conv_backward_strided(
                    nb, Cin, Cout, P, _ptr(x[b0:]), _ptr(w2), _ld(w2), _ptr(dy[b0:]), _ptr(dx[b0:]) if need_x else None, 0,
                    _ptr(dw_run) if need_w else None, Cin, _ptr(work), wb, _stream(dy)), "pointwise_conv_backward")
                if need_w and b0:
                    dw += dw_run
            if need_c:
                _lib.check(lib.amc3d_cloud_term_grad(B, Cout, P, _ptr(dy), _ptr(dc), _stream(dy)), "cloud_term_grad")
        return dx, (dw.view(ctx.wshape) if need_w else None), dc


def pointwise_conv_cloud_term(x, weight, cloud_term):
    return PointwiseConvCloudTerm.apply(x, weight, cloud_term)


def _split_columns(w2, c1):
    """w2 (rows, c1 + c2) fp32 on the GPU -> contiguous (rows, c1), (rows, c2) in one launch (no autograd)"""
    w2 = w2.detach().contiguous()
    rows, c2 = w2.shape[0], w2.shape[1] - c1
    a = torch.empty(rows, c1, dtype=torch.float32, device=w2.device)
    b = torch.empty(rows, c2, dtype=torch.float32, device=w2.device)
    with torch.cuda.device(w2.device):
        _lib.check(_lib.load().amc3d_split_columns(rows, c1, c2, _ptr(w2), _ptr(a), _ptr(b), _stream(w2)), "split_columns")
    return a, b


def _join_columns(a, b):
    """(rows, c1), (rows, c2) -> (rows, c1 + c2) in one launch"""
    a, b = a.contiguous(), b.contiguous()
    rows, c1, c2 = a.shape[0], a.shape[1], b.shape[1]
    w = torch.empty(rows, c1 + c2, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().amc3d_join_columns(rows, c1, c2, _ptr(a), _ptr(b), _ptr(w), _stream(a)), "join_columns")
    return w


class SplitWeight(Function):
    """(w[:, :c1], w[:, c1:]) of a 1x1-conv weight (Cout, C1+C2, 1) as two (Cout, C) column views -- the two halves of a
    FeaturePropogation conv applied to the skip features and to the coarse features separately.  As torch slices the
    backward is zeros + copy per slice, an add, and zeros + copy for the select (7 launches per decoder level); here it is
    one concatenation."""

    @staticmethod
    def forward(ctx, weight, c1):
        w = weight.reshape(weight.shape[0], -1)
        ctx.wshape = tuple(weight.shape)
        if w.is_cuda and w.dtype == torch.float32 and w.stride(1) == 1:
            # the two column blocks where they lie: the conv kernels take a row stride, the library GEMMs a leading dimension
            return w[:, :c1], w[:, c1:]
        return w[:, :c1].contiguous(), w[:, c1:].contiguous()

    @staticmethod
    def backward(ctx, g1, g2):
        if g1.is_cuda and g1.dtype == torch.float32 and g2.dtype == torch.float32:
            return _join_columns(g1, g2).view(ctx.wshape), None
        return torch.cat((g1, g2), dim=1).view(ctx.wshape), None


def split_weight(weight, c1):
    return SplitWeight.apply(weight, c1)


class MaskedRefineDual(Function):
    """RefinementMethod.DualMasks with fusion 'MIN' (openpoints/AMContrast3D/MaskedRefine.py:55-131) on csrc/refine.hip: two
    launches forward, two backward, instead of ~25 tensor operations per decoder level.  feature (B,D,n) fp32, ambiguity
    (B,1,n) or (B*n,[1]) fp32 (no gradient: it only enters comparisons and an arg-min), neighbor_idx (B*n, K-1) int32 (a view
    with a row stride is fine).  -> (refined feature, count of refined points as a 0-dim int32 tensor)."""

    @staticmethod
    def forward(ctx, feature, ambiguity, neighbor_idx, threshold, threshold_max, gamma):
        _need_gpu(feature, ambiguity, neighbor_idx)
        _need_dtype(torch.float32, feature=feature, ambiguity=ambiguity)
        _need_dtype(torch.int32, neighbor_idx=neighbor_idx)
        f = feature.contiguous()
        a = ambiguity.detach().contiguous().view(-1)
        B, D, n = f.shape
        assert a.numel() == B * n and neighbor_idx.dim() == 2 and neighbor_idx.shape[0] == B * n
        nptr, k, stride, keep = _nbr_view(neighbor_idx)
        dev = f.device
        lib = _lib.load()
        out = torch.empty_like(f)
        best = torch.empty(B * n, dtype=torch.int32, device=dev)
        mask = torch.empty(B * n, dtype=torch.uint8, device=dev)
        count = torch.empty((), dtype=torch.int32, device=dev)
        work = torch.empty(max(int(lib.amc3d_masked_refine_workspace_ints(B * n)), 1), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev), timing.span("masked_refine_forward", f.numel() * 12 + B * n * (4 * k + 13)):
            _lib.check(lib.amc3d_masked_refine_forward(B, D, n, k, stride, _ptr(f), _ptr(a), nptr, float(threshold),
                                                       float(threshold_max), float(gamma), _ptr(out), _ptr(best), _ptr(mask),
                                                       _ptr(count), _ptr(work), _stream(f)), "masked_refine_forward")
        ctx.save_for_backward(best, mask)
        ctx.gamma = float(gamma)
        ctx.det = deterministic()
        ctx.mark_non_differentiable(count)
        return out, count

    @staticmethod
    def backward(ctx, dout, _dcount):
        best, mask = ctx.saved_tensors
        dout = dout.contiguous()
        B, D, n = dout.shape
        df = torch.empty_like(dout)
        if ctx.det:
            # the lists of best depend on the predicted ambiguity: built in the step itself, the B*n rows as one cloud
            rev_start, rev_edge = group_csr(best.view(1, B * n, 1), B * n)
            with torch.cuda.device(dout.device), timing.span("masked_refine_backward_csr", dout.numel() * 12 + B * n * 9):
                _lib.check(_lib.load().amc3d_masked_refine_backward_csr(B, D, n, ctx.gamma, _ptr(dout), _ptr(best), _ptr(mask),
                                                                        _ptr(rev_start), _ptr(rev_edge), _ptr(df), _stream(dout)),
                           "masked_refine_backward_csr")
            return df, None, None, None, None, None
        with torch.cuda.device(dout.device), timing.span("masked_refine_backward", dout.numel() * 12):
            _lib.check(_lib.load().amc3d_masked_refine_backward(B, D, n, ctx.gamma, _ptr(dout), _ptr(best), _ptr(mask), _ptr(df),
                                                                _stream(dout)), "masked_refine_backward")
        return df, None, None, None, None, None


class SAResidual(Function):
    """out = relu(y + skipconv(f[:, :, fps_idx])): the residual branch of a strided SetAbstraction block with use_res
    (pointnext_AA.py:157-168: torch.gather -> Conv1d with bias -> add -> ReLU) on csrc/sa_res.hip -- one launch forward;
    backward: ReLU mask + bias gradient + zero-fill, W^T . g scattered to the sampled columns, and the weight gradient.
    y (B,Cout,M) pooled main branch, f (B,Cin,N), fps_idx (B,M) int32, weight (Cout,Cin,1), bias (Cout) or None."""

    @staticmethod
    def forward(ctx, y, f, fps_idx, weight, bias, dup_flag=None):
        _need_gpu(y, f, fps_idx, weight)
        if dup_flag is not None:
            _need_gpu(dup_flag)
            _need_dtype(torch.int32, dup_flag=dup_flag)
        _need_dtype(torch.float32, y=y, f=f, weight=weight, bias=bias)
        _need_dtype(torch.int32, fps_idx=fps_idx)
        y, f, fps_idx = y.contiguous(), f.contiguous(), fps_idx.contiguous()
        B, Cin, N = f.shape
        Cout, M = weight.shape[0], fps_idx.shape[1]
        assert y.shape == (B, Cout, M) and fps_idx.shape[0] == B and weight.numel() == Cout * Cin
        w2 = weight.reshape(Cout, Cin).contiguous()
        bias = bias.contiguous() if bias is not None else None
        out = torch.empty_like(y)
        keep = any(ctx.needs_input_grad)
        fi = torch.empty(B, Cin, M, dtype=torch.float32, device=f.device) if keep else None
        with torch.cuda.device(f.device), timing.span("sa_residual_forward", 4 * B * M * (Cin * (2 if keep else 1) + 2 * Cout) + 4 * B * M,
                                                      2.0 * B * M * Cin * Cout):
            _lib.check(_lib.load().amc3d_sa_residual_forward(B, Cin, Cout, N, M, _ptr(f), _ptr(fps_idx), _ptr(w2),
                                                             _ptr(bias) if bias is not None else None, _ptr(y), _ptr(out),
                                                             _ptr(fi) if keep else None, _stream(f)), "sa_residual_forward")
        if keep:
            ctx.save_for_backward(out, fi, fps_idx, w2, *([dup_flag] if dup_flag is not None else []))
        ctx.n, ctx.wshape, ctx.has_bias = N, tuple(weight.shape), bias is not None
        ctx.det = deterministic()
        ctx.mark_non_differentiable(fps_idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, fi, fps_idx, w2 = ctx.saved_tensors[:4]
        dup_flag = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        B, Cout, M = out.shape
        Cin, N = w2.shape[1], ctx.n
        dout = dout.contiguous()
        dev = dout.device
        need_f, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        need_b = ctx.has_bias and ctx.needs_input_grad[4]
        if ctx.det and need_f:
            # unique picks take plain stores; duplicate picks (or picks nobody checked) add with float atomics
            if dup_flag is None:
                dup_flag = index_duplicates(fps_idx, N)
            if not torch.cuda.is_current_stream_capturing() and int(dup_flag):
                raise _no_route("sa_residual_backward", "fps_idx repeats an index")
        g = torch.empty_like(out)
        df = torch.empty(B, Cin, N, dtype=torch.float32, device=dev) if need_f else None
        dw = torch.empty(Cout, Cin, dtype=torch.float32, device=dev) if need_w else None
        db = torch.empty(Cout, dtype=torch.float32, device=dev) if need_b else None
        lib = _lib.load()
        wb = int(lib.amc3d_sa_residual_workspace_bytes(B, Cin, Cout, M))
        work = torch.empty(max(wb, 4), dtype=torch.uint8, device=dev)
        nbytes = 4 * B * M * 3 * Cout + (4 * B * Cin * N + 4 * B * M * Cout) * int(need_f) + 4 * B * M * (Cin + Cout) * int(need_w)
        with torch.cuda.device(dev), timing.span("sa_residual_backward", nbytes,
                                                 2.0 * B * M * Cin * Cout * (int(need_f) + int(need_w))):
            _lib.check(lib.amc3d_sa_residual_backward(B, Cin, Cout, N, M, _ptr(dout), _ptr(out), _ptr(fi), _ptr(fps_idx),
                                                      _ptr(dup_flag) if dup_flag is not None else None,
                                                      _ptr(w2), _ptr(g), _ptr(df) if need_f else None,
                                                      _ptr(dw) if need_w else None, _ptr(db) if need_b else None,
                                                      _ptr(work), wb, _stream(dout)), "sa_residual_backward")
        return g, df, None, (dw.view(ctx.wshape) if need_w else None), db, None


def sa_residual(y, f, fps_idx, weight, bias, dup_flag=None):
    """dup_flag: index_duplicates(fps_idx, N) of the plan, or None (the backward then adds with float atomics, right for any picks)"""
    return SAResidual.apply(y, f, fps_idx, weight, bias, dup_flag)


@torch.no_grad()
def index_duplicates(idx, n):
    """int32 [1] on the device: 1 if some row of idx (B, M) int32 into n points repeats an index, else 0 (no host sync)"""
    _need_gpu(idx)
    _need_dtype(torch.int32, idx=idx)
    idx = idx.contiguous()
    B, M = idx.shape
    flag = torch.empty(1, dtype=torch.int32, device=idx.device)
    lib = _lib.load()
    wb = int(lib.amc3d_index_duplicates_workspace_bytes(B, int(n)))
    work = torch.empty(max(wb, 4), dtype=torch.uint8, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.check(lib.amc3d_index_duplicates(B, int(n), M, _ptr(idx), _ptr(flag), _ptr(work), wb, _stream(idx)), "index_duplicates")
    return flag


def _library_wgrad(dy3, x3):
    """dW (Cout,Cin) = sum_b dy[b] . x[b]^T of a deep short layer.  Longer layers: batched library GEMM + sum over the
    batch.  The shortest ones (< 1024 positions per cloud, >= 128 channels: the two coarsest FeaturePropagation levels), where
    the batched form hits a slow library heuristic (256x256x375: 97 us) and one GEMM over (batch x positions) needs
    transposed copies of both operands: this library's streaming weight-gradient kernel (csrc/gemm.hip, fixed-order
    partial sums; the step takes the same time, measured, with 8 copies and 4 library launches fewer).  The form is a pure
    function of the shape -- the same in eager and captured runs and on every rank; AMC3D_WGRAD_FORM=bmm|flat|own
    overrides it."""
    import os
    B, Cout, P = dy3.shape
    Cin = x3.shape[1]
    form = os.environ.get("AMC3D_WGRAD_FORM") or ("own" if P < 1024 and min(Cin, Cout) >= 128 else "bmm")
    if form == "own":
        lib = _lib.load()
        dw = torch.empty(Cout, Cin, dtype=torch.float32, device=dy3.device)
        wb = int(lib.amc3d_pointwise_conv_workspace_bytes(B, Cin, Cout, P))
        work = torch.empty(max(wb, 4), dtype=torch.uint8, device=dy3.device)
        with torch.cuda.device(dy3.device):
            _lib.check(lib.amc3d_pointwise_conv_backward(B, Cin, Cout, P, _ptr(x3), None, _ptr(dy3), None, _ptr(dw), _ptr(work),
                                                         wb, _stream(dy3)), "pointwise_conv_backward")
        return dw
    if form == "flat":
        return torch.matmul(dy3.transpose(0, 1).reshape(Cout, B * P), x3.transpose(0, 1).reshape(Cin, B * P).t())
    return torch.bmm(dy3, x3.transpose(1, 2)).sum(0)


class LibraryGemmConv(Function):
    """1x1 convolution of a deep, short layer (>= 64 channels on both sides, < 65536 positions: SetAbstraction 4 and the
    coarse FeaturePropagation stages) as three plain library GEMMs.  These are small MFMA-bound GEMMs that rocBLAS does
    at ~80 TFLOP/s, twice what csrc/gemm.hip reaches at this size; what is avoided is the convolution library's
    weight-gradient path, which wraps an implicit-GEMM kernel in NCHW<->NHWC transposes (60-70 us per layer).
    x (B,Cin,*spatial) fp32 contiguous, weight (Cout,Cin,1[,1]), no bias."""

    @staticmethod
    def forward(ctx, x, weight, dx_position_major=False):
        x = x.contiguous()
        B, Cin = x.shape[0], x.shape[1]
        Cout = weight.shape[0]
        w2 = weight.reshape(Cout, Cin)
        ctx.dx_pm = bool(dx_position_major)
        timing.note("library_gemm_conv")
        # under bf16 autocast (use_amp, main_AA.py:389): bf16 operands for the three library GEMMs, fp32 accumulation inside the
        # library, fp32 results (tests/test_gpu_bf16.py) -- cfg 5 (XL + ++, 1 x 120000): 16.8 ms per step, 17.1 when the
        # results were still rounded to bf16 and widened again
        ctx.bf16 = bool(torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16)
        # bmm with the weight expanded along the batch (stride 0): torch.matmul(2-d, 3-d) would fold the batch into one
        # GEMM by way of a transposed copy of x.
        with torch.autocast("cuda", enabled=False):
            if ctx.bf16:  # bf16 operands, fp32 accumulation AND fp32 results (out_dtype: a bf16 result would be rounded)
                x16, w16 = x.view(B, Cin, -1).to(torch.bfloat16), w2.to(torch.bfloat16)
                y = torch.bmm(w16.unsqueeze(0).expand(B, Cout, Cin), x16, out_dtype=torch.float32)
                ctx.save_for_backward(x16, w16)
            else:
                y = torch.bmm(w2.unsqueeze(0).expand(B, Cout, Cin), x.view(B, Cin, -1))
                ctx.save_for_backward(x, w2)
        ctx.wshape = tuple(weight.shape)
        ctx.xshape = tuple(x.shape)
        return y.view((B, Cout) + tuple(x.shape[2:]))

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        B, Cin = x.shape[0], x.shape[1]
        dy3 = dy.contiguous().view(B, w2.shape[0], -1)
        if ctx.bf16:
            with torch.autocast("cuda", enabled=False):
                dy16 = dy3.to(torch.bfloat16)
                dx = (torch.bmm(w2.t().unsqueeze(0).expand(B, Cin, w2.shape[0]), dy16, out_dtype=torch.float32).view(ctx.xshape)
                      if ctx.needs_input_grad[0] else None)
                # each cloud's partial stays fp32 up to the fp32 sum over the batch
                dw = (torch.bmm(dy16, x.transpose(1, 2), out_dtype=torch.float32).sum(0).view(ctx.wshape)
                      if ctx.needs_input_grad[1] else None)
            return dx, dw, None
        with torch.autocast("cuda", enabled=False):
            dx = None
            if ctx.needs_input_grad[0] and ctx.dx_pm:
                # dy^T . W = (B,P,Cin) position-major rows, handed over as the permuted (B,Cin,*spatial) view
                rows = torch.bmm(dy3.transpose(1, 2), w2.unsqueeze(0).expand(B, w2.shape[0], Cin))
                rows = rows.view((B,) + tuple(x.shape[2:]) + (Cin,))
                dx = rows.permute(0, rows.dim() - 1, *range(1, rows.dim() - 1))
            elif ctx.needs_input_grad[0]:
                dx = torch.bmm(w2.t().unsqueeze(0).expand(B, Cin, w2.shape[0]), dy3).view(x.shape)
            dw = _library_wgrad(dy3, x.view(B, Cin, -1)).view(ctx.wshape) if ctx.needs_input_grad[1] else None
        return dx, dw, None


def library_gemm_conv(x, weight, dx_position_major=False):
    if deterministic():
        # the BLAS library's reduction order is not this library's to fix: csrc/gemm.hip (fp32) or gemm_bf16.hip (autocast),
        # both fixed-order
        return pointwise_conv(x, weight, None, mixed_precision(), dx_position_major)
    return LibraryGemmConv.apply(x, weight, dx_position_major)


def confusion_update(cm, invalid, logits, target, ignore_index=None):
    """cm (v,v) int64 += histogram of (target, argmax_c logits) for logits (B,C,N) fp32 and target (B,N) int64 -- the
    trainer's `cm.update(logits.argmax(dim=1), target)` (main_AA.py:414-415) as one launch; v = C (+1 with an ignore label:
    such points count in the extra row / column, openpoints/utils/metrics.py).  invalid (1) int64 += out-of-range targets."""
    _need_gpu(logits, target, cm, invalid)
    _need_dtype(torch.float32, logits=logits)
    _need_dtype(torch.int64, target=target, cm=cm, invalid=invalid)
    logits, target = logits.contiguous(), target.contiguous()
    B, C, N = logits.shape
    v = C + (1 if ignore_index is not None else 0)
    assert cm.is_contiguous() and cm.shape == (v, v) and target.shape == (B, N)
    with torch.cuda.device(logits.device), timing.span("confusion_update", logits.numel() * 4 + target.numel() * 8):
        _lib.check(_lib.load().amc3d_confusion_update(B, C, N, _ptr(logits), _ptr(target), int(ignore_index if ignore_index is not None else 0),
                                                      int(ignore_index is not None), _ptr(cm), _ptr(invalid), _stream(logits)),
                   "confusion_update")


_POINT_LOSS_DEN = {"count": 0, "weight": 1, "one": 2}


def _opt_ptr(t):
    return _ptr(t) if t is not None else None


def _class_table(t, C, name, dtype=torch.float32):
    """an optional per-class table of the point losses: contiguous, one entry per class"""
    if t is None:
        return None
    _need_gpu(t)
    _need_dtype(dtype, **{name: t})
    assert t.shape == (C,), f"{name} must hold one value per class: {tuple(t.shape)} for {C} classes"
    return t.contiguous()


def _ploss_begin(logits, target):
    """What every point-loss forward starts from: fp32 logits (B, C, *) and int64 targets on the GPU, the logits contiguous,
    the targets as (B, N) -> logits, target, (B, C, N)."""
    _need_gpu(logits, target)
    _need_dtype(torch.float32, logits=logits)
    _need_dtype(torch.int64, target=target)
    logits = logits.contiguous()
    B, C = logits.shape[0], logits.shape[1]
    N = logits[0, 0].numel()
    return logits, target.reshape(B, N).contiguous(), (B, C, N)


def _ploss_finish(ctx, op, span, nbytes, moved, logits, target, form, with_lse=True):
    """The rest of the forward: the lse (B, N) where the family saves one, {loss, den}, the workspace, the timing span, the call
    amc3d_<op>_forward(B, C, N, logits, target, *form(), [lse,] loss_den, workspace, bytes, stream) and what the backward reads.
    form() -> the entry's own arguments; the closure keeps its tables alive.  span: the stem of the span's name, stated by the
    caller (cross_entropy_general runs the softmax family's entries under its own)."""
    B, C = logits.shape[0], logits.shape[1]
    N = target.shape[1]
    dev = logits.device
    lse = [torch.empty(B, N, dtype=torch.float32, device=dev)] if with_lse else []
    loss_den = torch.empty(2, dtype=torch.float32, device=dev)
    lib = _lib.load()
    wb = int(lib.amc3d_cross_entropy_workspace_bytes(B, N))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), timing.span(span + "_forward", nbytes, moved=moved):
        _lib.check(getattr(lib, f"amc3d_{op}_forward")(B, C, N, _ptr(logits), _ptr(target), *form(), *map(_ptr, lse), _ptr(loss_den),
                                                       _ptr(work), wb, _stream(logits)), span + "_forward")
    ctx.save_for_backward(logits, target, *lse, loss_den)
    ctx.op, ctx.span, ctx.form = op, span, form
    return loss_den[0]


def _ploss_backward(ctx, g, n_args):
    """dlogits by amc3d_<op>_backward(B, C, N, logits, target, *form(), [lse,] loss_den, g, dlogits, stream), and a None for
    each of the forward's n_args other arguments."""
    logits, target, *lse, loss_den = ctx.saved_tensors
    B, C = logits.shape[0], logits.shape[1]
    N = target.shape[1]
    g = g.contiguous().to(torch.float32)
    d = torch.empty_like(logits)
    with torch.cuda.device(logits.device), timing.span(ctx.span + "_backward", B * N * (8 * C + 8 + 4 * len(lse))):
        _lib.check(getattr(_lib.load(), f"amc3d_{ctx.op}_backward")(B, C, N, _ptr(logits), _ptr(target), *ctx.form(), *map(_ptr, lse),
                                                                    _ptr(loss_den), _ptr(g), _ptr(d), _stream(logits)),
                   ctx.span + "_backward")
    return (d,) + (None,) * n_args


class CrossEntropyMean(Function):
    """nn.CrossEntropyLoss()(logits.transpose(1, 2).reshape(-1, C), target.flatten()) -- default arguments: mean
    over the targets != ignore_index -- on the channel-major logits (B, C, N) as the model returns them
    (loss/build.py:328,338-340), in one pass forward and one backward: the softmax family's form with only the ignore value
    set, on the native exp / log instructions (csrc/loss.hip)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        logits, target, (B, C, N) = _ploss_begin(logits, target)
        ignore_index = int(ignore_index)
        return _ploss_finish(ctx, "cross_entropy", "cross_entropy", B * N * (4 * C + 12), None, logits, target,
                             lambda: (ignore_index,))

    @staticmethod
    def backward(ctx, g):
        return _ploss_backward(ctx, g, 2)


def cross_entropy_mean(logits, target, ignore_index=-100):
    return CrossEntropyMean.apply(logits, target, ignore_index)


class PointLossSoftmax(Function):
    """The softmax family of csrc/loss.hip (pl_softmax_*; formulas in include/amc3d.h) on channel-major logits (B, C, N) with
    targets (B, N): F.cross_entropy with weight and label_smoothing, SmoothCrossEntropy, MaskedCrossEntropy, FocalLoss and
    Poly1CrossEntropyLoss of openpoints.loss are forms of it.  Two launches forward, one backward; the saved lse (B, N) spares
    the backward the two reduction walks."""

    @staticmethod
    def forward(ctx, logits, target, remap, ignore_index, mask, weight, weight_per_class, eps, eps_rule, gamma, alpha, poly, den,
                span="point_loss_softmax"):
        logits, target, (B, C, N) = _ploss_begin(logits, target)
        weight, alpha = _class_table(weight, C, "weight"), _class_table(alpha, C, "alpha")
        if remap is not None:
            _need_gpu(remap)
            _need_dtype(torch.int64, remap=remap)
            remap = remap.contiguous()
        if mask is not None:
            _need_gpu(mask)
            _need_dtype(torch.int32, mask=mask)
            mask = mask.reshape(B, N).contiguous()
        form = lambda: (_opt_ptr(remap), 0 if remap is None else remap.numel(), int(ignore_index if ignore_index is not None else 0),
                        int(ignore_index is not None), _opt_ptr(mask), _opt_ptr(weight), int(bool(weight_per_class)), float(eps),
                        int(eps_rule), float(gamma), _opt_ptr(alpha), float(poly), _POINT_LOSS_DEN[den])
        extra = 12 + (4 if mask is not None else 0)
        return _ploss_finish(ctx, "point_loss_softmax", span, B * N * (4 * C + extra), B * N * (4 * C * (3 if eps else 2) + extra),
                             logits, target, form)

    @staticmethod
    def backward(ctx, g):
        return _ploss_backward(ctx, g, 13)


def point_loss_softmax(logits, target, *, remap=None, ignore_index=None, mask=None, weight=None, weight_per_class=False,
                       eps=0.0, eps_rule=0, gamma=0.0, alpha=None, poly=0.0, den="count"):
    """logits (B, C, N) fp32, target (B, N) int64 -> the scalar loss.  remap: int64 label -> class table; ignore_index None: no
    target is ignored; mask (B, N) int32, a point counts iff its entry is 1; weight / alpha (C) fp32; eps_rule 0: torch's
    eps / C on every class, 1: SmoothCrossEntropy's eps / (C - 1) on the others; den 'count', 'weight' (sum of w[y]) or 'one'
    (a sum).  No table takes a gradient.  Safe under ops.deterministic_mode() and graph capture: fixed-order sums, no atomics."""
    return PointLossSoftmax.apply(logits, target, remap, ignore_index, mask, weight, weight_per_class, eps, eps_rule, gamma, alpha,
                                  poly, den)


def cross_entropy_general(logits, target, ignore_index=-100, label_smoothing=0.0, weight=None):
    """F.cross_entropy(logits, target, weight, ignore_index=..., reduction='mean', label_smoothing=...) on channel-major
    logits (B, C, N) with targets (B, N): the plain PointNeXt trainer's criterion (examples/segmentation/main.py:224-230), a form
    of the softmax family under spans of its own.  ignore_index None: no target is ignored.  The class weights take no gradient."""
    return PointLossSoftmax.apply(logits, target, None, ignore_index, None, weight, True, label_smoothing, 0, 0.0, None, 0.0,
                                  "weight", "cross_entropy_general")


class PointLossSigmoid(Function):
    """The sigmoid family of csrc/loss.hip (pl_sigmoid_*; formulas in include/amc3d.h): elementwise over (B, C, N) against the
    one-hot of target (B, N), formed on the fly -- BCELogits and Poly1FocalLoss of openpoints.loss.  Two launches forward, one
    backward; the backward recomputes each element from the logits (nothing per element is saved)."""

    @staticmethod
    def forward(ctx, logits, target, weight, pos_weight, alpha, gamma, poly, den):
        logits, target, (B, C, N) = _ploss_begin(logits, target)
        weight, pos_weight = _class_table(weight, C, "weight"), _class_table(pos_weight, C, "pos_weight")
        form = lambda: (_opt_ptr(weight), _opt_ptr(pos_weight), float(-1.0 if alpha is None else alpha), float(gamma), float(poly),
                        _POINT_LOSS_DEN[den])
        return _ploss_finish(ctx, "point_loss_sigmoid", "point_loss_sigmoid", B * N * (4 * C + 8), None, logits, target, form,
                             with_lse=False)

    @staticmethod
    def backward(ctx, g):
        return _ploss_backward(ctx, g, 7)


def point_loss_sigmoid(logits, target, *, weight=None, pos_weight=None, alpha=None, gamma=0.0, poly=0.0, den="count"):
    """logits (B, C, N) fp32, target (B, N) int64 -> the scalar loss over the elements of the counted points (target in
    [0, C)): mean (den 'count') or sum (den 'one').  weight / pos_weight (C) fp32 per class; alpha None or negative: no
    alpha_t.  Safe under ops.deterministic_mode() and graph capture."""
    return PointLossSigmoid.apply(logits, target, weight, pos_weight, alpha, gamma, poly, den)


class SATail(Function):
    """pooled (B,C2,M) = max_k [relu2](bn2(conv2(relu(bn1(y1)))))  -- the tail of a two-layer SetAbstraction block
    (pointnext_AA.py:104-127, 164-166) from the first conv's raw output y1 (B,C1,M,32), with batch statistics for both
    BatchNorms, without materialising any (B,C,M,32) tensor after y1 (csrc/sa_tail.hip re-creates them per tile).
    `bn1`, `bn2`: the nn.BatchNorm2d modules whose running buffers are updated (or None)."""

    @staticmethod
    def forward(ctx, y1, g1, b1, eps1, w2, g2, b2, eps2, relu2, bn1=None, bn2=None):
        _need_gpu(y1, g1, b1, w2, g2, b2)
        y1 = y1.contiguous()
        B, C1, M, K = y1.shape
        C2 = w2.shape[0]
        dev = y1.device
        lib = _lib.load()
        assert w2.numel() == C2 * C1 and lib.amc3d_sa_tail_supported(C1, C2, K)
        w2f = w2.reshape(C2, C1).contiguous()
        mean1, invstd1, var1 = _bn_stat_bufs(C1, dev)
        mean2, invstd2, var2 = _bn_stat_bufs(C2, dev)
        pooled = torch.empty(B, C2, M, dtype=torch.float32, device=dev)
        # the raw extreme the pool selected and the neighbour that held it: the backward then recomputes nothing (csrc/sa_tail.hip)
        zext = torch.empty(B, C2, M, dtype=torch.float32, device=dev)
        arg = torch.empty(B, C2, M, dtype=torch.uint8, device=dev)
        work1, wb1 = _bn_ws(C1, dev)
        wb = int(lib.amc3d_sa_tail_workspace_bytes(B, C1, C2, M))
        work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        mom2, rm2, rv2, nbt2 = _bn_running_args(bn2)
        flops = 2.0 * B * M * K * C1 * C2 * 2  # the 1x1 conv is evaluated twice (statistics pass, max pass)
        with torch.cuda.device(dev), timing.span("sa_tail_forward", y1.numel() * 4 + pooled.numel() * 5, flops, moved=y1.numel() * 4 * 3 + pooled.numel() * 5):
            _lib.check(lib.amc3d_bn_stats(B, C1, M * K, float(eps1), _ptr(y1), _ptr(mean1), _ptr(invstd1), _ptr(var1),
                                          _ptr(work1), wb1, _stream(y1)), "bn_stats")
            _lib.check(lib.amc3d_sa_tail_forward(B, C1, C2, M, K, _ptr(y1), _ptr(mean1), _ptr(invstd1), _ptr(g1), _ptr(b1),
                                                 _ptr(w2f), _ptr(g2), _ptr(b2), float(eps2), mom2, int(bool(relu2)),
                                                 _ptr(pooled), _ptr(mean2), _ptr(invstd2), _ptr(var2), rm2, rv2,
                                                 nbt2, _ptr(zext), _ptr(arg), _ptr(work), wb, _stream(y1)), "sa_tail_forward")
        if bn1 is not None and bn1.track_running_stats and bn1.running_mean is not None:
            bn_update_running(bn1, mean1, var1)
        if bn2 is not None and bn2.track_running_stats and bn2.running_mean is not None and bn2.momentum is None:
            bn_update_running(bn2, mean2, var2)  # cumulative average: its own launch
        ctx.save_for_backward(y1, g1, b1, w2f, g2, b2, mean1, invstd1, mean2, invstd2, zext, arg)
        ctx.relu2, ctx.wshape = bool(relu2), tuple(w2.shape)
        ctx.pool_seq = _next_pool_seq() if _pool_log is not None else None
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        y1, g1, b1, w2f, g2, b2, mean1, invstd1, mean2, invstd2, zext, arg_ext = ctx.saved_tensors
        B, C1, M, K = y1.shape
        C2 = w2f.shape[0]
        dev = y1.device
        dpooled = dpooled.contiguous()
        lib = _lib.load()
        dx1 = torch.empty_like(y1)
        dw2 = torch.empty(C2, C1, dtype=torch.float32, device=dev)
        dg2, db2 = torch.empty_like(g2), torch.empty_like(b2)
        wb = int(lib.amc3d_sa_tail_workspace_bytes(B, C1, C2, M))
        work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        dy1 = torch.empty_like(y1)
        dg1, db1 = torch.empty_like(g1), torch.empty_like(b1)
        work1, wb1 = _bn_ws(C1, dev, extra=C1 * 8)
        arg = None
        if ctx.pool_seq is not None and _pool_log is not None:  # tests: the forward pass keeps no arg-max, backward re-derives it
            arg = _pool_log[ctx.pool_seq] = torch.empty(B, C2, M, dtype=torch.uint8, device=dev)
        flops = 2.0 * B * M * K * C1 * C2 * 4  # recompute twice + dx1 + dW2
        with torch.cuda.device(dev), timing.span("sa_tail_backward", y1.numel() * 4 * 2 + dpooled.numel() * 10, flops, moved=y1.numel() * 4 * 6 + dpooled.numel() * 10):
            _lib.check(lib.amc3d_sa_tail_backward(B, C1, C2, M, K, _ptr(y1), _ptr(mean1), _ptr(invstd1), _ptr(g1), _ptr(b1),
                                                  _ptr(w2f), _ptr(mean2), _ptr(invstd2), _ptr(g2), _ptr(b2), int(ctx.relu2),
                                                  _ptr(dpooled), _ptr(zext), _ptr(arg_ext), _ptr(dx1), 0, _ptr(dw2), _ptr(dg2), _ptr(db2),
                                                  _ptr(arg) if arg is not None else None,
                                                  _ptr(work), wb, _stream(y1)), "sa_tail_backward")
            # BN1 + ReLU backward on the raw y1 (csrc/bn.hip)
            _lib.check(lib.amc3d_bn_backward(B, C1, M * K, 1, 1, _ptr(y1), _ptr(dx1), None, _ptr(mean1), _ptr(invstd1),
                                             _ptr(g1), _ptr(b1), _ptr(dy1), _ptr(dg1), _ptr(db1), _ptr(work1), wb1,
                                             _stream(y1)), "bn_backward")
        return dy1, dg1, db1, None, dw2.view(ctx.wshape), dg2, db2, None, None, None, None


_identity_bn = {}  # (C, device) -> (zeros, ones): BatchNorm parameters under which relu(bn(x)) == x for x >= 0


class SATailActivated(Function):
    """pooled (B,C2,M) = max_k [relu2](bn2(conv2(x1))) from the ACTIVATED first-layer output x1 = relu(bn1(y1)) >= 0
    (ops.GroupedConvBN): SATail's recomputing kernels with an identity first BatchNorm; the gradient it returns is dx1."""

    @staticmethod
    def forward(ctx, x1, w2, g2, b2, eps2, relu2, bn2=None):
        _need_gpu(x1, w2, g2, b2)
        x1 = x1.contiguous()
        B, C1, M, K = x1.shape
        C2 = w2.shape[0]
        dev = x1.device
        lib = _lib.load()
        assert w2.numel() == C2 * C1 and lib.amc3d_sa_tail_supported(C1, C2, K)
        key = (C1, str(dev))
        if key not in _identity_bn:
            _identity_bn[key] = (torch.zeros(C1, dtype=torch.float32, device=dev), torch.ones(C1, dtype=torch.float32, device=dev))
        zeros, ones = _identity_bn[key]
        w2f = w2.reshape(C2, C1).contiguous()
        mean2, invstd2, var2 = _bn_stat_bufs(C2, dev)
        pooled = torch.empty(B, C2, M, dtype=torch.float32, device=dev)
        zext = torch.empty(B, C2, M, dtype=torch.float32, device=dev)
        arg = torch.empty(B, C2, M, dtype=torch.uint8, device=dev)
        wb = int(lib.amc3d_sa_tail_workspace_bytes(B, C1, C2, M))
        work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        mom2, rm2, rv2, nbt2 = _bn_running_args(bn2)
        with torch.cuda.device(dev), timing.span("sa_tail_forward", x1.numel() * 4 + pooled.numel() * 10, 2.0 * B * M * K * C1 * C2):
            _lib.check(lib.amc3d_sa_tail_forward(B, C1, C2, M, K, _ptr(x1), _ptr(zeros), _ptr(ones), _ptr(ones), _ptr(zeros),
                                                 _ptr(w2f), _ptr(g2), _ptr(b2), float(eps2), mom2, int(bool(relu2)),
                                                 _ptr(pooled), _ptr(mean2), _ptr(invstd2), _ptr(var2), rm2, rv2,
                                                 nbt2, _ptr(zext), _ptr(arg), _ptr(work), wb, _stream(x1)), "sa_tail_forward")
        if bn2 is not None and bn2.track_running_stats and bn2.running_mean is not None and bn2.momentum is None:
            bn_update_running(bn2, mean2, var2)
        ctx.save_for_backward(x1, w2f, g2, b2, mean2, invstd2, zeros, ones, zext, arg)
        ctx.relu2, ctx.wshape = bool(relu2), tuple(w2.shape)
        ctx.pool_seq = _next_pool_seq() if _pool_log is not None else None
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        x1, w2f, g2, b2, mean2, invstd2, zeros, ones, zext, arg_ext = ctx.saved_tensors
        B, C1, M, K = x1.shape
        C2 = w2f.shape[0]
        dev = x1.device
        dpooled = dpooled.contiguous()
        lib = _lib.load()
        # x1 comes from GroupedConvBN, whose backward gathers position-major rows: the gradient is written as
        # (B,M,K,C1) and returned as a (B,C1,M,K) view of it -- no transpose pass between the two (393 MB at SA1)
        import os
        pm = C1 % 4 == 0 and C1 > 1 and not os.environ.get("AMC3D_SAT_DX1_CM")
        if pm:
            dx1_buf = torch.empty(B, M, K, C1, dtype=torch.float32, device=dev)
            dx1 = dx1_buf.permute(0, 3, 1, 2)
        else:
            dx1_buf = dx1 = torch.empty_like(x1)
        dw2 = torch.empty(C2, C1, dtype=torch.float32, device=dev)
        dg2, db2 = torch.empty_like(g2), torch.empty_like(b2)
        wb = int(lib.amc3d_sa_tail_workspace_bytes(B, C1, C2, M))
        work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        arg = None
        if ctx.pool_seq is not None and _pool_log is not None:
            arg = _pool_log[ctx.pool_seq] = torch.empty(B, C2, M, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev), timing.span("sa_tail_backward", x1.numel() * 4 * 2 + dpooled.numel() * 10,
                                                 2.0 * B * M * K * C1 * C2 * 4, moved=x1.numel() * 4 * 3 + dpooled.numel() * 10):
            _lib.check(lib.amc3d_sa_tail_backward(B, C1, C2, M, K, _ptr(x1), _ptr(zeros), _ptr(ones), _ptr(ones), _ptr(zeros),
                                                  _ptr(w2f), _ptr(mean2), _ptr(invstd2), _ptr(g2), _ptr(b2), int(ctx.relu2),
                                                  _ptr(dpooled), _ptr(zext), _ptr(arg_ext), _ptr(dx1_buf), int(pm), _ptr(dw2), _ptr(dg2), _ptr(db2),
                                                  _ptr(arg) if arg is not None else None,
                                                  _ptr(work), wb, _stream(x1)), "sa_tail_backward")
        return dx1, dw2.view(ctx.wshape), dg2, db2, None, None, None


def sa_tail_supported(c1, c2, k):
    return bool(_lib.load().amc3d_sa_tail_supported(int(c1), int(c2), int(k)))


def sa_tail_pays(c1, c2):
    return bool(_lib.load().amc3d_sa_tail_pays(int(c1), int(c2)))


def vote_parts(logits, parts_tables):
    """The vote of whole-room testing over a voxel partition (csrc/room_eval.hip): logits (P,C,nvox) fp32, the stacked
    model outputs of the P sub-clouds of input_pipeline.room_parts, whose result is `parts_tables` -> (voted (N,C) fp32,
    pred (N) int64).  A point of rank r in a voxel of count c lies in parts r, r + c, ... < P; its logits are summed in
    that order and divided by their number, so the bits do not change from run to run (torch_scatter's mean, main_AA.py:662,
    sums in the order its atomics land).  pred = argmax as torch.argmax (first maximum, NaN counts as maximum)."""
    t = parts_tables
    _need_gpu(logits, t["where"], t["start"], t["count"], t["idx_sort"], t["voxel_idx"])
    _need_dtype(torch.float32, logits=logits)
    _need_dtype(torch.int32, where=t["where"], start=t["start"], count=t["count"], idx_sort=t["idx_sort"],
                voxel_idx=t["voxel_idx"])
    logits = logits.contiguous()
    P, C, nvox = logits.shape
    N = t["idx_sort"].shape[0]
    if t["where"].shape != (P, nvox) or t["count"].shape != (nvox,) or t["start"].shape[0] < nvox or t["voxel_idx"].shape != (N,):
        raise ValueError(f"vote_parts: logits {tuple(logits.shape)} do not belong to these tables "
                         f"(where {tuple(t['where'].shape)}, {t['count'].shape[0]} voxels)")
    voted = torch.empty(N, C, dtype=torch.float32, device=logits.device)
    pred = torch.empty(N, dtype=torch.int64, device=logits.device)
    with torch.cuda.device(logits.device), timing.span("vote_parts", logits.numel() * 4 + N * C * 4 + N * 28):
        _lib.check(_lib.load().amc3d_vote_parts(N, P, C, nvox, _ptr(logits), _ptr(t["where"].contiguous()),
                                                _ptr(t["start"].contiguous()), _ptr(t["count"].contiguous()),
                                                _ptr(t["idx_sort"].contiguous()), _ptr(t["voxel_idx"].contiguous()),
                                                _ptr(voted), _ptr(pred), _stream(logits)), "vote_parts")
    return voted, pred


def expand_parts(logits, tables):
    """`test_mode: nearest_neighbor` (main.py:605, all_logits[reverse_idx_part][voxel_idx][reverse_idx]) as one gather
    (csrc/room_eval.hip): logits (1,C,nvox) fp32, the model output of the single sub-cloud of
    input_pipeline.room_representatives, whose result is `tables` -> (voted (N,C) fp32, pred (N) int64).  Every room point
    takes the logits of its voxel's representative; pred = argmax as torch.argmax (first maximum, NaN counts as maximum)."""
    t = tables
    _need_gpu(logits, t["where"], t["idx_sort"], t["voxel_idx"])
    _need_dtype(torch.float32, logits=logits)
    _need_dtype(torch.int32, where=t["where"], idx_sort=t["idx_sort"], voxel_idx=t["voxel_idx"])
    logits = logits.contiguous()
    if logits.dim() != 3 or logits.shape[0] != 1:
        raise ValueError(f"expand_parts: logits (1,C,nvox) of the one sub-cloud of representatives, got {tuple(logits.shape)}")
    _, C, nvox = logits.shape
    N = t["idx_sort"].shape[0]
    if t["where"].shape != (1, nvox) or t["count"].shape != (nvox,) or t["voxel_idx"].shape != (N,):
        raise ValueError(f"expand_parts: logits {tuple(logits.shape)} do not belong to these tables "
                         f"(where {tuple(t['where'].shape)}, {t['count'].shape[0]} voxels)")
    voted = torch.empty(N, C, dtype=torch.float32, device=logits.device)
    pred = torch.empty(N, dtype=torch.int64, device=logits.device)
    with torch.cuda.device(logits.device), timing.span("expand_parts", nvox * C * 4 + N * C * 4 + N * 20):
        _lib.check(_lib.load().amc3d_expand_parts(N, C, nvox, _ptr(logits), _ptr(t["where"].contiguous()),
                                                  _ptr(t["idx_sort"].contiguous()), _ptr(t["voxel_idx"].contiguous()),
                                                  _ptr(voted), _ptr(pred), _stream(logits)), "expand_parts")
    return voted, pred


# ----------------------------------------------------------------------------------------------
# separable neighbourhood aggregation of ASSA (csrc/assa.hip)
# ----------------------------------------------------------------------------------------------
_ASSA_REDUCTION = {"mean": 0, "avg": 0, "sum": 1, "max": 2}


def _transpose_cn(x, B, C, n):
    """(B,C,n) -> (B,n,C) fp32, the coalesced LDS-tiled transpose of PointMajorRows"""
    out = torch.empty(B, n, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().amc3d_transpose_cn(B, C, n, _ptr(x), _ptr(out), _stream(x)), "transpose_cn")
    return out


class SeparableAggregation(Function):
    """out[b, d*C + c, m] = red_k dp[b,d,m,k] * f[b,c,idx[b,m,k]] (d in 0..2; reduction 'mean' / 'sum' / 'max'): the
    aggregation between ASSA's pre- and post-convolutions (local_aggregation.py:127-131) without a (B,C,M,K) or
    (B,3C,M,K) tensor.  f (B,C,N) fp32, idx (B,M,K) int32, dp (B,3,M,K) fp32 -> (B,3C,M), d-major.  The gradient reaches f
    only.  csr: group_csr(idx, N) of the geometry plan or None; read in deterministic mode only, which builds the lists in
    backward when the plan has none (the default backward scatters with float atomics and ignores them).
    The arithmetic and its order are fixed (include/amc3d.h; tests/assa_ref.py restates them in NumPy)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, f, idx, dp, reduction="mean", csr=None):
        _need_gpu(f, idx, dp)
        _need_dtype(torch.float32, f=f, dp=dp)
        _need_dtype(torch.int32, idx=idx)
        if reduction not in _ASSA_REDUCTION:
            raise NotImplementedError(f"reduction {reduction} not implemented")
        red = _ASSA_REDUCTION[reduction]
        f, idx, dp = f.contiguous(), idx.contiguous(), dp.contiguous()
        B, C, N = f.shape
        _, M, K = idx.shape
        if idx.shape[0] != B or dp.shape != (B, 3, M, K):
            raise ValueError(f"SeparableAggregation: f {tuple(f.shape)}, idx {tuple(idx.shape)}, dp {tuple(dp.shape)} do not fit")
        if K > 255:
            raise ValueError("SeparableAggregation: at most 255 neighbours per query")
        out = torch.empty(B, 3 * C, M, dtype=torch.float32, device=f.device)
        arg = torch.empty(B, M, 3 * C, dtype=torch.uint8, device=f.device) if red == 2 else None
        with torch.cuda.device(f.device), timing.span("assa_aggregate", f.numel() * 8 + idx.numel() * 16 + out.numel() * 4):
            f_pm = _transpose_cn(f, B, C, N)
            _lib.check(_lib.load().amc3d_assa_aggregate_forward(B, C, N, M, K, red, _ptr(f_pm), _ptr(idx), _ptr(dp), _ptr(out),
                                                                _ptr(arg) if arg is not None else None, _stream(f)),
                       "assa_aggregate_forward")
        ctx.assa = (idx, dp, arg, csr, red, N)
        ctx.det = deterministic()
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        idx, dp, arg, csr, red, N = ctx.assa
        g = grad_out.detach().contiguous()
        B, C3, M = g.shape
        C, K = C3 // 3, idx.shape[-1]
        lib = _lib.load()
        aptr = _ptr(arg) if arg is not None else None
        gathers = ctx.det  # default mode scatters at every shape (the lists cost a sort the gather does not win back)
        if gathers and csr is None:
            csr = group_csr(idx, N)
        df_pm = torch.empty(B, N, C, dtype=torch.float32, device=g.device)  # both entries write every element
        with torch.cuda.device(g.device), timing.span("assa_aggregate_grad", g.numel() * 8 + idx.numel() * 16 + idx.numel() * C * 4):
            g_pm = _transpose_cn(g, B, C3, M)
            if gathers:
                _lib.check(lib.amc3d_assa_aggregate_backward_csr(B, C, N, M, K, red, _ptr(g_pm), _ptr(dp), aptr, _ptr(csr[0]),
                                                                 _ptr(csr[1]), _ptr(df_pm), _stream(g)),
                           "assa_aggregate_backward_csr")
            else:
                _lib.check(lib.amc3d_assa_aggregate_backward(B, C, N, M, K, red, _ptr(g_pm), _ptr(idx), _ptr(dp), aptr,
                                                             _ptr(df_pm), _stream(g)), "assa_aggregate_backward")
            df = torch.empty(B, C, N, dtype=torch.float32, device=g.device)
            _lib.check(lib.amc3d_transpose_cn(B, N, C, _ptr(df_pm), _ptr(df), _stream(g)), "transpose_cn")
        return df, None, None, None, None


def separable_aggregation(f, idx, dp, reduction="mean", csr=None):
    """SeparableAggregation.apply; csr = (rev_start, rev_edge) of group_csr(idx, N) where the plan has them"""
    return SeparableAggregation.apply(f, idx, dp, reduction, csr)


# the offset-layout (ragged-batch) operators of the pointops surface -- furthest sampling, ball query, grouping,
# subtraction, aggregation, interpolation -- live in offset_ops.py (ops.offset_ops.Grouping, ...): this file's BallQuery and
# friends are the dense (B,N,.) forms of the same names
from . import offset_ops  # noqa: E402,F401
