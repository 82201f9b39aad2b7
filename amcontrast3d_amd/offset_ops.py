"""The offset-layout ("pointops") operators on MI355X: autograd front-ends over csrc/pointops.hip.

Ragged batches: rows (n_total, .) plus cumulative segment ends `offset`, clouds of different sizes in one batch.  These
mirror the reference's openpoints/cpp/pointops/functions/pointops.py (argument meaning, dtypes, shapes, outputs):

    FurthestSampling, BallQuery, Grouping, Subtraction, Aggregation, Interpolation     pointops.py:10-29, 59-109, 181-305

Features are channel-last; indices are int32 global row ids.  In deterministic mode (ops.deterministic) the four
scatter gradients gather over reverse lists (amc3d_group_csr with b = 1, then amc3d_pointops_scatter_csr); the row-local
gradients never use atomics.  CPU tensors are rejected: there is no fallback path.
"""
import torch
from torch.autograd import Function

from . import _lib, timing
from . import ops as _o


def _ptr(t):
    return _o._ptr(t)


def _ends(name, t):
    """the cumulative segment ends as host ints (one read-back, as the reference's wrapper does for n_max)"""
    if t.dim() != 1 or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty 1-D tensor of cumulative segment ends")
    ends = [int(v) for v in t.tolist()]
    if ends[0] < 0 or any(b < a for a, b in zip(ends, ends[1:])):
        raise ValueError(f"{name} is not non-decreasing: {ends}")
    return ends


def _check_offsets(offset, new_offset, n, m=None):
    off, noff = _ends("offset", offset), _ends("new_offset", new_offset)
    if len(off) != len(noff):
        raise ValueError(f"offset has {len(off)} segments, new_offset {len(noff)}")
    if off[-1] != n:
        raise ValueError(f"offset ends at {off[-1]} but xyz has {n} rows")
    if m is not None and noff[-1] != m:
        raise ValueError(f"new_offset ends at {noff[-1]} but new_xyz has {m} rows")
    return off, noff


def _counts(ends):
    return [b - a for a, b in zip([0] + ends[:-1], ends)]


class FurthestSampling(Function):
    @staticmethod
    def forward(ctx, xyz, offset, new_offset):
        """xyz (n,3), offset (b), new_offset (b) int32 cumulative ends -> idx (m) int32 global rows, the first pick of a
        segment its first row.  Segments of one length and one sample count run on the dense sampler (the same picks)."""
        assert xyz.is_contiguous()
        n = xyz.shape[0]
        off, noff = _check_offsets(offset, new_offset, n)
        cn, cm = _counts(off), _counts(noff)
        for s, (a, b) in enumerate(zip(cn, cm)):
            if b > a:
                raise ValueError(f"segment {s} asks for {b} samples of {a} points")
        _o._need_gpu(xyz, offset, new_offset)
        _o._need_dtype(torch.float32, xyz=xyz)
        _o._need_dtype(torch.int32, offset=offset, new_offset=new_offset)
        nb, m = len(off), noff[-1]
        lib = _lib.load()
        dev = xyz.device
        idx = torch.empty(m, dtype=torch.int32, device=dev)
        if m and len(set(cn)) == 1 and len(set(cm)) == 1:
            ns, msamp = cn[0], cm[0]
            temp = torch.full((nb, ns), 1e10, dtype=torch.float32, device=dev) if ns > 262144 else None
            wb = int(lib.amc3d_fps_workspace_bytes(nb, ns))
            with torch.cuda.device(dev), timing.span("pointops_furthestsampling", n * 12 + m * 4):
                work = torch.empty(max(wb, 4), dtype=torch.uint8, device=dev)
                _lib.check(lib.amc3d_furthest_point_sampling(nb, ns, msamp, _ptr(xyz), _ptr(temp) if temp is not None else None,
                                                             _ptr(idx), _ptr(work), wb, _o._stream(xyz)),
                           "furthest_point_sampling")
            idx = (idx.view(nb, msamp) + torch.arange(nb, dtype=torch.int32, device=dev).mul_(ns).unsqueeze(1)).view(m)
        elif m:
            tmp = torch.full((n,), 1e10, dtype=torch.float32, device=dev)
            offset, new_offset = offset.contiguous(), new_offset.contiguous()
            with torch.cuda.device(dev), timing.span("pointops_furthestsampling", n * 12 + m * 4):
                _lib.check(lib.amc3d_pointops_furthestsampling(nb, max(cn), n, _ptr(xyz), _ptr(offset), _ptr(new_offset),
                                                               _ptr(tmp), _ptr(idx), _o._stream(xyz)),
                           "pointops_furthestsampling")
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


furthestsampling = FurthestSampling.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz, offset, new_offset):
        """xyz (n,3), new_xyz (m,3), offset / new_offset (b) -> idx (m,nsample) int32 global rows: the first nsample support
        rows of the query's segment within the radius, padded with the first hit; zeros where there is none"""
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.is_contiguous() and new_xyz.is_contiguous()
        n, m = xyz.shape[0], new_xyz.shape[0]
        off, _ = _check_offsets(offset, new_offset, n, m)
        _o._need_gpu(xyz, new_xyz, offset, new_offset)
        _o._need_dtype(torch.float32, xyz=xyz, new_xyz=new_xyz)
        _o._need_dtype(torch.int32, offset=offset, new_offset=new_offset)
        nsample = int(nsample)
        idx = torch.empty(m, nsample, dtype=torch.int32, device=xyz.device)
        offset, new_offset = offset.contiguous(), new_offset.contiguous()
        with torch.cuda.device(xyz.device), timing.span("pointops_ballquery", (n + m) * 12 + m * nsample * 4):
            _lib.check(_lib.load().amc3d_pointops_ballquery(m, float(radius), nsample, n, len(off), _ptr(xyz), _ptr(new_xyz),
                                                            _ptr(offset), _ptr(new_offset), _ptr(idx), _o._stream(xyz)),
                       "pointops_ballquery")
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None, None, None


ballquery = BallQuery.apply


def _index(idx, rows, name="idx"):
    _o._need_dtype(torch.int32, **{name: idx})
    assert idx.is_contiguous() and idx.dim() == 2 and idx.shape[0] == rows, (tuple(idx.shape), rows)
    return idx


def _scatter_csr(kind, idx, n_targets, c, per, w_c, g, w):
    """out (n_targets,c): the scatter of `kind` as a gather over the reverse lists of idx (every element written)"""
    rev_start, rev_edge = _o.group_csr(idx.view(1, idx.shape[0], idx.shape[1]), n_targets)
    return _scatter_csr_lists(kind, rev_start, rev_edge, n_targets, c, per, w_c, g, w)


def _scatter_csr_lists(kind, rev_start, rev_edge, n_targets, c, per, w_c, g, w):
    """_scatter_csr over reverse lists the caller already holds (ops.group_csr with b = 1)"""
    out = torch.empty(n_targets, c, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device), timing.span("pointops_scatter_csr", g.numel() * 4 + rev_edge.numel() * 8 + out.numel() * 4):
        _lib.check(_lib.load().amc3d_pointops_scatter_csr(kind, n_targets, c, per, w_c, _ptr(g), _ptr(w) if w is not None else None,
                                                          _ptr(rev_start), _ptr(rev_edge), _ptr(out), _o._stream(g)),
                   "pointops_scatter_csr")
    return out


class Grouping(Function):
    @staticmethod
    def forward(ctx, input, idx):
        """input (n,c), idx (m,nsample) -> (m,nsample,c)"""
        assert input.is_contiguous() and idx.is_contiguous()
        _o._need_gpu(input, idx)
        _o._need_dtype(torch.float32, input=input)
        _index(idx, idx.shape[0])
        m, nsample, n, c = idx.shape[0], idx.shape[1], input.shape[0], input.shape[1]
        output = torch.empty(m, nsample, c, dtype=torch.float32, device=input.device)
        with torch.cuda.device(input.device), timing.span("pointops_grouping", output.numel() * 8 + idx.numel() * 4):
            _lib.check(_lib.load().amc3d_pointops_grouping_forward(m, nsample, c, n, _ptr(input), _ptr(idx), _ptr(output),
                                                                   _o._stream(input)), "pointops_grouping_forward")
        ctx.n = n
        ctx.det = _o.deterministic()
        ctx.save_for_backward(idx)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        n = ctx.n
        idx, = ctx.saved_tensors
        m, nsample, c = grad_output.shape
        g = grad_output.detach().contiguous()
        if ctx.det:
            return _scatter_csr(0, idx, n, c, 1, 1, g, None), None
        grad_input = torch.zeros(n, c, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device), timing.span("pointops_grouping_grad", g.numel() * 8 + idx.numel() * 4):
            _lib.check(_lib.load().amc3d_pointops_grouping_backward(m, nsample, c, n, _ptr(g), _ptr(idx), _ptr(grad_input),
                                                                    _o._stream(g)), "pointops_grouping_backward")
        return grad_input, None


grouping = Grouping.apply


class Subtraction(Function):
    @staticmethod
    def forward(ctx, input1, input2, idx):
        """input1 (n,c), input2 (n,c), idx (n,nsample) -> (n,nsample,c) = input1[i] - input2[idx[i,j]]"""
        assert input1.is_contiguous() and input2.is_contiguous()
        _o._need_gpu(input1, input2, idx)
        _o._need_dtype(torch.float32, input1=input1, input2=input2)
        n, c = input1.shape
        _index(idx, n)
        nsample = idx.shape[-1]
        output = torch.empty(n, nsample, c, dtype=torch.float32, device=input1.device)
        with torch.cuda.device(input1.device), timing.span("pointops_subtraction", output.numel() * 8 + idx.numel() * 4):
            _lib.check(_lib.load().amc3d_pointops_subtraction_forward(n, nsample, c, _ptr(input1), _ptr(input2), _ptr(idx),
                                                                      _ptr(output), _o._stream(input1)),
                       "pointops_subtraction_forward")
        ctx.n2 = input2.shape[0]
        ctx.det = _o.deterministic()
        ctx.save_for_backward(idx)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        idx, = ctx.saved_tensors
        n, nsample, c = grad_output.shape
        g = grad_output.detach().contiguous()
        dev = g.device
        grad_input1 = torch.empty(n, c, dtype=torch.float32, device=dev)
        grad_input2 = None if ctx.det else torch.zeros(ctx.n2, c, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), timing.span("pointops_subtraction_grad", g.numel() * 8 + idx.numel() * 4):
            _lib.check(_lib.load().amc3d_pointops_subtraction_backward(n, nsample, c, _ptr(idx), _ptr(g), _ptr(grad_input1),
                                                                       _ptr(grad_input2) if grad_input2 is not None else None,
                                                                       _o._stream(g)), "pointops_subtraction_backward")
        if ctx.det:
            grad_input2 = _scatter_csr(2, idx, ctx.n2, c, 1, 1, g, None)
        return grad_input1, grad_input2, None


subtraction = Subtraction.apply


class Aggregation(Function):
    @staticmethod
    def forward(ctx, input, position, weight, idx):
        """input (n,c), position (n,nsample,c), weight (n,nsample,c'), idx (n,nsample) -> (n,c)"""
        assert input.is_contiguous() and position.is_contiguous() and weight.is_contiguous()
        _o._need_gpu(input, position, weight, idx)
        _o._need_dtype(torch.float32, input=input, position=position, weight=weight)
        n, nsample, c = position.shape
        _index(idx, n)
        w_c = weight.shape[-1]
        output = torch.empty(n, c, dtype=torch.float32, device=input.device)
        with torch.cuda.device(input.device), timing.span("pointops_aggregation", position.numel() * 8 + weight.numel() * 4):
            _lib.check(_lib.load().amc3d_pointops_aggregation_forward(n, nsample, c, w_c, 0, _ptr(input), _ptr(position),
                                                                      _ptr(weight), _ptr(idx), _ptr(output),
                                                                      _o._stream(input)), "pointops_aggregation_forward")
        ctx.det = _o.deterministic()
        ctx.save_for_backward(input, position, weight, idx)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        input, position, weight, idx = ctx.saved_tensors
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        g = grad_output.detach().contiguous()
        dev = g.device
        grad_input = None if ctx.det else torch.zeros(input.shape[0], c, dtype=torch.float32, device=dev)
        grad_position = torch.empty(n, nsample, c, dtype=torch.float32, device=dev)
        grad_weight = torch.empty(n, nsample, w_c, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), timing.span("pointops_aggregation_grad", position.numel() * 12 + weight.numel() * 8):
            _lib.check(_lib.load().amc3d_pointops_aggregation_backward(
                n, nsample, c, w_c, _ptr(input), _ptr(position), _ptr(weight), _ptr(idx), _ptr(g),
                _ptr(grad_input) if grad_input is not None else None, _ptr(grad_position), _ptr(grad_weight), _o._stream(g)),
                "pointops_aggregation_backward")
        if ctx.det:
            grad_input = _scatter_csr(3, idx, input.shape[0], c, nsample, w_c, g, weight)
        return grad_input, grad_position, grad_weight, None


aggregation = Aggregation.apply


class Interpolation(Function):
    @staticmethod
    def forward(ctx, xyz, new_xyz, input, offset, new_offset, k=3):
        """xyz (m,3), new_xyz (n,3), input (m,c), offset / new_offset (b) -> (n,c): inverse-distance weights over the k
        nearest rows of the same segment (the weights are the reference's torch expression, pointops.py:276-280)"""
        assert xyz.is_contiguous() and new_xyz.is_contiguous() and input.is_contiguous()
        _o._need_gpu(xyz, new_xyz, input)
        _o._need_dtype(torch.float32, input=input)
        idx, dist = _o.knnquery(k, xyz, new_xyz, offset, new_offset)  # (n,k), (n,k)
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=1, keepdim=True)
        weight = (dist_recip / norm).contiguous()
        n, c, m = new_xyz.shape[0], input.shape[1], input.shape[0]
        output = torch.empty(n, c, dtype=torch.float32, device=input.device)
        with torch.cuda.device(input.device), timing.span("pointops_interpolation", output.numel() * 4 * (k + 1) + idx.numel() * 8):
            _lib.check(_lib.load().amc3d_pointops_interpolation_forward(n, c, k, m, 0, _ptr(input), _ptr(idx), _ptr(weight),
                                                                        _ptr(output), _o._stream(input)),
                       "pointops_interpolation_forward")
        ctx.m, ctx.k = m, k
        ctx.det = _o.deterministic()
        ctx.save_for_backward(idx, weight)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        m, k = ctx.m, ctx.k
        idx, weight = ctx.saved_tensors
        n, c = grad_output.shape
        g = grad_output.detach().contiguous()
        if ctx.det:
            return None, None, _scatter_csr(1, idx, m, c, k, 1, g, weight), None, None, None
        grad_input = torch.zeros(m, c, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device), timing.span("pointops_interpolation_grad", g.numel() * 4 * (k + 1) + idx.numel() * 8):
            _lib.check(_lib.load().amc3d_pointops_interpolation_backward(n, c, k, m, _ptr(g), _ptr(idx), _ptr(weight),
                                                                         _ptr(grad_input), _o._stream(g)),
                       "pointops_interpolation_backward")
        return None, None, grad_input, None, None, None


interpolation2 = Interpolation.apply
