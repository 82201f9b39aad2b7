"""NumPy restatements of the offset-layout pointops kernels (csrc/pointops.hip; the reference's
cpp/pointops/src/{ballquery,sampling,grouping,interpolation,subtraction,aggregation}), thread for thread where the order
matters: the furthest-sampling tie rule, the ball query's index order and padding, the sequential fp32 sums.  Every fp32
operation is one NumPy ufunc call on float32 arrays, so each is rounded once and nothing is contracted.

Layouts: xyz (n,3), new_xyz (m,3), features channel-last (rows,c), idx (rows,nsample) int32 global row ids, offset /
new_offset cumulative segment ends.  The scatters are summed per target in ascending position order from +0.0f -- the
order of deterministic mode; the default mode's atomics are held against the fp64 forms (`*_exact`), which return
(exact sum, sum of |terms|, in-degree) per output element for the any-order bound.

`as_pointops_cuda()` wraps the restatements as the in-place entry points of the reference's extension module, for
tools/record_pointops_fixtures.py and for tests that drive a Python layer on the CPU.
"""
import types

import numpy as np

F = np.float32


def segment_of(q, ends):
    """first s with q < ends[s], clamped to the last segment"""
    return min(int(np.searchsorted(np.asarray(ends), q, side="right")), len(ends) - 1)


def segments(ends):
    ends = [int(e) for e in ends]
    return list(zip([0] + ends[:-1], ends))


def dist2(a, b):
    """((dx*dx + dy*dy) + dz*dz) with dx = a - b, fp32, left to right"""
    d = (a.astype(F) - b.astype(F)).astype(F)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ------------------------------------------------------------------------------------------------ searches
def ballquery(radius, nsample, xyz, new_xyz, offset, new_offset):
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    m = new_xyz.shape[0]
    r2 = F(radius) * F(radius)
    seg = segments(offset)
    idx = np.zeros((m, nsample), np.int32)
    for q in range(m):
        start, end = seg[segment_of(q, new_offset)]
        if end <= start:
            continue
        hits = np.nonzero(dist2(new_xyz[q][None], xyz[start:end]) < r2)[0][:nsample] + start
        if hits.size:
            idx[q, :] = hits[0]
            idx[q, :hits.size] = hits
    return idx


def _brev10(t):
    t = np.asarray(t, np.int64)
    r = np.zeros_like(t)
    for b in range(10):
        r |= ((t >> b) & 1) << (9 - b)
    return r


def furthestsampling(xyz, offset, new_offset, tmp=None):
    """-> (idx (m,), tmp (n,)): tmp starts at 1e10 unless given and comes back as the final running minima.  Among equal
    running minima the pick has the smallest bit-reversed (k - start) mod 1024, then the lowest k."""
    xyz = np.asarray(xyz, F)
    n = xyz.shape[0]
    tmp = np.full(n, 1e10, F) if tmp is None else np.array(tmp, F)
    new_seg = segments(new_offset)
    idx = np.zeros(int(new_offset[-1]), np.int32)
    for (start, end), (ms, me) in zip(segments(offset), new_seg):
        if end <= start or me <= ms:
            continue
        idx[ms] = old = start
        k = np.arange(start, end)
        key = _brev10((k - start) & 1023) * (1 << 31) + k
        for j in range(ms + 1, me):
            d2 = np.minimum(dist2(xyz[start:end], xyz[old][None]), tmp[start:end])
            tmp[start:end] = d2
            tied = np.nonzero(d2 == d2.max())[0]
            old = int(k[tied[np.argmin(key[tied])]])
            idx[j] = old
    return idx, tmp


# ------------------------------------------------------------------------------------- sequential scatter
def _scatter_seq(n_targets, c, targets, terms):
    """out[targets[p], :] += terms[p, :] for p ascending, fp32, from +0.0f (np.add.at is unbuffered and in order)"""
    out = np.zeros((n_targets, c), F)
    np.add.at(out, np.asarray(targets).reshape(-1).astype(np.int64), np.asarray(terms, F).reshape(-1, c))
    return out


def _scatter_exact(n_targets, c, targets, terms):
    t = np.asarray(targets).reshape(-1).astype(np.int64)
    terms = np.asarray(terms, np.float64).reshape(-1, c)
    exact, mag = np.zeros((n_targets, c)), np.zeros((n_targets, c))
    np.add.at(exact, t, terms)
    np.add.at(mag, t, np.abs(terms))
    deg = np.bincount(t, minlength=n_targets)[:, None] * np.ones((1, c), np.int64)
    return exact, mag, deg


# ------------------------------------------------------------------------------------------------ grouping
def grouping_forward(inp, idx):
    return np.asarray(inp, F)[np.asarray(idx).astype(np.int64)]


def grouping_backward(grad_output, idx, n):
    g = np.asarray(grad_output, F)
    return _scatter_seq(n, g.shape[-1], idx, g)


def grouping_backward_exact(grad_output, idx, n):
    g = np.asarray(grad_output, F)
    return _scatter_exact(n, g.shape[-1], idx, g)


# ------------------------------------------------------------------------------------------- interpolation
def interpolation_forward(inp, idx, weight, out=None):
    """out (n,c) starts from +0.0f, or from `out` (the accumulate form)"""
    inp, weight, idx = np.asarray(inp, F), np.asarray(weight, F), np.asarray(idx).astype(np.int64)
    acc = np.zeros((idx.shape[0], inp.shape[1]), F) if out is None else np.array(out, F)
    for t in range(idx.shape[1]):
        acc = acc + inp[idx[:, t]] * weight[:, t:t + 1]
    return acc


def _interp_terms(grad_output, weight, dtype):
    g, w = np.asarray(grad_output, F), np.asarray(weight, F)
    if dtype is F:
        return g[:, None, :] * w[:, :, None]  # (n,k,c), each product rounded once
    return g.astype(np.float64)[:, None, :] * w.astype(np.float64)[:, :, None]


def interpolation_backward(grad_output, idx, weight, m):
    return _scatter_seq(m, np.asarray(grad_output).shape[1], idx, _interp_terms(grad_output, weight, F))


def interpolation_backward_exact(grad_output, idx, weight, m):
    return _scatter_exact(m, np.asarray(grad_output).shape[1], idx, _interp_terms(grad_output, weight, np.float64))


# --------------------------------------------------------------------------------------------- subtraction
def subtraction_forward(input1, input2, idx):
    a, b = np.asarray(input1, F), np.asarray(input2, F)
    return a[:, None, :] - b[np.asarray(idx).astype(np.int64)]


def subtraction_backward(grad_output, idx, n=None):
    """-> grad_input1 (sequential over j from +0.0f), grad_input2 (sequential scatter of -grad_output)"""
    g = np.asarray(grad_output, F)
    n = g.shape[0] if n is None else n
    g1 = np.zeros((g.shape[0], g.shape[2]), F)
    for j in range(g.shape[1]):
        g1 = g1 + g[:, j]
    return g1, _scatter_seq(n, g.shape[2], idx, -g)


def subtraction_backward_exact(grad_output, idx, n=None):
    g = np.asarray(grad_output, F)
    return _scatter_exact(g.shape[0] if n is None else n, g.shape[2], idx, -g)


# --------------------------------------------------------------------------------------------- aggregation
def _wexp(weight, c):
    """weight (n,ns,w_c) -> (n,ns,c) with channel ch reading ch % w_c"""
    weight = np.asarray(weight, F)
    return weight[:, :, np.arange(c) % weight.shape[2]]


def aggregation_forward(inp, position, weight, idx, out=None):
    inp, position, idx = np.asarray(inp, F), np.asarray(position, F), np.asarray(idx).astype(np.int64)
    n, ns, c = position.shape
    w = _wexp(weight, c)
    acc = np.zeros((n, c), F) if out is None else np.array(out, F)
    for j in range(ns):
        acc = acc + (inp[idx[:, j]] + position[:, j]) * w[:, j]
    return acc


def aggregation_backward(inp, position, weight, idx, grad_output):
    """-> grad_input (sequential scatter), grad_position, grad_weight (sequential over ch = wc, wc + w_c, ...)"""
    inp, position, g = np.asarray(inp, F), np.asarray(position, F), np.asarray(grad_output, F)
    idx = np.asarray(idx).astype(np.int64)
    n, ns, c = position.shape
    w_c = np.asarray(weight).shape[2]
    grad_position = g[:, None, :] * _wexp(weight, c)
    prod = g[:, None, :] * (inp[idx] + position)  # (n,ns,c)
    grad_weight = np.zeros((n, ns, w_c), F)
    for ch in range(c):
        grad_weight[:, :, ch % w_c] = grad_weight[:, :, ch % w_c] + prod[:, :, ch]
    return _scatter_seq(inp.shape[0], c, idx, grad_position), grad_position, grad_weight


def aggregation_backward_exact(inp, weight, idx, grad_output):
    g = np.asarray(grad_output, F).astype(np.float64)
    c = g.shape[1]
    terms = g[:, None, :] * _wexp(weight, c).astype(np.float64)
    return _scatter_exact(np.asarray(inp).shape[0], c, idx, terms)


# ------------------------------------------------------------- the extension module's in-place entry points
def _np(t):
    return t.detach().cpu().numpy()


def as_pointops_cuda(knnquery_cuda=None):
    """A stand-in `pointops_cuda` over the restatements: torch CPU tensors in, outputs written in place, the reference's
    positional order (pointops_api.cpp:14-24).  `+=` outputs are added into, as the reference's kernels do."""
    import torch

    def put(dst, arr):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(dst.shape))

    def furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx):
        i, t = furthestsampling(_np(xyz), _np(offset), _np(new_offset), _np(tmp))
        put(idx, i), put(tmp, t)

    def ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx):
        put(idx, ballquery(radius, nsample, _np(xyz), _np(new_xyz), _np(offset), _np(new_offset)))

    def grouping_forward_cuda(m, nsample, c, inp, idx, output):
        put(output, grouping_forward(_np(inp), _np(idx)))

    def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input):
        put(grad_input, _np(grad_input) + grouping_backward(_np(grad_output), _np(idx), grad_input.shape[0]))

    def interpolation_forward_cuda(n, c, k, inp, idx, weight, output):
        put(output, interpolation_forward(_np(inp), _np(idx), _np(weight), out=_np(output)))

    def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input):
        put(grad_input, _np(grad_input) + interpolation_backward(_np(grad_output), _np(idx), _np(weight), grad_input.shape[0]))

    def subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output):
        put(output, subtraction_forward(_np(input1), _np(input2), _np(idx)))

    def subtraction_backward_cuda(n, nsample, c, idx, grad_output, grad_input1, grad_input2):
        g1, g2 = subtraction_backward(_np(grad_output), _np(idx), grad_input2.shape[0])
        put(grad_input1, g1), put(grad_input2, _np(grad_input2) + g2)

    def aggregation_forward_cuda(n, nsample, c, w_c, inp, position, weight, idx, output):
        put(output, aggregation_forward(_np(inp), _np(position), _np(weight), _np(idx), out=_np(output)))

    def aggregation_backward_cuda(n, nsample, c, w_c, inp, position, weight, idx, grad_output, grad_input, grad_position,
                                  grad_weight):
        gi, gp, gw = aggregation_backward(_np(inp), _np(position), _np(weight), _np(idx), _np(grad_output))
        put(grad_input, _np(grad_input) + gi), put(grad_position, gp), put(grad_weight, gw)

    mod = types.ModuleType("pointops_cuda")
    fns = [furthestsampling_cuda, ballquery_cuda, grouping_forward_cuda, grouping_backward_cuda, interpolation_forward_cuda,
           interpolation_backward_cuda, subtraction_forward_cuda, subtraction_backward_cuda, aggregation_forward_cuda,
           aggregation_backward_cuda]
    for f in fns:
        setattr(mod, f.__name__, f)
    if knnquery_cuda is not None:
        mod.knnquery_cuda = knnquery_cuda
    return mod


ENTRY_POINTS = ("furthestsampling_cuda", "knnquery_cuda", "ballquery_cuda", "grouping_forward_cuda", "grouping_backward_cuda",
                "interpolation_forward_cuda", "interpolation_backward_cuda", "subtraction_forward_cuda",
                "subtraction_backward_cuda", "aggregation_forward_cuda", "aggregation_backward_cuda")  # pointops_api.cpp:14-24


# ------------------------------------------------------------------------------------------- test clouds
def cloud(seed, n, kind):
    """(n,3) fp32: `uniform` in [0,2)^3, `lattice` on a 0.25 grid of 6^3 nodes (exact distance ties everywhere), `dup`
    every point drawn from n//3 distinct ones, `room` a synthetic scene"""
    rng = np.random.default_rng(seed)
    if kind == "room":
        from amcontrast3d_amd import synthetic
        return np.ascontiguousarray(synthetic.make_batch(1, n, first_id=seed)["pos"][0], F)
    if kind == "uniform":
        return rng.uniform(0, 2, size=(n, 3)).astype(F)
    if kind == "lattice":
        return (rng.integers(0, 6, size=(n, 3)) * 0.25).astype(F)
    if kind == "dup":
        base = rng.uniform(0, 1, size=(max(n // 3, 1), 3)).astype(F)
        return np.ascontiguousarray(base[rng.integers(0, base.shape[0], size=n)])
    raise ValueError(kind)


def ends(counts):
    return np.cumsum(np.asarray(counts, np.int64)).astype(np.int32)
