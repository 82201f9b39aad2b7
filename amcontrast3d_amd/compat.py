"""Module-shaped views of the C-ABI with the reference's pybind11 entry points.

``pointnet2_batch_cuda`` and ``pointops_cuda`` below expose exactly the names and
positional arguments of the reference's two extension modules
(cpp/pointnet2_batch/src/pointnet2_api.cpp:10-24, cpp/pointops/src/pointops_api.cpp:14-24):
torch tensors in, outputs written in place.  Registering them in ``sys.modules``
under those names lets the reference's own, unmodified Python wrappers
(models/layers/group.py, subsample.py, upsampling.py, cpp/pointops/functions/pointops.py)
run on the MI355X kernels -- see INTEGRATION.md.
"""
import ctypes
import sys
import types

import torch

from . import _lib


def _p(t, dtype=None):
    if not t.is_cuda:
        raise RuntimeError("expected a GPU tensor (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")  # reference: CHECK_CONTIGUOUS -> exit(-1)
    if dtype is not None and t.dtype != dtype:  # reference: data_ptr<float>() / data_ptr<int>() throw on another dtype
        raise RuntimeError(f"expected scalar type {dtype} but found {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


def _f(t):
    return _p(t, torch.float32)


def _i(t):
    return _p(t, torch.int32)


def _s(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _call(name, dev_tensor, *args):
    with torch.cuda.device(dev_tensor.device):
        _lib.check(getattr(_lib.load(), name)(*args, _s(dev_tensor)), name)


def _grid_ws(b, n_support, m_queries, device):
    wb = int(_lib.load().amc3d_grid_search_workspace_bytes(b, n_support, m_queries))
    return torch.empty(max(wb, 4), dtype=torch.uint8, device=device), wb


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx):
    work, wb = _grid_ws(b, n, m, xyz.device)
    _call("amc3d_ball_query", xyz, b, n, m, float(radius), nsample, _f(new_xyz), _f(xyz), _i(idx), _p(work), wb)
    return 1


def group_points_wrapper(b, c, n, npoints, nsample, points, idx, out):
    _call("amc3d_group_points", points, b, c, n, npoints, nsample, _f(points), _i(idx), _f(out))
    return 1


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points):
    _call("amc3d_group_points_grad", grad_out, b, c, n, npoints, nsample, _f(grad_out), _i(idx), _f(grad_points),
          None, 0)
    return 1


def gather_points_wrapper(b, c, n, npoints, points, idx, out):
    _call("amc3d_gather_points", points, b, c, n, npoints, _f(points), _i(idx), _f(out))
    return 1


def gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points):
    _call("amc3d_gather_points_grad", grad_out, b, c, n, npoints, _f(grad_out), _i(idx), _f(grad_points))
    return 1


def furthest_point_sampling_wrapper(b, n, m, points, temp, idx):
    wb = int(_lib.load().amc3d_fps_workspace_bytes(b, n))
    work = torch.empty(max(wb, 4), dtype=torch.uint8, device=points.device)
    _call("amc3d_furthest_point_sampling", points, b, n, m, _f(points), _f(temp) if temp is not None else None, _i(idx),
          _p(work), wb)
    return 1


def three_nn_wrapper(b, n, m, unknown, known, dist2, idx):
    work, wb = _grid_ws(b, m, n, unknown.device)
    _call("amc3d_three_nn", unknown, b, n, m, _f(unknown), _f(known), _f(dist2), _i(idx), _p(work), wb)


def three_interpolate_wrapper(b, c, m, n, points, idx, weight, out):
    _call("amc3d_three_interpolate", points, b, c, m, n, _f(points), _i(idx), _f(weight), _f(out))


def three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, grad_points):
    _call("amc3d_three_interpolate_grad", grad_out, b, c, n, m, _f(grad_out), _i(idx), _f(weight), _f(grad_points),
          None, 0)


def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
    n, nb = xyz.shape[0], offset.shape[0]
    lib = _lib.load()
    wbytes = int(lib.amc3d_knnquery_workspace_bytes(n, m, nsample, nb))
    work = torch.empty(wbytes, dtype=torch.uint8, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.check(lib.amc3d_knnquery(m, nsample, n, nb, _f(xyz), _f(new_xyz), _i(offset), _i(new_offset), _i(idx),
                                      _f(dist2), _p(work), wbytes, 0, _s(xyz)), "amc3d_knnquery")


# The other ten entry points of pointops_api.cpp:14-24, in the positional order of the .cpp wrapper beside each kernel.
# Sizes the reference does not pass (rows of the gathered array, the segment count) are read from the tensors; outputs the
# reference adds into are added into (accumulate = 1), so a caller's non-zero buffer behaves as it does there.
def furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx):
    _call("amc3d_pointops_furthestsampling", xyz, int(b), int(n_max), xyz.shape[0], _f(xyz), _i(offset), _i(new_offset),
          _f(tmp), _i(idx))


def ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx):
    _call("amc3d_pointops_ballquery", xyz, m, float(radius), nsample, xyz.shape[0], offset.shape[0], _f(xyz), _f(new_xyz),
          _i(offset), _i(new_offset), _i(idx))


def grouping_forward_cuda(m, nsample, c, input, idx, output):
    _call("amc3d_pointops_grouping_forward", input, m, nsample, c, input.shape[0], _f(input), _i(idx), _f(output))


def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input):
    _call("amc3d_pointops_grouping_backward", grad_output, m, nsample, c, grad_input.shape[0], _f(grad_output), _i(idx),
          _f(grad_input))


def interpolation_forward_cuda(n, c, k, input, idx, weight, output):
    _call("amc3d_pointops_interpolation_forward", input, n, c, k, input.shape[0], 1, _f(input), _i(idx), _f(weight),
          _f(output))


def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input):
    _call("amc3d_pointops_interpolation_backward", grad_output, n, c, k, grad_input.shape[0], _f(grad_output), _i(idx),
          _f(weight), _f(grad_input))


def subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output):
    _call("amc3d_pointops_subtraction_forward", input1, n, nsample, c, _f(input1), _f(input2), _i(idx), _f(output))


def subtraction_backward_cuda(n, nsample, c, idx, grad_output, grad_input1, grad_input2):
    _call("amc3d_pointops_subtraction_backward", grad_output, n, nsample, c, _i(idx), _f(grad_output), _f(grad_input1),
          _f(grad_input2))


def aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output):
    _call("amc3d_pointops_aggregation_forward", input, n, nsample, c, w_c, 1, _f(input), _f(position), _f(weight), _i(idx),
          _f(output))


def aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output, grad_input, grad_position,
                              grad_weight):
    _call("amc3d_pointops_aggregation_backward", input, n, nsample, c, w_c, _f(input), _f(position), _f(weight), _i(idx),
          _f(grad_output), _f(grad_input), _f(grad_position), _f(grad_weight))


def _module(name, fns):
    mod = types.ModuleType(name)
    mod.__doc__ = "MI355X implementation of the reference's %s extension (amcontrast3d_amd.compat)" % name
    for f in fns:
        setattr(mod, f.__name__, f)
    return mod


pointnet2_batch_cuda = _module("pointnet2_batch_cuda", [
    ball_query_wrapper, group_points_wrapper, group_points_grad_wrapper, gather_points_wrapper,
    gather_points_grad_wrapper, furthest_point_sampling_wrapper, three_nn_wrapper, three_interpolate_wrapper,
    three_interpolate_grad_wrapper])
pointops_cuda = _module("pointops_cuda", [
    furthestsampling_cuda, knnquery_cuda, ballquery_cuda, grouping_forward_cuda, grouping_backward_cuda,
    interpolation_forward_cuda, interpolation_backward_cuda, subtraction_forward_cuda, subtraction_backward_cuda,
    aggregation_forward_cuda, aggregation_backward_cuda])


def register_native_modules():
    """Make ``import pointnet2_batch_cuda`` / ``import pointops_cuda`` resolve to this library."""
    sys.modules["pointnet2_batch_cuda"] = pointnet2_batch_cuda
    sys.modules["pointops_cuda"] = pointops_cuda
