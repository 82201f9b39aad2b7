"""1x1-conv / norm / activation block factories.

Same call signatures and module nesting as the reference
(models/layers/conv.py:8-102, norm.py:57-97, activation.py:5-51) so that
state-dict keys are identical: a block is ``nn.Sequential(conv[, norm][, act])``
-> ``<block>.0.weight`` (conv), ``<block>.1.{weight,bias,running_mean,...}`` (norm);
the conv has no bias when a norm follows it.
"""
import copy
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from amcontrast3d_amd import ops


class Conv2d(nn.Conv2d):
    """nn.Conv2d that defaults to a 1x1 kernel when only (cin, cout) are given."""

    def __init__(self, *args, **kwargs):
        if len(args) == 2 and 'kernel_size' not in kwargs:
            args = (*args, (1, 1))
        super().__init__(*args, **kwargs)


class Conv1d(nn.Conv1d):
    """nn.Conv1d that defaults to kernel size 1 when only (cin, cout) are given."""

    def __init__(self, *args, **kwargs):
        if len(args) == 2 and 'kernel_size' not in kwargs:
            args = (*args, 1)
        super().__init__(*args, **kwargs)


_NORMS = {
    'bn1d': nn.BatchNorm1d, 'bn2d': nn.BatchNorm2d, 'bn': nn.BatchNorm2d,
    'in1d': nn.InstanceNorm1d, 'in2d': nn.InstanceNorm2d,
    'gn': nn.GroupNorm, 'syncbn': nn.SyncBatchNorm, 'ln': nn.LayerNorm,
}

_ACTS = {
    'silu': nn.SiLU, 'swish': nn.SiLU, 'mish': nn.Mish, 'relu': nn.ReLU, 'relu6': nn.ReLU6,
    'leaky_relu': nn.LeakyReLU, 'leakyrelu': nn.LeakyReLU, 'elu': nn.ELU, 'prelu': nn.PReLU,
    'celu': nn.CELU, 'selu': nn.SELU, 'gelu': nn.GELU, 'sigmoid': nn.Sigmoid, 'tanh': nn.Tanh,
    'hard_sigmoid': nn.Hardsigmoid, 'hard_swish': nn.Hardswish,
}


def create_norm(norm_args, channels, dimension=None):
    """norm.py:74-97: 'bn' + dimension '1d'/'2d' -> BatchNorm1d/2d; extra keys are ctor kwargs."""
    if norm_args is None:
        return None
    if isinstance(norm_args, dict):
        kwargs = copy.deepcopy(dict(norm_args))
        norm = kwargs.pop('norm', None)
    else:
        norm, kwargs = norm_args, {}
    if norm is None:
        return None
    if isinstance(norm, str):
        norm = norm.lower()
        if dimension is not None:
            dimension = str(dimension).lower()
            if dimension not in norm:
                norm += dimension
        assert norm in _NORMS, f"input {norm} is not supported"
        norm = _NORMS[norm]
    return norm(channels, **kwargs)


def create_act(act_args):
    """activation.py:25-51: in-place by default (except gelu/sigmoid)."""
    if act_args is None:
        return None
    act_args = {'act': act_args} if isinstance(act_args, str) else copy.deepcopy(dict(act_args))
    act = act_args.pop('act', None)
    if act is None:
        return None
    if isinstance(act, str):
        act = act.lower()
        assert act in _ACTS, f"input {act} is not supported"
        layer = _ACTS[act]
    inplace = act_args.pop('inplace', True)
    if act in ('gelu', 'sigmoid'):
        return layer(**act_args)
    return layer(inplace=inplace, **act_args)


def _convblock(conv_cls, dim, args, norm_args, act_args, order, kwargs):
    cin, cout = args[0], args[1]
    bias = kwargs.pop('bias', True)
    if order not in ('conv-norm-act', 'norm-act-conv', 'conv-act-norm'):
        raise NotImplementedError(f"{order} is not supported")
    norm = create_norm(norm_args, cin if order == 'norm-act-conv' else cout, dimension=dim)
    if norm is not None:
        bias = False
    conv = conv_cls(*args, bias=bias, **kwargs)
    act = create_act(act_args)
    parts = {'conv': conv, 'norm': norm, 'act': act if act_args is not None else None}
    return nn.Sequential(*[parts[k] for k in order.split('-') if parts[k] is not None])


def create_convblock2d(*args, norm_args=None, act_args=None, order='conv-norm-act', **kwargs):
    return _convblock(Conv2d, '2d', args, norm_args, act_args, order, kwargs)


def create_convblock1d(*args, norm_args=None, act_args=None, order='conv-norm-act', **kwargs):
    return _convblock(Conv1d, '1d', args, norm_args, act_args, order, kwargs)


def conv_bn_block(blk):
    """(conv, bn, relu) when `blk` is nn.Sequential(conv, norm[, act]) with a 1x1 convolution of stride 1, no padding and one
    group, one of the BatchNorm classes and, optionally, an nn.ReLU (relu: that module or None) -- the form every fused route
    below starts from; None for anything else.  Pure module inspection: bias, widths, mode and tensors are the caller's."""
    if not isinstance(blk, nn.Sequential) or len(blk) not in (2, 3):
        return None
    conv, bn, relu = blk[0], blk[1], blk[2] if len(blk) == 3 else None
    if (not isinstance(conv, (nn.Conv1d, nn.Conv2d)) or not isinstance(bn, nn.modules.batchnorm._BatchNorm)
            or (relu is not None and type(relu) is not nn.ReLU) or isinstance(conv.padding, str)
            or any(v != 1 for v in conv.kernel_size) or any(v != 1 for v in conv.stride) or any(v != 0 for v in conv.padding)
            or conv.groups != 1):
        return None
    return conv, bn, relu


def _bn_grid_fits(x):
    """the BatchNorm kernels put batch * channels on the grid's y axis (csrc/bn.hip refuses more than 65535)"""
    return x.dim() >= 2 and x.shape[0] * x.shape[1] <= 65535


def _fusable_bn(bn, x):
    """plain training-mode BatchNorm1d/2d on a contiguous fp32 GPU tensor (SyncBatchNorm, eval mode, other norms
    and a batch * channels beyond the kernels' grid take the ordinary torch modules)"""
    return (type(bn) in (nn.BatchNorm1d, nn.BatchNorm2d) and bn.training and bn.affine and bn.track_running_stats
            and x.is_cuda and x.dtype == torch.float32 and _bn_grid_fits(x))


def _eval_bn(bn, x):
    """inference-mode BatchNorm (any of the BatchNorm classes) on a contiguous fp32 GPU tensor outside autograd:
    the fused kernels with the running statistics (ops.bn_eval)"""
    return (isinstance(bn, nn.modules.batchnorm._BatchNorm) and not bn.training and bn.affine
            and bn.track_running_stats and bn.running_mean is not None and x.is_cuda and x.dtype == torch.float32
            and not torch.is_grad_enabled() and _bn_grid_fits(x))


def _synced_bn_group(bn, x):
    """process group of a training-mode nn.SyncBatchNorm whose statistics really span several ranks (then the fused
    kernels exchange their per-channel sums: ops.SyncBatchNormFused), else None"""
    if not (type(bn) is nn.SyncBatchNorm and bn.training and bn.affine and bn.track_running_stats and x.is_cuda
            and x.dtype == torch.float32 and _bn_grid_fits(x) and dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 or _FORCE_SYNCED_BN else None


_FORCE_SYNCED_BN = False  # tests: take the cross-rank path in a one-rank group too


def batchnorm_act(bn, y, relu, pool=False, residual=None):
    """relu(bn(y)) (relu: the block's nn.ReLU or None), then the max over the last (neighbour) dimension if `pool`, then
    relu(. + residual) if a residual is given -- an InvResMLP block's `f += identity; act(f)`.  Inference mode outside
    autograd: ops.bn_eval; nn.SyncBatchNorm over several ranks: ops.SyncBatchNormFused; plain training-mode BatchNorm on a
    fp32 GPU tensor: ops.BatchNormMax / BatchNormResidualAct / BatchNormAct (statistics, normalisation, ReLU, pool or
    residual and nn.BatchNorm's running-stat bookkeeping in the same launches, csrc/bn.hip); anything else: the stored torch
    modules.  What the chosen kernels do not cover of pool and residual follows in torch."""
    act = relu is not None
    fused_pool = pool and y.dim() == 4 and y.shape[-1] <= 255
    group = _synced_bn_group(bn, y)
    pooled = added = False
    if _eval_bn(bn, y):
        x, pooled = ops.bn_eval(y, bn, act, fused_pool), fused_pool
    elif group is not None:
        x, pooled = ops.SyncBatchNormFused.apply(y, bn.weight, bn.bias, bn.eps, act, fused_pool, bn, group)[0], fused_pool
    elif _fusable_bn(bn, y):
        if fused_pool:
            x, pooled = ops.BatchNormMax.apply(y, bn.weight, bn.bias, bn.eps, act, bn)[0], True
        elif (residual is not None and not act and not pool and residual.shape == y.shape and residual.is_cuda
              and residual.dtype == torch.float32 and not os.environ.get("AMC3D_NO_BN_RESIDUAL")):
            x, added = ops.BatchNormResidualAct.apply(y, residual, bn.weight, bn.bias, bn.eps, bn)[0], True
        else:
            x = ops.BatchNormAct.apply(y, bn.weight, bn.bias, bn.eps, act, bn)[0]
    else:
        x = bn(y)
        if act:
            x = relu(x)
    if pool and not pooled:
        x = torch.max(x, dim=-1, keepdim=False)[0]
    if residual is not None and not added:
        x = torch.relu(x + residual)
    return x


def conv1x1(conv, x, rows_grad=False, library=True):
    """conv(x); a plain 1x1 convolution on a contiguous fp32 GPU tensor runs on the MFMA kernels of
    csrc/pwconv.hip (same parameters, same autograd contract), anything else on the stored torch module.
    `rows_grad`: the only consumer of x's gradient reads position-major rows (wants_rows_grad): the backward-data product
    then stores (B,*spatial,Cin) and hands over the permuted view, where the route has that form.
    `library=False`: never the BLAS / convolution library -- this library's own kernel also where the library measured
    faster, so that the result does not depend on which kernel that library picks in a session (ConvPool: a max over the
    neighbours follows, and an arg-max that flips on the last bit moves the gradients by their own size)."""
    if (type(conv) in (nn.Conv1d, nn.Conv2d, Conv1d, Conv2d) and x.is_cuda and x.dtype == torch.float32
            and conv.groups == 1 and conv.padding_mode == 'zeros'
            and all(k == 1 for k in conv.kernel_size) and all(v == 1 for v in conv.stride)
            and all(v == 0 for v in conv.padding) and x.dim() == conv.weight.dim()):
        if ops.mixed_precision() and _bf16_pays(conv, x):
            # use_amp (main_AA.py:389-394): bf16 operands, fp32 accumulation on the bf16 MFMA; activations, BatchNorm,
            # searches and the loss stay fp32 (tensors are never stored in bf16)
            return ops.pointwise_conv(x, conv.weight, conv.bias, True)
        if _pw_pays(conv, x) or not library:
            return ops.pointwise_conv(x, conv.weight, conv.bias, False, rows_grad)
        if (conv.bias is None and min(conv.in_channels, conv.out_channels) >= 64 and conv.in_channels % 4 == 0
                and torch.is_grad_enabled()):
            # deep and short (SA4, coarse FP stages): three plain library GEMMs instead of the convolution library,
            # whose weight gradient is wrapped in layout transposes (scratch/pw_bench3.py: 30-50 us per layer)
            return ops.library_gemm_conv(x, conv.weight, rows_grad)
        # what is left (small layers with a bias: the skip convs of SA2-4): the convolution library -- this library's own
        # kernel measured 0.35 ms/step slower on these three layers (deterministic mode takes it: its sums have a fixed order,
        # the convolution library's are not this library's to fix)
        if ops.deterministic():
            return ops.pointwise_conv(x, conv.weight, conv.bias, False, rows_grad)
        with torch.autocast("cuda", enabled=False):
            return conv(x)
    return conv(x)


def conv1x1_weight(x, w):
    """1x1 convolution of x (B,Cin,P) with an explicit bias-free weight w (Cout,Cin): the routing of conv1x1 for a slice
    of a module's weight (the two halves of a FeaturePropogation conv)"""
    cin, cout = w.shape[1], w.shape[0]
    positions = x.numel() // x.shape[1]
    w3 = w.reshape(cout, cin, 1)
    if ops.mixed_precision() and min(cin, cout) >= 64 and positions >= _BF16_MIN_POSITIONS:
        return ops.pointwise_conv(x, w3, None, True)
    if min(cin, cout) >= 64 and positions < 65536 and cin % 4 == 0 and torch.is_grad_enabled():
        return ops.library_gemm_conv(x, w3)
    return ops.pointwise_conv(x, w3, None)


def cloud_term_form(blk, f1, f2, e):
    """True when the first FeaturePropagation block `blk` CAN take its class-conditioned input channels e (B,E) -- constant
    along the points of a cloud -- as a per-cloud additive term: Conv1d -> BatchNorm1d -> ReLU without bias over
    [e ; f1 ; up(f2)], fp32 tensors on the GPU.  Pure inspection of the module and of shapes / dtypes / devices: launches
    nothing and moves no statistics."""
    m = conv_bn_block(blk)
    return not (m is None or m[2] is None or type(m[0]) not in (nn.Conv1d, Conv1d) or m[0].bias is not None or f1 is None
                or f1.dim() != 3 or e.dim() != 2 or not (f1.is_cuda and f2.is_cuda and e.is_cuda)
                or any(t.dtype != torch.float32 for t in (f1, f2, e, m[0].weight))
                or m[0].in_channels != e.shape[1] + f1.shape[1] + f2.shape[1])


def cloud_term_route(blk, f1, f2, e):
    """'cloud_term' when the block has the form for the per-cloud term (cloud_term_form) AND the term pays at its shape;
    'composition' for anything else: the caller then expands e along the points and concatenates, as the reference does.
    Like cloud_term_form it launches nothing.

    Shape dispatch (tools/cloud_term_bench.py): the term saves E channels of concatenation forward and of dx
    backward, and costs one more pass over dy (Cout channels) for its gradient plus a handful of small launches.  The rule
    is E >= 32 or 2 E >= Cout: of the 30 measured shapes the term is behind forward + backward exactly where E = 16 stands
    in front of 64 or 128 output channels (by 0.3-12 %), and one more time by 1.1 % (E = 32, Cout = 64 at 32 x 2048).  The
    boundary lies between the measured E = 16 and E = 32 for those widths and between Cout = 32 and 64 for E = 16; nothing
    was measured in between, nor at other E below 32."""
    if not cloud_term_form(blk, f1, f2, e):
        return 'composition'
    E, cout = e.shape[1], conv_bn_block(blk)[0].out_channels
    return 'cloud_term' if (E >= 32 or 2 * E >= cout) else 'composition'


def cloud_term(e, w_cls):
    """c (B,Cout) = e (B,E) @ w_cls (Cout,E)^T, in fp32 also under autocast.  Deterministic mode: products and a row sum instead
    of the BLAS library's matmul (whose kernels are not this library's to fix), forward and backward"""
    with torch.autocast("cuda", enabled=False):
        if ops.deterministic():
            return (e.unsqueeze(1) * w_cls.unsqueeze(0)).sum(-1)
        return e @ w_cls.t()


def feature_propagation_first_block(blk, f1, f2, geom, cloud=None, force_cloud_term=False):
    """First block of FeaturePropogation (pointnext_AA.py:210-226: interpolate f2 onto the fine cloud, concatenate with the
    skip features f1, Conv1d -> BatchNorm1d -> ReLU) with the conv applied BEFORE the interpolation:
        W . [f1 ; up(f2)] = W1 . f1 + up(W2 . f2)
    (the 3-NN interpolation is linear and mixes points, the 1x1 conv mixes channels: they commute).  The interpolated
    tensor has Cout instead of C2 channels (half at every level), its conv runs on the coarse cloud (4x fewer points), and
    no concatenated (B, C1+C2, n) tensor exists.  -> the block's output, or None when it is not of that form.

    `cloud` = (e, n_lead): the block's first n_lead input channels are e (B, n_lead) repeated along the points -- the shape
    category embedding of the part-segmentation decoders, concatenated IN FRONT of the skip features (pointnext.py:662-663,
    pointnetv2.py:507-510); f1 holds the skip features alone.  The weight splits into [W_cls | W_skip | W_up] and
        W . [e ; f1 ; up(f2)] = W_skip . f1 + up(W_up . f2) + c,   c[b] = W_cls . e[b]
    with c added inside the skip conv's kernel (ops.pointwise_conv_cloud_term): no (B, n_lead + C1, n) tensor exists and
    that conv's reduction shrinks from n_lead + C1 to C1.  None when cloud_term_route says 'composition'.
    `force_cloud_term`: take the term wherever the block has the form for it (cloud_term_form), whatever the shape dispatch
    says -- for measuring the route on both sides of the dispatch rule (tools/cloud_term_bench.py)."""
    if cloud is not None:
        e, n_lead = cloud
        assert e.dim() == 2 and e.shape[1] == n_lead, "cloud = (e (B, n_lead), n_lead)"
        if not (cloud_term_form(blk, f1, f2, e) if force_cloud_term else cloud_term_route(blk, f1, f2, e) == 'cloud_term'):
            return None
        conv, bn, relu = conv_bn_block(blk)
        w_cls, w_rest = ops.split_weight(conv.weight, n_lead)
        w_skip, w_up = ops.split_weight(w_rest, f1.shape[1])
        y1 = ops.pointwise_conv_cloud_term(f1, w_skip, cloud_term(e, w_cls))
        y = ops.three_interpolate_add(conv1x1_weight(f2, w_up), geom['idx'], geom['weight'], y1, geom.get('csr'))
        return batchnorm_act(bn, y, relu)
    m = conv_bn_block(blk)
    if (m is None or m[2] is None or type(m[0]) not in (nn.Conv1d, Conv1d) or f1 is None or not f1.is_cuda
            or f1.dtype != torch.float32 or f2.dtype != torch.float32):
        return None
    conv, bn, relu = m
    c1 = f1.shape[1]
    if conv.bias is not None or conv.in_channels != c1 + f2.shape[1]:
        return None
    w1, w2 = ops.split_weight(conv.weight, c1)
    y = ops.three_interpolate_add(conv1x1_weight(f2, w2), geom['idx'], geom['weight'], conv1x1_weight(f1, w1), geom.get('csr'))
    return batchnorm_act(bn, y, relu)


def expand_cloud_channels(e, f1):
    """the reference's composition: e (B,E) repeated along the points, in front of the skip features f1 (B,C1,n)"""
    return torch.cat((e.unsqueeze(-1).expand(-1, -1, f1.shape[-1]), f1), dim=1)


# (round 3, cfg 5 = XL + ++ at 1 x 120000: threshold 4096 -> 19.8 ms per step, 16384 -> 19.1, 65536 -> 19.4, never -> 19.3; the
# shorter deep layers take the library GEMMs, which run on bf16 operands under autocast: ops.LibraryGemmConv)
_BF16_MIN_POSITIONS = 16384


def _bf16_pays(conv, x):
    """Under autocast the 1x1 convs with >= 64 channels on both sides over >= 16384 positions run on the bf16 MFMA
    (scratch/gemm_bench.py: 1.2-2x the fp32 kernels there).  Narrower layers are HBM-bound and shorter ones fill a fraction
    of the chip with 128 x 128 tiles: both keep their fp32 route, which is at least as accurate as what autocast asks for."""
    return min(conv.in_channels, conv.out_channels) >= 64 and x.numel() // x.shape[1] >= _BF16_MIN_POSITIONS


def _pw_pays(conv, x):
    """Measured on MI355X (scratch/pw_bench.py): the kernel beats MIOpen/rocBLAS (which wrap the weight gradient
    in NCHW<->NHWC transposes) on the wide, shallow layers -- stem, head, the two finest FeaturePropagation stages;
    the deep, narrow ones (>= 128 channels over <= 10^5 positions) are MFMA-bound GEMMs the library does better."""
    positions = x.numel() // x.shape[1]
    cin, cout = conv.in_channels, conv.out_channels
    if min(cin, cout) >= 64:  # csrc/gemm.hip: double-buffered 128x128 MFMA tiles, on par with the library GEMMs and
        return positions >= 65536  # without MIOpen's layout transposes around the weight gradient
    return positions >= 131072 and max(cin, cout) <= 128 or (max(cin, cout) <= 64 and positions >= 32768)


def run_convblocks(blocks, x, pool_max=False, pre=None, activated=False, residual=None, library=True):
    """Evaluate a stack of conv blocks (the nn.Sequential the factories above build), optionally followed by
    the max over the last (neighbour) dimension.  Where a block is conv -> BatchNorm [-> ReLU] (conv_bn_block), the conv
    takes conv1x1's route and BatchNorm, ReLU and (for the last block) the max-pool batchnorm_act's; everything else runs
    the stored modules as they are.  Parameters, buffers and their bookkeeping stay those of the nn modules.
    `pre`: the already computed output of the first block's convolution (the fused gather+conv kernel).
    `activated`: x is the activated output of a first block evaluated elsewhere (fused_first_block); `blocks` are the rest.
    `residual`: the result is relu(stack(x) + residual) -- an InvResMLP block's `f += identity; act(f)` -- inside the last
    block's BatchNorm kernels where that block is conv -> plain training-mode BatchNorm without activation.
    `library`: conv1x1's switch, handed to every conv of the stack."""
    mods = list(blocks)
    fused = _sa_tail_activated(mods, x, pool_max) if activated else _sa_tail(mods, pool_max, pre)
    if fused is not None:
        return fused
    finished = False  # the last block's batchnorm_act has pooled and added the residual
    for bi, blk in enumerate(mods):
        last = bi == len(mods) - 1
        m = conv_bn_block(blk)
        if m is not None:
            conv, bn, relu = m
            y = pre if (bi == 0 and pre is not None) else conv1x1(conv, x, bi == 0 and activated and wants_rows_grad(x), library)
            x = batchnorm_act(bn, y, relu, last and pool_max, residual if last else None)
            finished = last
        else:
            assert not (bi == 0 and pre is not None), "pre needs a conv -> norm block"
            sub = list(blk) if isinstance(blk, nn.Sequential) else None
            if sub is not None and len(sub) >= 1 and isinstance(sub[0], (nn.Conv1d, nn.Conv2d)):
                x = conv1x1(sub[0], x, library=library)
                for mod in sub[1:]:
                    x = mod(x)
            else:
                x = blk(x)
    if not finished:
        if pool_max:
            x = torch.max(x, dim=-1, keepdim=False)[0]
        if residual is not None:
            x = torch.relu(x + residual)
    return x


def wants_rows_grad(x1):
    """x1 is the output of an ops.GroupedConvBN that walks reverse edge lists in its backward (fused_first_block marks it):
    that gather reads the gradient as position-major (B,M,K,C) rows, and transposes any other layout first"""
    return bool(getattr(x1, '_amc3d_rows_grad', False))


def _sa_tail_conv(blk, x1):
    """(conv2, bn2, relu) of a second block the kernels of csrc/sa_tail.hip cover on the (B,C1,M,32) tensor x1 -- bias-free
    1x1 conv from C1 channels, plain training-mode BatchNorm, widths the kernels support and for which recomputing pays --
    or None"""
    m = conv_bn_block(blk)
    if (m is None or x1.dim() != 4 or not _fusable_bn(m[1], x1) or m[0].bias is not None or m[0].in_channels != x1.shape[1]
            or not ops.sa_tail_supported(x1.shape[1], m[0].out_channels, x1.shape[-1])
            or not ops.sa_tail_pays(x1.shape[1], m[0].out_channels)):
        return None
    return m


def _sa_tail(mods, pool_max, pre):
    """[conv0 (already applied: `pre`), BN, ReLU] -> [1x1 conv, BN (, ReLU)] -> max over 32 neighbours as one recomputing
    kernel family (csrc/sa_tail.hip), or None when the stack is not of that form."""
    if pre is None or not pool_max or len(mods) != 2:
        return None
    m0 = conv_bn_block(mods[0])
    if m0 is None or m0[2] is None or not _fusable_bn(m0[1], pre):
        return None
    m1 = _sa_tail_conv(mods[1], pre)
    if m1 is None:
        return None
    bn1, (conv2, bn2, relu) = m0[1], m1
    return ops.SATail.apply(pre, bn1.weight, bn1.bias, bn1.eps, conv2.weight, bn2.weight, bn2.bias, bn2.eps,
                            relu is not None, bn1, bn2)


def _sa_tail_activated(mods, x1, pool_max):
    """[1x1 conv, BN (, ReLU)] -> max over 32 neighbours on the activated first-layer output x1, as the recomputing
    kernel family of csrc/sa_tail.hip (ops.SATailActivated), or None"""
    if not pool_max or len(mods) != 1:
        return None
    m = _sa_tail_conv(mods[0], x1)
    if m is None:
        return None
    conv2, bn2, relu = m
    return ops.SATailActivated.apply(x1, conv2.weight, bn2.weight, bn2.bias, bn2.eps, relu is not None, bn2)


def _grouped_first_block(blocks, f, geom, feature_type):
    """(conv, bn, relu) of blocks[0] when the layer convolves [dp ; f[idx]] -- feature recipe 'dp_fj', a query in the plan,
    fp32 features on the GPU, a bias-free conv_bn_block from C + 3 channels -- so that the conv can run on the source points
    before the gather; else None"""
    if feature_type != 'dp_fj' or geom is None or 'idx' not in geom or f is None or not f.is_cuda or f.dtype != torch.float32:
        return None
    m = conv_bn_block(blocks[0])
    if m is None or m[0].bias is not None or m[0].in_channels != f.shape[1] + 3:
        return None
    return m


def fused_local_aggregation(blocks, f, geom, feature_type):
    """A stack of ONE conv block -- Conv2d 1x1 -> BatchNorm2d [-> ReLU] -- followed by the max over the neighbours (every
    LocalAggregation of InvResMLP, the single-layer SetAbstraction of PointNeXt-B/L/XL) as convolve-before-gather
    (amcontrast3d_amd/csrc/lagg.hip): the pooled (B,C,M) output, or None when the layer is not of that form."""
    m = _grouped_first_block(blocks, f, geom, feature_type) if len(blocks) == 1 else None
    if m is None or geom.get('mom') is None or not ops.local_aggregation_supported(m[0].out_channels, geom['idx'].shape[-1]):
        return None
    conv, bn, relu = m
    if _eval_bn(bn, f):
        return ops.local_aggregation_eval(f, geom['dp'], geom['idx'], conv.weight, bn, relu is not None)
    group = _synced_bn_group(bn, f)  # nn.SyncBatchNorm over several ranks: the statistics are exchanged between two phases
    if group is None and not _fusable_bn(bn, f):
        return None
    csr = geom.get('csr')  # deterministic mode: the plan's reverse lists, which the backward gathers over
    return ops.LocalAggregationFused.apply(f, geom['dp'], geom['idx'], geom['mom'], conv.weight, bn.weight, bn.bias, bn.eps,
                                           relu is not None, bn, group, (csr['start'], csr['edge']) if csr is not None else None)


def fused_first_block(blocks, f, geom, feature_type):
    """First block -- Conv2d 1x1 -> BatchNorm2d -> ReLU -- of a multi-layer neighbourhood MLP (PointNeXt-S'
    SetAbstraction, sa_layers = 2) convolved before the gather, its ACTIVATED output x1 (B,C,M,32) materialised for the
    blocks that follow (ops.GroupedConvBN), or None when the stack is not of that form."""
    m = _grouped_first_block(blocks, f, geom, feature_type) if len(blocks) >= 2 else None
    if (m is None or m[2] is None or geom.get('mom') is None
            or not ops.grouped_conv_bn_supported(m[0].out_channels, geom['idx'].shape[-1])):
        return None
    conv, bn, _ = m
    if _eval_bn(bn, f):
        return ops.grouped_conv_bn_eval(f, geom['dp'], geom['idx'], conv.weight, bn, True)
    group = _synced_bn_group(bn, f)
    if group is None and not _fusable_bn(bn, f):
        return None
    csr = geom.get('csr')
    if csr is not None:
        csr = (csr['start'], csr['edge'], csr.get('edge_dp'))
    x1 = ops.GroupedConvBN.apply(f, geom['dp'], geom['idx'], geom['mom'], conv.weight, bn.weight, bn.bias, bn.eps, True, bn,
                                 csr, group)
    if csr is not None and x1.requires_grad:
        x1._amc3d_rows_grad = True  # run_convblocks: the conv that consumes x1 writes its gradient as rows
    return x1


def fused_first_conv(blocks, f, geom, feature_type):
    """Output of the first block's 1x1 conv on [dp ; f[idx]] from the fused gather+conv MFMA kernel, or None
    when the layer is not of that form (then the caller groups, concatenates and convolves as usual)."""
    m = _grouped_first_block(blocks, f, geom, feature_type)
    if m is None or not ops.grouped_conv_supported(f.shape[1], m[0].out_channels):
        return None
    return ops.grouped_conv(f, geom['dp'], geom['idx'], m[0].weight)


# input width of the first grouped conv for each neighbourhood feature recipe
# (models/layers/local_aggregation.py:13-29)
CHANNEL_MAP = {
    'fj': lambda x: x, 'df': lambda x: x, 'assa': lambda x: x * 3, 'assa_dp': lambda x: x * 3 + 3,
    'dp_fj': lambda x: 3 + x, 'pj': lambda x: x, 'dp': lambda x: 3, 'pi_dp': lambda x: x + 3,
    'pj_dp': lambda x: x + 3, 'dp_fj_df': lambda x: x * 2 + 3, 'dp_fi_df': lambda x: x * 2 + 3,
    'pi_dp_fj_df': lambda x: x * 2 + 6, 'pj_dp_fj_df': lambda x: x * 2 + 6, 'pj_dp_df': lambda x: x + 6,
    'dp_df': lambda x: x + 3,
}
