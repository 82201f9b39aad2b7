"""LOSS registry and the cross-entropy + adaptive-margin-contrast criterion.

Drop-in for openpoints/loss/build.py: ``LOSS`` (:9-12), ``CrossEntropyAce`` (:324-346),
``build_criterion_from_cfg`` (:348-357), and the plain criteria of :14-274 (SmoothCrossEntropy, MaskedCrossEntropy, BCELogits,
FocalLoss, Poly1CrossEntropyLoss, Poly1FocalLoss, MultiShapeCrossEntropy) under the reference's names, constructor keywords,
attribute names and call signatures.  On fp32 CUDA contiguous (B, C, N) logits with (B, N) int64 targets and a scalar
reduction each of them is one form of ops.point_loss_softmax / ops.point_loss_sigmoid; every other input (CPU tensors, (M, C)
rows, other dtypes, reduction='none', return_valid=True) takes the torch composition written next to it.
"""
import torch
import torch.nn.functional as F
from torch.nn import BCEWithLogitsLoss, CrossEntropyLoss

from openpoints.AMContrast3D.MarginContrast import ContrastHead
from openpoints.utils import registry

LOSS = registry.Registry('loss')


class CrossEntropy(CrossEntropyLoss):
    """What the registry builds for 'CrossEntropy' / 'CrossEntropyLoss' (loss/build.py:10-11 registers torch's class): the
    criterion of the plain PointNeXt trainer, `criterion(logits, target)` on the model's (B, ncls, N) logits
    (examples/segmentation/main.py:224-230, 357-358).  With label smoothing and / or class weights, mean reduction, fp32 CUDA
    logits and (B, N) int64 targets it is one fused pass (ops.cross_entropy_general); every other input is torch's forward,
    unchanged -- the module without smoothing and weights included.  CrossEntropyAce / CrossEntropyAcePre construct torch's
    class themselves and never come here."""

    def forward(self, input, target):
        if ((self.label_smoothing > 0.0 or self.weight is not None) and self.reduction == 'mean' and _kernel_route(input, target)
                and (self.weight is None or (self.weight.is_cuda and self.weight.dtype == torch.float32))):
            from amcontrast3d_amd.ops import cross_entropy_general
            return cross_entropy_general(input, target, self.ignore_index, self.label_smoothing, self.weight)
        return super().forward(input, target)


LOSS.register_module(name='CrossEntropy', module=CrossEntropy)
LOSS.register_module(name='CrossEntropyLoss', module=CrossEntropy)
LOSS.register_module(name='BCEWithLogitsLoss', module=BCEWithLogitsLoss)


# ---- the plain criteria (loss/build.py:14-274) --------------------------------------------------------------------------------
def _kernel_route(logits, target):
    """the inputs the point-loss kernels take: channel-major fp32 logits as the model returns them, one int64 label per point"""
    return (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
            and torch.is_tensor(target) and target.dtype == torch.int64 and target.shape == (logits.shape[0], logits.shape[2]))


def _class_table(values):
    """class weights as the constructors get them (numpy array, list, tensor or None) -> fp32 tensor (C) or None (the
    reference squeezes a (1, C) array; flattening is the same, and keeps one class a vector)"""
    return None if values is None else torch.as_tensor(values).detach().float().reshape(-1)


def _follow(module, name, like):
    """a plain tensor attribute (the reference keeps these outside the buffers) follows the logits' device at the first call"""
    t = getattr(module, name, None)
    if torch.is_tensor(t) and t.device != like.device:
        t = t.to(like.device)
        setattr(module, name, t)
    return t


def _fits(table, C):
    return table is None or (table.dtype == torch.float32 and table.shape == (C,))


def _rows(logits):
    return logits.transpose(1, 2).reshape(-1, logits.shape[1]) if logits.dim() > 2 else logits


@LOSS.register_module()
class SmoothCrossEntropy(torch.nn.Module):
    """loss/build.py:14-66.  Kept as there: points with gt == ignore_index are dropped and the others' labels go through
    `reducing_list` (range(num_classes + 1) with a 0 inserted at ignore_index: labels above a non-negative ignore_index move down
    by one, and under a NEGATIVE ignore_index the slice puts the 0 in front, so every label >= 1 moves down by one); with
    smoothing the target distribution is (1 - eps) on the label and eps / (C - 1) on the others, class weights enter per class
    inside the sum and the mean is over the counted points; without, it is F.cross_entropy(pred, gt, weight)."""

    def __init__(self, label_smoothing=0.2, ignore_index=None, num_classes=None, weight=None, return_valid=False):
        super().__init__()
        self.label_smoothing = label_smoothing
        self.ignore_index = ignore_index
        self.return_valid = return_valid
        if ignore_index is not None:
            labels = list(range(num_classes + 1))
            self.reducing_list = torch.tensor(labels[:ignore_index] + [0] + labels[ignore_index:], dtype=torch.int64)
        self.weight = _class_table(weight)

    def forward(self, pred, gt):
        weight = _follow(self, 'weight', pred)
        remap = _follow(self, 'reducing_list', pred) if self.ignore_index is not None else None
        eps = self.label_smoothing
        if not self.return_valid and _kernel_route(pred, gt) and _fits(weight, pred.shape[1]) and 0 <= eps < 1:
            from amcontrast3d_amd.ops import point_loss_softmax
            return point_loss_softmax(pred, gt, remap=remap, ignore_index=self.ignore_index, weight=weight, weight_per_class=eps > 0,
                                      eps=eps, eps_rule=1, den='count' if eps > 0 else 'weight')
        pred, gt = _rows(pred), gt.contiguous().view(-1)
        if self.ignore_index is not None:
            valid = gt != self.ignore_index
            pred, gt = pred[valid, :], remap[gt[valid]]
        if eps > 0:
            hot = F.one_hot(gt, pred.shape[1]).to(pred.dtype)
            q = hot * (1 - eps) + (1 - hot) * eps / (pred.shape[1] - 1)
            terms = q * F.log_softmax(pred, dim=1)
            loss = -(terms if weight is None else terms * weight).sum(dim=1).mean()
        else:
            loss = F.cross_entropy(pred, gt, weight=weight)
        return (loss, pred, gt) if self.return_valid else loss


@LOSS.register_module()
class MaskedCrossEntropy(torch.nn.Module):
    """loss/build.py:69-81: nn.CrossEntropyLoss(label_smoothing) over the points whose mask is 1; `criterion(logit, target, mask)`"""

    def __init__(self, label_smoothing=0.2):
        super().__init__()
        self.creterion = CrossEntropyLoss(label_smoothing=label_smoothing)  # attribute name as in the reference

    def forward(self, logit, target, mask):
        crit = self.creterion
        if _kernel_route(logit, target) and mask.is_cuda and mask.numel() == target.numel() and crit.weight is None and crit.reduction == 'mean':
            from amcontrast3d_amd.ops import point_loss_softmax
            return point_loss_softmax(logit, target, ignore_index=crit.ignore_index, mask=(mask == 1).to(torch.int32),
                                      eps=crit.label_smoothing, eps_rule=0)
        idx = mask.flatten() == 1
        return crit(_rows(logit)[idx], target.flatten()[idx])


@LOSS.register_module()
class BCELogits(torch.nn.Module):
    """loss/build.py:83-95: nn.BCEWithLogitsLoss(**kwargs) against the one-hot of the labels, over all B*N*C elements"""

    def __init__(self, **kwargs):
        super().__init__()
        self.criterion = BCEWithLogitsLoss(**kwargs)

    def forward(self, logits, targets):
        crit = self.criterion
        if (_kernel_route(logits, targets) and crit.reduction in ('mean', 'sum') and _fits(crit.weight, logits.shape[1])
                and _fits(crit.pos_weight, logits.shape[1]) and all(t is None or t.is_cuda for t in (crit.weight, crit.pos_weight))):
            from amcontrast3d_amd.ops import point_loss_sigmoid
            return point_loss_sigmoid(logits, targets, weight=crit.weight, pos_weight=crit.pos_weight,
                                      den='count' if crit.reduction == 'mean' else 'one')
        logits = _rows(logits)
        hot = F.one_hot(targets.contiguous().view(-1), num_classes=logits.shape[-1]).to(device=logits.device, dtype=logits.dtype)
        return crit(logits, hot)


@LOSS.register_module()
class FocalLoss(torch.nn.Module):
    """loss/build.py:97-129: -(1 - pt)^gamma alpha[y] log_softmax[y], mean (size_average) or sum.  Kept as there: pt is DETACHED,
    so (1 - pt)^gamma is a constant of the backward, and a float alpha becomes the two-class table [alpha, 1 - alpha]."""

    def __init__(self, gamma=0, alpha=None, size_average=True):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha
        if isinstance(alpha, (float, int)):
            self.alpha = torch.Tensor([alpha, 1 - alpha])
        if isinstance(alpha, list):
            self.alpha = torch.Tensor(alpha)
        self.size_average = size_average

    def forward(self, logit, target):
        alpha = _follow(self, 'alpha', logit)
        if _kernel_route(logit, target) and _fits(alpha, logit.shape[1]) and self.gamma >= 0:
            from amcontrast3d_amd.ops import point_loss_softmax
            return point_loss_softmax(logit, target, gamma=self.gamma, alpha=alpha, den='count' if self.size_average else 'one')
        if logit.dim() > 2:
            logit = _rows(logit.reshape(logit.size(0), logit.size(1), -1))
        target = target.reshape(-1)
        logpt = F.log_softmax(logit, dim=1).gather(1, target.view(-1, 1)).view(-1)
        pt = logpt.detach().exp()
        if alpha is not None:
            logpt = logpt * alpha.to(logit.dtype).gather(0, target)
        loss = -1 * (1 - pt) ** self.gamma * logpt
        return loss.mean() if self.size_average else loss.sum()


@LOSS.register_module()
class Poly1CrossEntropyLoss(torch.nn.Module):
    """loss/build.py:134-178: w[y] CE + epsilon (1 - p[y]) per point, then mean / sum / none.  Kept as there: 'mean' is the plain
    mean over the points also with class weights (not torch's weighted mean)."""

    def __init__(self, num_classes: int = 50, epsilon: float = 1.0, reduction: str = "mean", weight: torch.Tensor = None):
        super().__init__()
        self.num_classes = num_classes
        self.epsilon = epsilon
        self.reduction = reduction
        self.weight = _class_table(weight)

    def forward(self, logits, labels):
        weight = _follow(self, 'weight', logits)
        if (_kernel_route(logits, labels) and self.reduction in ('mean', 'sum') and logits.shape[1] == self.num_classes
                and _fits(weight, logits.shape[1])):
            from amcontrast3d_amd.ops import point_loss_softmax
            return point_loss_softmax(logits, labels, weight=weight, poly=self.epsilon, den='count' if self.reduction == 'mean' else 'one')
        logits, labels = _rows(logits), labels.contiguous().view(-1)
        hot = F.one_hot(labels, num_classes=self.num_classes).to(device=logits.device, dtype=logits.dtype)
        pt = (hot * F.softmax(logits, dim=-1)).sum(dim=-1)
        poly1 = F.cross_entropy(logits, labels, reduction='none', weight=weight) + self.epsilon * (1 - pt)
        if self.reduction == "mean":
            return poly1.mean()
        return poly1.sum() if self.reduction == "sum" else poly1


@LOSS.register_module()
class Poly1FocalLoss(torch.nn.Module):
    """loss/build.py:181-257: per element of the logits against the one-hot labels, FL = bce (1 - pt)^gamma, times alpha_t when
    alpha >= 0, plus epsilon (1 - pt)^(gamma + 1); mean / sum / none over all elements.  A `weight` / `pos_weight` broadcasts along
    the LAST axis of (B, C, N) there (the points, not the classes): such calls stay on the torch composition, which keeps that."""

    def __init__(self, epsilon: float = 1.0, alpha: float = 0.25, gamma: float = 2.0, reduction: str = "mean",
                 weight: torch.Tensor = None, pos_weight: torch.Tensor = None, label_is_onehot: bool = False, **kwargs):
        super().__init__()
        self.epsilon = epsilon
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction
        self.weight = weight
        self.pos_weight = pos_weight
        self.label_is_onehot = label_is_onehot

    def forward(self, logits, labels):
        if (not self.label_is_onehot and _kernel_route(logits, labels) and self.weight is None and self.pos_weight is None
                and self.reduction in ('mean', 'sum') and self.gamma >= 0 and self.alpha <= 1):
            from amcontrast3d_amd.ops import point_loss_sigmoid
            return point_loss_sigmoid(logits, labels, alpha=self.alpha, gamma=self.gamma, poly=self.epsilon,
                                      den='count' if self.reduction == 'mean' else 'one')
        if not self.label_is_onehot:
            labels = F.one_hot(labels, logits.shape[1])
            if labels.dim() > 2:
                labels = labels.movedim(-1, 1)
        labels = labels.to(device=logits.device, dtype=logits.dtype)
        p = torch.sigmoid(logits)
        bce = F.binary_cross_entropy_with_logits(logits, labels, reduction="none", weight=self.weight, pos_weight=self.pos_weight)
        pt = labels * p + (1 - labels) * (1 - p)
        focal = bce * (1 - pt) ** self.gamma
        if self.alpha >= 0:
            focal = (self.alpha * labels + (1 - self.alpha) * (1 - labels)) * focal
        poly1 = focal + self.epsilon * torch.pow(1 - pt, self.gamma + 1)
        if self.reduction == "mean":
            return poly1.mean()
        return poly1.sum() if self.reduction == "sum" else poly1


@LOSS.register_module()
class MultiShapeCrossEntropy(torch.nn.Module):
    """loss/build.py:259-274: the mean over the batch of an inner criterion (built from the registry) applied to each cloud's
    logits, taken from the entry of `logits_all_shapes` its shape label names.  A host loop, as there."""

    def __init__(self, criterion_args, **kwargs):
        super().__init__()
        self.criterion = build_criterion_from_cfg(criterion_args)

    def forward(self, logits_all_shapes, points_labels, shape_labels):
        batch_size = shape_labels.shape[0]
        losses = 0
        for i in range(batch_size):
            logits = logits_all_shapes[shape_labels[i]][i].unsqueeze(0)
            losses = losses + self.criterion(logits, points_labels[i].unsqueeze(0))
        return losses / batch_size


def _cross_entropy(crit, logit, target):
    """(CE value, flattened target): nn.CrossEntropyLoss on the (B*N, ncls) view of the logits, through the fused
    kernel when the module is the plain default"""
    if (type(crit) is CrossEntropyLoss and crit.weight is None and crit.label_smoothing == 0.0
            and crit.reduction == 'mean' and logit.is_cuda and logit.dtype == torch.float32 and logit.dim() == 3):
        # same value without the (B*N, ncls) transposed copy: one fused pass over the (B,ncls,N) logits
        from amcontrast3d_amd.ops import cross_entropy_mean
        return cross_entropy_mean(logit, target, crit.ignore_index), target.flatten()
    target = target.flatten()
    return crit(logit.transpose(1, 2).reshape(-1, logit.shape[1]), target), target


def _l1_mean(crit, pred, target, rows=1024):
    """nn.L1Loss()(pred, target) in two small reduction stages on the GPU.  torch reduces a long vector to one number with a
    multi-block kernel whose arrival counters it zeroes with cudaMemsetAsync; recorded into a graph that is a memset NODE, and
    ROCm 7.2 does not reliably order a memset node before the kernel nodes behind it at replay (the fault
    the radix sort's memsets caused) -- here the counters of a reduction, i.e. a sum that may silently come out wrong.  Rows
    of `rows` elements summed per row, then the row sums: neither stage crosses workgroups.  Same value up to the order of the
    fp32 additions (1e-7 relative); anything but the plain mean on CUDA tensors goes to the module itself."""
    if not (type(crit) is torch.nn.L1Loss and crit.reduction == 'mean' and pred.is_cuda and pred.dim() == 1
            and pred.shape == target.shape and pred.numel() > rows):
        return crit(pred, target)
    d = (pred - target).abs()
    n = d.numel()
    pad = (-n) % rows
    if pad:
        d = torch.nn.functional.pad(d, (0, pad))
    return d.view(-1, rows).sum(1).sum() / n


@LOSS.register_module()
class CrossEntropyAce(torch.nn.Module):
    """w1 * CE(logits, target) + w2 * sum_stage contrast(stage).  Like the reference, the
    constructor accepts and ignores label_smoothing / weight / ignore_index (build.py:326-329)."""

    def __init__(self, **kwargs):
        super().__init__()
        self.creterion = CrossEntropyLoss()  # attribute name as in the reference
        self.contrast_head = ContrastHead()

    def forward(self, logit, target, stageACE_list, num_classes, ignore_index, ambiguity_args):
        ce, target = _cross_entropy(self.creterion, logit, target)
        # (w2 * contrast: the head applies the weight, in the loss kernels where one call takes every stage)
        contrast, _, _ = self.contrast_head(logit, target, stageACE_list, num_classes, ignore_index, ambiguity_args,
                                            scale=ambiguity_args.w2)
        return ambiguity_args.w1 * ce + contrast


@LOSS.register_module()
class CrossEntropyAcePre(torch.nn.Module):
    """AMContrast3D++ objective (loss/build.py:281-319): w1 * CE + w2 * contrast for the segmentation, and
    w3 * L1(predicted ambiguity, AEF ambiguity) for the APM, returned separately:
    (segmentation loss, w1*CE, w2*contrast, w3*regression)."""

    def __init__(self, **kwargs):
        super().__init__()
        self.creterion = CrossEntropyLoss()
        self.contrast_head = ContrastHead()
        self.MAE = torch.nn.L1Loss()
        self.MSE = torch.nn.MSELoss()
        self.HUBER = torch.nn.HuberLoss(reduction='mean', delta=0.1)

    def forward(self, logit, target, stageACE_list, num_classes, ignore_index, ambiguity_args):
        ce, target = _cross_entropy(self.creterion, logit, target)
        contrast, target_ai, _ = self.contrast_head(logit, target, stageACE_list, num_classes, ignore_index,
                                                    ambiguity_args, scale=ambiguity_args.w2)  # = w2 * contrast
        logits_ai = torch.cat(stageACE_list['ambiguity']).flatten()
        regression = _l1_mean(self.MAE, logits_ai, target_ai)
        ce = ambiguity_args.w1 * ce
        regression = ambiguity_args.w3 * regression
        return ce + contrast, ce, contrast, regression


def build_criterion_from_cfg(cfg, **kwargs):
    """Build the criterion named by ``cfg.NAME``."""
    return LOSS.build(cfg, **kwargs)
