"""The plain criteria of openpoints.loss written out from their formulas, in the dtype of the logits (float64 for the reference
values, float32 to measure what the number format alone costs) -- torch only, nothing of the product is imported.  The list of
forms (`forms`), their inputs (`inputs`) and `evaluate` are shared by tools/record_loss_fixtures.py, which records what the
reference's own classes give for them, tests/test_loss_family_host.py and tests/test_gpu_loss_family.py.

The rule for labels outside [0, C) is the project's (include/amc3d.h): the point is left out of sums and denominators and gets a
zero gradient row.  The reference's classes raise on such labels, so no fixture depends on it.
"""
import numpy as np
import torch
import torch.nn.functional as F


def class_weights(C):
    return 0.5 + 1.5 * ((np.arange(C) * 7) % 5) / 4.0


def forms(C):
    """[{'id', 'cls', 'kwargs', 'labels'}]: the forms the issue lists.  labels: how the raw labels are drawn -- 'plain' in [0, C),
    'ignore3' (classes above 2 one higher, a quarter set to 3), 'negative' in [0, C] (ignore_index = -100 shifts labels >= 1 down)"""
    w = class_weights(C)
    alpha = [float(v) for v in 0.25 + 0.5 * ((np.arange(C) * 3) % 4) / 3.0]
    out = [("smooth_default", "SmoothCrossEntropy", {}, "plain"),
           ("smooth_eps0", "SmoothCrossEntropy", {"label_smoothing": 0}, "plain"),
           ("smooth_ignore3", "SmoothCrossEntropy", {"ignore_index": 3, "num_classes": C}, "ignore3"),
           ("smooth_ignore_negative", "SmoothCrossEntropy", {"ignore_index": -100, "num_classes": C}, "negative"),
           ("smooth_weight", "SmoothCrossEntropy", {"weight": w}, "plain"),
           ("smooth_weight_eps0", "SmoothCrossEntropy", {"weight": w, "label_smoothing": 0}, "plain"),
           ("masked", "MaskedCrossEntropy", {}, "plain"),
           ("bce", "BCELogits", {}, "plain"),
           ("focal_gamma0", "FocalLoss", {"gamma": 0}, "plain"),
           ("focal_gamma0.5", "FocalLoss", {"gamma": 0.5}, "plain"),
           ("focal_gamma2", "FocalLoss", {"gamma": 2}, "plain"),
           ("focal_alpha", "FocalLoss", {"gamma": 2, "alpha": alpha}, "plain"),
           ("focal_sum", "FocalLoss", {"gamma": 2, "size_average": False}, "plain"),
           ("poly1ce_mean", "Poly1CrossEntropyLoss", {"num_classes": C}, "plain"),
           ("poly1ce_sum", "Poly1CrossEntropyLoss", {"num_classes": C, "reduction": "sum"}, "plain"),
           ("poly1ce_weight", "Poly1CrossEntropyLoss", {"num_classes": C, "weight": torch.from_numpy(w).float()}, "plain"),
           ("poly1focal_default", "Poly1FocalLoss", {}, "plain"),
           ("poly1focal_noalpha", "Poly1FocalLoss", {"alpha": -1, "gamma": 1.5, "epsilon": 0.5}, "plain")]
    return [dict(id=i, cls=c, kwargs=k, labels=l) for i, c, k, l in out]


def inputs(C, N, labels="plain", B=2, seed=0):
    """-> logits (B, C, N) float32, raw labels (B, N) int64, mask (B, N) int64 with about 30 % zeros"""
    g = torch.Generator().manual_seed(1000 * C + N + 7 * seed)
    logits = torch.randn(B, C, N, generator=g) * 3
    if labels == "negative":
        target = torch.randint(0, C + 1, (B, N), generator=g)
    else:
        target = torch.randint(0, C, (B, N), generator=g)
    if labels == "ignore3":
        target = torch.where(target >= 3, target + 1, target)
        target[torch.rand(B, N, generator=g) < 0.25] = 3
    mask = (torch.rand(B, N, generator=g) >= 0.3).long()
    return logits, target, mask


def _rows(x):
    return x.transpose(1, 2).reshape(-1, x.shape[1]) if x.dim() == 3 else x


def _table(v, like):
    return None if v is None else torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(like.dtype).reshape(-1)


def _in_range(y, C):
    return (y >= 0) & (y < C)


def smooth_cross_entropy(logits, gt, label_smoothing=0.2, ignore_index=None, num_classes=None, weight=None, return_valid=False):
    x, gt = _rows(logits), gt.reshape(-1)
    C = x.shape[1]
    keep = torch.ones_like(gt, dtype=torch.bool)
    y = gt
    if ignore_index is not None:
        labels = list(range(num_classes + 1))
        table = torch.tensor(labels[:ignore_index] + [0] + labels[ignore_index:])
        keep = (gt != ignore_index) & (gt >= 0) & (gt < len(table))
        y = table[gt.clamp(0, len(table) - 1)]
    keep = keep & _in_range(y, C)
    lp, y = F.log_softmax(x[keep], dim=1), y[keep]
    w = _table(weight, x)
    w = torch.ones(C, dtype=x.dtype) if w is None else w
    own = lp.gather(1, y.view(-1, 1)).view(-1)
    if label_smoothing > 0:
        others = (lp * w).sum(1) - w[y] * own
        off = torch.tensor(label_smoothing, dtype=x.dtype) / (C - 1)  # (C = 1: inf, and inf * 0 = NaN as in the reference)
        return -((1 - label_smoothing) * w[y] * own + off * others).sum() / keep.sum()
    return -(w[y] * own).sum() / w[y].sum()


def masked_cross_entropy(logits, gt, mask, label_smoothing=0.2):
    x, gt = _rows(logits), gt.reshape(-1)
    C = x.shape[1]
    keep = (mask.reshape(-1) == 1) & _in_range(gt, C)
    lp, y = F.log_softmax(x[keep], dim=1), gt[keep]
    own = lp.gather(1, y.view(-1, 1)).view(-1)
    return -((1 - label_smoothing) * own + label_smoothing / C * lp.sum(1)).sum() / keep.sum()


def focal_loss(logits, gt, gamma=0, alpha=None, size_average=True):
    x, gt = _rows(logits), gt.reshape(-1)
    keep = _in_range(gt, x.shape[1])
    y = gt[keep]
    own = F.log_softmax(x[keep], dim=1).gather(1, y.view(-1, 1)).view(-1)
    focus = (1 - own.detach().exp()) ** gamma
    a = 1 if alpha is None else _table(alpha, x)[y]
    total = -(focus * a * own).sum()
    return total / keep.sum() if size_average else total


def poly1_cross_entropy(logits, gt, num_classes=50, epsilon=1.0, reduction="mean", weight=None):
    x, gt = _rows(logits), gt.reshape(-1)
    assert x.shape[1] == num_classes
    keep = _in_range(gt, num_classes)
    y = gt[keep]
    own = F.log_softmax(x[keep], dim=1).gather(1, y.view(-1, 1)).view(-1)
    w = 1 if weight is None else _table(weight, x)[y]
    total = (-w * own + epsilon * (1 - own.exp())).sum()
    return total / keep.sum() if reduction == "mean" else total


def _elements(logits, gt):
    """the counted points' logits (M, C), their one-hot bits, z = t ? -x : x"""
    x, gt = _rows(logits), gt.reshape(-1)
    keep = _in_range(gt, x.shape[1])
    x = x[keep]
    t = torch.zeros_like(x, dtype=torch.bool)
    t[torch.arange(x.shape[0]), gt[keep]] = True
    return x, t, torch.where(t, -x, x)


def bce_logits(logits, gt, weight=None, pos_weight=None, reduction="mean"):
    x, t, z = _elements(logits, gt)
    value = -F.logsigmoid(-z)  # -log(pt)
    if pos_weight is not None:
        value = torch.where(t, _table(pos_weight, x) * value, value)
    if weight is not None:
        value = value * _table(weight, x)
    return value.sum() / x.numel() if reduction == "mean" else value.sum()


def poly1_focal(logits, gt, epsilon=1.0, alpha=0.25, gamma=2.0, reduction="mean"):
    x, t, z = _elements(logits, gt)
    u = torch.sigmoid(z)  # 1 - pt
    focal = -F.logsigmoid(-z) * u ** gamma
    if alpha >= 0:
        focal = torch.where(t, alpha * focal, (1 - alpha) * focal)
    value = focal + epsilon * u ** (gamma + 1)
    return value.sum() / x.numel() if reduction == "mean" else value.sum()


def multi_shape(inner, logits_all_shapes, points_labels, shape_labels):
    total = 0
    for i in range(shape_labels.shape[0]):
        total = total + inner(logits_all_shapes[int(shape_labels[i])][i][None], points_labels[i][None])
    return total / shape_labels.shape[0]


def label_smoothing_ce(x, y, label_smoothing=0.1):
    lp = F.log_softmax(x, dim=1)
    own = lp.gather(1, y.view(-1, 1)).view(-1)
    return -((1 - label_smoothing) * own + label_smoothing * lp.mean(1)).mean()


def soft_target_ce(x, q):
    return -(q.to(x.dtype) * F.log_softmax(x, dim=1)).sum(1).mean()


RESTATEMENTS = {"SmoothCrossEntropy": smooth_cross_entropy, "MaskedCrossEntropy": masked_cross_entropy, "BCELogits": bce_logits,
                "FocalLoss": focal_loss, "Poly1CrossEntropyLoss": poly1_cross_entropy, "Poly1FocalLoss": poly1_focal}


def evaluate(form, logits, target, mask=None, dtype=torch.float64, scale=1.0):
    """-> (loss, d(scale * loss) / d logits) of the restatement evaluated in `dtype`, both as float64 CPU tensors"""
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    args = (x, target.cpu()) + ((mask.cpu(),) if form["cls"] == "MaskedCrossEntropy" else ())
    loss = RESTATEMENTS[form["cls"]](*args, **form["kwargs"])
    grad = torch.autograd.grad(loss * scale, x, allow_unused=True)[0] if loss.requires_grad else None
    grad = torch.zeros_like(x) if grad is None else grad
    return loss.detach().double(), grad.double()
