"""The two classification criteria of openpoints/loss/cross_entropy.py, on (M, C) rows: plain torch modules, no kernel
(they are not on a segmentation path: one row per cloud)."""
import torch
import torch.nn.functional as F

from .build import LOSS


@LOSS.register_module()
class LabelSmoothingCrossEntropy(torch.nn.Module):
    """(1 - s) * NLL + s * (mean over the classes of -log_softmax), averaged over the rows"""

    def __init__(self, label_smoothing=0.1):
        super().__init__()
        self.smoothing = label_smoothing
        self.confidence = 1. - self.smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        logprobs = F.log_softmax(x, dim=1)
        nll = -logprobs.gather(dim=1, index=target.unsqueeze(1)).squeeze(1)
        uniform = -logprobs.mean(dim=-1)
        return (self.confidence * nll + self.smoothing * uniform).mean()


@LOSS.register_module()
class SoftTargetCrossEntropy(torch.nn.Module):
    """cross entropy against a row of class probabilities, averaged over the rows"""

    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return torch.sum(-target * F.log_softmax(x, dim=-1), dim=-1).mean()
