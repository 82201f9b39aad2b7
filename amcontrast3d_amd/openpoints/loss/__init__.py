from .build import LOSS, CrossEntropyAce, build_criterion_from_cfg
from .cross_entropy import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
