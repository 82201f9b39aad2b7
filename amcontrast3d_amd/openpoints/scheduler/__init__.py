from .cosine_lr import CosineLRScheduler, build_scheduler_from_cfg  # noqa: F401
from .multistep_lr import MultiStepLRScheduler  # noqa: F401
