"""Multi-step learning-rate schedule with optional linear warm-up (openpoints/scheduler/multistep_lr.py,
scheduler_factory.py:12-86; ``sched: multistep``, ``decay_epochs: [70, 90]``, ``decay_rate: 0.1`` in
cfgs/scannet/default.yaml:78-80).

The driver-facing interface of CosineLRScheduler.  The lr of epoch t is ``base * decay_rate ** k`` with k the number of
decay epochs ``<= t + 1``: the trainer calls ``step(epoch)`` at the END of epoch ``epoch`` (epochs count from 1), so the value
set then is the one epoch ``epoch + 1`` trains with, and a decay epoch of 70 takes effect from the 70th epoch on.  The
lr-noise options are not built and raise, as in cosine_lr.py.
"""
import bisect

from .cosine_lr import CosineLRScheduler


class MultiStepLRScheduler(CosineLRScheduler):
    def __init__(self, optimizer, decay_t, decay_rate=1., warmup_t=0, warmup_lr_init=0, t_in_epochs=True, noise_range_t=None,
                 noise_pct=0.67, noise_std=1.0, noise_seed=42, initialize=True):
        if noise_range_t is not None:
            raise NotImplementedError("lr noise is not part of the AMContrast3D configs")
        self.optimizer = optimizer
        for group in optimizer.param_groups:
            if initialize:
                group.setdefault("initial_lr", group["lr"])
            elif "initial_lr" not in group:
                raise KeyError("initial_lr is not specified in param_groups when resuming a scheduler")
        self.base_values = [g["initial_lr"] for g in optimizer.param_groups]
        self.decay_t = sorted(decay_t)  # bisect assumes a sorted list
        self.decay_rate = decay_rate
        self.warmup_t, self.warmup_lr_init, self.t_in_epochs = warmup_t, warmup_lr_init, t_in_epochs
        if warmup_t:
            self.warmup_steps = [(v - warmup_lr_init) / warmup_t for v in self.base_values]
            self._set([warmup_lr_init] * len(self.base_values))
        else:
            self.warmup_steps = [1 for _ in self.base_values]
            self._set(self.base_values)

    def get_curr_decay_steps(self, t):
        return bisect.bisect_right(self.decay_t, t + 1)

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        return [v * (self.decay_rate ** self.get_curr_decay_steps(t)) for v in self.base_values]

    def get_cycle_length(self, cycles=0):
        raise NotImplementedError("a multi-step schedule has no cycle")
