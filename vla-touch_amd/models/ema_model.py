"""EMAModel — mirror of the reference's VLA/models/ema_model.py (`EMAModel(model, update_after_step, inv_gamma, power, min_value, max_value)`,
`get_decay`, `step`) over an `RdtTrainer`'s EMA copy.

The reference keeps a second RDTRunner and averages into it on the host side of torch; here the averaged weights are the trainer's `shadow`
tensors, updated on the device inside `RdtTrainer.optimizer_step` (one launch with AdamW).  This class is the reference's surface for it: it
carries the warm-up parameters into the trainer, answers `get_decay`, and `step()` reports the decay the trainer applied.
"""
from __future__ import annotations

from vlatouch.rdt_train import ema_decay


class EMAModel:
    def __init__(self, model, update_after_step=0, inv_gamma=1.0, power=2 / 3, min_value=0.0, max_value=0.9999):
        """model: an `RdtTrainer` (its EMA copy is the averaged model) or None (schedule only)."""
        self.averaged_model = model
        self.update_after_step = update_after_step
        self.inv_gamma = inv_gamma
        self.power = power
        self.min_value = min_value
        self.max_value = max_value
        self.decay = 0.0
        self.optimization_step = 0
        if model is not None:
            if getattr(model, "ema_updates", 0):
                raise RuntimeError("EMAModel: attach before the trainer's first optimizer step")
            model.ema_cfg = dict(update_after_step=update_after_step, inv_gamma=inv_gamma, power=power, min_value=min_value, max_value=max_value)

    def get_decay(self, optimization_step):
        return ema_decay(optimization_step, self.update_after_step, self.inv_gamma, self.power, self.min_value, self.max_value)

    def step(self, new_model=None):
        """The trainer's optimizer_step has already averaged on the device; this advances the reference's counter and records the decay it used."""
        tr = self.averaged_model
        if tr is not None and tr.ema_updates != self.optimization_step + 1:
            raise RuntimeError("EMAModel.step: call it once after each RdtTrainer.optimizer_step")
        self.decay = self.get_decay(self.optimization_step)
        self.optimization_step += 1

    def state_dict(self):
        return self.averaged_model.ema_state_dict()
