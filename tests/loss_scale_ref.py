"""The statement of fp16 fine-tuning's loss scaling (vlatouch/rdt_train.py: LossScaler, RdtTrainer.optimizer_step;
csrc/vt_train_rdt.hip: vt_grad_unscale_clip_multi), in torch on the CPU, written apart from the code it states.

Order of one optimizer step (the reference's loop, VLA/train/train.py:404-453, under accelerate's fp16 mode):
    accelerator.backward (loss * S) -> accelerator.clip_grad_norm_ (GradScaler.unscale_, then clip_grad_norm_) -> scaler.step(optimizer)
    -> scaler.update() -> lr_scheduler.step() (not after a skipped optimizer step) -> ema_model.step() (always) -> global_step += 1 (always)

Scale arithmetic (torch/amp/grad_scaler.py `update`, ATen _amp_update_scale_), all in fp32 like GradScaler's scale tensor:
    overflow:  S *= backoff_factor, tracker = 0
    clean:     tracker += 1; if tracker == growth_interval: S *= growth_factor (unless the product is not finite), tracker = 0
Unscale-then-clip over the scaled gradients g:
    found_inf = any(!isfinite(g))                    on the RAW element (_amp_foreach_non_finite_check_and_unscale_)
    inv_S     = float(1 / double(S))                 (`self._scale.double().reciprocal().float()`)
    u         = g * inv_S                            one fp32 multiplication
    norm      = || u ||_2,  coef = min(max_norm / (norm + 1e-6), 1)     (clip_grad_norm_, fp32)
    g        <- u * coef                             a SECOND fp32 multiplication, always (torch multiplies by the clamped coefficient)
With found_inf set nothing is stepped; the device kernel then writes no gradient either."""
import torch

F32 = torch.float32
DEFAULTS = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)

# 40 optimizer steps, True = the gradients overflowed.  With growth_interval 3 it holds two overflows in a row (steps 4, 5), an overflow on the step
# where growth would have fired (step 11: the tracker stands at 2 after the clean steps 9, 10), growth (e.g. after steps 0-2) and a final run of growth.
OVERFLOW_SEQUENCE = [n in (4, 5, 11, 17, 18, 19, 27, 33) for n in range(40)]


def inv_scale(scale: float) -> torch.Tensor:
    """float(1 / double(S)) as a 0-d fp32 tensor."""
    return torch.tensor(scale, dtype=F32).double().reciprocal().float()


class Scaler:
    """scale (0-d fp32 tensor) and growth tracker under `update(found_inf)`; dynamic=False: a static scale that only counts."""

    def __init__(self, init_scale=DEFAULTS["init_scale"], growth_factor=DEFAULTS["growth_factor"], backoff_factor=DEFAULTS["backoff_factor"],
                 growth_interval=DEFAULTS["growth_interval"], dynamic=True):
        self.scale = torch.tensor(init_scale, dtype=F32)
        self.growth_factor, self.backoff_factor, self.growth_interval, self.dynamic = growth_factor, backoff_factor, growth_interval, dynamic
        self.tracker = 0
        self.skipped = 0

    def update(self, found_inf: bool) -> None:
        if found_inf:
            self.skipped += 1
            self.tracker = 0
            if self.dynamic:
                self.scale = self.scale * torch.tensor(self.backoff_factor, dtype=F32)
            return
        self.tracker += 1
        if self.tracker == self.growth_interval:
            self.tracker = 0
            grown = self.scale * torch.tensor(self.growth_factor, dtype=F32)
            if self.dynamic and bool(torch.isfinite(grown)):
                self.scale = grown

    @property
    def value(self) -> float:
        return float(self.scale)


def total_norm(tensors) -> torch.Tensor:
    """clip_grad_norm_'s norm: the 2-norm of the tensors' 2-norms (fp32, torch's own summation)."""
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(t, 2.0) for t in tensors]), 2.0)


def unscale_clip(grads, scale: float, max_norm: float, norm=None):
    """grads: fp32 tensors holding S-times-too-large gradients -> (found_inf, norm, coef, new gradients).  `norm` overrides the norm of the
    unscaled gradients (a 0-d fp32 tensor or a float: a device kernel sums in its own fixed order, and the coefficient follows ITS norm);
    None takes torch's.  With found_inf the gradients come back untouched."""
    found_inf = any(not bool(torch.isfinite(g).all()) for g in grads)
    inv = inv_scale(scale)
    u = [g * inv for g in grads]
    norm = total_norm(u) if norm is None else torch.as_tensor(norm, dtype=F32)
    coef = torch.clamp(torch.tensor(max_norm, dtype=F32) / (norm + torch.tensor(1e-6, dtype=F32)), max=1.0)
    if found_inf:
        return True, norm, coef, [g.clone() for g in grads]
    return False, norm, coef, [t * coef for t in u]


def mixed_magnitudes(n: int = 200_000, seed: int = 0) -> torch.Tensor:
    """n fp32 values of both signs over 14 decades (1e-9 .. 1e5), a few zeros and subnormals among them."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 14.0 - 9.0)
    v[::977] = 0.0
    v[5::4999] = 1e-41
    return v.to(F32)
