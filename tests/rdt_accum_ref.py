"""Reference side of the gradient-accumulation tests: the reference's loop (VLA/train/train.py:405-448) under
`accelerate.Accelerator(gradient_accumulation_steps=k)`, restated in plain torch at any dtype on top of tests/rdt_train_ref.py.  What accelerate
does there: `accelerator.backward` divides each micro-batch loss by k, so after k micro-batches the gradient is (1/k) sum of theirs; clipping,
`optimizer.step`, the scheduler and `zero_grad` act on the k-th micro-batch only; `EMAModel.step` runs after every micro-batch; the scheduler
is built with `lr_warmup_steps * k` warm-up steps and advances once per optimizer step.  accelerate itself is not imported."""
from __future__ import annotations

from collections import OrderedDict

import torch

from tests import rdt_train_ref as R

# the run tests/golden/g17_rdt_accum.npz records (tools/make_golden_rdt_accum.py imports these)
G17_K, G17_B, G17_LANG_LEN = 4, 3, 12
G17_SEEDS = tuple(6 + 10 * i for i in range(12))                 # 12 micro-batches = 3 optimizer steps; the first three are g16's
G17_HP = R.G16_HP
G17_MAX_GRAD_NORM = R.G16_MAX_GRAD_NORM
G17_WARMUP = 1                                                    # lr_warmup_steps of the constant_with_warmup run: k scheduler steps of ramp
# How far the two "fp64" statements of an accumulated gradient, (1/k) sum of the micro-batch gradients and the gradient of the concatenated batch,
# may be apart per tensor, relative to its norm.  They are equal in exact arithmetic, but not to fp64 rounding: oracle.rdt._sdpa casts q, k and v
# to fp32 and forms both attention products there whatever the dtype of the run, so each statement carries roundings of 2^-24 = 6e-8 per
# attention output, and the batched products of 2 B and of 2 k B samples are blocked differently, so the roundings differ between the two.  A
# gradient passes at most 2 products x 2 attentions x 4 blocks = 16 of them in the deepest test model: 16 x 2^-24 = 9.5e-7, taken as 1e-6,
# which is also 1 % of the 1e-4 bar the device gradients are held to against either statement.
REFS_AGREE = 1e-6
G17_RUNS = (("meansq", "constant"), ("var", "constant"), ("meansq", "constant_with_warmup"))


def lr_multiplier(scheduler: str, steps_done: int, warmup: int) -> float:
    """diffusers.optimization's `constant` / `constant_with_warmup` lambdas after `steps_done` scheduler steps; `warmup` already holds the factor k."""
    if scheduler == "constant":
        return 1.0
    if scheduler == "constant_with_warmup":
        return float(steps_done) / float(max(1.0, warmup)) if steps_done < warmup else 1.0
    raise ValueError(scheduler)


def accumulated_grads(sd, batches, cfg, dtype=torch.float64, **kw):
    """(1/k) sum of the micro-batch gradients at fixed weights -> ([losses], {key: fp64})."""
    k = len(batches)
    total, losses = None, []
    for b in batches:
        loss, g = R.loss_and_grads(sd, b, cfg, dtype=dtype, **kw)
        losses.append(loss)
        total = g if total is None else OrderedDict((n, total[n] + g[n]) for n in g)
    return losses, OrderedDict((n, v / k) for n, v in total.items())


def concat_batch(batches):
    """The micro-batches as one batch of sum(B) samples: with equal-size micro-batches its mean loss is the mean of theirs."""
    return {key: torch.cat([b[key] for b in batches], dim=0) for key in batches[0]}


def accum_train_steps(sd, batches, cfg, k, *, dtype=torch.float64, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0,
                      lr_scheduler="constant", lr_warmup_steps=500, **kw):
    """The accumulated loop, one entry per micro-batch: dict(loss, ema_decay, lr (the scheduler's last lr after this micro-batch, what train.py:477
    logs), sync, ema {k: fp64}) and on sync micro-batches also grad_norm, grad {k: fp64, the accumulated gradient before clipping}, lr_used,
    params {k: fp64}."""
    leaves = R.leaf_sd(sd, dtype)
    ema = OrderedDict((n, v.detach().clone()) for n, v in leaves.items())
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    warm = lr_warmup_steps * k
    sched_steps = 0
    for grp in opt.param_groups:
        grp["lr"] = lr * lr_multiplier(lr_scheduler, 0, warm)
    out = []
    for n, b in enumerate(batches):
        with torch.enable_grad():
            loss = R.loss_fn(leaves, b, cfg, dtype=dtype, **kw)
            (loss / k).backward()                                    # accelerator.backward; .grad accumulates until zero_grad
        rec = dict(loss=float(loss.detach()), sync=(n + 1) % k == 0)
        if rec["sync"]:
            rec["grad"] = OrderedDict((key, v.grad.detach().double().clone()) for key, v in leaves.items())
            rec["grad_norm"] = float(torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_grad_norm))
            rec["lr_used"] = opt.param_groups[0]["lr"]
            opt.step()
            sched_steps += 1
            for grp in opt.param_groups:
                grp["lr"] = lr * lr_multiplier(lr_scheduler, sched_steps, warm)
            opt.zero_grad(set_to_none=True)
            rec["params"] = OrderedDict((key, v.detach().double().clone()) for key, v in leaves.items())
        rec["lr"] = opt.param_groups[0]["lr"]
        dec = R.ema_decay(n)                                         # EMAModel.step: get_decay at the count before this update
        with torch.no_grad():
            for key, v in leaves.items():
                ema[key].mul_(dec).add_(v.detach(), alpha=1 - dec)
        rec["ema_decay"] = dec
        rec["ema"] = OrderedDict((key, v.double().clone()) for key, v in ema.items())
        out.append(rec)
    return out
