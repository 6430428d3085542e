#!/usr/bin/env python
"""Golden vectors for RDT fine-tuning WITH GRADIENT ACCUMULATION, captured from the reference's own parts driven the way its loop drives them
(VLA/train/train.py:405-448) under a real `accelerate.Accelerator(gradient_accumulation_steps=4, cpu=True)`: the reference's
`RDTRunner.compute_loss`, `accelerator.backward`, `accelerator.clip_grad_norm_` on sync steps, `torch.optim.AdamW`, a scheduler prepared by the
accelerator and built with `lr_warmup_steps * k` warm-up steps (train.py:299-303), and the reference's `EMAModel.step` after every micro-batch,
outside `accelerator.accumulate`.  `RDT_TINY`, 12 micro-batches of batch 3 (3 optimizer steps), fp32, `sample` prediction, both RmsNorm forms
with the `constant` scheduler plus one `constant_with_warmup` run.

As in tools/make_golden_rdt_train.py the random draws of compute_loss are pinned to tests/rdt_train_ref.batch and `DDPMScheduler.add_noise` is
the closed-form stand-in (diffusers is absent, hence UNPINNED in `add_noise`); for the same reason the scheduler is a `LambdaLR` over the two
published diffusers multipliers (field `lr_lambda`).  The reference trains under DeepSpeed ZeRO-2, which is not installed: plain accelerate
states the same arithmetic.  Stored per run `<rms>_<scheduler>_`: `scalars` [12, 4] = loss, EMA decay, logged lr (train.py:477),
sync_gradients per micro-batch; `norms` [3] = gradient norm before clipping per optimizer step; `s<j>_grad / _update / _ema` per optimizer step
and parameter tensor (norm, projection on a seeded direction, first 4 values) of the accumulated gradient, of p - p_0 and of ema - p_0; and
`m<i>_ema` the same summary of the EMA after every micro-batch -> tests/golden/g17_rdt_accum.npz.
    python tools/make_golden_rdt_accum.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import cases  # noqa: E402
from tests import rdt_train_ref as R  # noqa: E402
from tests import rdt_accum_ref as A  # noqa: E402
import ref_import  # noqa: E402
from make_golden_rdt_train import build, summary  # noqa: E402


def run(rms_mode: str, scheduler: str, out: dict):
    from accelerate import Accelerator
    from models.ema_model import EMAModel                                               # reference
    ref_import.RMS_MODE = rms_mode
    k = A.G17_K
    accelerator = Accelerator(gradient_accumulation_steps=k, cpu=True)
    runner = build("sample")
    names = [n for n, _ in runner.named_parameters()]
    p0 = {n: p.detach().clone() for n, p in runner.named_parameters()}
    ema = EMAModel(copy.deepcopy(runner))
    opt = torch.optim.AdamW(runner.parameters(), **A.G17_HP)
    warm = A.G17_WARMUP * k                                                             # train.py:302
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: A.lr_multiplier(scheduler, s, warm))
    model, opt, sched = accelerator.prepare(runner, opt, sched)
    tag = f"{rms_mode}_{scheduler}"
    orig_randn, orig_randint = torch.randn, torch.randint
    scalars, norms, step = [], [], 0
    for n, seed in enumerate(A.G17_SEEDS):
        b = R.batch(cases.RDT_TINY, A.G17_B, A.G17_LANG_LEN, seed=seed)
        with accelerator.accumulate(model):
            torch.randn = lambda *a, **kw: b["noise"].clone()
            torch.randint = lambda *a, **kw: b["timesteps"].clone()
            try:
                loss = model.compute_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"],
                                          b["ctrl_freqs"])
            finally:
                torch.randn, torch.randint = orig_randn, orig_randint
            accelerator.backward(loss)
            if accelerator.sync_gradients:
                step += 1
                named = list(accelerator.unwrap_model(model).named_parameters())
                out[f"{tag}_s{step}_grad"] = np.stack([summary(kk, p.grad) for kk, p in named])
                norms.append(float(accelerator.clip_grad_norm_(model.parameters(), A.G17_MAX_GRAD_NORM)))
            opt.step()
            sched.step()
            opt.zero_grad(set_to_none=True)
        ema.step(accelerator.unwrap_model(model))
        named = list(accelerator.unwrap_model(model).named_parameters())
        out[f"{tag}_m{n + 1}_ema"] = np.stack([summary(kk, p.detach() - p0[kk]) for kk, p in ema.averaged_model.named_parameters()])
        if accelerator.sync_gradients:
            out[f"{tag}_s{step}_update"] = np.stack([summary(kk, p.detach() - p0[kk]) for kk, p in named])
            out[f"{tag}_s{step}_ema"] = out[f"{tag}_m{n + 1}_ema"]
        scalars.append([float(loss.detach()), ema.decay, sched.get_last_lr()[0], float(accelerator.sync_gradients)])
        print(tag, n + 1, scalars[-1], norms[-1:] if accelerator.sync_gradients else "")
    assert step == len(A.G17_SEEDS) // k
    out[f"{tag}_scalars"], out[f"{tag}_norms"] = np.array(scalars), np.array(norms)
    out["names"] = np.array(names)


def main():
    ref_import.setup()
    import accelerate
    out = {"add_noise": np.array("UNPINNED: closed-form stand-in for diffusers.DDPMScheduler.add_noise over oracle/dpm_solver.make_betas"),
           "lr_lambda": np.array("UNPINNED: LambdaLR over the constant / constant_with_warmup multipliers of diffusers.optimization"),
           "accelerate": np.array(accelerate.__version__), "seeds": np.array(A.G17_SEEDS),
           "hyper": np.array([A.G17_HP["lr"], A.G17_HP["weight_decay"], A.G17_MAX_GRAD_NORM, A.G17_K, A.G17_WARMUP])}
    for rms_mode, scheduler in A.G17_RUNS:
        run(rms_mode, scheduler, out)
    path = os.path.join(cases.GOLDEN, "g17_rdt_accum.npz")
    np.savez_compressed(path, **out)
    print("wrote g17_rdt_accum", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
