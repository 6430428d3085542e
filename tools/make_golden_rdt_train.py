#!/usr/bin/env python
"""Golden vectors for the RDT FINE-TUNING step, captured from the REFERENCE ITSELF with torch autograd on the CPU: the reference's own
`RDTRunner.compute_loss` (VLA/models/rdt_runner.py:168-222) on its own `RDT` / adaptors, `loss.backward()`, `clip_grad_norm_(1.0)`,
`torch.optim.AdamW` and the reference's `EMAModel` (VLA/models/ema_model.py), three consecutive steps (train/train.py:404-448) on the
`RDT_TINY` weights of tests/cases.py, batch 3, language length 12 with padded tokens, fp32, for both RmsNorm forms and both prediction types.

The reference draws `torch.randn` / `torch.randint` inside compute_loss; both are pinned here to the seeded tensors of
tests/rdt_train_ref.batch, which the tests regenerate.  diffusers is absent: `DDPMScheduler.add_noise` is a stand-in with the published
closed form over oracle/dpm_solver.make_betas (hence UNPINNED in the field `add_noise`, like g9); timm is the shim of tools/ref_import.py.
Stored per run `<rms>_<ptype>_s<k>_*`: loss, gradient norm before clipping, EMA decay, and per parameter tensor (norm, projection on a seeded
direction, first 4 values) of the gradient, of the update p_k - p_0 and of ema_k - p_0 -> tests/golden/g16_rdt_train.npz.
    python tools/make_golden_rdt_train.py
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
import ref_import  # noqa: E402
from oracle import dpm_solver  # noqa: E402

B, LANG_LEN, SEEDS, HP, MAX_GRAD_NORM, direction = R.G16_B, R.G16_LANG_LEN, R.G16_SEEDS, R.G16_HP, R.G16_MAX_GRAD_NORM, R.direction


def summary(name: str, a: torch.Tensor) -> np.ndarray:
    v = a.detach().double().numpy()
    return np.concatenate([[np.sqrt((v * v).sum()), (v * direction(name, v.shape).astype(np.float64)).sum()], v.reshape(-1)[:4]])


class _DDPM:
    """Stand-in for diffusers.DDPMScheduler as compute_loss uses it: add_noise's closed form (Ho et al. 2020, eq. 4)."""

    def __init__(self, num_train_timesteps, beta_schedule, prediction_type, clip_sample):
        self.alphas_cumprod = torch.cumprod(1.0 - torch.from_numpy(dpm_solver.make_betas(num_train_timesteps, beta_schedule)), dim=0)

    def add_noise(self, original, noise, timesteps):
        ac = self.alphas_cumprod.to(dtype=original.dtype)
        a = (ac[timesteps] ** 0.5).flatten()
        s = ((1 - ac[timesteps]) ** 0.5).flatten()
        while a.dim() < original.dim():
            a, s = a.unsqueeze(-1), s.unsqueeze(-1)
        return a * original + s * noise


def build(prediction_type: str):
    import models.rdt_runner as rr                                                      # reference
    rr.DDPMScheduler, rr.DPMSolverMultistepScheduler = _DDPM, (lambda **k: None)
    cfg = cases.RDT_TINY
    config = {"rdt": {"hidden_size": cfg["hidden"], "depth": cfg["depth"], "num_heads": cfg["heads"]}, "lang_adaptor": "mlp2x_gelu",
              "img_adaptor": "mlp2x_gelu", "state_adaptor": "mlp3x_gelu",
              "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "prediction_type": prediction_type,
                                  "beta_schedule": "squaredcos_cap_v2", "clip_sample": False}}
    runner = rr.RDTRunner(action_dim=cfg["action_dim"], pred_horizon=cfg["horizon"], config=config, lang_token_dim=cfg["lang_token_dim"],
                          img_token_dim=cfg["img_token_dim"], state_token_dim=cfg["state_token_dim"], max_lang_cond_len=cfg["max_lang_cond_len"],
                          img_cond_len=cfg["img_cond_len"], lang_pos_embed_config=None, img_pos_embed_config=None, dtype=torch.float32)
    runner.float()                                                                      # the constructor casts the adaptors to bf16
    missing, unexpected = runner.load_state_dict(cases.rdt_sd(cfg), strict=True)
    assert not missing and not unexpected
    for p in runner.parameters():
        p.requires_grad_(True)                                                          # the position embeddings train too (train.py optimises rdt.parameters())
    return runner


def run(rms_mode: str, prediction_type: str, out: dict):
    from models.ema_model import EMAModel                                               # reference
    ref_import.RMS_MODE = rms_mode
    runner = build(prediction_type)
    names = [k for k, _ in runner.named_parameters()]
    p0 = {k: p.detach().clone() for k, p in runner.named_parameters()}
    ema = EMAModel(copy.deepcopy(runner))
    opt = torch.optim.AdamW(runner.parameters(), **HP)
    tag = f"{rms_mode}_{prediction_type}"
    orig_randn, orig_randint = torch.randn, torch.randint
    for n, seed in enumerate(SEEDS):
        b = R.batch(cases.RDT_TINY, B, LANG_LEN, seed=seed)
        torch.randn = lambda *a, **k: b["noise"].clone()
        torch.randint = lambda *a, **k: b["timesteps"].clone()
        try:
            opt.zero_grad()
            loss = runner.compute_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"],
                                       b["ctrl_freqs"])
            loss.backward()
        finally:
            torch.randn, torch.randint = orig_randn, orig_randint
        named = list(runner.named_parameters())
        assert all(p.grad is not None for _, p in named)
        out[f"{tag}_s{n + 1}_grad"] = np.stack([summary(k, p.grad) for k, p in named])
        norm = torch.nn.utils.clip_grad_norm_(runner.parameters(), MAX_GRAD_NORM)
        opt.step()
        ema.step(runner)
        out[f"{tag}_s{n + 1}_scalars"] = np.array([float(loss.detach()), float(norm), ema.decay])
        out[f"{tag}_s{n + 1}_update"] = np.stack([summary(k, p.detach() - p0[k]) for k, p in named])
        out[f"{tag}_s{n + 1}_ema"] = np.stack([summary(k, p.detach() - p0[k]) for k, p in ema.averaged_model.named_parameters()])
        print(tag, n + 1, out[f"{tag}_s{n + 1}_scalars"])
    out["names"] = np.array(names)


def main():
    ref_import.setup()
    out = {"add_noise": np.array("UNPINNED: closed-form stand-in for diffusers.DDPMScheduler.add_noise over oracle/dpm_solver.make_betas"),
           "seeds": np.array(SEEDS), "hyper": np.array([HP["lr"], HP["weight_decay"], MAX_GRAD_NORM])}
    for rms_mode in ("meansq", "var"):
        for ptype in ("sample", "epsilon"):
            run(rms_mode, ptype, out)
    path = os.path.join(cases.GOLDEN, "g16_rdt_train.npz")
    np.savez_compressed(path, **out)
    print("wrote g16_rdt_train", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
