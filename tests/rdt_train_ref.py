"""Reference side of the RDT fine-tuning tests: torch autograd through the oracle (`oracle.rdt.adaptor` / `oracle.rdt.rdt_forward`) with the
DDPM forward process and the MSE of `RDTRunner.compute_loss` (VLA/models/rdt_runner.py:168-222) in front of / behind it, and the reference's
training step around it (clip_grad_norm_, torch.optim.AdamW, EMAModel: VLA/train/train.py:404-448).  Plain functional torch on the CPU in
any dtype: fp64 is the yardstick, fp32 / bf16 runs of the same code give the error the reference's own arithmetic has."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dpm_solver, rdt as orr
from tests import cases
from vlatouch import synth

TIMESTEPS = (3, 437, 998)
# the run tests/golden/g16_rdt_train.npz records (tools/make_golden_rdt_train.py imports these)
G16_B, G16_LANG_LEN, G16_SEEDS = 3, 12, (6, 16, 26)
G16_HP = dict(lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
G16_MAX_GRAD_NORM = 1.0


def direction(name: str, shape) -> np.ndarray:
    """Seeded direction a tensor is projected on in the golden's summaries."""
    return synth.tensor("proj." + name, tuple(shape), "rdt_train")


def batch(cfg: dict, B: int, lang_len: int, seed: int = 6) -> Dict[str, torch.Tensor]:
    """compute_loss's arguments + the two random draws, seeded (fp32): cases.rdt_inputs plus an action chunk and the noise."""
    d = cases.rdt_inputs(cfg, B, lang_len, seed=seed)
    g = synth.inputs_rng(1000 + seed)
    out = dict(lang_tokens=d["lang_tokens"], lang_attn_mask=d["lang_mask"], img_tokens=d["img_tokens"], state_tokens=d["state_tokens"],
               action_mask=d["action_mask"], ctrl_freqs=torch.tensor([10.0, 25.0, 30.0, 15.0][:B]),
               action_gt=cases.T(g.uniform(-1, 1, (B, cfg["horizon"], cfg["action_dim"])).astype(np.float32)) * d["action_mask"],
               noise=cases.T(g.standard_normal((B, cfg["horizon"], cfg["action_dim"]), dtype=np.float32)),
               timesteps=torch.tensor(TIMESTEPS[:B] if seed == 6 else [int(t) for t in g.integers(0, 1000, B)]))
    return out


def alphas_cumprod(num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2") -> torch.Tensor:
    return torch.cumprod(1.0 - torch.from_numpy(dpm_solver.make_betas(num_train_timesteps, beta_schedule)), dim=0)


def loss_fn(sd, b, cfg, *, rms_mode="meansq", prediction_type="sample", dtype=torch.float64, num_train_timesteps=1000,
            beta_schedule="squaredcos_cap_v2") -> torch.Tensor:
    """RDTRunner.compute_loss over the oracle, in `dtype` (sd already in `dtype`; the inputs are cast here)."""
    c = lambda k: b[k].to(dtype)
    ab = alphas_cumprod(num_train_timesteps, beta_schedule).to(b["timesteps"].device)[b["timesteps"]]            # DDPMScheduler.add_noise: fp32 table, then .to(dtype)
    sa_, sb_ = (ab ** 0.5).to(dtype)[:, None, None], ((1 - ab) ** 0.5).to(dtype)[:, None, None]
    noisy = sa_ * c("action_gt") + sb_ * c("noise")
    traj = torch.cat([c("state_tokens"), noisy], dim=1)
    traj = torch.cat([traj, c("action_mask").expand(-1, traj.shape[1], -1)], dim=2)
    lang_c, img_c = orr.adaptor(sd, "lang_adaptor", c("lang_tokens")), orr.adaptor(sd, "img_adaptor", c("img_tokens"))
    traj = orr.adaptor(sd, "state_adaptor", traj)
    pred = orr.rdt_forward(sd, traj, b["ctrl_freqs"], b["timesteps"], lang_c, img_c, lang_mask=b["lang_attn_mask"], heads=cfg["heads"],
                           horizon=cfg["horizon"], rms_mode=rms_mode)
    if prediction_type == "epsilon":
        target = c("noise")
    elif prediction_type == "sample":
        target = c("action_gt")
    else:
        raise ValueError(f"Unsupported prediction type {prediction_type}")
    if dtype == torch.bfloat16:
        return F.mse_loss(pred.float(), target.float())
    return F.mse_loss(pred, target)


def leaf_sd(sd, dtype):
    return OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())


def loss_and_grads(sd, b, cfg, dtype=torch.float64, **kw):
    """-> (loss as a python float, {key: gradient in fp64}); `sd` is rounded to `dtype` first (the reference holds its weights in it)."""
    leaves = leaf_sd(sd, dtype)
    with torch.enable_grad():                      # other test modules switch autograd off process-wide
        loss = loss_fn(leaves, b, cfg, dtype=dtype, **kw)
        loss.backward()
    return float(loss.detach()), OrderedDict((k, (torch.zeros_like(v) if v.grad is None else v.grad).double()) for k, v in leaves.items())


def ema_decay(step, update_after_step=0, inv_gamma=1.0, power=2 / 3, min_value=0.0, max_value=0.9999):
    """models/ema_model.py:45-55 restated."""
    s = max(0, step - update_after_step - 1)
    if s <= 0:
        return 0.0
    return max(min_value, min(1 - (1 + s / inv_gamma) ** -power, max_value))


def train_steps(sd, batches, cfg, *, dtype=torch.float64, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, **kw):
    """The reference's loop body for each batch: loss.backward(), clip_grad_norm_, AdamW.step, EMAModel.step.
    -> list per step of dict(loss, grad_norm, params {k: fp64}, ema {k: fp64})."""
    leaves = leaf_sd(sd, dtype)
    ema = OrderedDict((k, v.detach().clone()) for k, v in leaves.items())
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    out = []
    for n, b in enumerate(batches):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            loss = loss_fn(leaves, b, cfg, dtype=dtype, **kw)
            loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_grad_norm)
        opt.step()
        dec = ema_decay(n)
        with torch.no_grad():
            for k, v in leaves.items():
                ema[k].mul_(dec).add_(v.detach(), alpha=1 - dec)
        out.append(dict(loss=float(loss.detach()), grad_norm=float(norm), params=OrderedDict((k, v.detach().double().clone()) for k, v in leaves.items()),
                        ema=OrderedDict((k, v.double().clone()) for k, v in ema.items())))
    return out


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """|a - ref| / |ref| over the whole tensor (fp64); a zero reference demands an exactly zero `a`."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    n = float(ref.norm())
    if n == 0.0:
        return 0.0 if float(a.abs().max()) == 0.0 else float("inf")
    return float((a - ref).norm()) / n


def summary(name: str, a: torch.Tensor) -> np.ndarray:
    """The summary form of tests/golden/g16_rdt_train.npz: norm, projection on a seeded direction, first 4 values."""
    v = a.detach().double().cpu().numpy()
    return np.concatenate([[np.sqrt((v * v).sum()), (v * direction(name, v.shape).astype(np.float64)).sum()], v.reshape(-1)[:4]])


def worst_summary(table, names, tensors):
    """Largest |summary - golden row| over the tensors, relative to the golden tensor's norm -> (error, key)."""
    worst, wk = 0.0, None
    for i, k in enumerate(names):
        want = table[i]
        e = float(np.abs(summary(k, tensors[k]) - want).max()) / max(want[0], 1e-30)
        if e > worst:
            worst, wk = e, k
    return worst, wk


def round_bf16(d):
    """Floating tensors of a dict rounded to the bf16 grid (kept in fp32): what a bf16 run and its fp64 yardstick both start from."""
    return type(d)((k, v.bfloat16().float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items())
