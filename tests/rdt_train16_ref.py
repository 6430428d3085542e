"""Reference side of the fp16 fine-tuning tests: tests/rdt_train_ref.py's oracle run in IEEE half on the CPU under a static loss scale, as
torch.amp.GradScaler arranges it (the loss times S before `backward`, the gradients divided by S afterwards), and the fp64 / oracle
gradients of the two model sizes computed once per process and shared."""
import json
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import rdt as orr
from tests import cases
from tests import rdt_train_ref as R

H16 = torch.float16


def round_fp16(d):
    """Floating tensors of a dict rounded to the fp16 grid (kept in fp32): what an fp16 run and its fp64 yardstick both start from."""
    return type(d)((k, v.half().float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items())


def loss_fn16(sd, b, cfg, *, rms_mode="meansq", prediction_type="sample"):
    """R.loss_fn in fp16 with the MSE taken in fp32 (`F.mse_loss(pred.float(), target.float())`, what R.loss_fn does for bf16 and what
    autocast does for mse_loss), so that the scaled d loss / d pred is formed in fp32 and rounded once to fp16."""
    c = lambda k: b[k].to(H16)
    ab = R.alphas_cumprod()[b["timesteps"]]
    sa_, sb_ = (ab ** 0.5).to(H16)[:, None, None], ((1 - ab) ** 0.5).to(H16)[:, None, None]
    noisy = sa_ * c("action_gt") + sb_ * c("noise")
    traj = torch.cat([c("state_tokens"), noisy], dim=1)
    traj = torch.cat([traj, c("action_mask").expand(-1, traj.shape[1], -1)], dim=2)
    lang_c, img_c = orr.adaptor(sd, "lang_adaptor", c("lang_tokens")), orr.adaptor(sd, "img_adaptor", c("img_tokens"))
    traj = orr.adaptor(sd, "state_adaptor", traj)
    pred = orr.rdt_forward(sd, traj, b["ctrl_freqs"], b["timesteps"], lang_c, img_c, lang_mask=b["lang_attn_mask"], heads=cfg["heads"],
                           horizon=cfg["horizon"], rms_mode=rms_mode)
    target = c("noise") if prediction_type == "epsilon" else c("action_gt")
    return F.mse_loss(pred.float(), target.float())


def oracle_fp16(sd, b, cfg, scale: float, **kw):
    """-> (unscaled loss, {key: gradient / scale in fp64}) of the oracle in fp16 under the static loss scale `scale`."""
    leaves = R.leaf_sd(sd, H16)
    with torch.enable_grad():
        loss = loss_fn16(leaves, b, cfg, **kw)
        (loss * scale).backward()
    return float(loss.detach()), OrderedDict((k, (torch.zeros_like(v) if v.grad is None else v.grad).double() / scale) for k, v in leaves.items())


SIZES = {"tiny": (cases.RDT_TINY, 3, 12), "wide": (cases.RDT_WIDE, 2, 20)}
_CACHE = {}


def problem(name: str):
    """(cfg, fp16-rounded weights, fp16-rounded batch, fp64 loss, fp64 gradients) of a model size; shared, never modified."""
    key = ("p16", name)
    if key not in _CACHE:
        cfg, B, Ll = SIZES[name]
        sd, b = round_fp16(cases.rdt_sd(cfg)), round_fp16(R.batch(cfg, B, Ll))
        _CACHE[key] = (cfg, sd, b) + R.loss_and_grads(sd, b, cfg)
    return _CACHE[key]


def oracle(name: str, scale: float):
    key = ("o16", name, scale)
    if key not in _CACHE:
        cfg, sd, b, _, _ = problem(name)
        _CACHE[key] = oracle_fp16(sd, b, cfg, scale)
    return _CACHE[key]


ORACLE_SCALE, ORACLE_GOLDEN = 1024.0, "g21_fp16_oracle_errors.json"


def oracle_errors_fresh(name: str) -> dict:
    """The fp16 oracle under ORACLE_SCALE against fp64, computed now: loss, per-tensor || g_ref - g64 ||, the same over all parameters, || g64 ||."""
    _, _, _, _, g64 = problem(name)
    loss, gref = oracle(name, ORACLE_SCALE)
    tot, gall = total_error(gref, g64)
    return {"loss": loss, "tensor_error": {k: float((gref[k] - g64[k]).norm()) for k in g64}, "total_error": tot, "grad_norm": gall}


def oracle_errors(name: str) -> dict:
    """The same as recorded in tests/golden (tools/make_golden_fp16_oracle.py): torch's fp16 matmul on a CPU without native half arithmetic
    takes over a minute for RDT_WIDE, so the GPU test reads what the oracle reached instead of running it."""
    key = ("golden",)
    if key not in _CACHE:
        with open(os.path.join(cases.GOLDEN, ORACLE_GOLDEN)) as f:
            _CACHE[key] = json.load(f)
    assert _CACHE[key]["loss_scale"] == ORACLE_SCALE
    return _CACHE[key][name]


def problem_bf16(name: str):
    """The same weights and batch rounded to bf16 instead, with their own fp64 gradients: what the bf16 trainer is measured against."""
    key = ("pbf", name)
    if key not in _CACHE:
        cfg, B, Ll = SIZES[name]
        sd, b = R.round_bf16(cases.rdt_sd(cfg)), R.round_bf16(R.batch(cfg, B, Ll))
        _CACHE[key] = (cfg, sd, b) + R.loss_and_grads(sd, b, cfg)
    return _CACHE[key]


def total_error(grads, g64):
    """(|| g - g64 || over all parameters, || g64 ||)."""
    e = sum(float((grads[k].double() - g64[k]).norm()) ** 2 for k in g64) ** 0.5
    return e, sum(float(v.norm()) ** 2 for v in g64.values()) ** 0.5
