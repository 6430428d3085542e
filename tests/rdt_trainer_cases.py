"""What `RdtTrainer` (vlatouch/rdt_train.py) computes on seven small runs, as sha256 digests: one `get_loss`, then a few `train_step`s, through
the trainer's public surface only, so that the same file runs on any version of the trainer.  tests/golden/g23_rdt_trainer_parent.json holds
what the commit BEFORE `get_loss` was cut into stages (one attention sub-block, one block forward / backward) and the three ways of closing an
accumulation window became one gave on an MI355X (tools/make_golden_rdt_trainer_parent.py wrote it); tests/test_gpu_rdt_trainer_parent.py
recomputes them.  That refactor moved host code only, so every bit must be where it was.

Model: cases.RDT_TINY, B = 3, 12 language tokens, the three batches of rdt_train_ref.G16_SEEDS, lr 1e-3.  The cases are the smallest set that
takes every branch of the forward / backward and of the step: both norm modes and prediction types, a fully masked language row, a depth-1
model (no block attends to the image tokens), bf16 under both attention backwards and weight gradients, an accumulation window of two
(accumulate + ema_step), and fp16 from a loss scale of 2^24 with the 8-bit optimizer (skipped steps, back-off, clean steps, growth).

Every tensor gets its own sha256; to keep the recorded file small a group of tensors (the gradients, the parameters, the shadows, the moments
of one run, in the parameters' order) is recorded as the sha256 over its tensors' digests plus, under `<key>/tags`, the first four hex digits
of each, so that a differing group still names its tensors (`differing`)."""
import hashlib
from collections import OrderedDict

import torch

from tests import cases
from tests import rdt_train_ref as R
from tests.train16_cases import digest

GOLDEN_NAME = "g23_rdt_trainer_parent.json"
KEYS = ("lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs")
B, LANG_LEN, LR = 3, 12, 1e-3
FP16_MAX_STEPS = 15                # test_overflow_backoff_recovery's cap on the calls from 2^24 until two clean steps in a row

# name -> (model overrides, trainer keyword arguments, micro-batches (None: until two clean steps in a row), mask sample 1's language)
CASES = OrderedDict([
    ("fp32_meansq_sample", ({}, dict(rms_mode="meansq", prediction_type="sample"), 3, False)),
    ("fp32_var_epsilon", ({}, dict(rms_mode="var", prediction_type="epsilon"), 3, False)),
    ("fp32_masked_row", ({}, {}, 3, True)),
    ("fp32_depth1", (dict(depth=1), {}, 3, False)),
    ("bf16_wave_gemm", ({}, dict(precision="bf16", attention_backward="wave", weight_gradient="gemm"), 3, False)),
    ("bf16_mfma_tn_k2", ({}, dict(precision="bf16", attention_backward="mfma", weight_gradient="tn", gradient_accumulation_steps=2), 6, False)),
    ("fp16_mfma_tn_adam8", ({}, dict(precision="fp16", attention_backward="mfma", weight_gradient="tn", optimizer="adamw8bit",
                                     loss_scale=dict(init_scale=2.0 ** 24, growth_interval=2)), None, False)),
])


def _batches(cfg, masked):
    out = []
    for seed in R.G16_SEEDS:
        b = R.batch(cfg, B, LANG_LEN, seed=seed)
        if masked:
            b["lang_attn_mask"] = b["lang_attn_mask"].clone()
            b["lang_attn_mask"][1] = False
        out.append(b)
    return out


def _trainer(cfg, sd, dev, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], lr=LR, device=dev, **kw)


def _args(b):
    return [b[k] for k in KEYS], dict(noise=b["noise"], timesteps=b["timesteps"])


def _put(out, key, tensors) -> None:
    ds = [digest(t) for t in tensors]
    out[key], out[key + "/tags"] = hashlib.sha256("".join(ds).encode()).hexdigest(), "".join(d[:4] for d in ds)


def _case(out, name, dev) -> None:
    over, kw, micro, masked = CASES[name]
    cfg = dict(cases.RDT_TINY, **over)
    sd, batches = cases.rdt_sd(cfg), _batches(cfg, masked)

    # one get_loss (an accumulating trainer shows its gradients only folded, so this one is built without the window)
    tr = _trainer(cfg, sd, dev, **{k: v for k, v in kw.items() if k != "gradient_accumulation_steps"})
    a, k = _args(batches[0])
    out[f"{name}/get_loss/loss"] = digest(tr.get_loss(*a, **k).reshape(1))
    _put(out, f"{name}/get_loss/grads", tr.grads().values())

    # the steps
    tr = _trainer(cfg, sd, dev, **kw)
    j = clean = 0
    while (j < micro) if micro is not None else (clean < 2 and j < FP16_MAX_STEPS):
        a, k = _args(batches[j % len(batches)])
        out[f"{name}/step{j}/loss"] = digest(tr.train_step(*a, **k).reshape(1))
        out[f"{name}/step{j}/state"] = repr((tr.step_count, tr.ema_updates, tr.global_step, tr.micro_step, bool(tr.sync_gradients), float(tr.lr)))
        if micro is None:
            out[f"{name}/step{j}/scaler"] = repr((float(tr.loss_scale_value), tr.growth_tracker, tr.skipped_steps, tr.skipped_nonfinite_loss,
                                                  bool(tr.last_step_skipped)))
            clean = 0 if tr.last_step_skipped else clean + 1
        j += 1
    out[f"{name}/steps"] = repr(j)
    out[f"{name}/grad_norm"] = digest(tr.grad_norm.reshape(1))
    p, ema = tr.state_dict(), tr.ema_state_dict()
    _put(out, f"{name}/params", p.values())
    _put(out, f"{name}/ema", ema.values())
    _put(out, f"{name}/moments", (torch.stack([t.float() for t in tr.moments(key)]) for key in p))


def trainer_cases(dev) -> "OrderedDict[str, str]":
    out = OrderedDict()
    for name in CASES:
        _case(out, name, dev)
    return out


def differing(want, got) -> list:
    """The keys at which `got` differs from `want`; a `/tags` key is followed by the names of the tensors whose tags differ."""
    out = []
    for k in want:
        if got[k] != want[k]:
            out.append(k)
            if k.endswith("/tags"):
                names = list(cases.rdt_sd(dict(cases.RDT_TINY, **CASES[k.split("/")[0]][0])))
                out += [n for i, n in enumerate(names) if got[k][4 * i:4 * i + 4] != want[k][4 * i:4 * i + 4]]
    return out
