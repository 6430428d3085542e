#!/usr/bin/env python
"""Golden results of fine-tuning's periodic sampling evaluation, captured from the reference's own `log_sample_res` (VLA/train/sample.py:7-98)
run on the CPU under a real `accelerate.Accelerator(cpu=True)` (its gather_for_metrics / gather / is_main_process are the reference's calls).

The function is driven with stand-in objects: an `rdt` whose `predict_action` returns the prescribed predictions of
tests/sample_eval_ref.golden_batches in turn, a `vision_encoder` with `hidden_size` that returns zeros, an `args` namespace.  So the golden
pins the metric and aggregation semantics (masked MSE, state-norm-relative L2, per-dataset means, the `num_sample_batches` divisor, the
4-decimal rounding, where NaN lands) independently of the sampler, which stays UNPINNED as in the other RDT goldens.  weight_dtype is fp32.
Runs (tests/sample_eval_ref.G18_RUNS): `main`, two batches of 3 with (H, A) = (8, 128), three dataset names of which one occurs in one batch
only, sparse masks, exact zeros in state_norm, one sample with a single unmasked element; `nanmask`, the same shapes with one all-zero-mask
sample; `short`, `main` with num_sample_batches = 3 while the loader ends after 2.  Stored per run `<run>_keys` (the returned dict's keys in
order) and `<run>_values` -> tests/golden/g18_sample_eval.npz.
    python tools/make_golden_sample_eval.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import cases  # noqa: E402
from tests import sample_eval_ref as S  # noqa: E402
import ref_import  # noqa: E402


class _Rdt:
    def __init__(self, preds):
        self.preds, self.calls, self.mode = list(preds), 0, []

    def eval(self):
        self.mode.append("eval")

    def train(self):
        self.mode.append("train")

    def predict_action(self, *, lang_tokens, lang_attn_mask, img_tokens, state_tokens, action_mask, ctrl_freqs):
        B = lang_tokens.shape[0]
        assert state_tokens.shape[1] == 1 and action_mask.shape == (B, 1, S.G18_A) and img_tokens.shape == (B, 2 * 5, 7)
        self.calls += 1
        return self.preds[self.calls - 1].clone()


class _Vision:
    hidden_size = 7

    def __call__(self, images):
        return torch.zeros(images.shape[0], 5, self.hidden_size)


class _Logger:
    def info(self, *a, **k):
        pass


def main():
    assert "train" not in sys.modules, "the product's train package must not be imported before the reference's"
    ref_import.setup()
    import accelerate
    from accelerate import Accelerator
    from train.sample import log_sample_res                                         # reference (the product directory is off sys.path now)
    assert os.path.realpath(sys.modules["train.sample"].__file__).startswith(os.path.realpath(ref_import.REF)), sys.modules["train.sample"].__file__
    accelerator = Accelerator(cpu=True)
    out = {"accelerate": np.array(accelerate.__version__), "sampler": np.array("UNPINNED: predict_action is a stand-in that returns prescribed tensors")}
    for run, (_, _, nsb) in S.G18_RUNS.items():
        batches = S.golden_batches(run)
        rdt = _Rdt([b["pred"] for b in batches])
        args = types.SimpleNamespace(num_sample_batches=nsb, precomp_lang_embed=True)
        loader = [{k: v for k, v in b.items() if k not in ("pred", "x_init", "img_tokens")} for b in batches]
        res = log_sample_res(None, _Vision(), rdt, args, accelerator, torch.float32, S.G18_ID2NAME, loader, _Logger())
        assert rdt.calls == len(batches) and rdt.mode == ["eval", "train"]
        out[f"{run}_keys"], out[f"{run}_values"] = np.array(list(res)), np.array([res[k] for k in res], dtype=np.float64)
        print(run, res)
    path = os.path.join(cases.GOLDEN, "g18_sample_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote g18_sample_eval", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
