"""Reference side of the sampling-evaluation tests: seeded inputs and the restatement of the reference's `log_sample_res`
(VLA/train/sample.py:55-98) in plain torch at any dtype.  With dtype=torch.float32 it is the reference's own statement (the `.float()` tensors,
the per-sample `.item()` reads added up in Python floats); with torch.float64 it is the yardstick.  tools/make_golden_sample_eval.py runs the
reference itself on `golden_batches` -> tests/golden/g18_sample_eval.npz."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional

import numpy as np
import torch

from tests import cases
from vlatouch import synth

# the runs tests/golden/g18_sample_eval.npz records: name -> (seed, all-zero-mask sample (batch, sample) or None, num_sample_batches)
G18_ID2NAME = {0: "agilex", 1: "rh20t", 2: "bridge", 3: "never_sampled"}
G18_INDICES = ([0, 1, 0], [1, 2, 1])                      # "bridge" occurs in the second batch only, "never_sampled" in none
G18_B, G18_H, G18_A = 3, 8, 128
G18_RUNS = OrderedDict((("main", (181, None, 2)), ("nanmask", (182, (1, 0), 2)), ("short", (181, None, 3))))    # "short": the iterable ends early
METRIC_KEYS = ("_sample_mse", "_sample_l2err")


def metric_inputs(B: int, H: int, A: int, seed: int, zero_mask_sample: Optional[int] = None, n_datasets: int = 3) -> Dict[str, torch.Tensor]:
    """pred / target [B, H, A], mask [B, A] (about 10 % ones, never empty unless asked for; sample 0 has a single one when A > 1),
    state_norm [B, A] (a third exact zeros, one of them where the mask is on) and dataset_idx [B], all fp32 / int."""
    g = synth.inputs_rng(seed)
    target = g.uniform(-1, 1, (B, H, A)).astype(np.float32)
    pred = (target + g.standard_normal((B, H, A)) * g.choice([1e-3, 0.05, 0.5], (B, 1, A))).astype(np.float32)
    mask = (g.random((B, A)) < 0.1).astype(np.float32)
    state_norm = g.uniform(0.05, 2.0, (B, A)).astype(np.float32)
    state_norm[g.random((B, A)) < 1 / 3] = 0.0
    if A > 1:
        mask[0] = 0.0
        mask[0, int(g.integers(0, A))] = 1.0
    for b in range(B):
        if mask[b].sum() == 0:
            mask[b, int(g.integers(0, A))] = 1.0
        state_norm[b, int(np.flatnonzero(mask[b])[0])] = 0.0            # the + 1e-3 decides this element's l2
    if zero_mask_sample is not None:
        mask[zero_mask_sample] = 0.0
    idx = g.integers(0, n_datasets, B).astype(np.int32)
    return dict(pred=cases.T(pred), target=cases.T(target), mask=cases.T(mask), state_norm=cases.T(state_norm), dataset_idx=cases.T(idx))


def batch_metrics(pred, target, mask, state_norm, dtype=torch.float64):
    """sample.py:55-65 and :79-86 for one batch -> (per_sample [B, 2], overall [2]) in `dtype`; pred / target are cast first, so with fp64 the
    difference, the square, the root and every sum are fp64."""
    pred, target, mask, state_norm = (t.to(dtype) for t in (pred, target, mask, state_norm))
    B, H, _ = pred.shape
    m = mask.unsqueeze(1).tile((1, H, 1))
    sn = state_norm.unsqueeze(1).tile((1, H, 1))
    loss = (pred - target) ** 2
    msum = m.reshape(B, -1).sum(1)
    mse = (loss * m).reshape(B, -1).sum(1) / msum
    l2e = loss.sqrt() / (sn + 1e-3)
    l2 = (l2e * m).reshape(B, -1).sum(1) / msum
    overall = torch.stack([(loss * m).sum() / m.sum(), (l2e * m).sum() / m.sum()])
    return torch.stack([mse, l2], dim=1), overall


def running_sums(batches: List[Dict[str, torch.Tensor]], n_datasets: int, dtype=torch.float64):
    """acc [n_datasets + 1][2] (Python-float sums, as the reference adds `.item()` values) and count [n_datasets + 1] after every batch of
    `batches` (metric_inputs dicts): row dataset_idx[b] gets sample b's pair, in index order, row n_datasets the overall pair."""
    acc, count, out = np.zeros((n_datasets + 1, 2)), np.zeros(n_datasets + 1, dtype=np.int64), []
    for b in batches:
        per, overall = batch_metrics(b["pred"], b["target"], b["mask"], b["state_norm"], dtype)
        for s, d in enumerate(b["dataset_idx"].tolist()):
            acc[d] += [per[s, 0].item(), per[s, 1].item()]
            count[d] += 1
        acc[n_datasets] += [overall[0].item(), overall[1].item()]
        count[n_datasets] += 1
        out.append((acc.copy(), count.copy()))
    return out


def log_sample_res_restated(batches, preds, dataset_id2name, num_sample_batches: int, dtype=torch.float64, ndigits: Optional[int] = None) -> dict:
    """sample.py:18-98 on collator batches and the predictions `predict_action` gave for them; ndigits=4 rounds like the reference."""
    loss_for_log, counter = OrderedDict(), {}
    for step, (batch, pred) in enumerate(zip(batches, preds)):
        if step >= num_sample_batches:
            break
        per, overall = batch_metrics(pred, batch["actions"], batch["state_elem_mask"], batch["state_norm"], dtype)
        for col, suffix in enumerate(METRIC_KEYS):
            for s, d in enumerate(batch["data_indices"]):
                name = dataset_id2name[d] + suffix
                loss_for_log[name] = loss_for_log.get(name, 0.0) + per[s, col].item()
                counter[name] = counter.get(name, 0) + 1
        for col, name in enumerate(("overall_avg_sample_mse", "overall_avg_sample_l2err")):
            loss_for_log[name] = loss_for_log.get(name, 0.0) + overall[col].item()
    out = {}
    for name, v in loss_for_log.items():
        v = v / (num_sample_batches if name.startswith("overall_avg_") else counter[name])
        out[name] = v if ndigits is None else round(v, ndigits)
    return out


def collator_batch(cfg: dict, B: int, lang_len: int, seed: int, data_indices, zero_mask_sample: Optional[int] = None, images: bool = False):
    """One batch in the reference collator's layout for a model of `cfg`: metric_inputs' target / mask / state_norm as actions /
    state_elem_mask / state_norm, cases.rdt_inputs' tokens, two past states (the last one is the state token), and `pred`, a prescribed
    prediction for stand-in samplers.  images=True: `images` [B, 2, 3, 4, 4] instead of `img_tokens` (a stub encoder turns them into tokens)."""
    m = metric_inputs(B, cfg["horizon"], cfg["action_dim"], seed, zero_mask_sample)
    d = cases.rdt_inputs(cfg, B, lang_len, seed=seed)
    g = synth.inputs_rng(2000 + seed)
    out = dict(data_indices=list(data_indices), ctrl_freqs=torch.tensor([10.0, 25.0, 30.0, 15.0][:B]), state_norm=m["state_norm"],
               states=torch.cat([cases.T(g.standard_normal((B, 1, cfg["state_token_dim"]), dtype=np.float32)), d["state_tokens"]], dim=1),
               actions=m["target"], state_elem_mask=m["mask"], lang_attn_mask=d["lang_mask"], lang_embeds=d["lang_tokens"], x_init=d["x_init"],
               pred=m["pred"])
    if images:
        out["images"] = cases.T(g.uniform(0, 1, (B, 2, 3, 4, 4)).astype(np.float32))
    else:
        out["img_tokens"] = d["img_tokens"]
    return out


def golden_batches(run: str):
    """The batches of one g18 run: two of 3 samples, (H, A) = (8, 128), RDT_TINY's token shapes, `images` as the reference wants them."""
    seed, zero, _ = G18_RUNS[run]
    return [collator_batch(cases.RDT_TINY, G18_B, 12, seed + 10 * j, G18_INDICES[j], zero_mask_sample=zero[1] if zero and zero[0] == j else None,
                           images=True) for j in range(2)]


def same_nan_places(a: dict, b: dict) -> bool:
    return set(a) == set(b) and all(np.isnan(a[k]) == np.isnan(b[k]) for k in a)
