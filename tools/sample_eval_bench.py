#!/usr/bin/env python
"""Cost of fine-tuning's periodic sampling evaluation (vlatouch.rdt_train.sample_eval) at RDT-1B dimensions (bench.py's RDT config: hidden 2048,
depth 28, 32 heads, horizon 64, 4 374 image tokens, 32 language tokens, synthetic weights, a bf16 runner) with the reference recipe's
sample_batch_size 4, 2 batches and the runner's 5 inference steps -> profiles/sample_eval_bench.json.  Device-synchronised wall times of
  * the weight hand-over: `trainer.sampler()` after the weights changed (device-to-device copies + repack; also the first call, which builds
    the engine) against `trainer.sync_to(runner)` + `runner.engine()` in the same process (every weight through host memory, a new engine);
  * the metrics of one batch: one vt_sample_metrics call against the reference's torch statement on the device with its `.item()` loop;
  * a whole evaluation visit (hand-over + 2 x predict_action + metrics + the one read), in ms and as a share of 1000 training steps at the
    241 ms per step of DESIGN.md section 8.
    python tools/sample_eval_bench.py [--depth 28] [--repeats 5] [--out profiles/sample_eval_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vlatouch import synth  # noqa: E402

TRAIN_STEP_MS = 241.0            # the bf16 step at batch 4


def _stats(ms):
    t = sorted(ms)
    n = len(t)
    return {"median": t[n // 2] if n % 2 else 0.5 * (t[n // 2 - 1] + t[n // 2]), "min": t[0], "max": t[-1], "n": n}


def build_runner(a, dev, sd=None):
    from models.rdt_runner import RDTRunner
    cfg = {"rdt": {"hidden_size": a.hidden, "depth": a.depth, "num_heads": a.hidden // 64, "rms_norm": "meansq"}, "lang_adaptor": "mlp2x_gelu",
           "img_adaptor": "mlp2x_gelu", "state_adaptor": "mlp3x_gelu",
           "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "beta_schedule": "squaredcos_cap_v2", "prediction_type": "sample"}}
    r = RDTRunner(action_dim=128, pred_horizon=64, config=cfg, lang_token_dim=4096, img_token_dim=1152, state_token_dim=128, max_lang_cond_len=1024,
                  img_cond_len=a.img_len, dtype=torch.bfloat16, device=dev, init_weights=False)
    if sd is not None:
        r.load_state_dict(sd, assign=True)
    return r


def torch_statement(pred, actions, mask, state_norm, data_indices, names, loss_for_log, counter):
    """sample.py:55-86 as the reference writes it, on the device."""
    B, H = pred.shape[:2]
    m = mask.unsqueeze(1).tile((1, H, 1)).float()
    sn = state_norm.unsqueeze(1).tile((1, H, 1)).float()
    loss = torch.nn.functional.mse_loss(pred, actions.to(pred.dtype), reduction="none").float()
    mse = (loss * m).reshape(B, -1).sum(1) / m.reshape(B, -1).sum(1)
    l2 = loss.sqrt() / (sn + 1e-3)
    l2 = (l2 * m).reshape(B, -1).sum(1) / m.reshape(B, -1).sum(1)
    for suffix, losses in zip(("_sample_mse", "_sample_l2err"), (mse, l2)):
        for d, t in zip(data_indices, losses):
            loss_for_log[names[d] + suffix] = loss_for_log.get(names[d] + suffix, 0.0) + t.item()
            counter[names[d] + suffix] = counter.get(names[d] + suffix, 0) + 1
    loss_for_log["overall_avg_sample_mse"] = loss_for_log.get("overall_avg_sample_mse", 0.0) + ((loss * m).sum() / m.sum()).item()
    l2o = loss.sqrt() / (sn + 1e-3)
    loss_for_log["overall_avg_sample_l2err"] = loss_for_log.get("overall_avg_sample_l2err", 0.0) + ((l2o * m).sum() / m.sum()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--img-len", type=int, default=4374)
    ap.add_argument("--lang-len", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--num-sample-batches", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_eval_bench.json"))
    a = ap.parse_args()
    from vlatouch import _lib as L
    from vlatouch.rdt_train import sample_eval
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    c = dict(hidden=a.hidden, depth=a.depth, heads=a.hidden // 64, horizon=64, action_dim=128, lang_token_dim=4096, img_token_dim=1152,
             state_token_dim=128, max_lang_cond_len=1024, img_cond_len=a.img_len)
    sd = synth.fill_state_dict_device(synth.rdt_runner_shapes(**c), dev, torch.float32, seed=7)
    params = sum(v.numel() for v in sd.values())
    tr = build_runner(a, dev, sd).trainer(precision="bf16", lr=1e-4)
    del sd
    B, names = a.batch, {0: "agilex", 1: "rh20t", 2: "bridge"}
    g = torch.Generator(device=dev).manual_seed(99)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    batches = []
    for j in range(a.num_sample_batches):
        mask = torch.zeros(B, 128, device=dev)
        mask[:, :10] = 1.0
        batches.append(dict(data_indices=[(j + s) % 3 for s in range(B)], ctrl_freqs=torch.full((B,), 25.0, device=dev), state_norm=rn(B, 128).abs() * mask,
                            states=rn(B, 1, 128), actions=torch.tanh(rn(B, 64, 128)) * mask.unsqueeze(1), state_elem_mask=mask,
                            lang_attn_mask=torch.ones(B, a.lang_len, dtype=torch.bool, device=dev), lang_embeds=rn(B, a.lang_len, 4096),
                            img_tokens=rn(B, a.img_len, 1152)))
    b0 = batches[0]
    tr.train_step(b0["lang_embeds"], b0["lang_attn_mask"], b0["img_tokens"], b0["states"], b0["actions"], b0["state_elem_mask"].unsqueeze(1), b0["ctrl_freqs"])
    rec = {"config": c, "parameters": params, "batch": B, "num_sample_batches": a.num_sample_batches, "inference_steps": 5, "lang_len": a.lang_len,
           "trainer_precision": "bf16", "runner_dtype": "bfloat16", "device": torch.cuda.get_device_name(dev), "repeats": a.repeats}

    # ---- weight hand-over
    sync(); t0 = time.perf_counter()
    s = tr.sampler()
    sync(); first = 1e3 * (time.perf_counter() - t0)
    rec["sampler_compute_dtype"] = str(s.compute_dtype).replace("torch.", "")
    hand = []
    for _ in range(a.repeats):
        tr.weights_version += 1                              # as an optimizer step leaves it
        sync(); t0 = time.perf_counter()
        tr.sampler()
        sync(); hand.append(1e3 * (time.perf_counter() - t0))
    sync(); t0 = time.perf_counter()
    tr.sampler()
    sync(); unchanged = 1e3 * (time.perf_counter() - t0)
    host = []
    for _ in range(min(a.repeats, 2)):
        fresh = build_runner(a, dev)
        sync(); t0 = time.perf_counter()
        tr.sync_to(fresh).engine()
        sync(); host.append(1e3 * (time.perf_counter() - t0))
        del fresh
        torch.cuda.empty_cache()
    rec["hand_over"] = {"sampler_first_call_ms": first, "sampler_after_a_step_ms": _stats(hand), "sampler_unchanged_weights_ms": unchanged,
                        "sync_to_plus_engine_ms": sorted(host), "fp32_master_bytes": 4 * params}      # two repeats: the values, no median or ratio
    print(json.dumps(rec["hand_over"]))

    # ---- metrics of one batch
    pred = s.predict_action(lang_tokens=b0["lang_embeds"], lang_attn_mask=b0["lang_attn_mask"], img_tokens=b0["img_tokens"], state_tokens=b0["states"],
                            action_mask=b0["state_elem_mask"].unsqueeze(1), ctrl_freqs=b0["ctrl_freqs"]).contiguous()
    n = len(names)
    rows = torch.tensor(b0["data_indices"], dtype=torch.int32, device=dev)
    acc, count = torch.zeros(2 * (n + 1), dtype=torch.float64, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev)
    out, ws = torch.empty(2 * B + 2, device=dev), torch.empty(3 * B, dtype=torch.float64, device=dev)
    sp = L.stream_ptr(dev)
    call = lambda: L.check(L.lib().vt_sample_metrics(L.ptr(pred), L.dt_code(pred.dtype), L.ptr(b0["actions"]), L.ptr(b0["state_elem_mask"]), L.ptr(b0["state_norm"]),
                                                      L.ptr(rows), B, 64, 128, n, L.ptr(out), L.ptr(out[2 * B:]), L.ptr(acc), L.ptr(count), L.ptr(ws), sp),
                           "vt_sample_metrics")
    hip_ms, torch_ms = [], []
    for k in range(3 + 20):
        sync(); t0 = time.perf_counter()
        call()
        sync(); t1 = time.perf_counter()
        torch_statement(pred, b0["actions"], b0["state_elem_mask"], b0["state_norm"], b0["data_indices"], names, {}, {})
        sync(); t2 = time.perf_counter()
        if k >= 3:
            hip_ms.append(1e3 * (t1 - t0)), torch_ms.append(1e3 * (t2 - t1))
    rec["metrics_one_batch"] = {"vt_sample_metrics_ms": _stats(hip_ms), "torch_statement_with_item_loop_ms": _stats(torch_ms),
                                "host_reads_torch_statement": 2 * B + 2, "host_reads_vt_sample_metrics": 0,
                                "note": "both timed between device synchronisations: launch latency dominates either"}
    print(json.dumps(rec["metrics_one_batch"]))

    # ---- a whole visit
    visit, metrics = [], None
    for k in range(1 + a.repeats):
        tr.weights_version += 1
        sync(); t0 = time.perf_counter()
        metrics = sample_eval(tr.sampler(), batches, num_sample_batches=a.num_sample_batches, dataset_id2name=names)
        sync(); t1 = time.perf_counter()
        if k >= 1:
            visit.append(1e3 * (t1 - t0))
    med = _stats(visit)["median"]
    rec["visit"] = {"ms": _stats(visit), "share_of_1000_training_steps": med / (1000 * TRAIN_STEP_MS), "training_step_ms_assumed": TRAIN_STEP_MS,
                    "metrics": metrics, "peak_memory_gib": torch.cuda.max_memory_allocated(dev) / 2 ** 30}
    print(json.dumps(rec["visit"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
