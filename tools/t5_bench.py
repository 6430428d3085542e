#!/usr/bin/env python
"""T5 v1.1-XXL encoder on one MI355X (vlatouch.t5, synthetic bf16 device weights): ms per call for
  (a) B=1, L=32   — the online instruction of the robot wrapper; a pure weight stream (reported as GB/s against 8 TB/s and the 6.3 TB/s copy ceiling)
  (b) B=64, L=120 — encode_lang_batch's padded labelling batch; a GEMM problem (reported as TFLOP/s against 2.5 PF dense bf16)
and, when transformers imports, HF T5EncoderModel in bf16 on the same GPU with the same weights (the reference's own execution): its time
and max |delta| against ours.  One JSON line on stdout.

    timeout -k 10 600 python tools/t5_bench.py [--iters 20] [--layers 24]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vla-touch_amd")]

import torch  # noqa: E402

from vlatouch import synth  # noqa: E402
from vlatouch import t5 as T5  # noqa: E402

DEV = "cuda:0"
PEAK_BW, COPY_BW, PEAK_BF16 = 8.0e12, 6.3e12, 2.5e15


def time_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def flops(cfg, B, L):
    D, I, F, n = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"], cfg["num_layers"]
    M = B * L
    gemm = 2 * M * D * (3 * I + I + 3 * F)
    attn = 4 * B * L * L * I
    return n * (gemm + attn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=24)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    cfg = synth.t5_config("xxl", num_layers=a.layers)
    sd = synth.fill_state_dict_device(synth.t5_shapes(**cfg), DEV, torch.bfloat16, seed=7)
    eng = T5.T5Engine(sd, cfg, precision="bf16", device=DEV)
    c = T5.t5_config(cfg)
    # bytes one call must stream: every GEMM weight once (the embedding table is gathered, not streamed)
    w_bytes = sum(w.numel() * w.element_size() for w in eng.weights[2:])
    g = torch.Generator().manual_seed(0)
    res = {"workload": "t5_v1_1_xxl_encoder", "precision": "bf16", "layers": a.layers, "weight_bytes": w_bytes}
    hf = None
    try:
        from transformers import T5Config, T5EncoderModel
        hcfg = T5Config(**{k: v for k, v in cfg.items() if k not in ("is_gated_act", "dense_act_fn")}, dropout_rate=0.0, is_encoder_decoder=False,
                        use_cache=False)
        with torch.device("meta"):
            hf = T5EncoderModel(hcfg)
        full = {k: (sd["shared.weight"] if k == "encoder.embed_tokens.weight" else sd[k]) for k in hf.state_dict()}
        hf.load_state_dict(full, assign=True)
        hf = hf.to(DEV).eval()
        res["hf"] = "transformers T5EncoderModel bf16, same weights"
    except Exception as e:      # no transformers on the box, or a version without these names
        hf = None
        res["hf"] = f"unavailable ({type(e).__name__}: {e})"[:200]
    for tag, B, L in (("a_b1_l32", 1, 32), ("b_b64_l120", 64, 120)):
        ids = torch.randint(2, c["vocab_size"], (B, L), generator=g)
        mask = torch.ones(B, L, dtype=torch.long)
        if B > 1:
            lens = torch.randint(8, L + 1, (B,), generator=g)
            lens[0] = L
            mask = (torch.arange(L)[None, :] < lens[:, None]).long()
        ms = time_ms(lambda: eng.forward(ids, mask), a.iters)
        r = {"ms": round(ms, 3), "tflops": round(flops(c, B, L) / ms / 1e9, 1)}
        r["pct_of_2p5_pf"] = round(100 * flops(c, B, L) / ms / 1e-3 / PEAK_BF16, 1)
        r["gb_per_s"] = round(w_bytes / ms / 1e6, 1)
        r["pct_of_8_tb_s"] = round(100 * w_bytes / ms / 1e-3 / PEAK_BW, 1)
        r["pct_of_6p3_tb_s_copy"] = round(100 * w_bytes / ms / 1e-3 / COPY_BW, 1)
        if hf is not None:
            ids_d, mask_d = ids.to(DEV), mask.to(DEV)
            r["hf_ms"] = round(time_ms(lambda: hf(input_ids=ids_d, attention_mask=mask_d), max(3, a.iters // 2)), 3)
            ours = eng.forward(ids, mask).float()
            theirs = hf(input_ids=ids_d, attention_mask=mask_d).last_hidden_state.float()
            r["hf_max_abs_delta"] = float((ours - theirs).abs().max())
            r["hf_speedup"] = round(r["hf_ms"] / r["ms"], 2)
        res[tag] = r
        print(tag, r, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
