#!/usr/bin/env python
"""Octopi's tactile video encoder on one MI355X (vlatouch.clip, synthetic CLIP ViT-L/14 weights, n_ctx / prompt depth of
synth.CLIP_CONFIGS["vit-l14"]), fp16 storage: ms per call at l = 10 frames of 224 px, for 1 and 8 videos, of
  tower         ClipEngine.forward on the b * l frames -> pooler_output
  tower_heads   + video feature, retrieval against a bank of 300 (k = 3), Adapter, PropertyClassifier
  project       project(features) at E = 3584 (Linear(1024, E), GELU, Linear(E, E)) on the b * l features alone
against HF CLIPVisionModel in fp16 on the same GPU with the same weights and the prompt steps applied in torch between its encoder layers
(the reference's execution; its own prompt classes do not import under this transformers), the heads in torch fp16.  Medians of 7 alternated
repeats (ours, baseline, ours, ...).  Writes profiles/tactile_bench.json and prints the same JSON line.

    timeout -k 10 600 python tools/tactile_bench.py [--iters 10] [--layers 24] [--out profiles/tactile_bench.json]

profiles/tactile_project_kernels.txt:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/tactile_bench.py --project-only 200
    python tools/tactile_bench.py --trace-summary <dir>/<name>_results.db > profiles/tactile_project_kernels.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vla-touch_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vlatouch import synth  # noqa: E402
from vlatouch.clip import ClipEngine, LinearHead, TactileHeads  # noqa: E402

DEV = "cuda:0"
REPEATS = 7


def time_ms(fn, iters, warmup=2):
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


def alternated(ours, base, iters):
    a, b = [], []
    for _ in range(REPEATS):
        a.append(time_ms(ours, iters))
        if base is not None:
            b.append(time_ms(base, iters))
    r = {"ms": round(statistics.median(a), 3)}
    if b:
        r["hf_ms"] = round(statistics.median(b), 3)
        r["hf_over_ours"] = round(r["hf_ms"] / r["ms"], 2)
    return r


def hf_tower(sd, c, layers):
    """HF CLIPVisionModel (fp16, same weights) + the prompt steps in torch -> a function frames [B, 3, S, S] -> pooler_output."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    cfg = CLIPVisionConfig(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=layers, num_attention_heads=c["heads"],
                           image_size=c["image_size"], patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    m = CLIPVisionModel(cfg)
    own = m.state_dict()
    pre = "vision_model." if any(k.startswith("vision_model.") for k in own) else ""
    m.load_state_dict({k: sd[k[len(pre):]] for k in own})
    m = m.half().to(DEV).eval()
    vm = getattr(m, "vision_model", m)
    P, n = min(c["prompt_depth"], layers), c["n_ctx"]
    vpt = sd["VPT"].half().to(DEV)
    shallow = {i: sd[f"encoder.layers.{i}.VPT_shallow"].half().to(DEV) for i in range(1, P)}
    gate = {i: torch.sigmoid(sd[f"encoder.layers.{i}.VPT_gamma"]).half().to(DEV) for i in range(layers - 1)}
    last = layers - 1

    def fwd(x):
        t = vm.embeddings(x)
        t = vm.pre_layrnorm(torch.cat([t, vpt.expand(t.shape[0], -1, -1)], dim=1))
        for i, layer in enumerate(vm.encoder.layers):
            before = t[:, -n:] if i != last else None
            add = 1 <= i < P
            if add:
                t = torch.cat([t[:, :-n], shallow[i].expand(t.shape[0], -1, -1)], dim=1)
            elif i == P:
                t = t[:, :-n]
            y = layer(t, attention_mask=None)
            t = y[0] if isinstance(y, tuple) else y
            if add and i != last:
                t = torch.cat([t[:, :-n], gate[i] * t[:, -n:] + (1 - gate[i]) * before], dim=1)
        return vm.post_layernorm(t[:, 0])

    return fwd


def project_only(D, E, calls):
    """The two sides of the `project` comparison alone, so that a kernel trace holds nothing else."""
    hs = synth.tactile_head_shapes(D, E)["project"]
    sd = {n: torch.from_numpy(np.asarray(v)) for n, v in synth.fill_state_dict(hs, prefix="tactile-bench-project.").items()}
    project = LinearHead(sd, precision="bf16", device=DEV)
    w = {n: v.half().to(DEV) for n, v in sd.items()}
    F = torch.nn.functional
    for rows in (10, 80):
        f = torch.randn(rows, D, device=DEV)
        f16 = f.half()
        for _ in range(calls):
            project(f, torch.bfloat16)
        torch.cuda.synchronize()
        for _ in range(calls):
            F.linear(F.gelu(F.linear(f16, w["0.weight"], w["0.bias"])), w["2.weight"], w["2.bias"])
        torch.cuda.synchronize()


def trace_summary(db):
    """Calls, average and total microseconds per kernel name of a rocprofv3 `*_results.db`, the ten largest: profiles/tactile_project_kernels.txt."""
    import sqlite3
    con = sqlite3.connect(db)
    print("project(features) alone on one MI355X: Linear(1024, 3584), GELU, Linear(3584, 3584) at 10 and 80 rows; ours (bf16: act_copy + two gemm_kernel),")
    print("then torch fp16 (two hipBLASLt Cijk kernels + GeluCUDAKernelImpl).  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/tactile_bench.py")
    print("--project-only 200, summarised by tools/tactile_bench.py --trace-summary <dir>/..._results.db: kernel name (110 characters), calls, average, total.")
    print()
    for name, n, avg, tot in con.execute("select name, count(*), avg(end - start) / 1000.0, sum(end - start) / 1000.0 from kernels group by name order by 4 desc limit 10"):
        print(f"{name[:110]:110s} calls {n:4d}  avg {avg:7.2f} us  total {tot:9.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tactile_bench.json"))
    ap.add_argument("--project-only", type=int, default=0, metavar="CALLS",
                    help="run nothing but `project`: CALLS calls of ours, then of torch fp16, at 10 and 80 rows, and write no file (for a kernel trace)")
    ap.add_argument("--trace-summary", metavar="DB", help="print the kernel dispatches of a rocprofv3 results database grouped by kernel name and exit (no GPU)")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    c = dict(synth.CLIP_CONFIGS["vit-l14"], layers=a.layers)
    E, R, K = 3584, 300, 3
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    if a.project_only:
        return project_only(c["hidden"], E, a.project_only)
    shapes = synth.clip_shapes(c["hidden"], c["layers"], c["inter"], c["image_size"], n_ctx=c["n_ctx"], prompt_depth=min(c["prompt_depth"], a.layers))
    sd = synth.fill_state_dict_device(shapes, DEV, torch.float32, seed=11)
    sd = {k: v.cpu() for k, v in sd.items()}
    eng = ClipEngine(sd, heads=c["heads"], precision="fp16", device=DEV, prompt_depth=min(c["prompt_depth"], a.layers))
    hs = synth.tactile_head_shapes(c["hidden"], E)
    hsd = {k: {n: torch.from_numpy(np.asarray(v)) for n, v in synth.fill_state_dict(s, prefix=f"tactile-bench-{k}.").items()} for k, s in hs.items()}
    adapter = LinearHead({n.replace("rfc.", ""): v for n, v in hsd["adapter"].items()}, precision="bf16", device=DEV, residual=True)
    p = hsd["property_classifier"]
    prop = LinearHead({"0.weight": p["fc.0.weight"], "0.bias": p["fc.0.bias"], "2.weight": p["fc.2.weight"], "2.bias": p["fc.2.bias"],
                       "4.weight": torch.cat([p["hardness_fc.weight"], p["roughness_fc.weight"]]), "4.bias": torch.cat([p["hardness_fc.bias"], p["roughness_fc.bias"]])},
                      precision="bf16", device=DEV)
    project = LinearHead(hsd["project"], precision="bf16", device=DEV)
    heads = TactileHeads(DEV)
    g = torch.Generator().manual_seed(0)
    bank = torch.randn(R, c["hidden"], generator=g)
    heads.set_bank(bank)
    res = {"workload": "octopi_tactile_encoder", "model": "clip-vit-l14 (synthetic)", "layers": a.layers, "n_ctx": c["n_ctx"], "prompt_depth": eng.prompt_depth,
           "frames": a.frames, "storage": "fp16 tower, bf16 heads", "repeats": REPEATS, "iters": a.iters}
    try:
        base = hf_tower(sd, c, a.layers)
        res["hf"] = "transformers CLIPVisionModel fp16, same weights, prompt steps in torch"
    except Exception as e:
        base = None
        res["hf"] = f"unavailable ({type(e).__name__}: {e})"[:200]
    # torch fp16 heads of the baseline
    t16 = lambda d: {n: v.half().to(DEV) for n, v in d.items()}
    ha, hp, hj, bank16 = t16(hsd["adapter"]), t16(p), t16(hsd["project"]), bank.half().to(DEV)
    F = torch.nn.functional
    cos = torch.nn.CosineSimilarity(dim=1, eps=1e-8)

    def base_heads(feats, b):
        f = feats.reshape(b, a.frames, -1)
        v = f.mean(dim=1)
        v = v / v.norm(p=2, dim=-1, keepdim=True)
        for j in range(b):                                           # the reference retrieves one video at a time
            torch.topk(cos(bank16, v[j:j + 1]), k=K)
        F.linear(F.gelu(F.linear(feats, ha["rfc.0.weight"], ha["rfc.0.bias"])), ha["rfc.2.weight"], ha["rfc.2.bias"]) + feats
        h = F.gelu(F.linear(F.gelu(F.linear(feats, hp["fc.0.weight"], hp["fc.0.bias"])), hp["fc.2.weight"], hp["fc.2.bias"]))
        torch.cat([F.linear(h, hp["hardness_fc.weight"], hp["hardness_fc.bias"]), F.linear(h, hp["roughness_fc.weight"], hp["roughness_fc.bias"])], dim=1)

    for b in (1, 8):
        x = torch.randn(b * a.frames, 3, c["image_size"], c["image_size"], generator=g).to(DEV)
        x16 = x.half()

        def ours_heads():
            f = eng.forward(x)
            heads.retrieve(f.reshape(b, a.frames, -1), K)
            adapter(f)
            prop(f)

        r = {"tower": alternated(lambda: eng.forward(x), (lambda: base(x16)) if base else None, a.iters),
             "tower_heads": alternated(ours_heads, (lambda: base_heads(base(x16), b)) if base else None, a.iters)}
        f = eng.forward(x)
        f16 = f.half()
        r["project"] = alternated(lambda: project(f, torch.bfloat16),
                                  lambda: F.linear(F.gelu(F.linear(f16, hj["0.weight"], hj["0.bias"])), hj["2.weight"], hj["2.bias"]), a.iters)
        if base:
            theirs = base(x16).float()
            r["pooled_max_rel_delta"] = float(((f - theirs).abs().amax(-1) / theirs.abs().amax(-1)).max())
        res[f"videos_{b}"] = r
        print(f"videos {b}", r, file=sys.stderr, flush=True)
    line = json.dumps(res)
    with open(a.out, "w") as fjson:
        fjson.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
