#!/usr/bin/env python
"""Wall time and memory of the RDT fine-tuning step (vlatouch/rdt_train.py) at RDT-1B dimensions (bench.py's RDT config: hidden 2048, depth 28,
32 heads, horizon 64, 4 374 image tokens, 32 language tokens, synthetic weights) -> profiles/rdt_train_bench.json.

Default: `precision="bf16"` (the reference's execution dtype), batch 4 (main.py:54) and batch 32, 3 warm-up + 10 timed steps on one repeated
batch, device-synchronised wall time split into forward (get_loss without backward), backward, and clip + AdamW + EMA; peak device memory; the
loss of every timed step (it must fall on a repeated batch); algorithmic FLOPs per step from the shapes (3 x the forward's 2 x MAC count of the
Linears and attention products, no K/V cache credit) and the share of the bf16 MFMA peak they give as a WHOLE-STEP rate, not a kernel's.
Yardstick only: `loss.backward()` of the oracle (tests/rdt_train_ref.loss_fn, plain torch) on the same GPU in bf16 at the first batch size, and
the ratio; if it does not run, the field says "not measured" and why.
    python tools/rdt_train_bench.py [--precision bf16] [--batch 4 32] [--depth 28] [--steps 10] [--out profiles/rdt_train_bench.json]

`--accum K` (K > 1) measures the accumulated step instead (the reference's finetune.sh: batch 4, K = 4) at the first batch size: `--steps` windows
of K micro-batches after `--warmup` windows, every phase device-synchronised: forward, backward, vt_grad_accum_multi, and vt_ema_multi (the
K - 1 micro-batches without an optimizer step) or clip + AdamW + EMA (the K-th); median and min / max over the timed windows; samples/s over a
whole window; peak memory; the bytes the accumulate and EMA-only launches move (12 B per parameter each) against the HBM roof; and, from a K = 1
trainer in the same process, the clip + AdamW + EMA phase the two launches together are held against.  Added to `--out` under the key
`accumulation`; the other keys of the file stay as they are.

`--optimizer adamw8bit` measures the optimizer phase with block-wise 8-bit moments (csrc/vt_adam8.hip) beside the 32-bit one at the first batch
size: one trainer of each kind in one process, their steps alternating and swapping who goes first, `--steps` (at least 5) timed after `--warmup`,
device-synchronised host wall clock and device events:
the whole phase (clip + AdamW + EMA, and in bf16 the refresh of the 16-bit weight copies, as `clip_adamw_ema_ms` of the default run counts it)
and the AdamW + EMA launch alone with the bytes it moves (24 B per parameter of a quantised tensor plus its scales, 36 B otherwise) against the
HBM roof; optimizer state bytes; peak device memory of a step of each trainer.  Added to `--out` under the key `adamw8bit`; the other keys stay.

`--attention-backward mfma` measures the bf16 step with the MFMA attention backward (csrc/vt_attn_bwd.hip) beside the default "wave" kernels at
every `--batch` size: one trainer of each kind in one process, their steps alternating and swapping who goes first, `--warmup` warm-up and
`--steps` (default 21 here) timed steps, every phase device-synchronised: forward (get_loss without backward), backward, clip + AdamW + EMA,
medians with min / max; by device events the attention-backward launches alone of one image cross-attention (`--img-len` keys), one language
cross-attention and one self-attention at the trainer's strides; peak device memory of a step of each trainer; the bytes of `ws2`; the
torch-autograd yardstick of the same run.  Added to `--out` under the key `attention_backward_mfma`; the other keys stay.

`--weight-gradient tn` measures the bf16 step (under `attention_backward="mfma"`) with the transpose-free weight-gradient GEMM (csrc/vt_gemm_tn.hip)
beside the default "gemm" path (two transposes, the NT GEMM, a column sum: the path of every commit before it) at every `--batch` size: one trainer of
each kind in one process, their steps alternating and swapping who goes first, `--warmup` warm-up and `--steps` (default 21 here) timed steps, every
phase device-synchronised, medians with min / max; by device events the weight-gradient work alone, old and new, of the image K|V product
(`--img-len` x batch rows), a hidden x hidden product (67 x batch rows) and the timestep embedder's (batch rows), with the plan of each; peak device
memory of a step of each trainer.  Added to `--out` under the key `weight_gradient_tn`; the other keys stay.

`--small-batch-linear packed` measures the bf16 step (under `attention_backward="mfma"`, `weight_gradient="tn"`) with the packed-weight small-batch
Linears and the one-pass refresh (`RdtTrainer(small_batch_linear="packed")`, csrc/vt_refresh16.hip) beside the default "gemm" trainer at every
`--batch` size (4, 7 and 32 are the sizes of the record: the working point, the largest the path takes, and one it does not take), same method; by device
events the refresh of all weights alone after every timed step under either setting, and one hidden x hidden Linear (67 x batch rows), forward and
data gradient, on either route; how many launches were offered a packed copy and took the packed tile; the bytes of the packed copies and the scratch;
peak device memory of a step of each trainer.  Added to `--out` under the key `small_batch_linear_packed`; the other keys stay.

`--data-parallel fp32|bf16` measures the data-parallel step (`RdtTrainer(process_group=, comm_dtype=)`) at batch 4, bf16, `attention_backward="mfma"`
over an RCCL ("nccl") process group of world size 1, which is all a one-GPU machine allows: NO SCALING NUMBER CAN BE PRODUCED ON A ONE-GPU BOX, and a
world-size-1 all-reduce moves nothing between cards.  A grouped and an ungrouped trainer alternate in one process and swap who goes first; by device
events, `--warmup` + 21 timed: vt_grad_accum_multi (the fold) and vt_grad_fold_pack_multi (fold + pack) on the same table with the same fresh
gradients, the all-reduce on itself (the arena, or the bf16 buffer, in `comm_bucket_bytes` slices), vt_grad_unpack_multi, and the whole step of
each trainer; medians with min / max, bytes moved against the HBM roof, and whether fold + pack took no longer than the fold (medians, with the
min - max spread of the two as the only margin).  Added to `--out` under the key `data_parallel`; the other keys stay.

`--precision fp16` (with `--attention-backward mfma` and `--optimizer adamw8bit` as wanted): an fp16 trainer under dynamic loss scaling and a bf16
trainer of the same settings alternate in one process, swapping who goes first, 3 warm-up + 21 timed steps: forward, backward, optimizer phase
and step of each with min / max, the losses of both, the scale after every fp16 step and which steps it skipped, and by device events the
attention-backward launches of both kernels in fp16 against bf16 at the three attention shapes.  Added to `--out` under the key `fp16`.
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


def forward_macs(c: dict, B: int, lang_len: int) -> float:
    """Multiply-accumulates of one forward of compute_loss (Linears + attention products), from the shapes."""
    D, N, Li, A = c["hidden"], c["horizon"] + 3, c["img_cond_len"], c["action_dim"]
    M = B * N
    macs = B * lang_len * (c["lang_token_dim"] * D + D * D) + B * Li * (c["img_token_dim"] * D + D * D)
    macs += B * (c["horizon"] + 1) * (2 * A * D + 2 * D * D) + 2 * B * (256 * D + D * D)
    for i in range(c["depth"]):
        Lc = lang_len if i % 2 == 0 else Li
        macs += M * D * 3 * D + 2 * B * N * N * D + M * D * D                      # self-attention
        macs += M * D * D + B * Lc * D * 2 * D + 2 * B * N * Lc * D + M * D * D    # cross-attention
        macs += 2 * M * D * D                                                      # FFN
    return float(macs + M * D * D + M * D * A)


HBM_SPEC_BYTES_PER_S = 8.0e12    # MI355X HBM3E specification; a float4 copy reaches about 6.3e12 of it
HBM_COPY_BYTES_PER_S = 6.3e12
PEAK_BF16_FLOPS = 16 * 157.3e12   # MI355X dense bf16 MFMA peak (16 x the 157.3 TFLOP/s fp32 matrix rate), for the whole-step share only


def yardstick(sd, c, args, kw, dev):
    """forward + loss.backward() of the oracle under torch autograd on this GPU in bf16 (1 warm-up + 3 timed) -> dict, or "not measured: why"."""
    try:
        from tests import rdt_train_ref as R
        keys = ("lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs")
        b = dict(zip(keys, args), **kw)
        cfg = dict(heads=c["heads"], horizon=c["horizon"])
        leaves = R.leaf_sd(sd, torch.bfloat16)
        ts = []
        with torch.device(dev), torch.enable_grad():
            for n in range(4):
                for v in leaves.values():
                    v.grad = None
                torch.cuda.synchronize(dev); t0 = time.perf_counter()
                loss = R.loss_fn(leaves, b, cfg, dtype=torch.bfloat16)
                loss.backward()
                torch.cuda.synchronize(dev); ts.append(time.perf_counter() - t0)
        return {"what": "oracle forward + loss.backward() under torch autograd, bf16, same GPU", "fwd_bwd_ms": 1e3 * min(ts[1:]), "loss": float(loss.detach())}
    except Exception as e:                       # a yardstick only: record why it did not run
        return f"not measured: {type(e).__name__}: {str(e)[:200]}"
    finally:
        torch.cuda.empty_cache()


def _stats(ms):
    """median, min, max of a list of millisecond samples."""
    t = sorted(ms)
    n = len(t)
    return {"median": t[n // 2] if n % 2 else 0.5 * (t[n // 2 - 1] + t[n // 2]), "min": t[0], "max": t[-1], "n": n}


def inputs(a, B, dev):
    g = torch.Generator(device=dev).manual_seed(99)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    amask = torch.zeros(B, 1, 128, device=dev)
    amask[:, :, :10] = 1.0
    args = (rn(B, a.lang_len, 4096), torch.ones(B, a.lang_len, dtype=torch.bool, device=dev), rn(B, a.img_len, 1152), rn(B, 1, 128),
            torch.tanh(rn(B, 64, 128)) * amask, amask, torch.full((B,), 10.0, device=dev))
    kw = dict(noise=rn(B, 64, 128), timesteps=torch.randint(0, 1000, (B,), generator=g, device=dev))
    return args, kw


def timed_step(tr, args, kw, dev):
    """One step of `tr` between device synchronisations -> (forward only, forward + backward, optimizer phase) in host-clock ms, the loss."""
    sync = lambda: torch.cuda.synchronize(dev)
    sync(); t0 = time.perf_counter()
    tr.get_loss(*args, backward=False, **kw)
    sync(); t1 = time.perf_counter()
    loss = tr.get_loss(*args, **kw)
    sync(); t2 = time.perf_counter()
    tr.optimizer_step()
    sync(); t3 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), loss


def build_trainers(a, dev, args, kw, makers):
    """makers: {name: factory of a trainer}.  Builds and warms up each in turn -> ({name: trainer}, {name: peak device memory in GiB of one
    whole step of that trainer, over what was already resident})."""
    trs, peak = {}, {}
    for kind, make in makers.items():
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        tr = trs[kind] = make()
        for _ in range(max(1, a.warmup)):
            tr.get_loss(*args, **kw)
            tr.optimizer_step()
        torch.cuda.synchronize(dev)
        peak[kind] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30
    return trs, peak


def compare_steps(a, dev, args, kw, makers, each_step=None):
    """The comparison every two-trainer mode makes: the trainers of `makers` (build_trainers) take `a.steps` timed steps in turn, swapping who
    goes first, every phase device-synchronised -> {name: forward / backward / optimizer / step statistics, peak memory, losses}.
    each_step(name, trainer) is called after every timed step."""
    trs, peak = build_trainers(a, dev, args, kw, makers)
    kinds = tuple(makers)
    ph = {k: {n: [] for n in ("forward_ms", "backward_ms", "clip_adamw_ema_ms", "step_ms")} for k in kinds}
    losses = {k: [] for k in kinds}
    for n in range(a.steps):
        for kind in (kinds if n % 2 == 0 else kinds[::-1]):  # who goes first alternates
            f, fb, o, loss = timed_step(trs[kind], args, kw, dev)
            ph[kind]["forward_ms"].append(f), ph[kind]["backward_ms"].append(fb - f), ph[kind]["clip_adamw_ema_ms"].append(o), ph[kind]["step_ms"].append(fb + o)
            losses[kind].append(float(loss))
            if each_step is not None:
                each_step(kind, trs[kind])
    del trs
    torch.cuda.empty_cache()
    return {k: dict({n: _stats(v) for n, v in ph[k].items()}, peak_memory_gib_of_a_step=peak[k], losses=losses[k]) for k in kinds}


STEP_TIMING = "host wall clock between two device synchronisations; the two trainers alternate and swap who goes first every step"


def packed_attention_views(B, N, Nk, H, cross, dt, rn, dev):
    """(q, k, v), (dq, dk, dv) as [B, N | Nk, H, 64] views at the trainer's packed layouts: q beside a k | v buffer (cross) or one q | k | v
    buffer; the operands drawn from `rn`, the gradients uninitialised."""
    widths = ((N, 1), (Nk, 2)) if cross else ((N, 3),)
    bufs = [rn(B, rows, w * H * 64) for rows, w in widths]
    grads = [torch.empty(B, rows, w * H * 64, device=dev, dtype=dt) for rows, w in widths]
    v3 = lambda ts: tuple(t.view(B, rows, w, H, 64)[:, :, i] for t, (rows, w) in zip(ts, widths) for i in range(w))
    return v3(bufs), v3(grads)


def accum_run(a, c, sd, params, dev):
    """The accumulated step at batch a.batch[0], K = a.accum, and the K = 1 optimizer phase in the same process -> dict."""
    from vlatouch.rdt_train import RdtTrainer
    B, K = a.batch[0], a.accum
    sync = lambda: torch.cuda.synchronize(dev)
    args, kw = inputs(a, B, dev)
    # K = 1 first: the phase the two new launches are held against
    tr = RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision=a.precision, device=dev)
    k1 = []
    for n in range(a.warmup + a.steps):
        tr.get_loss(*args, **kw)
        sync(); t0 = time.perf_counter()
        tr.optimizer_step()
        sync(); t1 = time.perf_counter()
        if n >= a.warmup:
            k1.append(1e3 * (t1 - t0))
    del tr
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    tr = RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision=a.precision, gradient_accumulation_steps=K, device=dev)
    ph = {n: [] for n in ("forward_ms", "backward_ms", "accumulate_ms", "ema_only_ms", "sync_step_ms", "window_ms")}
    losses = []
    for n in range(a.warmup + a.steps):
        window = 0.0
        for j in range(K):
            sync(); t0 = time.perf_counter()
            tr.get_loss(*args, backward=False, **kw)
            sync(); t1 = time.perf_counter()
            loss = tr.get_loss(*args, **kw)
            sync(); t2 = time.perf_counter()
            tr.accumulate()
            sync(); t3 = time.perf_counter()
            if j == K - 1:
                tr.optimizer_step()
            else:
                tr.ema_step()
            sync(); t4 = time.perf_counter()
            window += t4 - t1                                        # the forward-only pass is there for the split, not part of a step
            if n >= a.warmup:
                ph["forward_ms"].append(1e3 * (t1 - t0)), ph["backward_ms"].append(1e3 * ((t2 - t1) - (t1 - t0))), ph["accumulate_ms"].append(1e3 * (t3 - t2))
                ph["sync_step_ms" if j == K - 1 else "ema_only_ms"].append(1e3 * (t4 - t3))
        if n >= a.warmup:
            ph["window_ms"].append(1e3 * window)
            losses.append(float(loss))
    out = {"batch": B, "accum": K, "precision": a.precision, "parameters": params, "warmup_windows": a.warmup, "timed_windows": a.steps}
    out.update({n: _stats(v) for n, v in ph.items()})
    out["samples_per_s"] = B * K / (out["window_ms"]["median"] / 1e3)
    out["peak_memory_gib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    out["losses_last_micro_batch_of_window"] = losses
    out["grad_norm_last"] = float(tr.grad_norm)
    out["k1_clip_adamw_ema_ms_same_session"] = _stats(k1)
    both = out["accumulate_ms"]["median"] + out["ema_only_ms"]["median"]
    out["accumulate_plus_ema_only_ms"] = both
    out["no_longer_than_k1_optimizer_phase"] = bool(both <= out["k1_clip_adamw_ema_ms_same_session"]["median"])
    for n in ("accumulate_ms", "ema_only_ms"):
        rate = 12.0 * params / (out[n]["median"] / 1e3)
        out[n]["bytes_per_s"] = rate
        out[n]["share_of_hbm_spec"], out[n]["share_of_float4_copy_rate"] = rate / HBM_SPEC_BYTES_PER_S, rate / HBM_COPY_BYTES_PER_S
    return out


def optimizer_run(a, c, sd, params, dev):
    """The optimizer phase of an "adamw8bit" and an "adamw" trainer, alternating in this process at batch a.batch[0] -> dict."""
    from vlatouch import _lib as L
    from vlatouch import adam8
    from vlatouch.rdt_train import RdtTrainer
    B = a.batch[0]
    steps = max(5, a.steps)
    sync = lambda: torch.cuda.synchronize(dev)
    args, kw = inputs(a, B, dev)
    kinds = ("adamw8bit", "adamw")
    make = lambda kind: lambda: RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision=a.precision, optimizer=kind, device=dev)
    trs, peak = build_trainers(a, dev, args, kw, {kind: make(kind) for kind in kinds})
    ev = lambda: torch.cuda.Event(enable_timing=True)
    phase = {k: [] for k in kinds}
    phase_dev = {k: [] for k in kinds}
    losses = {k: [] for k in kinds}
    for n in range(steps):
        for kind in (kinds if n % 2 == 0 else kinds[::-1]):  # who goes first alternates, so neither kind always follows the other's step
            tr = trs[kind]
            loss = tr.get_loss(*args, **kw)
            e0, e1 = ev(), ev()
            sync(); t0 = time.perf_counter()
            e0.record()
            tr.optimizer_step()
            e1.record()
            sync(); t1 = time.perf_counter()
            phase[kind].append(1e3 * (t1 - t0))              # host wall clock: the table's rows, the hyper floats' upload and the launches
            phase_dev[kind].append(e0.elapsed_time(e1))      # device events: from before the first launch to after the last
            losses[kind].append(float(loss))
    # the AdamW + EMA launch alone, on the state the steps left (it moves the same bytes whatever the values)
    launch = {k: [] for k in kinds}
    hy = torch.zeros(4)
    L.check(L.lib().vt_train_hyper(a.lr, 0.9, 0.999, steps + a.warmup + 1, 0.9999, L.ptr(hy)), "vt_train_hyper")
    hy = hy.to(dev)
    for n in range(2 + steps):
        for kind in (kinds if n % 2 == 0 else kinds[::-1]):
            tr = trs[kind]
            tab, nt, chunks = tr._table()
            e0, e1 = ev(), ev()
            sync()
            e0.record()
            tr.opt_state.step(tab, nt, chunks, hy, (0.9, 0.999), tr.eps, tr.wd)
            e1.record()
            sync()
            if n >= 2:
                launch[kind].append(e0.elapsed_time(e1))
    numels = [v.numel() for v in sd.values()]
    q = sum(n for n in numels if n >= adam8.MIN_8BIT_SIZE)
    moved = {"adamw": 36.0 * params, "adamw8bit": 24.0 * q + 16.0 * sum(adam8.nblocks(n) for n in numels if n >= adam8.MIN_8BIT_SIZE) + 36.0 * (params - q)}
    out = {"batch": B, "precision": a.precision, "parameters": params, "parameters_quantised": q, "warmup": a.warmup, "timed_steps": steps}
    for kind in kinds:
        ls = _stats(launch[kind])
        rate = moved[kind] / (ls["median"] / 1e3)
        ls.update(bytes_moved=moved[kind], bytes_per_s=rate, share_of_hbm_spec=rate / HBM_SPEC_BYTES_PER_S, share_of_float4_copy_rate=rate / HBM_COPY_BYTES_PER_S)
        out[kind] = {"optimizer_phase_ms": _stats(phase[kind]), "optimizer_phase_device_ms": _stats(phase_dev[kind]), "adamw_ema_launch_ms": ls, "optimizer_state_bytes": trs[kind].optimizer_state_bytes(),
                     "peak_memory_gib_of_a_step": peak[kind], "losses": losses[kind]}
    out["phase_8bit_over_32bit"] = out["adamw8bit"]["optimizer_phase_ms"]["median"] / out["adamw"]["optimizer_phase_ms"]["median"]
    out["launch_8bit_over_32bit"] = out["adamw8bit"]["adamw_ema_launch_ms"]["median"] / out["adamw"]["adamw_ema_launch_ms"]["median"]
    out["phase_device_8bit_over_32bit"] = out["adamw8bit"]["optimizer_phase_device_ms"]["median"] / out["adamw"]["optimizer_phase_device_ms"]["median"]
    out["timing"] = ("optimizer_phase_ms: host wall clock between two device synchronisations; optimizer_phase_device_ms and adamw_ema_launch_ms: "
                     "device events; the two trainers alternate and swap who goes first every step")
    out["no_slower_than_the_32bit_phase"] = bool(out["phase_8bit_over_32bit"] <= 1.0 and out["phase_device_8bit_over_32bit"] <= 1.0)
    return out


def attention_launches(a, c, B, dev):
    """Device-event time of the attention-backward launches alone, both kernels alternating, at the trainer's packed layouts -> dict."""
    from vlatouch import _lib as L
    from vlatouch.rdt_train import attention_bwd
    H, N = c["heads"], c["horizon"] + 3
    g = torch.Generator(device=dev).manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()
    out = {}
    for name, Nk, cross in (("image_cross_attention", a.img_len, True), ("language_cross_attention", a.lang_len, True), ("self_attention", N, False)):
        (q, k, v), (dq, dk, dv) = packed_attention_views(B, N, Nk, H, cross, torch.bfloat16, rn, dev)
        do = rn(B, N, H, 64)
        km = torch.ones(B, Nk, dtype=torch.uint8, device=dev) if name == "language_cross_attention" else None
        ms = {"wave": [], "mfma": []}
        for n in range(2 + 7):
            for kind in (("wave", "mfma") if n % 2 == 0 else ("mfma", "wave")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                attention_bwd(q, k, v, do, dq, dk, dv, kmask=km, kernel=kind)
                e1.record()
                torch.cuda.synchronize(dev)
                if n >= 2:
                    ms[kind].append(e0.elapsed_time(e1))
        out[name] = {"Nq": N, "Nk": Nk, "wave_ms": _stats(ms["wave"]), "mfma_ms": _stats(ms["mfma"]),
                     "mfma_over_wave": _stats(ms["mfma"])["median"] / _stats(ms["wave"])["median"],
                     "ws2_bytes": int(L.lib().vt_attention_bwd_mfma_ws_bytes(B, H, N, Nk))}
    out["timing"] = "device events around one attention_bwd call (workspace allocation from the caching allocator included), 2 warm-up + 7 timed, the two kernels alternating"
    return out


def attention_run(a, c, sd, params, dev, B):
    """The bf16 step under attention_backward="mfma" and "wave", alternating in this process at batch B -> dict."""
    from vlatouch.rdt_train import RdtTrainer
    args, kw = inputs(a, B, dev)
    kinds = ("mfma", "wave")
    make = lambda kind: lambda: RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision="bf16", attention_backward=kind, device=dev)
    out = {"batch": B, "precision": "bf16", "parameters": params, "warmup": a.warmup, "timed_steps": a.steps}
    out.update(compare_steps(a, dev, args, kw, {kind: make(kind) for kind in kinds}))
    for kind in kinds:
        out[kind]["loss_decreases"] = bool(out[kind]["losses"][-1] < out[kind]["losses"][0])
    out["backward_mfma_over_wave"] = out["mfma"]["backward_ms"]["median"] / out["wave"]["backward_ms"]["median"]
    out["step_mfma_over_wave"] = out["mfma"]["step_ms"]["median"] / out["wave"]["step_ms"]["median"]
    out["backward_faster_than_wave"] = bool(out["backward_mfma_over_wave"] < 1.0)
    out["attention_backward_launches"] = attention_launches(a, c, B, dev)
    y = "not measured: --no-yardstick" if a.no_yardstick else yardstick(sd, c, args, kw, dev)
    if isinstance(y, dict):
        for kind in kinds:
            y[f"ratio_torch_over_{kind}"] = y["fwd_bwd_ms"] / (out[kind]["forward_ms"]["median"] + out[kind]["backward_ms"]["median"])
    out["torch_autograd_yardstick"] = y
    out["timing"] = STEP_TIMING
    return out


def weight_gradient_launches(a, c, B, dev):
    """Device-event time of the weight-gradient work of one Linear alone, "gemm" (transpose_pad x 2, ops.gemm, colsum) and "tn" (weight_grad_tn)
    alternating, at three of the step's shapes -> dict."""
    from vlatouch import _lib as L
    from vlatouch import ops
    from vlatouch.rdt_train import colsum, transpose_pad, weight_grad_tn
    import ctypes as C
    D = c["hidden"]
    g = torch.Generator(device=dev).manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()
    old = lambda dy, x: (ops.gemm(transpose_pad(dy), transpose_pad(x), out_dtype=torch.float32), colsum(dy))
    out = {}
    for name, M, N, K in (("image_kv", a.img_len * B, 2 * D, D), ("hidden_square", (c["horizon"] + 3) * B, D, D), ("timestep_embedder", B, D, 256)):
        dy, x = rn(M, N), rn(M, K)
        ms = {"gemm": [], "tn": []}
        for n in range(2 + 7):
            for kind in (("gemm", "tn") if n % 2 == 0 else ("tn", "gemm")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                res = old(dy, x) if kind == "gemm" else weight_grad_tn(dy, x)
                e1.record()
                torch.cuda.synchronize(dev)
                if n >= 2:
                    ms[kind].append(e0.elapsed_time(e1))
        del res
        plan = L.GemmTnPlan()
        L.lib().vt_gemm_tn_plan(M, N, K, C.byref(plan))
        out[name] = {"M": M, "N": N, "K": K, "gemm_ms": _stats(ms["gemm"]), "tn_ms": _stats(ms["tn"]),
                     "tn_over_gemm": _stats(ms["tn"])["median"] / _stats(ms["gemm"])["median"], "launches": {"gemm": 4, "tn": 1 if plan.splits == 1 else 2},
                     "splits": plan.splits, "rows_per_split": plan.rows_per_split, "workspace_bytes": plan.ws_bytes,
                     "tn_tflops": 2.0 * M * N * K / (_stats(ms["tn"])["median"] * 1e-3) / 1e12}
        del dy, x
        torch.cuda.empty_cache()
    out["timing"] = ("device events around the calls of one weight gradient (output and workspace allocation from the caching allocator included), "
                     "2 warm-up + 7 timed, the two paths alternating")
    return out


def weight_gradient_run(a, c, sd, params, dev, B):
    """The bf16 step (attention_backward="mfma") under weight_gradient="tn" and "gemm", alternating in this process at batch B -> dict."""
    from vlatouch.rdt_train import RdtTrainer
    args, kw = inputs(a, B, dev)
    kinds = ("tn", "gemm")
    make = lambda kind: lambda: RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision="bf16", attention_backward="mfma",
                                           weight_gradient=kind, device=dev)
    out = {"batch": B, "precision": "bf16", "attention_backward": "mfma", "parameters": params, "warmup": a.warmup, "timed_steps": a.steps}
    out.update(compare_steps(a, dev, args, kw, {kind: make(kind) for kind in kinds}))
    for kind in kinds:
        out[kind]["loss_decreases"] = bool(out[kind]["losses"][-1] < out[kind]["losses"][0])
    out["backward_tn_over_gemm"] = out["tn"]["backward_ms"]["median"] / out["gemm"]["backward_ms"]["median"]
    out["step_tn_over_gemm"] = out["tn"]["step_ms"]["median"] / out["gemm"]["step_ms"]["median"]
    out["backward_faster_than_gemm"] = bool(out["backward_tn_over_gemm"] < 1.0)
    out["weight_gradient_launches"] = weight_gradient_launches(a, c, B, dev)
    out["timing"] = STEP_TIMING
    return out


def small_batch_linear_launches(a, c, B, dev):
    """Device-event time of one hidden x hidden Linear at the step's row count (67 x batch), forward and data gradient, with and without the
    packed copy (routes asked from the library), back to back and alternating -> dict."""
    from vlatouch import ops
    from vlatouch.rdt_train import PackedScratch, gemm_small_packed
    D, M = c["hidden"], (c["horizon"] + 3) * B
    g = torch.Generator(device=dev).manual_seed(5)
    w = torch.randn(D, D, generator=g, device=dev) * 0.02
    x, bias = torch.randn(M, D, generator=g, device=dev).bfloat16(), torch.zeros(D, device=dev)
    forms = ops.refresh16(w, torch.bfloat16, ops.REFRESH16_FORMS)
    scratch = PackedScratch(D, dev)
    legs = {"forward": (forms["w16"], forms["wp"], bias), "data_gradient": (forms["w16t"], forms["wtp"], None)}
    out = {"M": M, "N": D, "K": D}
    for leg, (w16, wp, b) in legs.items():
        calls = {"gemm": lambda: ops.gemm(x, w16, b), "packed": lambda: gemm_small_packed(x, w16, wp, scratch, b)}
        routes = {"gemm": ops.gemm_route(ops.gemm_params(x, w16, b)[0]),
                  "packed": ops.gemm_route(ops.gemm_params(x, w16, b, wp=wp, sk_ws=scratch.sk_ws, sk_cnt=scratch.sk_cnt)[0])}
        ms = {"gemm": [], "packed": []}
        for n in range(3 + 15):
            for kind in (("gemm", "packed") if n % 2 == 0 else ("packed", "gemm")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                for _ in range(8):                      # eight launches back to back: one is below the resolution of an event pair
                    res = calls[kind]()
                e1.record()
                torch.cuda.synchronize(dev)
                if n >= 3:
                    ms[kind].append(e0.elapsed_time(e1) / 8)
        del res
        out[leg] = {"route": routes, "gemm_ms": _stats(ms["gemm"]), "packed_ms": _stats(ms["packed"]),
                    "packed_over_gemm": _stats(ms["packed"])["median"] / _stats(ms["gemm"])["median"]}
    out["timing"] = ("device events around eight back-to-back launches of one Linear (output allocation from the caching allocator included), divided "
                     "by eight; 3 warm-up + 15 timed, the two routes alternating; outside a step: the weights stay in L2 between the launches")
    return out


def small_batch_linear_run(a, c, sd, params, dev, B):
    """The bf16 step (attention_backward="mfma", weight_gradient="tn") under small_batch_linear="packed" and "gemm", alternating in this process
    at batch B, with the refresh phase of each timed alone by device events -> dict."""
    from vlatouch.rdt_train import RdtTrainer
    args, kw = inputs(a, B, dev)
    kinds = ("packed", "gemm")
    make = lambda kind: lambda: RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision="bf16", attention_backward="mfma",
                                           weight_gradient="tn", small_batch_linear=kind, device=dev)
    out = {"batch": B, "rows": (c["horizon"] + 3) * B, "precision": "bf16", "attention_backward": "mfma", "weight_gradient": "tn", "parameters": params,
           "warmup": a.warmup, "timed_steps": a.steps}
    refresh = {k: [] for k in kinds}
    offered = {}

    def each_step(kind, tr):                                  # the refresh alone, again, on the weights the step just wrote
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        tr._refresh16()
        e1.record()
        torch.cuda.synchronize(dev)
        refresh[kind].append(e0.elapsed_time(e1))
        if kind == "packed" and not offered and tr.packed is not None:
            tr.packed.log = []
            tr.get_loss(*args, **kw)
            routes = [r for _, _, r in tr.packed.log]
            offered.update(launches_offered_a_packed_copy=len(routes), of_them_on_pws=routes.count("PWS"),
                           weights_with_wp=len(tr.wp), weights_with_wtp=len(tr.wtp),
                           packed_copies_gib=sum(t.numel() * 2 for d in (tr.wp, tr.wtp) for t in d.values()) / 2 ** 30,
                           splitk_scratch_gib=tr.packed.sk_ws.numel() * 4 / 2 ** 30)
            tr.packed.log = None

    out.update(compare_steps(a, dev, args, kw, {kind: make(kind) for kind in kinds}, each_step))
    for kind in kinds:
        out[kind]["loss_decreases"] = bool(out[kind]["losses"][-1] < out[kind]["losses"][0])
        out[kind]["refresh_ms"] = _stats(refresh[kind])
    out["packed"].update(offered)
    sp, sg = out["packed"]["step_ms"], out["gemm"]["step_ms"]
    out["step_packed_over_gemm"] = sp["median"] / sg["median"]
    spread = max(sp["max"] - sp["min"], sg["max"] - sg["min"])
    out["step_gain_ms"], out["larger_min_max_spread_ms"] = sg["median"] - sp["median"], spread
    out["step_faster_than_gemm_by_more_than_the_spread"] = bool(sg["median"] - sp["median"] > spread)
    rp, rg = out["packed"]["refresh_ms"], out["gemm"]["refresh_ms"]
    out["refresh_packed_over_gemm"] = rp["median"] / rg["median"]
    out["refresh_no_slower_than_cast_plus_transpose"] = bool(rp["median"] - rg["median"] <= max(rp["max"] - rp["min"], rg["max"] - rg["min"]))
    if out["rows"] <= 512:
        out["linear_launches"] = small_batch_linear_launches(a, c, B, dev)
    out["timing"] = STEP_TIMING + "; refresh_ms: device events around one _refresh16() call over all weights, after every timed step"
    return out


def fp16_attention_launches(a, c, B, dev):
    """Device-event time of the attention-backward launches alone in fp16 and in bf16, "wave" and "mfma", alternating, at the trainer's packed
    layouts and the three attention shapes of the step -> dict."""
    from vlatouch.rdt_train import attention_bwd
    H, N = c["heads"], c["horizon"] + 3
    g = torch.Generator(device=dev).manual_seed(5)
    out = {}
    for name, Nk, cross in (("image_cross_attention", a.img_len, True), ("language_cross_attention", a.lang_len, True), ("self_attention", N, False)):
        views = {}
        for dt in (torch.float16, torch.bfloat16):
            rn = lambda *s: (0.5 * torch.randn(*s, generator=g, device=dev)).to(dt)
            views[dt] = (*packed_attention_views(B, N, Nk, H, cross, dt, rn, dev), rn(B, N, H, 64))
        km = torch.ones(B, Nk, dtype=torch.uint8, device=dev) if name == "language_cross_attention" else None
        combos = [(dt, kind) for kind in ("mfma", "wave") for dt in (torch.float16, torch.bfloat16)]
        ms = {cb: [] for cb in combos}
        for n in range(2 + 7):
            for dt, kind in (combos if n % 2 == 0 else combos[::-1]):
                (q, k, v), (dq, dk, dv), do = views[dt]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                attention_bwd(q, k, v, do, dq, dk, dv, kmask=km, kernel=kind)
                e1.record()
                torch.cuda.synchronize(dev)
                if n >= 2:
                    ms[(dt, kind)].append(e0.elapsed_time(e1))
        rec = {"Nq": N, "Nk": Nk}
        for kind in ("mfma", "wave"):
            f, b = _stats(ms[(torch.float16, kind)]), _stats(ms[(torch.bfloat16, kind)])
            rec[kind] = {"fp16_ms": f, "bf16_ms": b, "fp16_over_bf16": f["median"] / b["median"]}
        out[name] = rec
    out["timing"] = "device events around one attention_bwd call (workspace allocation from the caching allocator included), 2 warm-up + 7 timed, the four (dtype, kernel) pairs alternating"
    return out


def fp16_run(a, c, sd, params, dev, B):
    """The fp16 step (dynamic loss scaling) beside the bf16 step, alternating in this process at batch B, both under a.attention_backward and
    a.optimizer -> dict with the phases, the losses and the scale trajectory."""
    from vlatouch.rdt_train import RdtTrainer
    args, kw = inputs(a, B, dev)
    make = lambda kind, **extra: lambda: RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision=kind,
                                                    attention_backward=a.attention_backward, optimizer=a.optimizer, device=dev, **extra)
    traj = []                                                # fp16: (scale, step skipped, steps skipped so far) after every timed step
    each_step = lambda kind, tr: traj.append((tr.loss_scale_value, bool(tr.last_step_skipped), tr.skipped_steps)) if kind == "fp16" else None
    out = {"batch": B, "attention_backward": a.attention_backward, "optimizer": a.optimizer, "parameters": params, "warmup": a.warmup, "timed_steps": a.steps}
    out.update(compare_steps(a, dev, args, kw, {"fp16": make("fp16", loss_scale="dynamic"), "bf16": make("bf16")}, each_step))
    out["fp16"].update(loss_scale_after_each_step=[t[0] for t in traj], step_skipped=[t[1] for t in traj], skipped_steps_warmup_included=traj[-1][2])
    for n in ("forward_ms", "backward_ms", "clip_adamw_ema_ms", "step_ms"):
        out[f"{n[:-3]}_fp16_over_bf16"] = out["fp16"][n]["median"] / out["bf16"][n]["median"]
        out[f"{n[:-3]}_fp16_minus_bf16_ms"] = out["fp16"][n]["median"] - out["bf16"][n]["median"]
    out["attention_backward_launches"] = fp16_attention_launches(a, c, B, dev)
    out["timing"] = STEP_TIMING
    return out


def data_parallel_run(a, c, sd, params, dev):
    """The grouped step (world size 1 over RCCL) beside the ungrouped one, and the exchange launches alone, at batch 4 -> dict."""
    import torch.distributed as dist
    from vlatouch import _lib as L
    from vlatouch import train as T
    from vlatouch.rdt_train import RdtTrainer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"), os.environ.setdefault("MASTER_PORT", "29571")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    G = dist.group.WORLD
    B, comm, timed = 4, a.data_parallel, 21
    sync = lambda: torch.cuda.synchronize(dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    args, kw = inputs(a, B, dev)
    mk = lambda **k: RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision="bf16", attention_backward="mfma", device=dev, **k)
    trs = {"grouped": mk(process_group=G, comm_dtype=comm), "ungrouped": mk()}
    kinds = tuple(trs)
    for _ in range(max(1, a.warmup)):
        for kind in kinds:
            trs[kind].train_step(*args, **kw)
    sync()
    step = {k: [] for k in kinds}
    losses = {k: [] for k in kinds}
    for n in range(timed):
        for kind in (kinds if n % 2 == 0 else kinds[::-1]):      # who goes first alternates
            e0, e1 = ev(), ev()
            sync()
            e0.record()
            loss = trs[kind].train_step(*args, **kw)
            e1.record()
            sync()
            step[kind].append(e0.elapsed_time(e1))
            losses[kind].append(float(loss))
    # the exchange's launches alone, on the grouped trainer's table with the last step's fresh gradients
    tr = trs["grouped"]
    tr.get_loss(*args, **kw)
    tab, nt, chunks = tr._table()
    fresh = torch.tensor([tr._fresh_grad(name).data_ptr() for name in tr.p], dtype=torch.int64).to(dev)
    buf16 = tr._comm if tr._comm is not None else torch.zeros(chunks * T.MT_CHUNK, dtype=torch.bfloat16, device=dev)
    lib, sp = L.lib(), lambda: L.stream_ptr(dev)
    launches = {
        "fold_store": lambda: L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(fresh), nt, chunks, 1.0, 0, sp()), "vt_grad_accum_multi"),
        "fold_pack_store": lambda: L.check(lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(fresh), nt, chunks, 1.0, 0, L.ptr(buf16), sp()), "vt_grad_fold_pack_multi"),
        "fold_add": lambda: L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(fresh), nt, chunks, 0.5, 1, sp()), "vt_grad_accum_multi"),
        "fold_pack_add": lambda: L.check(lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(fresh), nt, chunks, 0.5, 1, L.ptr(buf16), sp()), "vt_grad_fold_pack_multi"),
        "unpack": lambda: L.check(lib.vt_grad_unpack_multi(L.ptr(tab), L.ptr(buf16), nt, chunks, sp()), "vt_grad_unpack_multi"),
        "all_reduce": lambda: tr._all_reduce(tr._comm if comm == "bf16" else tr._arena),
    }
    ms = {k: [] for k in launches}
    order = tuple(launches)
    for n in range(2 + timed):
        for name in (order if n % 2 == 0 else order[::-1]):
            e0, e1 = ev(), ev()
            sync()
            e0.record()
            launches[name]()
            e1.record()
            sync()
            if n >= 2:
                ms[name].append(e0.elapsed_time(e1))
    elems = chunks * T.MT_CHUNK
    moved = {"fold_store": 8.0 * params, "fold_add": 12.0 * params, "fold_pack_store": 4.0 * params + 2.0 * elems, "fold_pack_add": 8.0 * params + 2.0 * elems,
             "unpack": 6.0 * params, "all_reduce": (2.0 if comm == "bf16" else 4.0) * elems}
    out = {"batch": B, "precision": "bf16", "attention_backward": "mfma", "comm_dtype": comm, "world_size": 1, "backend": dist.get_backend(),
           "parameters": params, "arena_elements": elems, "comm_bucket_bytes": tr.comm_bucket_bytes, "warmup": a.warmup, "timed": timed}
    for name, v in ms.items():
        st = _stats(v)
        if name != "all_reduce":
            rate = moved[name] / (st["median"] / 1e3)
            st.update(bytes_moved=moved[name], bytes_per_s=rate, share_of_hbm_spec=rate / HBM_SPEC_BYTES_PER_S, share_of_float4_copy_rate=rate / HBM_COPY_BYTES_PER_S)
        else:
            st.update(buffer_bytes=moved[name], note="world size 1: nothing crosses a link; this is RCCL's launch and its pass over the buffer")
        out[f"{name}_ms"] = st
    for mode in ("store", "add"):
        f, fp = out[f"fold_{mode}_ms"], out[f"fold_pack_{mode}_ms"]
        margin = max(f["max"] - f["min"], fp["max"] - fp["min"])
        out[f"fold_pack_{mode}_over_fold"] = fp["median"] / f["median"]
        out[f"fold_pack_{mode}_no_longer_than_fold"] = bool(fp["median"] <= f["median"] + margin)
        out[f"fold_pack_{mode}_margin_ms"] = margin
    for kind in kinds:
        out[f"step_{kind}_ms"] = _stats(step[kind])
        out[f"losses_{kind}"] = losses[kind]
    out["step_grouped_over_ungrouped"] = out["step_grouped_ms"]["median"] / out["step_ungrouped_ms"]["median"]
    out["scaling"] = "No scaling number can be produced on a one-GPU box; the all-reduce is not overlapped with the backward."
    out["timing"] = "device events between two device synchronisations; the trainers, and the launches, alternate and swap who goes first"
    dist.destroy_process_group()
    return out


SECTIONS = ("accumulation", "adamw8bit", "attention_backward_mfma", "data_parallel", "fp16", "small_batch_linear_packed", "weight_gradient_tn")      # the modes' keys of --out


def merge_record(path, key, section, sub=None) -> None:
    """Set `key` (or `key`[`sub`]) of the JSON record at `path` to `section`, keeping what else the file holds.  key=None is the default
    run: `section`'s keys become the record's and only the other modes' SECTIONS stay."""
    rec = {}
    if os.path.exists(path):
        with open(path) as f:
            rec = json.load(f)
    if key is None:
        rec = dict(section, **{k: rec[k] for k in SECTIONS if k in rec})
    elif sub is None:
        rec[key] = section
    else:
        rec.setdefault(key, {})[sub] = section
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", path)


def per_batch(run, a, *rest) -> list:
    """run(a, *rest, B) for every --batch size, each result printed as it arrives."""
    runs = []
    for B in a.batch:
        runs.append(run(a, *rest, B))
        print(json.dumps(runs[-1]))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp16"],
                    help="fp16 measures the fp16 step (dynamic loss scaling) beside the bf16 step in one process and adds it to --out")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--img-len", type=int, default=4374)
    ap.add_argument("--lang-len", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=None, help="timed steps: 10, or 21 with --attention-backward mfma")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--accum", type=int, default=1, help="gradient_accumulation_steps; > 1 measures the accumulated step and adds it to --out")
    ap.add_argument("--optimizer", default="adamw", choices=["adamw", "adamw8bit"],
                    help="adamw8bit measures the 8-bit optimizer phase beside the 32-bit one and adds it to --out")
    ap.add_argument("--attention-backward", default="wave", choices=["wave", "mfma"],
                    help="mfma measures the bf16 step with the MFMA attention backward beside the wave kernels and adds it to --out")
    ap.add_argument("--step-attention-backward", default="wave", choices=["wave", "mfma"],
                    help="the attention backward of the default run's trainer (a kernel trace of the step under \"mfma\" uses this)")
    ap.add_argument("--weight-gradient", default="gemm", choices=["gemm", "tn"],
                    help="tn measures the bf16 step with the transpose-free weight-gradient GEMM beside the gemm path and adds it to --out")
    ap.add_argument("--step-weight-gradient", default="gemm", choices=["gemm", "tn"],
                    help="the weight gradient of the default run's trainer (a kernel trace of the step under \"tn\" uses this)")
    ap.add_argument("--small-batch-linear", default="gemm", choices=["gemm", "packed"],
                    help="packed measures the bf16 mfma / tn step with the packed small-batch Linears beside the gemm path and adds it to --out")
    ap.add_argument("--step-small-batch-linear", default="gemm", choices=["gemm", "packed"],
                    help="the small-batch Linear of the default run's trainer (a kernel trace of the step under \"packed\" uses this)")
    ap.add_argument("--data-parallel", default=None, choices=["fp32", "bf16"],
                    help="measures the data-parallel step over an RCCL group of world size 1 beside the ungrouped one and adds it to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdt_train_bench.json"))
    a = ap.parse_args()
    if a.attention_backward == "mfma" and a.precision == "fp32":
        ap.error("--attention-backward mfma measures a 16-bit step")
    if "tn" in (a.weight_gradient, a.step_weight_gradient) and a.precision == "fp32":
        ap.error("weight_gradient tn is a 16-bit kernel")
    if "packed" in (a.small_batch_linear, a.step_small_batch_linear) and a.precision == "fp32":
        ap.error("small_batch_linear packed is a 16-bit path")
    if a.steps is None:
        a.steps = 21 if a.attention_backward == "mfma" or a.weight_gradient == "tn" or a.precision == "fp16" or a.small_batch_linear == "packed" else 10
    from vlatouch.rdt_train import RdtTrainer
    dev = torch.device("cuda:0")
    c = dict(hidden=a.hidden, depth=a.depth, heads=a.hidden // 64, horizon=64, action_dim=128, lang_token_dim=4096, img_token_dim=1152,
             state_token_dim=128, max_lang_cond_len=1024, img_cond_len=a.img_len)
    sd = synth.fill_state_dict_device(synth.rdt_runner_shapes(**c), dev, torch.float32, seed=7)
    params = sum(v.numel() for v in sd.values())
    meta = dict(config=c, lang_len=a.lang_len, lr=a.lr, device=torch.cuda.get_device_name(dev))
    if a.precision == "fp16":
        return merge_record(a.out, "fp16", dict(runs=per_batch(fp16_run, a, c, sd, params, dev), **meta))
    if a.data_parallel is not None:
        section = dict(data_parallel_run(a, c, sd, params, dev), **meta)
        print(json.dumps(section))
        return merge_record(a.out, "data_parallel", section, sub=a.data_parallel)
    if a.small_batch_linear == "packed":
        runs = per_batch(small_batch_linear_run, a, c, sd, params, dev)
        return merge_record(a.out, "small_batch_linear_packed", dict(runs=runs, **meta))
    if a.weight_gradient == "tn":
        runs = per_batch(weight_gradient_run, a, c, sd, params, dev)
        return merge_record(a.out, "weight_gradient_tn", dict(runs=runs, **meta, backward_faster_than_gemm_at_every_batch=all(r["backward_faster_than_gemm"] for r in runs)))
    if a.attention_backward == "mfma":
        runs = per_batch(attention_run, a, c, sd, params, dev)
        return merge_record(a.out, "attention_backward_mfma", dict(runs=runs, **meta, backward_faster_than_wave_at_every_batch=all(r["backward_faster_than_wave"] for r in runs)))
    if a.optimizer == "adamw8bit" or a.accum > 1:
        key, run = ("adamw8bit", optimizer_run) if a.optimizer == "adamw8bit" else ("accumulation", accum_run)
        section = dict(run(a, c, sd, params, dev), **meta)
        print(json.dumps(section))
        return merge_record(a.out, key, section)
    rec = {"config": c, "precision": a.precision, "parameters": params, "lang_len": a.lang_len, "warmup": a.warmup, "steps": a.steps, "lr": a.lr,
           "device": torch.cuda.get_device_name(dev), "runs": []}
    if a.step_attention_backward != "wave":
        rec["attention_backward"] = a.step_attention_backward
    if a.step_weight_gradient != "gemm":
        rec["weight_gradient"] = a.step_weight_gradient
    if a.step_small_batch_linear != "gemm":
        rec["small_batch_linear"] = a.step_small_batch_linear
    for B in a.batch:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        tr = RdtTrainer(sd, heads=c["heads"], horizon=64, action_dim=128, lr=a.lr, precision=a.precision, attention_backward=a.step_attention_backward,
                        weight_gradient=a.step_weight_gradient, small_batch_linear=a.step_small_batch_linear, device=dev)
        args, kw = inputs(a, B, dev)
        t_f = t_fb = t_o = 0.0
        losses = []
        for n in range(a.warmup + a.steps):
            f, fb, o, loss = timed_step(tr, args, kw, dev)
            if n >= a.warmup:
                t_f, t_fb, t_o = t_f + f, t_fb + fb, t_o + o
                losses.append(float(loss))
        k = 1.0 / a.steps
        flops = 3 * 2 * forward_macs(c, B, a.lang_len)
        step_ms = (t_fb + t_o) * k
        run = {"batch": B, "forward_ms": t_f * k, "backward_ms": (t_fb - t_f) * k, "clip_adamw_ema_ms": t_o * k, "step_ms": step_ms,
               "samples_per_s": B / (step_ms / 1e3), "peak_memory_gib": torch.cuda.max_memory_allocated(dev) / 2 ** 30,
               "algorithmic_tflop_per_step": flops / 1e12, "whole_step_tflops": flops / (step_ms / 1e3) / 1e12,
               "losses": losses, "loss_decreases": bool(losses[-1] < losses[0]), "grad_norm_last": float(tr.grad_norm),
               "share_of_bf16_mfma_peak": flops / (step_ms / 1e3) / PEAK_BF16_FLOPS if a.precision == "bf16" else None}
        del tr
        if B == a.batch[0]:
            run["torch_autograd_yardstick"] = "not measured: --no-yardstick" if a.no_yardstick else yardstick(sd, c, args, kw, dev)
            if isinstance(run["torch_autograd_yardstick"], dict):
                run["torch_autograd_yardstick"]["ratio_torch_over_this"] = run["torch_autograd_yardstick"]["fwd_bwd_ms"] / ((t_fb) * k)
        print(json.dumps(run))
        rec["runs"].append(run)
    merge_record(a.out, None, rec)                # the other modes' sections are not this run's to drop


if __name__ == "__main__":
    main()
