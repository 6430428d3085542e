"""RDT fine-tuning step on the MI355X: loss, backward, gradient clipping, AdamW, EMA.

Replaces, for one optimisation step, what the reference does with torch autograd (VLA/train/train.py:404-448):
  * `RDTRunner.compute_loss` (models/rdt_runner.py:168-222): DDPM forward process, state ‖ noisy-action ‖ mask tokens, the three adaptors,
    `RDT.forward` (models/rdt/model.py:126-165) and the MSE against the action chunk (`sample`) or the noise (`epsilon`);
  * `loss.backward()` through the final layer, `depth` blocks (self-attention, cross-attention alternating language (masked) / image, FFN, the
    three RMSNorms, the q / k head norms), the token assembly, the timestep / frequency embedders, the position embeddings, the adaptors;
  * `accelerator.clip_grad_norm_` (train.py:440-442), `torch.optim.AdamW` (train.py:229-237) and `EMAModel.step` (models/ema_model.py).

Design: fp32 master parameters in the reference's state-dict key layout (`model.*`, `lang_adaptor.*`, `img_adaptor.*`, `state_adaptor.*`);
every Linear — forward, data gradient, weight gradient — is a vt_gemm call in exact-fp32 MFMA mode (vlatouch.train.gemm: deterministic
split-K for the long reductions), the attention forward is vt_attention, the norms vt_rownorm / vt_headnorm, and everything autograd would
add is csrc/vt_train_rdt.hip.  The forward keeps what the backward reads (block inputs, pre-norm q / k, normed q / k / v, attention outputs,
FFN pre-activations); the image K / V of the odd blocks are kept, not recomputed.  Orchestration is host Python like the reference's loop.
`precision="fp32"` is the parity mode.  `precision="fp16"` (with `loss_scale=`) is the bf16 mode on IEEE half with GradScaler's dynamic loss
scaling and step skipping (the reference's --mixed_precision fp16; LossScaler below).  `precision="bf16"` is the reference's execution dtype: bf16 copies of the Linear weights (and of their
transposes) refreshed after each optimizer step, bf16 activations, activation gradients and MFMA operands, fp32 accumulators, fp32 master
weights / gradients / moments / EMA (what DeepSpeed's bf16 mode keeps); norm gains, biases and position embeddings are read in fp32.

Data parallelism (`process_group=`; the reference's `accelerate launch` with DeepSpeed ZeRO-2, finetune.sh) replicates all state: every rank
folds its micro-batches, scaled by 1 / (k W), into one fp32 gradient arena laid out as the multi-tensor table implies, the arena is summed over
the ranks once per optimizer step (fp32, or bf16 through vt_grad_fold_pack_multi / vt_grad_unpack_multi), and clip, AdamW and EMA then run
identically everywhere.  Nothing is sharded and the all-reduce is not overlapped with the backward.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from collections import OrderedDict
from typing import Dict, List, Optional

import torch

from . import _lib as L
from . import adam8
from . import ops
from . import train as T
from .train import _empty, _sp

F32 = torch.float32
LR_SCHEDULERS = ("constant", "constant_with_warmup")
PREDICTION_TYPES = ("sample", "epsilon")
OPTIMIZERS = ("adamw", "adamw8bit")
COMM_DTYPES = ("fp32", "bf16")
PRECISIONS = ("fp32", "bf16", "fp16")
LOSS_SCALE_DEFAULTS = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)      # torch.amp.GradScaler's


# ---------------------------------------------------------------------------------------------- host-side schedules
def alphas_cumprod(num_train_timesteps: int, beta_schedule: str) -> torch.Tensor:
    """DDPMScheduler's fp32 table of prod(1 - beta) over the published beta schedules (vlatouch.dpm._betas)."""
    from .dpm import _betas
    return torch.cumprod(1.0 - torch.from_numpy(_betas(num_train_timesteps, beta_schedule)).to(F32), dim=0)


def ema_decay(optimization_step: int, update_after_step: int = 0, inv_gamma: float = 1.0, power: float = 2 / 3, min_value: float = 0.0,
              max_value: float = 0.9999) -> float:
    """EMAModel.get_decay (models/ema_model.py:45-55)."""
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    return max(min_value, min(1 - (1 + step / inv_gamma) ** -power, max_value))


def lr_at(base: float, scheduler: str, steps_done: int, warmup: int) -> float:
    """diffusers.optimization.get_scheduler's `constant` and `constant_with_warmup` multipliers after `steps_done` scheduler steps."""
    if scheduler == "constant":
        return base
    if scheduler == "constant_with_warmup":
        return base * (min(1.0, steps_done / max(1, warmup)))
    raise ValueError(f"lr_scheduler must be one of {LR_SCHEDULERS}, got {scheduler!r}")


# ---------------------------------------------------------------------------------------------- loss scaling (host)
def _f32(x: float) -> float:
    """x rounded to fp32: GradScaler keeps its scale in an fp32 tensor, so every product below is an fp32 one."""
    return float(torch.tensor(x, dtype=torch.float64).to(F32))


def inv_scale(scale: float) -> float:
    """float(1 / double(S)), as GradScaler._unscale_grads_ forms it (`self._scale.double().reciprocal().float()`)."""
    return _f32(1.0 / _f32(scale))                     # the scale is an fp32 tensor there


def loss_scale_settings(loss_scale) -> dict:
    """RdtTrainer's `loss_scale` argument -> {init_scale, growth_factor, backoff_factor, growth_interval, dynamic}; ValueError for anything
    else.  "dynamic": GradScaler's defaults; a dict: any of its four keys over the defaults; a positive finite number: a static scale (it
    never changes, an overflow still skips the step)."""
    out = dict(LOSS_SCALE_DEFAULTS, dynamic=True)
    if isinstance(loss_scale, str):
        if loss_scale != "dynamic":
            raise ValueError(f"loss_scale must be 'dynamic', a dict of {sorted(LOSS_SCALE_DEFAULTS)} or a positive finite number, got {loss_scale!r}")
    elif isinstance(loss_scale, dict):
        unknown = sorted(set(loss_scale) - set(LOSS_SCALE_DEFAULTS))
        if unknown:
            raise ValueError(f"loss_scale: unknown keys {unknown} (known: {sorted(LOSS_SCALE_DEFAULTS)})")
        out.update(loss_scale)
    elif isinstance(loss_scale, (int, float)) and not isinstance(loss_scale, bool):
        out.update(init_scale=loss_scale, dynamic=False)
    else:
        raise ValueError(f"loss_scale must be 'dynamic', a dict of {sorted(LOSS_SCALE_DEFAULTS)} or a positive finite number, got {loss_scale!r}")
    for key in ("init_scale", "growth_factor", "backoff_factor"):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"loss_scale: {key} must be a finite number, got {v!r}")
        out[key] = float(v)
    if not out["init_scale"] > 0.0 or not math.isfinite(_f32(out["init_scale"])) or _f32(out["init_scale"]) == 0.0:
        raise ValueError(f"loss_scale: the scale must be positive and finite in fp32, got {out['init_scale']!r}")
    if not out["growth_factor"] > 1.0:
        raise ValueError(f"loss_scale: growth_factor must be > 1, got {out['growth_factor']!r}")
    if not 0.0 < out["backoff_factor"] < 1.0:
        raise ValueError(f"loss_scale: backoff_factor must be in (0, 1), got {out['backoff_factor']!r}")
    gi = out["growth_interval"]
    if isinstance(gi, bool) or not isinstance(gi, (int, float)) or int(gi) != gi or gi < 1:
        raise ValueError(f"loss_scale: growth_interval must be an integer >= 1, got {gi!r}")
    out["growth_interval"] = int(gi)
    return out


class LossScaler:
    """torch.amp.GradScaler's scale arithmetic on the host (torch/amp/grad_scaler.py `update`, ATen _amp_update_scale_), in fp32 like its
    scale tensor: an overflow multiplies the scale by backoff_factor and clears the tracker; a clean step advances the tracker and, when it
    reaches growth_interval, multiplies the scale by growth_factor (unless that would leave fp32's range) and clears it.  No floor.  A static
    scaler (`dynamic` False) counts the same but never changes the scale.  tests/loss_scale_ref.py pins this against torch."""

    def __init__(self, settings: dict):
        self.settings = dict(settings)
        self.reset()

    def reset(self) -> None:
        self.scale = _f32(self.settings["init_scale"])
        self.growth_tracker = 0
        self.skipped_steps = 0
        self.skipped_nonfinite_loss = 0

    def update(self, found_inf: bool) -> None:
        st = self.settings
        if found_inf:
            self.skipped_steps += 1
            self.growth_tracker = 0
            if st["dynamic"]:
                self.scale = _f32(self.scale * _f32(st["backoff_factor"]))
            return
        self.growth_tracker += 1
        if self.growth_tracker == st["growth_interval"]:
            self.growth_tracker = 0
            grown = _f32(self.scale * _f32(st["growth_factor"]))
            if st["dynamic"] and math.isfinite(grown):
                self.scale = grown

    def state(self) -> dict:
        return dict(scale=self.scale, growth_tracker=self.growth_tracker, skipped_steps=self.skipped_steps,
                    skipped_nonfinite_loss=self.skipped_nonfinite_loss, settings=dict(self.settings))

    def load_state(self, st: dict) -> None:
        self.settings = loss_scale_settings({k: st["settings"][k] for k in LOSS_SCALE_DEFAULTS})
        self.settings["dynamic"] = bool(st["settings"]["dynamic"])
        self.scale, self.growth_tracker = _f32(st["scale"]), int(st["growth_tracker"])
        self.skipped_steps, self.skipped_nonfinite_loss = int(st["skipped_steps"]), int(st["skipped_nonfinite_loss"])


# ---------------------------------------------------------------------------------------------- primitive wrappers
# Activations are fp32, bf16 or fp16 tensors; every wrapper takes the dtype from its operands.  Sums (weight / bias / gain gradients) are always fp32.
def _dt(t: torch.Tensor) -> int:
    return L.dt_code(t.dtype)


def transpose_pad(x2d: torch.Tensor) -> torch.Tensor:
    """[M, N] -> [N, Mp] with zero padding, Mp = M rounded up to the GEMM's reduction alignment (4 fp32, 8 bf16 / fp16): the operand form of a
    weight-gradient product (reduction over the M token rows) and of a data-gradient product (W -> W^T)."""
    M, N = x2d.shape
    al = 4 if x2d.dtype == F32 else 8
    Mp = (M + al - 1) // al * al
    out = torch.empty((N, Mp), dtype=x2d.dtype, device=x2d.device)
    L.check(L.lib().vt_transpose_pad(L.ptr(x2d), L.ptr(out), _dt(x2d), M, N, Mp, _sp(x2d.device)), "vt_transpose_pad")
    return out


def colsum(x2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    M, N = x2d.shape
    if out is None:
        out = _empty((N,), x2d.device)
    if x2d.dtype == F32:
        L.check(L.lib().vt_colsum(L.ptr(x2d), x2d.stride(0), L.ptr(out), M, N, 0, _sp(x2d.device)), "vt_colsum")
    else:
        L.check(L.lib().vt_colsum_dt(L.ptr(x2d), _dt(x2d), x2d.stride(0), L.ptr(out), M, N, _sp(x2d.device)), "vt_colsum_dt")
    return out


def add_(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if a.dtype == F32:
        return T.add_(a, b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
    L.check(L.lib().vt_add_dt(L.ptr(a), L.ptr(b), a.numel(), _dt(a), _sp(a.device)), "vt_add_dt")
    return a


def copy_cols(src: torch.Tensor, off: int, dst: torch.Tensor, doff: int, cols: int) -> None:
    """dst[:, doff:doff+cols] = src[:, off:off+cols] on 2-D views of row-contiguous buffers of one dtype."""
    if src.dtype == F32:
        return T.copy_cols(src, off, dst, doff, cols)
    assert src.dtype == dst.dtype
    L.check(L.lib().vt_copy_cols_dt(L.ptr(src), src.stride(0), off, L.ptr(dst), dst.stride(0), doff, src.shape[0], cols, _dt(src), _sp(src.device)),
            "vt_copy_cols_dt")


WEIGHT_GRADIENTS = ("gemm", "tn")
SMALL_BATCH_LINEARS = ("gemm", "packed")
PACKED_MAX_ROWS = 512      # launches above it never get a packed pointer: the dispatcher would move them to another tile


class PackedScratch:
    """What the small-batch packed Linears of one trainer share: the split-K scratch of the small-M tile (fp32 slabs and zeroed, self-resetting
    ticket counters, sized by the library as the inference engine's workspace sizes them) and, when `log` is a list, a record
    (tag, rows, route) of every launch that was offered a packed copy."""

    def __init__(self, max_cols: int, device):
        lib = L.lib()
        self.sk_ws = torch.empty(max(1, lib.vt_splitk_slab_bytes(PACKED_MAX_ROWS, max_cols) // 4), dtype=F32, device=device)
        self.sk_cnt = torch.zeros(lib.vt_splitk_counters(), dtype=torch.int32, device=device)
        self.log: Optional[list] = None


def gemm_small_packed(x: torch.Tensor, w: torch.Tensor, wp: Optional[torch.Tensor], scratch: Optional[PackedScratch], bias=None, residual=None,
                      tag: str = "") -> torch.Tensor:
    """ops.gemm(x, w, bias, residual=residual), on the small-M packed-weight tile (csrc/vt_gemm_pws.hip) when `wp`, the fragment-packed copy of
    w, exists, x has at most PACKED_MAX_ROWS rows and the library's dispatcher then routes the block there (ops.gemm_route on the block: the
    predicate is not restated here).  Any other launch goes without the packed pointer, exactly as ops.gemm sends it."""
    if wp is not None and scratch is not None and x.shape[0] <= PACKED_MAX_ROWS:
        p, out = ops.gemm_params(x, w, bias, residual=residual, wp=wp, sk_ws=scratch.sk_ws, sk_cnt=scratch.sk_cnt)
        route = ops.gemm_route(p)
        if scratch.log is not None:
            scratch.log.append((tag, x.shape[0], route))
        if route == "PWS":
            return ops.gemm_launch(p, out)
    return ops.gemm(x, w, bias, residual=residual)


def weight_grad_tn(dy: torch.Tensor, x: torch.Tensor, *, bias: bool = True):
    """dy [M, N], x [M, K], both bf16 or both fp16, unit inner stride and row strides in multiples of 8 (column slices are read in place)
    -> (dw [N, K] fp32 = dy^T x, db [N] fp32 = the column sums of dy, or None without `bias`): vt_gemm_tn (csrc/vt_gemm_tn.hip), one launch with
    both operands read transposed out of LDS, plus the sum over the row splits where vt_gemm_tn_plan cuts the rows.  A shape or dtype the
    kernel does not take raises, nothing falls back."""
    if dy.dtype != x.dtype or dy.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"weight_grad_tn takes two bf16 or two fp16 tensors, got {dy.dtype} and {x.dtype}")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0] or dy.stride(1) != 1 or x.stride(1) != 1:
        raise ValueError(f"weight_grad_tn: dy [M, N] and x [M, K] with unit inner stride, got {tuple(dy.shape)} and {tuple(x.shape)}")
    (M, N), K = dy.shape, x.shape[1]
    plan = L.GemmTnPlan()
    if L.lib().vt_gemm_tn_plan(M, N, K, C.byref(plan)) != 0:
        raise ValueError(f"weight_grad_tn does not take M={M}, N={N}, K={K}: {L.lib().vt_last_error().decode()}")
    dw, db = _empty((N, K), dy.device), (_empty((N,), dy.device) if bias else None)
    ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=dy.device) if plan.ws_bytes else None
    L.check(L.lib().vt_gemm_tn(L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0), _dt(dy), M, N, K, L.ptr(dw), L.ptr(db), L.ptr(ws), plan.ws_bytes,
                               _sp(dy.device)), "vt_gemm_tn")
    return dw, db


def linear_bwd(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, need_dx: bool = True, wt: Optional[torch.Tensor] = None, kernel: str = "gemm",
               wtp: Optional[torch.Tensor] = None, scratch: Optional[PackedScratch] = None, tag: str = ""):
    """y = x w^T + b -> (dx | None, dw fp32, db fp32).  fp32: exact-fp32 MFMA with the deterministic split-K of vlatouch.train.gemm;
    bf16 operands (w, or its cached transpose wt, in bf16): bf16 MFMA with fp32 accumulation, dx rounded to bf16, dw written in fp32.
    kernel="tn" (16-bit operands only) forms dw and db in one weight_grad_tn call instead of two transposes, a GEMM and a column sum; dx is the
    same launch either way.  wtp (with wt and scratch): the fragment-packed copy of wt, which sends a dx of few rows to the small-M packed tile
    (gemm_small_packed)."""
    if kernel not in WEIGHT_GRADIENTS:
        raise ValueError(f"linear_bwd: kernel must be one of {WEIGHT_GRADIENTS}, got {kernel!r}")
    if x.dtype == F32:
        if kernel == "tn":
            raise ValueError("linear_bwd: kernel='tn' is a 16-bit kernel, got fp32 operands")
        dx = T.gemm(dy, T.transpose(w)) if need_dx else None
        return dx, T.gemm(transpose_pad(dy), transpose_pad(x)), colsum(dy)
    dx = gemm_small_packed(dy, wt if wt is not None else transpose_pad(w), wtp if wt is not None else None, scratch, tag=tag) if need_dx else None
    if kernel == "tn":
        return (dx, *weight_grad_tn(dy, x))
    return dx, ops.gemm(transpose_pad(dy), transpose_pad(x), out_dtype=F32), colsum(dy)


def act(x: torch.Tensor, kind: int, dy: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty_like(x)
    L.check(L.lib().vt_act_bwd(L.ptr(x), L.ptr(dy), L.ptr(out), x.numel(), kind, _dt(x), _sp(x.device)), "vt_act_bwd")
    return out


def rmsnorm_bwd(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, eps: float, mode: int):
    M, D = x.shape
    dx, dyxr = torch.empty_like(x), _empty((M, D), x.device)
    L.check(L.lib().vt_rmsnorm_bwd(L.ptr(x), L.ptr(w), L.ptr(dy), L.ptr(dx), L.ptr(dyxr), M, D, eps, mode, _dt(x), _sp(x.device)), "vt_rmsnorm_bwd")
    return dx, T.colsum(dyxr)


def headnorm_bwd_(x: torch.Tensor, dy: torch.Tensor, heads: int, w: torch.Tensor, eps: float, mode: int) -> torch.Tensor:
    """x (pre-norm), dy: 2-D views [tokens, heads * 64] of row-strided buffers; dy becomes dx; -> d w [64]."""
    tokens = x.shape[0]
    assert x.shape == dy.shape == (tokens, heads * 64) and x.stride(1) == 1 and dy.stride(1) == 1 and x.dtype == dy.dtype
    part = _empty(((tokens * heads + 63) // 64, 64), x.device)
    L.check(L.lib().vt_headnorm_bwd(L.ptr(x), x.stride(0), L.ptr(dy), dy.stride(0), heads, tokens, L.ptr(w), L.ptr(part), eps, mode, _dt(x),
                                    _sp(x.device)), "vt_headnorm_bwd")
    return T.colsum(part)


ATTENTION_BACKWARDS = ("wave", "mfma")


def attention_bwd(q, k, v, do, dq, dk, dv, *, kmask: Optional[torch.Tensor] = None, scale: Optional[float] = None, kernel: str = "wave") -> torch.Tensor:
    """q, do, dq [B, Nq, H, 64]; k, v, dk, dv [B, Nk, H, 64] (any strides with unit inner stride, one dtype: fp32, bf16 or fp16); kmask [B, Nk] uint8.
    kernel="wave": vt_attention_bwd (fp32 probabilities, one wave per row).  kernel="mfma": vt_attention_bwd_mfma (bf16 or fp16 operands,
    Nq <= 128, strides in multiples of 8: P and dS are rounded to the operands' type, csrc/vt_attn_bwd.hip); a shape or dtype it does not take raises, nothing falls back.
    -> the row statistics [B * H * Nq, 3] = (max, 1 / sum, delta)."""
    if kernel not in ATTENTION_BACKWARDS:
        raise ValueError(f"attention_bwd: kernel must be one of {ATTENTION_BACKWARDS}, got {kernel!r}")
    B, Nq, H, hd = q.shape
    Nk = k.shape[1]
    assert hd == 64 and k.shape == v.shape == dk.shape == dv.shape == (B, Nk, H, 64) and do.shape == dq.shape == q.shape
    p = L.AttnBwdParams()
    for name, t in (("q", q), ("k", k), ("v", v), ("do", do), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert t.stride(3) == 1 and t.dtype == q.dtype
        setattr(p, {"q": "Q", "k": "K", "v": "V", "do": "dO", "dq": "dQ", "dk": "dK", "dv": "dV"}[name], t.data_ptr())
        setattr(p, f"{name}_bs", t.stride(0)), setattr(p, f"{name}_rs", t.stride(1)), setattr(p, f"{name}_hs", t.stride(2))
    ws = _empty((B * H * Nq * 3,), q.device)
    p.ws = ws.data_ptr()
    if kmask is not None:
        assert kmask.dtype == torch.uint8 and kmask.shape == (B, Nk) and kmask.is_contiguous()
        p.kmask, p.km_bs = kmask.data_ptr(), Nk
    p.B, p.H, p.Nq, p.Nk, p.hd, p.dtype = B, H, Nq, Nk, 64, L.dt_code(q.dtype)
    p.scale = scale if scale is not None else hd ** -0.5
    if kernel == "mfma":
        if q.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"attention_bwd: kernel='mfma' takes bf16 or fp16 tensors, got {q.dtype}")
        nbytes = L.lib().vt_attention_bwd_mfma_ws_bytes(B, H, Nq, Nk)
        if nbytes < 0:
            raise ValueError(f"attention_bwd: kernel='mfma' does not take B={B}, H={H}, Nq={Nq}, Nk={Nk} (1 <= Nq <= 128, B * H <= 65535)")
        ws2 = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        L.check(L.lib().vt_attention_bwd_mfma(C.byref(p), L.ptr(ws2), nbytes, _sp(q.device)), "vt_attention_bwd_mfma")
    else:
        L.check(L.lib().vt_attention_bwd(C.byref(p), _sp(q.device)), "vt_attention_bwd")
    return ws.view(-1, 3)


def ddpm_qsample(state, action, noise, mask, timesteps, ab, dtype=F32) -> torch.Tensor:
    """state [B,1,A], action / noise [B,H,A], mask [B,1,A] fp32, timesteps [B] int64, ab [T] -> [B, H+1, 2A] in `dtype` (rdt_runner.py:197-204)."""
    B, H, A = action.shape
    out = torch.empty((B, H + 1, 2 * A), dtype=dtype, device=action.device)
    L.check(L.lib().vt_ddpm_qsample(L.ptr(state), L.ptr(action), L.ptr(noise), L.ptr(mask), L.ptr(timesteps), L.ptr(ab), ab.numel(), L.ptr(out), _dt(out),
                                    B, H, A, _sp(action.device)), "vt_ddpm_qsample")
    return out


def timestep_freqs(dim: int = 256, max_period: float = 10000.0) -> torch.Tensor:
    """The fp32 frequency table exactly as blocks.py:53-56 computes it."""
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=F32) / half)


def timestep_embed(t: torch.Tensor, freqs: torch.Tensor, dtype=F32) -> torch.Tensor:
    dim = 2 * freqs.numel()
    out = torch.empty((t.shape[0], dim), dtype=dtype, device=t.device)
    L.check(L.lib().vt_timestep_embed(L.ptr(t), L.ptr(freqs), L.ptr(out), _dt(out), t.shape[0], dim, _sp(t.device)), "vt_timestep_embed")
    return out


def add_rowvec_(a2d: torch.Tensor, v: torch.Tensor) -> None:
    rows, cols = a2d.shape
    assert a2d.is_contiguous() and v.is_contiguous() and v.dtype == F32 and v.numel() >= cols
    L.check(L.lib().vt_add_rowvec_(L.ptr(a2d), _dt(a2d), L.ptr(v), rows, cols, _sp(a2d.device)), "vt_add_rowvec_")


def mse_loss(pred: torch.Tensor, target: torch.Tensor, grad_scale: Optional[float] = None):
    """pred (activation dtype), target fp32 -> (loss [1] fp32, d pred in pred's dtype).  grad_scale (fp16 training): d pred is multiplied by
    it before its one rounding (vt_mse_loss_scaled); the loss is not."""
    dpred, loss = torch.empty_like(pred), _empty((1,), pred.device)
    if grad_scale is not None:
        L.check(L.lib().vt_mse_loss_scaled(L.ptr(pred), L.ptr(target), L.ptr(dpred), L.ptr(loss), pred.numel(), _dt(pred), grad_scale, _sp(pred.device)),
                "vt_mse_loss_scaled")
        return loss, dpred
    L.check(L.lib().vt_mse_loss(L.ptr(pred), L.ptr(target), L.ptr(dpred), L.ptr(loss), pred.numel(), _dt(pred), _sp(pred.device)), "vt_mse_loss")
    return loss, dpred


def _cols(src2d: torch.Tensor, off: int, cols: int) -> torch.Tensor:
    out = torch.empty((src2d.shape[0], cols), dtype=src2d.dtype, device=src2d.device)
    copy_cols(src2d, off, out, 0, cols)
    return out


# ---------------------------------------------------------------------------------------------- the trainer
def _load_matching(path: str, rel, shapes, what: str) -> Dict[str, torch.Tensor]:
    """The file `rel` of the checkpoint under `path` if it holds fp32 tensors of exactly these names and shapes; ValueError otherwise."""
    from safetensors.torch import load_file
    d = load_file(os.path.join(path, *rel))
    if set(d) != set(shapes) or any(d[k].shape != s or d[k].dtype != F32 for k, s in shapes.items()):
        raise ValueError(f"checkpoint {path}: the {what} tensors do not match this trainer's parameters")
    return d


class Moments32:
    """The AdamW moments of a trainer's tensors as fp32 tensors of the parameters' shapes; adam8.Moments8 is the block-wise 8-bit form with
    the same interface.  Nothing here but `step` launches.

    shapes: parameter name -> shape, in the order of the multi-tensor table's rows.  The state appears with `zero()` or `load()`; it is
    checkpoint/adam_m.safetensors and checkpoint/adam_v.safetensors under the parameters' names, and adds nothing (`state_json`) to
    trainer_state.json: a file without `optimizer` is an "adamw" one."""
    state_json: dict = {}

    def __init__(self, shapes, device):
        self.shapes, self.device = dict(shapes), torch.device(device)
        self.m: Dict[str, torch.Tensor] = {}
        self.v: Dict[str, torch.Tensor] = {}

    def _zeros(self):
        return {k: torch.zeros(tuple(s), dtype=F32, device=self.device) for k, s in self.shapes.items()}

    def zero(self) -> None:
        self.m, self.v = self._zeros(), self._zeros()

    def columns(self, k):
        """The m / v addresses of tensor k's row of the multi-tensor table."""
        return self.m[k].data_ptr(), self.v[k].data_ptr()

    def step(self, table, ntensors, chunks, hyper, betas, eps, wd) -> None:
        """AdamW + EMA over a table whose m / v columns are `columns()` of every tensor: one launch."""
        L.check(L.lib().vt_adamw_ema_multi(L.ptr(table), ntensors, chunks, L.ptr(hyper), betas[0], betas[1], eps, wd, _sp(self.device)), "vt_adamw_ema_multi")

    def moments(self, k):
        """(m, v) of tensor k: copies, not views of the state."""
        return self.m[k].clone(), self.v[k].clone()

    def nbytes(self) -> int:
        """Bytes of the state, held or, before it appears, counted from the shapes."""
        return 8 * sum(math.prod(s) for s in self.shapes.values())

    def save(self, path: str) -> None:
        from safetensors.torch import save_file
        for tag, d in (("m", self.m), ("v", self.v)):
            save_file({k: t.detach().cpu().contiguous() for k, t in (d if d else self._zeros()).items()},
                      os.path.join(path, "checkpoint", f"adam_{tag}.safetensors"))

    def load(self, path: str, state: dict) -> None:
        """Adopt what `save` wrote under `path`; raises ValueError, leaving this store as it was, unless both files hold fp32 tensors of exactly
        the parameters' names and shapes."""
        m, v = [_load_matching(path, ("checkpoint", f"adam_{tag}.safetensors"), self.shapes, tag) for tag in ("m", "v")]
        self.m, self.v = ({k: d[k].to(self.device).contiguous() for k in self.shapes} for d in (m, v))


class RdtTrainer:
    """get_loss + backward + clip + AdamW + EMA for `RDTRunner` (all of its parameters train, the three position embeddings included).

    sd: the runner's state dict (reference keys).  Hyper-parameters default to main.py:125-210 (lr 5e-6, betas 0.9 / 0.999, eps 1e-8, weight decay
    1e-2, max_grad_norm 1.0) and EMAModel's constructor.

    optimizer="adamw8bit" (the reference's --use_8bit_adam, train.py:216-237) keeps the AdamW moments of every tensor of at least
    adam8.MIN_8BIT_SIZE elements as uint8 codes with one fp32 scale per 256 elements (vlatouch/adam8.py, csrc/vt_adam8.hip; DESIGN.md §8 states
    the arithmetic, UNPINNED against bitsandbytes); smaller tensors keep fp32 moments and the bits of the default step.  Either way the moments
    live in one store, `opt_state` (Moments32 or adam8.Moments8: zero state, table columns, the AdamW + EMA launch, checkpoint files, byte count);
    `moments(name)` reads them as fp32.

    weight_gradient="tn" (bf16 / fp16 only; the default "gemm" is two transposes, the NT GEMM and a column sum per Linear) forms every Linear's
    weight and bias gradient in one vt_gemm_tn launch (weight_grad_tn, csrc/vt_gemm_tn.hip).  Like attention_backward it is an execution choice,
    not state: gradient bits change, checkpoints do not record it and resume under either setting.  Every 2-D weight must then have dimensions
    that are multiples of 8 (ValueError at construction, naming the tensor).

    small_batch_linear="packed" (bf16 / fp16 only; the default "gemm" is the trainer as it was, launch for launch) keeps two more 16-bit copies of
    the Linear weights, in MFMA fragment order (w and w^T), and sends the forward and data-gradient Linears of at most 512 rows to the small-M
    packed-weight tile the denoise loop uses (csrc/vt_gemm_pws.hip) wherever the library's dispatcher takes them there; launches above 512 rows
    get no packed pointer and keep their kernels and bits.  Every refresh of the 16-bit copies is then one vt_refresh16 launch per weight
    (csrc/vt_refresh16.hip: one read of the fp32 master writes all four forms) instead of a cast and a transpose.  An execution choice like
    attention_backward: output bits change (another summation order), checkpoints do not record it and resume under either setting.

    precision="fp16" with loss_scale= ("dynamic", a dict of GradScaler's init_scale / growth_factor / backoff_factor / growth_interval, or a
    positive number for a static scale) is torch.amp.GradScaler around the bf16 mode's step on IEEE half: dL/dpred is multiplied by the scale S
    (the loss is reported unscaled), the accumulators and the exchange hold scaled gradients, and optimizer_step unscales, checks and clips in
    one launch group (vt_grad_unscale_clip_multi), reads the overflow flag, the norm and the loss in one small copy and either steps or skips:
    a skipped step moves no parameter, moment, step_count or lr, runs the EMA update alone, multiplies S by backoff_factor and closes the
    window.  `loss_scale_value`, `growth_tracker`, `skipped_steps`, `skipped_nonfinite_loss`, `last_step_skipped` read the state;
    `global_step` counts skipped steps too, as the reference's does.

    process_group: a torch.distributed group of W ranks, one process per GPU, for data-parallel training with replicated state (None, the
    default, is the one-process trainer: same launches, same bits).  The constructor is then collective: the ranks compare parameter names and
    shapes, gradient_accumulation_steps, precision, optimizer, comm_dtype, attention_backward, weight_gradient and small_batch_linear, every rank raising ValueError with the
    differing field if they disagree, and rank 0's master parameters are broadcast.  For any k the accumulators are views into one fp32
    arena (tensor i at first_chunk_i * MT_CHUNK, padding zeroed once); `accumulate` folds with scale 1 / (k W) and, after the window's last
    fold, sums the arena over the ranks in chunk-aligned slices of at most `comm_bucket_bytes`; comm_dtype="bf16" (an exchange format, allowed
    with either precision) sends bf16 instead, through vt_grad_fold_pack_multi and vt_grad_unpack_multi.  `load_checkpoint` is called on every
    rank; `save_checkpoint` is an ordinary call (`finetune` makes it on rank 0)."""

    def __init__(self, sd, *, heads: int, horizon: int, action_dim: int, rms_mode: str = "meansq", prediction_type: str = "sample",
                 num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2", precision: str = "fp32", lr: float = 5e-6,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, max_grad_norm: float = 1.0, lr_scheduler: str = "constant",
                 lr_warmup_steps: int = 500, ema: Optional[dict] = None, config: Optional[dict] = None, gradient_accumulation_steps: int = 1,
                 optimizer: str = "adamw", attention_backward: str = "wave", weight_gradient: str = "gemm", small_batch_linear: str = "gemm",
                 process_group=None,
                 comm_dtype: str = "fp32", comm_bucket_bytes: int = 256 << 20, loss_scale=None, device="cuda"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        if precision == "fp16" and loss_scale is None:
            raise ValueError("precision='fp16' needs loss_scale= ('dynamic', a dict of GradScaler's settings, or a static scale): its gradients "
                             "underflow without loss scaling")
        if precision != "fp16" and loss_scale is not None:
            raise ValueError(f"loss_scale belongs to precision='fp16', not {precision!r}")
        scale_settings = loss_scale_settings(loss_scale) if loss_scale is not None else None
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"Unsupported prediction type {prediction_type}")
        if rms_mode not in ("meansq", "var"):
            raise ValueError(f"rms_mode must be 'meansq' or 'var', got {rms_mode!r}")
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        if attention_backward not in ATTENTION_BACKWARDS:
            raise ValueError(f"attention_backward must be one of {ATTENTION_BACKWARDS}, got {attention_backward!r}")
        if attention_backward == "mfma" and precision == "fp32":
            raise ValueError("attention_backward='mfma' is a 16-bit kernel: it needs precision='bf16' or 'fp16' ('wave' is the fp32 path)")
        if attention_backward == "mfma" and horizon + 3 > 128:
            raise ValueError(f"attention_backward='mfma' holds at most 128 query rows, horizon + 3 = {horizon + 3}")
        if weight_gradient not in WEIGHT_GRADIENTS:
            raise ValueError(f"weight_gradient must be one of {WEIGHT_GRADIENTS}, got {weight_gradient!r}")
        if weight_gradient == "tn" and precision == "fp32":
            raise ValueError("weight_gradient='tn' is a 16-bit kernel: it needs precision='bf16' or 'fp16' ('gemm' is the fp32 path)")
        if weight_gradient == "tn":
            for k, v in sd.items():
                if k.endswith(".weight") and v.dim() == 2 and (v.shape[0] % 8 or v.shape[1] % 8):
                    raise ValueError(f"weight_gradient='tn' takes Linear weights whose dimensions are multiples of 8, {k} is {tuple(v.shape)}")
        if small_batch_linear not in SMALL_BATCH_LINEARS:
            raise ValueError(f"small_batch_linear must be one of {SMALL_BATCH_LINEARS}, got {small_batch_linear!r}")
        if small_batch_linear == "packed" and precision == "fp32":
            raise ValueError("small_batch_linear='packed' runs on a 16-bit kernel: it needs precision='bf16' or 'fp16' ('gemm' is the fp32 path)")
        if comm_dtype not in COMM_DTYPES:
            raise ValueError(f"comm_dtype must be one of {COMM_DTYPES}, got {comm_dtype!r} (the format of the gradient exchange, whatever the precision)")
        if int(comm_bucket_bytes) != comm_bucket_bytes or comm_bucket_bytes < 1:
            raise ValueError(f"comm_bucket_bytes must be an integer >= 1, got {comm_bucket_bytes!r}")
        lr_at(lr, lr_scheduler, 0, lr_warmup_steps)                       # raises on an unknown scheduler
        if int(gradient_accumulation_steps) != gradient_accumulation_steps or gradient_accumulation_steps < 1:
            raise ValueError(f"gradient_accumulation_steps must be an integer >= 1, got {gradient_accumulation_steps!r}")
        self.device = dev = L.require_gpu(device)
        self.p: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.detach().to(dev, F32).contiguous().clone()) for k, v in sd.items())
        self.g: Dict[str, torch.Tensor] = {}
        # data parallelism: None is the one-process trainer.  With a group the ranks first agree on what must be the same everywhere, then
        # rank 0's master parameters replace everyone's; from there on all state is replicated and only gradients travel.
        self.group, self.world, self.rank = process_group, 1, 0
        self.comm_dtype, self.comm_bucket_bytes = comm_dtype, int(comm_bucket_bytes)
        self._arena: Optional[torch.Tensor] = None            # grouped: the fp32 buffer the accumulators are views of
        self._comm: Optional[torch.Tensor] = None             # grouped, comm_dtype="bf16": the persistent bf16 exchange buffer
        if process_group is not None:
            import hashlib
            import torch.distributed as dist
            from . import dist as D
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
            digest = hashlib.sha256(repr([(k, tuple(v.shape)) for k, v in self.p.items()]).encode()).hexdigest()
            diff = D.differing_field(self.group_fields(digest, gradient_accumulation_steps, precision, optimizer, comm_dtype, attention_backward,
                                                       weight_gradient, small_batch_linear, scale_settings), process_group)
            if diff is not None:
                raise ValueError(f"RdtTrainer: the ranks of the process group disagree on {diff[0]}: {diff[1]}")
            D.broadcast_tensors(self.p.values(), src=dist.get_global_rank(process_group, 0), group=process_group)
        self.depth = 0
        while f"model.blocks.{self.depth}.norm1.weight" in self.p:
            self.depth += 1
        self.hidden = self.p["model.x_pos_embed"].shape[2]
        self.heads, self.horizon, self.action_dim = heads, horizon, action_dim
        if self.hidden != heads * 64:
            raise ValueError("RdtTrainer: head_dim must be 64")
        if self.p["model.x_pos_embed"].shape[1] != horizon + 3:
            raise ValueError("RdtTrainer: x_pos_embed does not match horizon + 3 tokens")
        self.rms_mode, self.norm_mode = rms_mode, (L.NORM_RMS_MEANSQ if rms_mode == "meansq" else L.NORM_RMS_VAR)
        self.prediction_type, self.num_train_timesteps, self.beta_schedule = prediction_type, num_train_timesteps, beta_schedule
        self.ab = alphas_cumprod(num_train_timesteps, beta_schedule).to(dev)
        self.freqs = timestep_freqs(256).to(dev)
        self.adaptors = {n: self._adaptor_layers(n) for n in ("lang_adaptor", "img_adaptor", "state_adaptor")}
        self.precision = precision
        self.attention_backward = attention_backward          # an execution choice, not state: checkpoints do not record it
        self.weight_gradient = weight_gradient                # likewise: a checkpoint written under either setting resumes under the other
        self.adt = {"fp32": F32, "bf16": torch.bfloat16, "fp16": torch.float16}[precision]      # dtype of activations, activation gradients and MFMA operands
        self.scaler: Optional[LossScaler] = LossScaler(scale_settings) if scale_settings is not None else None      # fp16: GradScaler's state
        self.last_step_skipped = False                                # the last optimizer_step found a non-finite gradient and took no step
        self.w16: Dict[str, torch.Tensor] = {}                        # 16-bit modes: copies of the Linear weights and of their transposes,
        self.w16t: Dict[str, torch.Tensor] = {}                       # refreshed after every optimizer step
        self.small_batch_linear = small_batch_linear          # an execution choice too
        self.wp: Dict[str, torch.Tensor] = {}                         # "packed": fragment-packed copies of w16 / w16t for the weights whose forward /
        self.wtp: Dict[str, torch.Tensor] = {}                        # data-gradient Linear the small-M tile can take; refreshed with the others
        self._forms: Dict[str, tuple] = {}                            # "packed": per 2-D weight, the forms vt_refresh16 writes for it
        self.packed: Optional[PackedScratch] = None
        if small_batch_linear == "packed":
            self._plan_packed()
        self._refresh16()
        self.base_lr, self.lr, self.wd, self.betas, self.eps, self.max_grad_norm = lr, lr, weight_decay, betas, eps, max_grad_norm
        self.lr_scheduler, self.lr_warmup_steps = lr_scheduler, lr_warmup_steps
        self.ema_cfg = dict(update_after_step=0, inv_gamma=1.0, power=2 / 3, min_value=0.0, max_value=0.9999)
        self.ema_cfg.update(ema or {})
        self.config = config
        self.k = int(gradient_accumulation_steps)             # micro-batches per optimizer step (accelerate's gradient_accumulation_steps)
        self.step_count = 0                                   # optimizer steps taken: feeds the lr schedule and AdamW's bias correction
        self.ema_updates = 0                                  # EMAModel.optimization_step: one per micro-batch
        self.micro_step = 0                                   # micro-batches folded into the open accumulation window
        self.sync_gradients = False                           # the last train_step took the optimizer step
        self._acc: Dict[str, torch.Tensor] = {}               # k > 1 or grouped: persistent fp32 accumulators, the table's g column
        self.optimizer = optimizer                            # AdamW moments and the EMA copy appear with the first optimizer step (the parameters are
        shapes = OrderedDict((k, v.shape) for k, v in self.p.items())     # still the initial ones then), so a trainer that only evaluates the loss holds one copy
        self.opt_state = adam8.Moments8(shapes, dev) if optimizer == "adamw8bit" else Moments32(shapes, dev)
        self.shadow: Dict[str, torch.Tensor] = {}
        # [norm, clip coefficient]; fp16: + [overflow flag as int32 bits, the last micro-batch's loss], what optimizer_step reads in one copy
        self._norm_coef = torch.zeros(2 if self.scaler is None else 4, dtype=F32, device=dev)
        self._table_key = None
        self.last_loss: Optional[torch.Tensor] = None
        self.weights_version = 0                              # optimizer steps and load_checkpoint calls: changes of the master parameters
        self.shadow_version = 0                               # the same plus EMA-only steps: changes of the shadows; `sampler` compares the one it reads
        self._sampler = None                                  # the RDTRunner `sampler` keeps, and the (source, its version) it was last refreshed at
        self._sampler_key = None
        self.sampler_repacks = 0                              # times `sampler` handed weights over (the first build included)

    @staticmethod
    def group_fields(shapes_digest, gradient_accumulation_steps, precision, optimizer, comm_dtype, attention_backward, weight_gradient,
                     small_batch_linear, scale_settings) -> dict:
        """What the ranks of a process group compare at construction (dist.differing_field names the first key that differs)."""
        return {"parameter names and shapes": shapes_digest, "gradient_accumulation_steps": int(gradient_accumulation_steps),
                "precision": precision, "optimizer": optimizer, "comm_dtype": comm_dtype,
                "attention_backward": attention_backward, "weight_gradient": weight_gradient, "small_batch_linear": small_batch_linear,
                **({} if scale_settings is None else {"loss_scale": repr(sorted(scale_settings.items()))})}

    def _adaptor_layers(self, name: str) -> List[str]:
        if f"{name}.weight" in self.p:
            return [name]
        out, i = [], 0
        while f"{name}.{i}.weight" in self.p:
            out.append(f"{name}.{i}")
            i += 2
        if not out:
            raise ValueError(f"no weights for {name}")
        return out

    def _ema_decay(self, step: int) -> float:
        """`step` = number of EMA updates including this one; EMAModel.step evaluates get_decay at the count before it."""
        return ema_decay(step - 1, **self.ema_cfg)

    # the store's dicts under the names tests and tools have always read on the trainer (codes or fp32 moments; scales, empty for "adamw")
    _m = property(lambda self: self.opt_state.m)
    _v = property(lambda self: self.opt_state.v)
    _am = property(lambda self: getattr(self.opt_state, "am", {}))
    _av = property(lambda self: getattr(self.opt_state, "av", {}))

    @property
    def global_step(self) -> int:
        """Optimizer steps taken or, in fp16 mode, skipped: train.py:451-453 counts every sync_gradients, whatever the scaler decided."""
        return self.step_count + self.skipped_steps

    # fp16 mode's GradScaler state, read-only (1.0 / zeros for the other precisions)
    loss_scale_value = property(lambda self: self.scaler.scale if self.scaler is not None else 1.0)
    growth_tracker = property(lambda self: self.scaler.growth_tracker if self.scaler is not None else 0)
    skipped_steps = property(lambda self: self.scaler.skipped_steps if self.scaler is not None else 0)
    skipped_nonfinite_loss = property(lambda self: self.scaler.skipped_nonfinite_loss if self.scaler is not None else 0)

    @property
    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the gradients before clipping at the last optimizer_step (0-d device tensor; reading it synchronises)."""
        return self._norm_coef[0]

    def _plan_packed(self) -> None:
        """small_batch_linear="packed": which packed forms each 2-D weight gets, decided once by asking the dispatcher (ops.packed_route) whether a
        one-row Linear with these weights and a packed copy goes to the small-M tile: w [N, K] for the forward, w^T [K, Np] for the data
        gradient.  Then the tile's split-K scratch, wide enough for the widest of those Linears."""
        widest = 0
        for k, v in self.p.items():
            if k.endswith(".weight") and v.dim() == 2:
                (N, K), Np = v.shape, (v.shape[0] + 7) // 8 * 8
                fwd, dgrad = ops.packed_route(1, N, K, self.adt) == "PWS", ops.packed_route(1, K, Np, self.adt) == "PWS"
                self._forms[k] = ("w16", "w16t") + (("wp",) if fwd else ()) + (("wtp",) if dgrad else ())
                widest = max(widest, N if fwd else 0, K if dgrad else 0)
        if widest:
            self.packed = PackedScratch(widest, self.device)

    def _refresh16(self) -> None:
        if self.adt == F32:
            return
        stores = {"w16": self.w16, "w16t": self.w16t, "wp": self.wp, "wtp": self.wtp}
        for k, v in self.p.items():
            if k.endswith(".weight") and v.dim() == 2:
                if self.small_batch_linear == "packed":           # one launch, one read of the master, every form in place
                    for f, t in ops.refresh16(v, self.adt, self._forms[k], out={f: stores[f].get(k) for f in self._forms[k]}).items():
                        stores[f][k] = t
                    continue
                self.w16[k] = ops.cast(v, self.adt, out=self.w16.get(k))
                self.w16t[k] = transpose_pad(self.w16[k])

    # ---- layers
    def _linear(self, name, x, residual=None):
        b = self.p[f"{name}.bias"]
        if self.packed is not None:
            k = f"{name}.weight"
            return gemm_small_packed(x, self.w16[k], self.wp.get(k), self.packed, b, residual, tag=f"{name}/forward")
        if self.adt != F32:
            return ops.gemm(x, self.w16[f"{name}.weight"], b, residual=residual)
        w = self.p[f"{name}.weight"]
        return ops.gemm(x, w, b, residual=residual) if residual is not None else T.gemm(x, w, b)

    def _linear_bwd(self, name, x, dy, need_dx=True):
        k = f"{name}.weight"
        dx, self.g[k], self.g[f"{name}.bias"] = linear_bwd(x, self.w16.get(k, self.p[k]), dy, need_dx, self.w16t.get(k),
                                                                 kernel=self.weight_gradient, wtp=self.wtp.get(k), scratch=self.packed,
                                                                 tag=f"{name}/dgrad")
        return dx

    def _norm(self, name, x):
        return ops.rownorm(x, self.p[f"{name}.weight"], None, 1e-6, self.norm_mode)

    def _norm_bwd(self, name, x, dy):
        dx, self.g[f"{name}.weight"] = rmsnorm_bwd(x, self.p[f"{name}.weight"], dy, 1e-6, self.norm_mode)
        return dx

    def _mlp_fwd(self, layers, x, kind):
        """Linear (act Linear)*: -> (output, tape of (layer input, layer output))."""
        tape, h = [], x
        for j, name in enumerate(layers):
            if j > 0:
                h = act(tape[-1][1], kind)
            a = self._linear(name, h)
            tape.append((h, a))
        return tape[-1][1], tape

    def _mlp_bwd(self, layers, tape, d, kind, need_dx=False):
        for j in range(len(layers) - 1, -1, -1):
            d = self._linear_bwd(layers[j], tape[j][0], d, need_dx or j > 0)
            if j > 0:
                d = act(tape[j - 1][1], kind, d)
        return d

    def _embed_fwd(self, name, t):
        return self._mlp_fwd([f"{name}.mlp.0", f"{name}.mlp.2"], timestep_embed(t, self.freqs, self.adt), L.ACT_SILU)

    def _empty(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=self.adt, device=self.device)

    def _heads4(self, cols2d, B):
        """A 2-D column view [B * N, hidden] (unit inner stride, any row stride) -> its [B, N, H, 64] view."""
        return cols2d.unflatten(0, (B, cols2d.shape[0] // B)).unflatten(2, (self.heads, 64))

    # ---- the attention sub-block the self- and the cross-attention share (timm Attention with q / k RmsNorm; blocks.py:102-138)
    def _attn_fwd(self, name, q, k, v, B, kmask=None):
        """q [B * Nq, hidden], k, v [B * Nk, hidden]: column views of the projections' outputs (unit inner stride, any row stride).  Saves the
        pre-norm q and k, applies `name`.q_norm / k_norm in place and attends -> (o [B * Nq, hidden], what `_attn_bwd` reads)."""
        raw = q.clone(), k.clone()
        for t, n in ((q, "q_norm"), (k, "k_norm")):
            ops.headnorm_(t, self.heads, self.p[f"{name}.{n}.weight"], 1e-6, self.norm_mode, tok_stride=t.stride(0), tokens=t.shape[0])
        return ops.attention(*(self._heads4(t, B) for t in (q, k, v)), kmask=kmask).view(q.shape[0], self.hidden), (q, k, v, *raw)

    def _attn_bwd(self, name, saved, do, dq, dk, dv, B, kmask=None) -> None:
        """do [B * Nq, hidden] -> dq, dk, dv: column views of the buffer the projections' backward reads, filled with the gradients of the
        pre-norm q, k and of v; leaves d `name`.q_norm / k_norm in `self.g`."""
        q, k, v, q_raw, k_raw = saved
        attention_bwd(*(self._heads4(t, B) for t in (q, k, v, do, dq, dk, dv)), kmask=kmask, kernel=self.attention_backward)
        for n, raw, d in (("q_norm", q_raw, dq), ("k_norm", k_raw, dk)):
            self.g[f"{name}.{n}.weight"] = headnorm_bwd_(raw, d, self.heads, self.p[f"{name}.{n}.weight"], 1e-6, self.norm_mode)

    # ---- one RDT block; its condition is c [B * Lc, hidden], the tokens it attends to, and km, their key mask or None
    def _block_fwd(self, i, x, c, km):
        """Block i: (x [B * N, hidden], condition) -> (x, tape entry)."""
        b, D, B = f"model.blocks.{i}", self.hidden, x.shape[0] // (self.horizon + 3)
        tb = {"x0": x}
        # self-attention
        tb["h1"] = self._norm(f"{b}.norm1", x)
        tb["o1"], tb["attn"] = self._attn_fwd(f"{b}.attn", *self._linear(f"{b}.attn.qkv", tb["h1"]).split(D, dim=1), B)
        x = tb["x1"] = self._linear(f"{b}.attn.proj", tb["o1"], residual=x)
        # cross-attention: q from the block, k | v from the condition
        tb["h2"] = self._norm(f"{b}.norm2", x)
        q = self._linear(f"{b}.cross_attn.q", tb["h2"])
        tb["o2"], tb["cross_attn"] = self._attn_fwd(f"{b}.cross_attn", q, *self._linear(f"{b}.cross_attn.kv", c).split(D, dim=1), B, km)
        x = tb["x2"] = self._linear(f"{b}.cross_attn.proj", tb["o2"], residual=x)
        # FFN (timm Mlp, tanh-GELU)
        tb["h3"] = self._norm(f"{b}.norm3", x)
        tb["a"] = self._linear(f"{b}.ffn.fc1", tb["h3"])
        tb["gl"] = act(tb["a"], L.ACT_GELU_TANH)
        return self._linear(f"{b}.ffn.fc2", tb["gl"], residual=x), tb

    def _block_bwd(self, i, tb, d, c, km):
        """Block i: (tape entry, d loss / d its output, condition) -> (d loss / d its input, d loss / d c)."""
        b, D, B = f"model.blocks.{i}", self.hidden, d.shape[0] // (self.horizon + 3)
        # FFN
        dg = self._linear_bwd(f"{b}.ffn.fc2", tb["gl"], d)
        dh = self._linear_bwd(f"{b}.ffn.fc1", tb["h3"], act(tb["a"], L.ACT_GELU_TANH, dg))
        d = add_(self._norm_bwd(f"{b}.norm3", tb["x2"], dh), d)
        # cross-attention
        do = self._linear_bwd(f"{b}.cross_attn.proj", tb["o2"], d)
        dq, dkv = self._empty(d.shape[0], D), self._empty(c.shape[0], 2 * D)
        self._attn_bwd(f"{b}.cross_attn", tb["cross_attn"], do, dq, *dkv.split(D, dim=1), B, km)
        dc = self._linear_bwd(f"{b}.cross_attn.kv", c, dkv)
        dh = self._linear_bwd(f"{b}.cross_attn.q", tb["h2"], dq)
        d = add_(self._norm_bwd(f"{b}.norm2", tb["x1"], dh), d)
        # self-attention
        do = self._linear_bwd(f"{b}.attn.proj", tb["o1"], d)
        dqkv = self._empty(d.shape[0], 3 * D)
        self._attn_bwd(f"{b}.attn", tb["attn"], do, *dqkv.split(D, dim=1), B)
        dh = self._linear_bwd(f"{b}.attn.qkv", tb["h1"], dqkv)
        return add_(self._norm_bwd(f"{b}.norm1", tb["x0"], dh), d), dc

    # ---- get_loss's stages: inputs, a forward that returns the tape, the loss, a backward that consumes the tape
    def _inputs(self, lang_tokens, lang_attn_mask, img_tokens, state_tokens, action_gt, action_mask, ctrl_freqs, noise, timesteps) -> dict:
        """get_loss's arguments checked and on the device: fp32 and contiguous, the language and image tokens in the activation dtype."""
        dev, hor, A = self.device, self.horizon, self.action_dim
        f = lambda a: torch.as_tensor(a).to(dev, F32).contiguous()
        lang, img, state, act_gt, amask, noise = f(lang_tokens), f(img_tokens), f(state_tokens), f(action_gt), f(action_mask), f(noise)
        B, Ll, Li = lang.shape[0], lang.shape[1], img.shape[1]
        if act_gt.shape != (B, hor, A) or noise.shape != act_gt.shape or state.shape != (B, 1, A) or amask.shape != (B, 1, A):
            raise ValueError("get_loss: state_tokens / action_mask must be [B, 1, action_dim], action_gt / noise [B, horizon, action_dim]")
        if Ll > self.p["model.lang_cond_pos_embed"].shape[1] or Li != self.p["model.img_cond_pos_embed"].shape[1]:
            raise ValueError("get_loss: language longer than max_lang_cond_len, or image token count != img_cond_len")
        ts = torch.as_tensor(timesteps)
        if ts.numel() != B:
            raise ValueError("get_loss: timesteps must hold one integer per sample")
        kmask = torch.as_tensor(lang_attn_mask).to(dev).to(torch.uint8).contiguous()
        if kmask.shape != (B, Ll):
            raise ValueError("get_loss: lang_attn_mask must be [B, lang_len]")
        if self.adt != F32:
            lang, img = ops.cast(lang, self.adt), ops.cast(img, self.adt)
        return dict(B=B, lang=lang, img=img, state=state, act_gt=act_gt, amask=amask, noise=noise, ts=ts.reshape(B).to(dev, torch.int64).contiguous(),
                    freqs=f(ctrl_freqs).reshape(B), kmask=kmask)

    def _forward(self, inp: dict) -> dict:
        """Tokens (DDPM forward process + layout, the three adaptors, the two embedders, position embeddings), the blocks and the final layer
        -> the tape: what the loss and `_backward` read."""
        p, D, hor, A, gelu = self.p, self.hidden, self.horizon, self.action_dim, L.ACT_GELU_TANH
        B, N, tape = inp["B"], hor + 3, {"B": inp["B"], "blocks": []}
        sa_in = ddpm_qsample(inp["state"], inp["act_gt"], inp["noise"], inp["amask"], inp["ts"], self.ab, self.adt).view(B * (hor + 1), 2 * A)
        sa, tape["state_adaptor"] = self._mlp_fwd(self.adaptors["state_adaptor"], sa_in, gelu)
        lang_c, tape["lang_adaptor"] = self._mlp_fwd(self.adaptors["lang_adaptor"], inp["lang"].flatten(0, 1), gelu)
        img_c, tape["img_adaptor"] = self._mlp_fwd(self.adaptors["img_adaptor"], inp["img"].flatten(0, 1), gelu)
        te, tape["t_embedder"] = self._embed_fwd("model.t_embedder", inp["ts"].to(F32))
        fe, tape["freq_embedder"] = self._embed_fwd("model.freq_embedder", inp["freqs"])
        x = self._empty(B, N * D)
        copy_cols(te, 0, x, 0, D)
        copy_cols(fe, 0, x, D, D)
        copy_cols(sa.view(B, (hor + 1) * D), 0, x, 2 * D, (hor + 1) * D)
        add_rowvec_(x, p["model.x_pos_embed"])
        add_rowvec_(lang_c.view(B, -1), p["model.lang_cond_pos_embed"])
        add_rowvec_(img_c.view(B, -1), p["model.img_cond_pos_embed"])
        x = x.view(B * N, D)
        tape["conds"] = ((lang_c, inp["kmask"]), (img_c, None))        # the blocks attend to the language (masked) and the image in turn
        for i in range(self.depth):
            x, tb = self._block_fwd(i, x, *tape["conds"][i % 2])
            tape["blocks"].append(tb)
        tape["x"] = x
        tape["hf"] = self._norm("model.final_layer.norm_final", x)
        tape["af"] = self._linear("model.final_layer.ffn_final.fc1", tape["hf"])
        tape["gf"] = act(tape["af"], gelu)
        tape["out"] = self._linear("model.final_layer.ffn_final.fc2", tape["gf"])      # [B*N, A]
        return tape

    def _backward(self, tape: dict, dpred: torch.Tensor) -> None:
        """d loss / d pred back through the final layer, the blocks (their tape entries are dropped as they are read), the token assembly,
        the position embeddings, the embedders and the adaptors: leaves every gradient in `self.g`."""
        p, g, D, hor, A, gelu = self.p, self.g, self.hidden, self.horizon, self.action_dim, L.ACT_GELU_TANH
        B, N, fl = tape["B"], hor + 3, "model.final_layer"
        dout = torch.zeros(B, N * A, dtype=self.adt, device=self.device)
        copy_cols(dpred, 0, dout, 3 * A, hor * A)
        d = self._linear_bwd(f"{fl}.ffn_final.fc2", tape["gf"], dout.view(B * N, A))
        d = self._linear_bwd(f"{fl}.ffn_final.fc1", tape["hf"], act(tape["af"], gelu, d))
        d = self._norm_bwd(f"{fl}.norm_final", tape["x"], d)                           # d loss / d x after the last block
        dconds = [None, None]
        for i in range(self.depth - 1, -1, -1):
            d, dc = self._block_bwd(i, tape["blocks"].pop(), d, *tape["conds"][i % 2])
            dconds[i % 2] = dc if dconds[i % 2] is None else add_(dconds[i % 2], dc)
        # token assembly, position embeddings, embedders, adaptors
        dx = d.view(B, N * D)
        g["model.x_pos_embed"] = colsum(dx).view(1, N, D)
        self._mlp_bwd(["model.t_embedder.mlp.0", "model.t_embedder.mlp.2"], tape["t_embedder"], _cols(dx, 0, D), L.ACT_SILU)
        self._mlp_bwd(["model.freq_embedder.mlp.0", "model.freq_embedder.mlp.2"], tape["freq_embedder"], _cols(dx, D, D), L.ACT_SILU)
        self._mlp_bwd(self.adaptors["state_adaptor"], tape["state_adaptor"], _cols(dx, 2 * D, (hor + 1) * D).view(B * (hor + 1), D), gelu)
        for name, dc, key in (("lang_adaptor", dconds[0], "model.lang_cond_pos_embed"), ("img_adaptor", dconds[1], "model.img_cond_pos_embed")):
            gp = g[key] = torch.zeros_like(p[key])
            if dc is None:                                        # depth 1: no block attends to the image tokens
                g.update({k: torch.zeros_like(v) for k, v in p.items() if k.startswith(name + ".")})
            else:
                colsum(dc.view(B, -1), gp)
                self._mlp_bwd(self.adaptors[name], tape[name], dc, gelu)

    def get_loss(self, lang_tokens, lang_attn_mask, img_tokens, state_tokens, action_gt, action_mask, ctrl_freqs, *, noise, timesteps,
                 backward: bool = True) -> torch.Tensor:
        """compute_loss's arguments (rdt_runner.py:168-182) plus the two random draws it makes: noise [B, horizon, action_dim] and timesteps [B]
        (integers in [0, num_train_timesteps)).  -> the loss as a 0-d fp32 device tensor; with backward=True the gradients are left in `self.g`."""
        inp = self._inputs(lang_tokens, lang_attn_mask, img_tokens, state_tokens, action_gt, action_mask, ctrl_freqs, noise, timesteps)
        tape = self._forward(inp)
        B, hor, A = inp["B"], self.horizon, self.action_dim
        pred = _cols(tape.pop("out").view(B, -1), 3 * A, hor * A)                      # x[:, -horizon:]
        target = (inp["act_gt"] if self.prediction_type == "sample" else inp["noise"]).view(B, hor * A)
        loss, dpred = mse_loss(pred, target, None if self.scaler is None else self.scaler.scale)      # fp16: d pred carries the loss scale
        self.last_loss, self.last_pred = loss.reshape(()), pred.view(B, hor, A)
        if backward:
            self._backward(tape, dpred)
        return self.last_loss

    # ---- optimizer
    def _fresh_grad(self, name: str) -> torch.Tensor:
        """The gradient get_loss left for one parameter, checked and made contiguous."""
        gt, pt = self.g.get(name), self.p[name]
        if gt is None:
            raise RuntimeError(f"no gradient for {name}: call get_loss first")
        if gt.dtype != F32 or gt.numel() != pt.numel():
            raise RuntimeError(f"gradient of {name}: fp32 with {pt.numel()} elements expected")
        if not gt.is_contiguous():
            gt = self.g[name] = gt.contiguous()
        return gt

    def _hyper(self, adam_step: int) -> torch.Tensor:
        """[lr, 1 - b1^t, sqrt(1 - b2^t), 1 - ema_decay] of the kernels that read the step's scalars from memory, uploaded."""
        host = torch.zeros(4, dtype=F32)
        L.check(L.lib().vt_train_hyper(self.lr, self.betas[0], self.betas[1], adam_step, self._ema_decay(self.ema_updates), L.ptr(host)), "vt_train_hyper")
        return host.to(self.device)

    def _table(self):
        """The multi-tensor table every optimizer launch reads (train.mt_table: {p, g, m, v, shadow, n, first_chunk} per tensor), on the device."""
        if self.group is not None and not self._acc:
            self._alloc_arena()
        if self.k > 1 and not self._acc:
            self._acc = {k: torch.empty_like(v) for k, v in self.p.items()}          # never read before the window's first, storing, accumulate
        if not self.shadow:
            self.opt_state.zero()
            self.shadow = {k: v.clone() for k, v in self.p.items()}
        g = self._acc if self._accumulates else {name: self._fresh_grad(name) for name in self.p}
        key = tuple(t.data_ptr() for t in g.values())
        if key != self._table_key:                                # gradients are fresh allocations each step: their addresses usually repeat, not always
                                                                  # (k > 1: the g column holds the accumulators, so the table is built once)
            rows, chunks = T.mt_table((pt.data_ptr(), g[name].data_ptr(), *self.opt_state.columns(name), self.shadow[name].data_ptr(), pt.numel())
                                      for name, pt in self.p.items())
            self._mt_dev = rows.to(self.device)
            self._chunk_part = _empty((chunks,), self.device)
            self._table_key, self._chunks = key, chunks
        return self._mt_dev, len(self.p), self._chunks

    @property
    def _accumulates(self) -> bool:
        """The table's g column holds persistent accumulators (k > 1, or any k with a process group) and not the fresh gradients."""
        return self.k > 1 or self.group is not None

    def _alloc_arena(self) -> None:
        """Grouped: the accumulators as views into one fp32 buffer of total_chunks * MT_CHUNK elements, tensor i at first_chunk_i * MT_CHUNK
        (the layout train.mt_table gives the rows, in the parameters' order), so that the exchange is a few large chunk-aligned messages.
        The padding behind each tensor's last element is zeroed here, once; no kernel writes it."""
        chunks = sum((v.numel() + T.MT_CHUNK - 1) // T.MT_CHUNK for v in self.p.values())
        self._arena = torch.zeros(chunks * T.MT_CHUNK, dtype=F32, device=self.device)
        if self.comm_dtype == "bf16":
            self._comm = torch.zeros(chunks * T.MT_CHUNK, dtype=torch.bfloat16, device=self.device)
        off = 0
        for k, v in self.p.items():
            self._acc[k] = self._arena[off:off + v.numel()].view(v.shape)
            off += (v.numel() + T.MT_CHUNK - 1) // T.MT_CHUNK * T.MT_CHUNK

    def _all_reduce(self, buf: torch.Tensor) -> None:
        """Sum `buf` (the arena or the bf16 buffer) over the ranks in chunk-aligned slices of at most comm_bucket_bytes, in order, on the
        current stream."""
        from . import dist as D
        step = max(1, self.comm_bucket_bytes // (T.MT_CHUNK * buf.element_size())) * T.MT_CHUNK
        for off in range(0, buf.numel(), step):
            D.all_reduce_sum_(buf[off:off + step], self.group)

    def optimizer_step(self, hyper: Optional[torch.Tensor] = None):
        """clip_grad_norm_(max_grad_norm) -> AdamW -> EMA (train.py:440-448), three launches over one table; fp32 / bf16: no host read.
        fp16: GradScaler.unscale_ with the clip -> scaler.step(optimizer) -> scaler.update -> scheduler -> EMAModel.step; a non-finite gradient
        skips the step, leaving parameters, moments, step_count and lr where they were (AcceleratedScheduler does not step after a skipped one)."""
        if hyper is not None:
            raise NotImplementedError("RdtTrainer: hipGraph capture of the step is not built")
        if self._accumulates and self.micro_step != self.k:
            raise RuntimeError(f"optimizer_step needs a full accumulation window ({self.micro_step} of {self.k} micro-batches accumulated)")
        tab, n, chunks = self._table()
        found_inf = self._prepare_grads(tab, n, chunks)
        self.ema_updates += 1
        (self._ema_alone if found_inf else self._take_step)(tab, n, chunks)      # a skipped step still moves the shadows: train.py:448 is unconditional
        if self.scaler is not None:
            self.scaler.update(found_inf)
        self.last_step_skipped = found_inf
        self._close(sync_gradients=True)

    def _prepare_grads(self, tab, n, chunks) -> bool:
        """Clip the table's gradients -> whether one is non-finite.  fp32 / bf16: nothing is checked or read back, the answer is False.
        fp16: one launch group unscales, checks and clips; the host reads (norm, coefficient, flag, loss) once, as GradScaler.step synchronises."""
        args = L.ptr(self._chunk_part), L.ptr(self._norm_coef)
        if self.scaler is None:
            L.check(L.lib().vt_grad_clip_multi(L.ptr(tab), n, chunks, self.max_grad_norm, *args, _sp(self.device)), "vt_grad_clip_multi")
            return False
        L.check(L.lib().vt_grad_unscale_clip_multi(L.ptr(tab), n, chunks, self.max_grad_norm, inv_scale(self.scaler.scale), *args,
                                                   C.c_void_p(self._norm_coef.data_ptr() + 8), _sp(self.device)), "vt_grad_unscale_clip_multi")
        if self.last_loss is not None:
            self._norm_coef[3:4].copy_(self.last_loss.reshape(1))
        host = self._norm_coef.cpu()
        found_inf = int(host.view(torch.int32)[2]) != 0
        if found_inf and self.last_loss is not None and not math.isfinite(float(host[3])):
            self.scaler.skipped_nonfinite_loss += 1               # the forward overflowed: no smaller scale repairs that
        return found_inf

    def _take_step(self, tab, n, chunks) -> None:
        """The scheduler's lr, then AdamW + EMA over the table (the EMA update counted by the caller) and the 16-bit copies of the new weights."""
        self.lr = lr_at(self.base_lr, self.lr_scheduler, self.step_count, self.lr_warmup_steps * self.k)      # train.py:302 scales the warm-up by k
        self.step_count += 1
        self.opt_state.step(tab, n, chunks, self._hyper(self.step_count), self.betas, self.eps, self.wd)
        self._refresh16()
        self.weights_version += 1

    def _ema_alone(self, tab, n, chunks) -> None:
        """EMAModel.step without an optimizer step (the EMA update counted by the caller): the shadows move toward the unchanged parameters."""
        L.check(L.lib().vt_ema_multi(L.ptr(tab), n, chunks, L.ptr(self._hyper(max(1, self.step_count))), _sp(self.device)), "vt_ema_multi")

    def _close(self, sync_gradients: bool) -> None:
        """The end of a micro-batch, after its EMA update; sync_gradients: it took (or skipped) the optimizer step, which closes the window."""
        self.micro_step, self.sync_gradients = 0 if sync_gradients else self.micro_step, sync_gradients
        self.shadow_version += 1

    def moments(self, name: str):
        """AdamW's (m, v) of one parameter as fp32 device tensors of its shape (zeros before the first optimizer step); adamw8bit: dequantised."""
        p = self.p[name]
        if not self.shadow:                                       # the moments appear with the shadows
            return torch.zeros_like(p), torch.zeros_like(p)
        m, v = self.opt_state.moments(name)
        return m.view(p.shape), v.view(p.shape)

    def optimizer_state_bytes(self) -> int:
        """Bytes of AdamW state (moments, and codes + scales for adamw8bit) this trainer holds once it has stepped; EMA shadows not counted."""
        return self.opt_state.nbytes()

    def accumulate(self) -> None:
        """k > 1: fold the gradients get_loss left in `self.g` into the accumulators, scaled by 1 / k (accelerator.backward's loss / k); the
        first micro-batch of a window stores, the others add.  One launch; the fresh gradients' addresses travel as a second device array.
        With a process group of W ranks (any k) the scale is 1 / (k W) and the window's last fold is followed by the sum over the ranks, so
        that the accumulators then hold the mean gradient of all k W micro-batches on every rank: comm_dtype="fp32" all-reduces the arena;
        "bf16" folds and rounds into the bf16 buffer in one launch (vt_grad_fold_pack_multi), all-reduces that and widens it back into the
        accumulators (vt_grad_unpack_multi).  The earlier micro-batches of a window call no collective."""
        if not self._accumulates:
            raise RuntimeError("accumulate: the trainer was built with gradient_accumulation_steps=1")
        if self.micro_step >= self.k:
            raise RuntimeError("accumulate: the window is full, call optimizer_step")
        tab, n, chunks = self._table()
        fresh = torch.tensor([self._fresh_grad(name).data_ptr() for name in self.p], dtype=torch.int64).to(self.device)
        scale, add, last = 1.0 / (self.k * self.world), int(self.micro_step > 0), self.micro_step == self.k - 1
        if self.group is not None and last and self.comm_dtype == "bf16":
            L.check(L.lib().vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(fresh), n, chunks, scale, add, L.ptr(self._comm), _sp(self.device)),
                    "vt_grad_fold_pack_multi")
            self._all_reduce(self._comm)
            L.check(L.lib().vt_grad_unpack_multi(L.ptr(tab), L.ptr(self._comm), n, chunks, _sp(self.device)), "vt_grad_unpack_multi")
        else:
            L.check(L.lib().vt_grad_accum_multi(L.ptr(tab), L.ptr(fresh), n, chunks, scale, add, _sp(self.device)), "vt_grad_accum_multi")
            if self.group is not None and last:
                self._all_reduce(self._arena)
        self.micro_step += 1

    def ema_step(self) -> None:
        """EMAModel.step alone (train.py:448 on a micro-batch without an optimizer step): the shadows move toward the unchanged parameters."""
        tab, n, chunks = self._table()
        self.ema_updates += 1
        self._ema_alone(tab, n, chunks)
        self._close(sync_gradients=False)

    def train_step(self, lang_tokens, lang_attn_mask, img_tokens, state_tokens, action_gt, action_mask, ctrl_freqs, *, noise=None, timesteps=None):
        B = torch.as_tensor(action_gt).shape[0]
        if noise is None:
            noise = torch.randn(tuple(torch.as_tensor(action_gt).shape), dtype=F32, device=self.device)
        if timesteps is None:
            timesteps = torch.randint(0, self.num_train_timesteps, (B,), device=self.device)
        loss = self.get_loss(lang_tokens, lang_attn_mask, img_tokens, state_tokens, action_gt, action_mask, ctrl_freqs, noise=noise, timesteps=timesteps)
        if self._accumulates:
            self.accumulate()
        if self._accumulates and self.micro_step < self.k:
            self.ema_step()                                       # the window stays open
        else:
            self.optimizer_step()
        return loss

    # ---- state
    def grads(self):
        src = self._acc if self._accumulates else self.g
        return OrderedDict((k, src[k].detach().cpu().reshape(self.p[k].shape)) for k in self.p)

    def state_dict(self):
        return OrderedDict((k, v.detach().cpu().clone()) for k, v in self.p.items())

    def ema_state_dict(self):
        return OrderedDict((k, self.shadow.get(k, self.p[k]).detach().cpu().clone()) for k in self.p)

    def sync_to(self, runner, ema: bool = False):
        """Hand the trained (or the averaged) weights to an RDTRunner: its engine rebuilds on the next call."""
        runner.load_state_dict(self.ema_state_dict() if ema else self.state_dict())
        return runner

    def sampler(self, ema: bool = False):
        """An RDTRunner on the live weights (ema=True: on the averaged ones) for sampling during training (train.py:462-475 evaluates
        `rdt.predict_action` on the weights being trained).  Built once from the runner's constructor arguments and kept; its engine holds
        copies of its own in the runner's execution dtype, overwritten from the fp32 master parameters (or the EMA shadows) by
        device-to-device copies, and repacked, only when the source changed since the last hand-over (an optimizer step or load_checkpoint;
        for the shadows also an EMA-only micro-batch) or `ema` changed (`sampler_repacks` counts the hand-overs).  No weight passes through host memory, unlike `sync_to`.
        `release_sampler()` frees the runner and its engine."""
        if self.config is None:
            raise RuntimeError("sampler needs the runner's constructor arguments: build the trainer with RDTRunner.trainer()")
        from_shadow = bool(ema) and bool(self.shadow)             # before the first optimizer step the average is the parameters
        key = (from_shadow, self.shadow_version if from_shadow else self.weights_version)
        if self._sampler is None:
            from models.rdt_runner import RDTRunner
            cfg = dict(self.config)
            dt = cfg.pop("dtype", "bfloat16")
            self._sampler = RDTRunner(dtype=getattr(torch, dt.replace("torch.", "")) if isinstance(dt, str) else dt, device=self.device,
                                      init_weights=False, **cfg)
            self._sampler_key = None
        if self._sampler_key != key:
            src = self.shadow if from_shadow else self.p
            self._sampler.adopt_weights(OrderedDict((k, src[k]) for k in self.p))
            self._sampler.engine()
            self._sampler_key = key
            self.sampler_repacks += 1
        return self._sampler

    def release_sampler(self) -> None:
        self._sampler = self._sampler_key = None

    def save_pretrained(self, path: str, ema: bool = False) -> None:
        """config.json (the runner's constructor arguments) + model.safetensors, as RDTRunner.from_pretrained reads them."""
        if self.config is None:
            raise RuntimeError("save_pretrained needs the runner's constructor arguments: build the trainer with RDTRunner.trainer()")
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as fjs:
            json.dump(self.config, fjs, indent=2)
        save_file({k: v.contiguous() for k, v in (self.ema_state_dict() if ema else self.state_dict()).items()}, os.path.join(path, "model.safetensors"))

    # ---- checkpoints (train.py:455-460 accelerator.save_state + the ema/ directory; :377-385 on resume)
    _HYPER = ("base_lr", "wd", "betas", "eps", "max_grad_norm", "lr_scheduler", "lr_warmup_steps", "ema_cfg")

    def save_checkpoint(self, path: str) -> None:
        """`path`/checkpoint/{model,adam_m,adam_v}.safetensors (fp32 master weights and AdamW moments), `path`/ema/ (the averaged weights as
        RDTRunner.from_pretrained reads them: the reference's checkpoint-N/ema placement) and `path`/trainer_state.json (the counters, k,
        precision, hyper-parameters, in fp16 mode `loss_scale` = the scaler's scale, tracker, skip counters and settings, and for information `world_size` and `comm_dtype`: all state is replicated, so a checkpoint resumes under any
        world size).  Only between accumulation windows, where the reference saves.  optimizer="adamw8bit" writes
        checkpoint/adam8.safetensors in place of adam_m / adam_v (codes `m8.` / `v8.` and scales `am.` / `av.` + parameter name, fp32 moments
        `m.` / `v.` of the small tensors, the two code tables) and adds `optimizer` and `block` to trainer_state.json."""
        if self.micro_step != 0:
            raise RuntimeError(f"save_checkpoint in the middle of an accumulation window ({self.micro_step} of {self.k} micro-batches): "
                               "the partial gradient sum is not part of a checkpoint")
        from safetensors.torch import save_file
        os.makedirs(os.path.join(path, "checkpoint"), exist_ok=True)
        os.makedirs(os.path.join(path, "ema"), exist_ok=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.p.items()}, os.path.join(path, "checkpoint", "model.safetensors"))
        self.opt_state.save(path)
        save_file({k: v.contiguous() for k, v in self.ema_state_dict().items()}, os.path.join(path, "ema", "model.safetensors"))
        if self.config is not None:
            with open(os.path.join(path, "ema", "config.json"), "w") as fjs:
                json.dump(self.config, fjs, indent=2)
        state = dict(step_count=self.step_count, ema_updates=self.ema_updates, global_step=self.global_step, gradient_accumulation_steps=self.k,
                     precision=self.precision, hyper={n: getattr(self, n) for n in self._HYPER}, world_size=self.world, comm_dtype=self.comm_dtype,
                     **self.opt_state.state_json)
        if self.scaler is not None:
            state["loss_scale"] = self.scaler.state()
        with open(os.path.join(path, "trainer_state.json"), "w") as fjs:
            json.dump(state, fjs, indent=2)

    def load_checkpoint(self, path: str) -> None:
        """Restore what save_checkpoint wrote into this trainer (built on the same model with the same gradient_accumulation_steps): weights,
        moments, EMA shadows, counters and hyper-parameters; training then continues bit for bit.  Unlike the reference, which starts its
        EMAModel.optimization_step at 0 again, the EMA update count is restored.  A checkpoint written by the other optimizer is refused (a
        trainer_state.json without the `optimizer` key is an "adamw" one): the two kinds of state are not converted into each other."""
        with open(os.path.join(path, "trainer_state.json")) as fjs:
            state = json.load(fjs)
        if state["gradient_accumulation_steps"] != self.k:
            raise ValueError(f"checkpoint was written with gradient_accumulation_steps={state['gradient_accumulation_steps']}, this trainer has {self.k}")
        if state.get("optimizer", "adamw") != self.optimizer:
            raise ValueError(f"checkpoint was written by optimizer={state.get('optimizer', 'adamw')!r}, this trainer has {self.optimizer!r}")
        shapes = {k: v.shape for k, v in self.p.items()}
        parts = {n: _load_matching(path, f, shapes, n) for n, f in (("p", ("checkpoint", "model.safetensors")), ("ema", ("ema", "model.safetensors")))}
        self.opt_state.load(path, state)                          # checks before it adopts: a mismatch leaves the trainer as it was
        for k, v in self.p.items():
            v.copy_(parts["p"][k])
        self.shadow = {k: parts["ema"][k].to(self.device).contiguous() for k in self.p}
        for n, val in state["hyper"].items():
            setattr(self, n, tuple(val) if n == "betas" else val)
        self.step_count, self.ema_updates = state["step_count"], state["ema_updates"]
        if self.scaler is not None:                               # an fp32 / bf16 checkpoint starts from init_scale; the other precisions ignore the key
            if "loss_scale" in state:
                self.scaler.load_state(state["loss_scale"])
            else:
                self.scaler.reset()
            self.last_step_skipped = False
        self.micro_step, self.sync_gradients, self._table_key = 0, False, None
        self.lr = lr_at(self.base_lr, self.lr_scheduler, max(0, self.step_count - 1), self.lr_warmup_steps * self.k)
        self._refresh16()
        self.weights_version += 1
        self.shadow_version += 1


# ---------------------------------------------------------------------------------------------- the loop around the trainer
def latest_checkpoint(output_dir: str) -> Optional[str]:
    """The `checkpoint-N` entry of `output_dir` with the largest N (train.py:364-367), or None."""
    if not os.path.isdir(output_dir):
        return None
    dirs = [d for d in os.listdir(output_dir) if d.startswith("checkpoint-") and d.split("-", 1)[1].isdigit()]
    return max(dirs, key=lambda d: int(d.split("-", 1)[1])) if dirs else None


def _batch_img_tokens(batch, B: int, who: str, vision_encoder, preprocessor, jitter, corrupt=None):
    """The image tokens of a collator batch: ready `img_tokens`; `images` [B, N, C, H, W] through `vision_encoder` (train.py:420-423,
    sample.py:34-36); or `frames`, B lists of N raw frames (None = missing), through `preprocessor` (vlatouch.imgprep.DevicePreprocessor,
    with the flat per-frame `jitter` and `corrupt` lists or B lists of N) and then `vision_encoder`."""
    if "img_tokens" in batch:
        return batch["img_tokens"]
    if vision_encoder is None:
        raise ValueError(f"{who}: a batch with `images` needs vision_encoder")
    if "images" in batch or "frames" not in batch:
        images = batch["images"]
        pixel_values = images.reshape(-1, *images.shape[2:])
    else:
        if preprocessor is None:
            raise ValueError(f"{who}: a batch with `frames` needs preprocessor")
        frames = batch["frames"]
        if len(frames) != B:
            raise ValueError(f"{who}: `frames` must hold B = {B} lists of frames")
        flat = [f for sample in frames for f in sample]
        if jitter is not None and len(jitter) == B and all(isinstance(j, (list, tuple)) for j in jitter):
            jitter = [p for sample in jitter for p in sample]
        if corrupt is not None and len(corrupt) == B and all(isinstance(c, (list, tuple)) for c in corrupt):
            corrupt = [p for sample in corrupt for p in sample]
        pixel_values = preprocessor(flat, jitter=jitter) if corrupt is None else preprocessor(flat, jitter=jitter, corrupt=corrupt)
    return vision_encoder(pixel_values).detach().reshape(B, -1, vision_encoder.hidden_size)


def _batch_lang_tokens(batch, who: str, text_encoder):
    if "lang_embeds" in batch:
        return batch["lang_embeds"]
    if text_encoder is None:
        raise ValueError(f"{who}: a batch with `input_ids` needs text_encoder")
    return text_encoder(input_ids=batch["input_ids"], attention_mask=batch["lang_attn_mask"])["last_hidden_state"].detach()


def prepare_batch(batch, *, vision_encoder=None, text_encoder=None, preprocessor=None, jitter=None, corrupt=None) -> dict:
    """What train.py:407-437 does between the loader and `rdt(...)`: the reference collator's mapping -> `train_step`'s keyword arguments.
    `states[:, -1:, :]` is the state token, `state_elem_mask.unsqueeze(1)` the action mask, `actions` the target, `ctrl_freqs` and
    `lang_attn_mask` pass as they are; the language is `lang_embeds` or `input_ids` through `text_encoder`; the image tokens are `img_tokens`,
    `images` through `vision_encoder`, or (not in the reference) raw `frames` through `preprocessor` and `vision_encoder`, with the colour
    augmentation `jitter` and the corruption `corrupt` (the arguments, or the batch's keys of those names; vlatouch.imgaug.draw_image_aug)
    applied on the device.  Optional
    `noise` / `timesteps` keys prescribe train_step's two random draws."""
    states = torch.as_tensor(batch["states"])
    B = states.shape[0]
    if jitter is None:
        jitter = batch.get("jitter")
    if corrupt is None:
        corrupt = batch.get("corrupt")
    kw = {"lang_tokens": _batch_lang_tokens(batch, "prepare_batch", text_encoder), "lang_attn_mask": batch["lang_attn_mask"],
          "img_tokens": _batch_img_tokens(batch, B, "prepare_batch", vision_encoder, preprocessor, jitter, corrupt),
          "state_tokens": states[:, -1:, :], "action_gt": batch["actions"], "action_mask": torch.as_tensor(batch["state_elem_mask"]).unsqueeze(1),
          "ctrl_freqs": batch["ctrl_freqs"]}
    for key in ("noise", "timesteps"):                # train_step's two random draws, where a batch prescribes them (tests)
        if batch.get(key) is not None:
            kw[key] = batch[key]
    return kw


def sample_eval(runner, batches, *, num_sample_batches: int, dataset_id2name, vision_encoder=None, text_encoder=None, return_raw: bool = False,
                preprocessor=None, group=None):
    """`log_sample_res` (train/sample.py:7-98): sample an action chunk with `runner.predict_action` for the first `num_sample_batches` items of
    `batches` and report, per dataset and overall, the masked MSE and the masked, state-norm-relative L2 error against the ground truth.

    A batch is the reference collator's mapping: `data_indices` (a list of dataset ids), `ctrl_freqs`, `state_norm` [B, A], `states`
    [B, T, A] (the last one is the state token), `actions` [B, horizon, A], `state_elem_mask` [B, A], `lang_attn_mask`; the language as
    `lang_embeds` or as `input_ids` for `text_encoder`; the images as `images` [B, N, C, H, W] for `vision_encoder` (reshaped to
    (B, -1, vision_encoder.hidden_size), sample.py:34-36) or, not in the reference, as ready `img_tokens` or as raw `frames` (B lists of N,
    through `preprocessor` and `vision_encoder`, see prepare_batch); an optional `x_init` replaces
    predict_action's draw of the start noise.  `dataset_id2name`: a mapping id -> name (or a sequence of names).

    One vt_sample_metrics launch per batch adds into sums on the device; they are read once, after the last batch.  -> the reference's dict:
    `<name>_sample_mse` / `<name>_sample_l2err` = mean over that dataset's samples, for the datasets that occurred, and
    `overall_avg_sample_mse` / `overall_avg_sample_l2err` = sum of the batches' overall values / num_sample_batches (also when `batches` ends
    early, as there), all rounded to 4 decimals.  return_raw=True: (that dict, the same keys unrounded).

    group: a process group of W ranks, each evaluating its own `num_sample_batches` items.  The device-resident sums and counts are
    all-reduced once, a dataset's sums are divided by its sample count over all ranks and the overall pair by num_sample_batches * W
    (`accelerator.gather(...).mean()`, sample.py:80-85); every rank returns the same dict, which names the datasets any rank saw."""
    acc, count, keys = sample_eval_sums(runner, batches, num_sample_batches=num_sample_batches, dataset_id2name=dataset_id2name,
                                        vision_encoder=vision_encoder, text_encoder=text_encoder, preprocessor=preprocessor, group=group)
    if acc is None:                                                      # no batch: the reference returns an empty dict
        return ({}, {}) if return_raw else {}
    world = 1
    if group is not None:
        import torch.distributed as dist
        world = dist.get_world_size(group)
    raw = sample_eval_means(acc, count, keys, num_sample_batches * world)
    metrics = {name: round(v, 4) for name, v in raw.items()}
    return (metrics, raw) if return_raw else metrics


def sample_eval_sums(runner, batches, *, num_sample_batches: int, dataset_id2name, vision_encoder=None, text_encoder=None, preprocessor=None,
                     group=None):
    """The sums behind `sample_eval` (its arguments): -> (acc [n + 1, 2] fp64: per dataset row, and overall in the last row, the summed MSE and
    L2 error; count [n + 1] int32: the samples per row; keys: result key -> (row, column)), all on the host, or (None, None, {}) when there
    was no batch and no group.  With a group the sums and counts are those of all ranks."""
    ids = list(dataset_id2name.keys()) if hasattr(dataset_id2name, "keys") else list(range(len(dataset_id2name)))
    if not ids:
        raise ValueError("sample_eval: dataset_id2name is empty")
    if int(num_sample_batches) != num_sample_batches or num_sample_batches < 1:
        raise ValueError(f"sample_eval: num_sample_batches must be an integer >= 1, got {num_sample_batches!r}")
    row_of = {i: r for r, i in enumerate(ids)}
    n = len(ids)
    state = None
    keys: "OrderedDict[str, tuple]" = OrderedDict()                      # result key -> (row, column), in the order the reference's dict gets them
    for step, batch in enumerate(batches):
        if step >= num_sample_batches:
            break
        data_indices = [int(i) for i in batch["data_indices"]]
        for i in data_indices:
            if i not in row_of:
                raise ValueError(f"sample_eval: data_indices entry {i} is not a key of dataset_id2name")
        if state is None:
            dev, lib = L.require_gpu(runner.device), L.lib()
            f32 = lambda t: torch.as_tensor(t).to(dev, F32).contiguous()
            # acc [n + 1][2] fp64 followed by count [n + 1] int32 in one buffer: one copy to the host ends the evaluation
            state = torch.zeros(2 * (n + 1) + (n + 2) // 2, dtype=torch.float64, device=dev)
            acc, count = state[:2 * (n + 1)], state[2 * (n + 1):].view(torch.int32)
        actions, mask, state_norm = f32(batch["actions"]), f32(batch["state_elem_mask"]), f32(batch["state_norm"])
        B, H, A = actions.shape
        if len(data_indices) != B or mask.shape != (B, A) or state_norm.shape != (B, A):
            raise ValueError("sample_eval: data_indices must hold B entries, state_elem_mask and state_norm must be [B, action_dim]")
        img_tokens = _batch_img_tokens(batch, B, "sample_eval", vision_encoder, preprocessor, batch.get("jitter"), batch.get("corrupt"))
        lang_attn_mask = batch["lang_attn_mask"]
        lang_tokens = _batch_lang_tokens(batch, "sample_eval", text_encoder)
        kw = {"x_init": batch["x_init"]} if batch.get("x_init") is not None else {}
        pred = runner.predict_action(lang_tokens=lang_tokens, lang_attn_mask=lang_attn_mask, img_tokens=img_tokens,
                                     state_tokens=torch.as_tensor(batch["states"])[:, -1:, :], action_mask=mask.unsqueeze(1),
                                     ctrl_freqs=batch["ctrl_freqs"], **kw).contiguous()
        if pred.shape != actions.shape or pred.device != actions.device:
            raise ValueError(f"sample_eval: predict_action returned {tuple(pred.shape)} on {pred.device}, actions are {tuple(actions.shape)} on {actions.device}")
        rows = torch.tensor([row_of[i] for i in data_indices], dtype=torch.int32).to(dev)
        out = _empty((2 * B + 2,), dev)                                  # per_sample [B][2] | overall [2]
        ws = torch.empty(3 * B, dtype=torch.float64, device=dev)
        L.check(lib.vt_sample_metrics(L.ptr(pred), _dt(pred), L.ptr(actions), L.ptr(mask), L.ptr(state_norm), L.ptr(rows), B, H, A, n, L.ptr(out),
                                      C.c_void_p(out.data_ptr() + 8 * B), L.ptr(acc), L.ptr(count), L.ptr(ws), _sp(dev)), "vt_sample_metrics")
        for col, suffix in enumerate(("_sample_mse", "_sample_l2err")):
            for i in data_indices:
                keys.setdefault(dataset_id2name[i] + suffix, (row_of[i], col))
        keys.setdefault("overall_avg_sample_mse", (n, 0))
        keys.setdefault("overall_avg_sample_l2err", (n, 1))
    if group is not None:
        from . import dist as D
        if state is None:                                                # this rank had no batch: it still takes part in the sum
            dev = L.require_gpu(runner.device)
            state = torch.zeros(2 * (n + 1) + (n + 2) // 2, dtype=torch.float64, device=dev)
            acc, count = state[:2 * (n + 1)], state[2 * (n + 1):].view(torch.int32)
        both = D.all_reduce_sum_(torch.cat([acc, count[:n + 1].to(torch.float64)]), group).cpu()      # counts are exact in fp64; one collective
        acc_h, count_h = both[:2 * (n + 1)].view(n + 1, 2), both[2 * (n + 1):].to(torch.int32)
        for col, suffix in enumerate(("_sample_mse", "_sample_l2err")):   # the datasets only other ranks saw
            for i in ids:
                if int(count_h[row_of[i]]) > 0:
                    keys.setdefault(dataset_id2name[i] + suffix, (row_of[i], col))
        if int(count_h[:n].sum()) > 0:
            keys.setdefault("overall_avg_sample_mse", (n, 0))
            keys.setdefault("overall_avg_sample_l2err", (n, 1))
        return acc_h, count_h, keys
    if state is None:
        return None, None, keys
    host = state.cpu()                                                   # the evaluation's one device read
    return host[:2 * (n + 1)].view(n + 1, 2), host[2 * (n + 1):].view(torch.int32)[:n + 1], keys


def sample_eval_means(acc, count, keys, num_sample_batches: int) -> dict:
    """The divisions at the end of log_sample_res (sample.py:88-93) on the sums vt_sample_metrics left: acc [n + 1][2] fp64, count [n + 1];
    keys: result key -> (row, column).  A dataset's sums are divided by its sample count, the overall sums (row n) by num_sample_batches."""
    last = acc.shape[0] - 1
    return {name: float(acc[r, c]) / (num_sample_batches if r == last else int(count[r])) for name, (r, c) in keys.items()}


def finetune(trainer: RdtTrainer, batches, *, max_train_steps: int, checkpointing_period: Optional[int] = None, output_dir: Optional[str] = None,
             resume_from_checkpoint: Optional[str] = None, sample_period: int = -1, sample_batches=None, num_sample_batches: int = 2,
             dataset_id2name=None, sample_ema: bool = False, log=None, vision_encoder=None, text_encoder=None, preprocessor=None) -> List[torch.Tensor]:
    """The reference's loop (train.py:359-489) around `trainer.train_step`: every item of `batches` is one micro-batch, a mapping of train_step's
    keyword arguments, or the reference collator's mapping (recognised by its `states` key, which train_step does not take), which goes through
    `prepare_batch` with the loop's `vision_encoder`, `text_encoder` and `preprocessor`.  Stops when `global_step` reaches `max_train_steps` (optimizer steps taken or, in fp16 mode, skipped: the reference counts both); writes `output_dir`/checkpoint-{global_step} every
    `checkpointing_period` of them; `resume_from_checkpoint` = a checkpoint's name under `output_dir` or "latest" (a missing one starts a
    new run, as there); ends with save_pretrained(output_dir) and the averaged weights in `output_dir`/ema.  Like the reference's loop it does
    not skip the batches an earlier run consumed: `batches` continues where the caller wants.  sample_period > 0: after every optimizer step with
    global_step % sample_period == 0, and after that step's checkpoint (train.py:455-475), `sample_eval` runs on `trainer.sampler(ema=sample_ema)`
    over `sample_batches` (iterated afresh at each visit; `vision_encoder` / `text_encoder` go to it for batches with `images` / `input_ids`)
    and `log(metrics, global_step)` is called if given (an fp16 trainer adds `loss_scale`, `skipped_steps` and `skipped_nonfinite_loss` to the metrics); the evaluation reads the weights and writes none.  -> the micro-batch losses (device tensors).
    A trainer built with a process group: every rank runs this loop on its own micro-batches (`EpisodeStore.batches(rank=, world_size=)`); rank 0
    alone writes the checkpoints and the final weights, with a barrier behind each write, and alone calls `log`; the sampling evaluation runs on
    every rank and is reduced over the group (`sample_eval(group=)`); a resume loads the checkpoint on every rank."""
    group = getattr(trainer, "group", None)
    writer = group is None or trainer.rank == 0

    def written():
        if group is not None:
            import torch.distributed as dist
            dist.barrier(group=group)
    if (checkpointing_period or resume_from_checkpoint) and output_dir is None:
        raise ValueError("finetune: checkpointing_period / resume_from_checkpoint need output_dir")
    if sample_period is not None and sample_period > 0 and (sample_batches is None or dataset_id2name is None):
        raise ValueError("finetune: sample_period > 0 needs sample_batches and dataset_id2name")
    if resume_from_checkpoint:
        name = latest_checkpoint(output_dir) if resume_from_checkpoint == "latest" else os.path.basename(os.path.normpath(resume_from_checkpoint))
        if name is not None and os.path.isdir(os.path.join(output_dir, name)):
            trainer.load_checkpoint(os.path.join(output_dir, name))
    losses = []
    for batch in batches:
        if trainer.global_step >= max_train_steps:
            break
        if "states" in batch:
            batch = prepare_batch(batch, vision_encoder=vision_encoder, text_encoder=text_encoder, preprocessor=preprocessor)
        losses.append(trainer.train_step(**batch))
        if trainer.sync_gradients and checkpointing_period and trainer.global_step % checkpointing_period == 0:
            if writer:
                trainer.save_checkpoint(os.path.join(output_dir, f"checkpoint-{trainer.global_step}"))
            written()
        if trainer.sync_gradients and sample_period is not None and sample_period > 0 and trainer.global_step % sample_period == 0:
            metrics = sample_eval(trainer.sampler(ema=sample_ema), sample_batches, num_sample_batches=num_sample_batches,
                                  dataset_id2name=dataset_id2name, vision_encoder=vision_encoder, text_encoder=text_encoder, preprocessor=preprocessor,
                                  group=group)
            if getattr(trainer, "scaler", None) is not None:   # fp16: where the scale stands and how often it backed off
                metrics = dict(metrics, loss_scale=trainer.loss_scale_value, skipped_steps=trainer.skipped_steps,
                               skipped_nonfinite_loss=trainer.skipped_nonfinite_loss)
            if log is not None and writer:
                log(metrics, trainer.global_step)
    if output_dir is not None:
        if trainer.micro_step != 0:
            raise RuntimeError("finetune: the batches ended in the middle of an accumulation window")
        if writer:
            trainer.save_pretrained(output_dir)
            trainer.save_pretrained(os.path.join(output_dir, "ema"), ema=True)
        written()
    return losses
