"""Plain-torch restatement of the T5 v1.1 encoder (HF T5EncoderModel, gated-gelu), used only by tests.

Pinned to HF's own output by tests/test_t5_host.py (g15), so GPU tests can compare sizes too large for a golden
(L = 1024, XXL width) without importing transformers.  Runs in fp32 (or fp64) on whatever device the tensors are on."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from vlatouch import synth
from vlatouch.t5 import bucket_table, embed_key


def t5_sd(name: str, **over) -> Dict[str, torch.Tensor]:
    """Deterministic synthetic HF state dict of synth.T5_CONFIGS[name] (the same weights tools/make_golden_t5.py gives HF)."""
    return synth.torch_state_dict(synth.t5_shapes(**synth.t5_config(name, **over)), prefix="t5.")


def _rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def encode(sd, cfg: Dict, ids: torch.Tensor, mask: Optional[torch.Tensor] = None, dtype=torch.float32, operands=None) -> torch.Tensor:
    """last_hidden_state [B, L, d_model] of HF T5EncoderModel for input_ids `ids` [B, L] and attention_mask `mask`.
    operands=torch.bfloat16 rounds the GEMM weights and every hand-off the engine's bf16 mode stores in bf16 (normed activations, q / k / v,
    softmax probabilities, attention output, wi_0 / wi_1 outputs, gated product); the residual stream stays `dtype` — the engine's precision model."""
    R = (lambda t: t.to(operands).to(dtype)) if operands is not None else (lambda t: t)  # noqa: E731
    W = lambda k: R(sd[k].to(dtype)) if sd[k].dim() == 2 and "relative_attention_bias" not in k else sd[k].to(dtype)  # noqa: E731
    dev = ids.device
    B, L = ids.shape
    H, dk, eps = cfg["num_heads"], cfg.get("d_kv", 64), cfg.get("layer_norm_epsilon", 1e-6)
    x = W(embed_key(sd.keys())).to(dev)[ids.long()]                              # (the embedding table is a weight: bf16 in that mode)
    tab = torch.from_numpy(bucket_table(cfg.get("relative_attention_num_buckets", 32), cfg.get("relative_attention_max_distance", 128)))
    rel = torch.arange(L)[None, :] - torch.arange(L)[:, None]                     # j - i
    buckets = tab.long()[rel + 1023].to(dev)
    bias = W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").to(dev)[buckets].permute(2, 0, 1)[None]  # [1, H, L, L]
    if mask is not None:
        bias = bias + (1.0 - mask.to(dev, dtype)[:, None, None, :]) * torch.finfo(dtype).min
    for i in range(cfg["num_layers"]):
        a = f"encoder.block.{i}.layer.0."
        h = R(_rms(x, W(a + "layer_norm.weight").to(dev), eps))
        q, k, v = (R(torch.nn.functional.linear(h, W(a + f"SelfAttention.{n}.weight").to(dev))).view(B, L, H, dk).transpose(1, 2) for n in "qkv")
        att = R(torch.softmax(q @ k.transpose(-1, -2) + bias, dim=-1))              # no 1/sqrt(d) scale
        o = R(att @ v).transpose(1, 2).reshape(B, L, H * dk)
        x = x + torch.nn.functional.linear(o, W(a + "SelfAttention.o.weight").to(dev))
        f = f"encoder.block.{i}.layer.1."
        h = R(_rms(x, W(f + "layer_norm.weight").to(dev), eps))
        g = R(torch.nn.functional.linear(h, W(f + "DenseReluDense.wi_0.weight").to(dev)))
        g = 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g.pow(3))))   # HF gelu_new
        x = x + torch.nn.functional.linear(R(g * R(torch.nn.functional.linear(h, W(f + "DenseReluDense.wi_1.weight").to(dev)))),
                                           W(f + "DenseReluDense.wo.weight").to(dev))
    return _rms(x, W("encoder.final_layer_norm.weight").to(dev), eps)
