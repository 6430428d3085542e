"""The LSTM residual head (csrc/vt_lstm.hip) restated in float64, and the grid of cases its tests walk.  No GPU code.

`reference` is oracle/controller.py::lstm_step without its .float() casts, looped over the ticks of a call: force MLP (Linear, erf-GELU,
Linear), concatenation with vla_n, `layers` LSTM cells (gate order i, f, g, o, bias b_ih + b_hh), [h_top | obs_cond] -> Linear ->
LayerNorm(eps 1e-5) -> erf-GELU -> Linear, + vla_n.  tests/test_lstm_ref_host.py holds it to torch.nn.LSTM in float64 and to the fp32 oracle;
tests/test_gpu_lstm.py holds the kernel to it."""
from __future__ import annotations

import functools
import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from tests import cases as _cases          # puts the package on sys.path
from vlatouch import synth

SD = Dict[str, torch.Tensor]
MODES = ("fp32", "x3", "bf16")
BARS = {"fp32": 2e-5, "x3": 1e-4, "bf16": 3e-2}      # tests/test_gpu_api.py::test_lstm_persistent_kernel_ragged_batches_vs_oracle's, here against float64
MODULES = ("force_encoder", "lstm", "output_head")


class Case(NamedTuple):
    hidden: int
    layers: int
    S: int          # state_dim
    F: int          # force_dim
    B: int
    T: int

    @property
    def id(self) -> str:
        return f"h{self.hidden}l{self.layers}-s{self.S}f{self.F}-b{self.B}t{self.T}"


# every (hidden, layers) pair lstm_seq_kernel is instantiated for: B = 19 is one full 16-row block and a 3-row ragged one
PAIR_CASES = [Case(H, L, 10, 3, 19, 5) for H in (128, 256, 384) for L in (1, 2, 3, 4) if (H, L) != (384, 4)]
# both maxima, both minima, and an odd pair that ends off every 4- and 8-element boundary
WIDTH_CASES = [Case(H, L, S, F, 19, 5) for H, L in ((128, 1), (256, 2), (384, 3)) for S, F in ((16, 32), (1, 1), (7, 17))]
# exactly one block, and one row past it
BLOCK_CASES = [Case(256, 2, 10, 3, 16, 1), Case(256, 2, 10, 3, 17, 5)]
CASES = PAIR_CASES + WIDTH_CASES + BLOCK_CASES

# Saturated gates: the LSTM weight matrices times a scale (biases as they are).  Times 40 the pre-activations reach +-80, but fp32 itself no
# longer resolves the recurrence there: the fp32 oracle is 7e-5 from float64 after one tick and 6e-3 after five (an unsaturated unit's sum of
# terms 40 times larger carries 40 times the rounding, and 40 W_hh amplifies it tick after tick).  The scale at which the oracle is back inside
# its 3e-6 is 3.5 over two ticks (1.9e-6; 2.9e-6 at 4, 3.7e-6 at 3.5 over five ticks): the parity bars are applied there, |W_hh h| up to 7 and
# whole pre-activations past 10.  Times SATURATED_TAIL_SCALE only what holds at any scale is asked: finite, |h| <= 1.
SATURATED = Case(256, 2, 10, 3, 19, 2)
SATURATED_SCALE = 3.5
SATURATED_TAIL_SCALE = 40.0

MISTAKES = ("state_column", "force_column", "bias_hh", "head_row", "gates_f_o")


@functools.lru_cache(maxsize=None)
def mods(hidden: int, layers: int, state_dim: int = 10, force_dim: int = 3) -> Dict[str, SD]:
    """The head's three modules as fp32 state dicts, their own deterministic weights per (hidden, layers, state_dim, force_dim)."""
    shp = synth.lstm_controller_shapes(384, state_dim, hidden, layers, force_dim)
    tag = f"lstm_ref.h{hidden}l{layers}s{state_dim}f{force_dim}."
    return {m: _cases.sd_torch(shp[m], prefix=f"{tag}{m}.") for m in MODULES}


def scaled(m: Dict[str, SD], scale: float) -> Dict[str, SD]:
    """`m` with the LSTM weight matrices times `scale`."""
    out = {k: dict(v) for k, v in m.items()}
    out["lstm"] = {k: v * scale if v.dim() == 2 else v for k, v in m["lstm"].items()}
    return out


def rounded(m: Dict[str, SD], dtype: torch.dtype = torch.bfloat16) -> Dict[str, SD]:
    """The weight matrices rounded to `dtype` and back; biases and LayerNorm parameters stay fp32, as LstmEngine keeps them."""
    return {name: {k: v.to(dtype).float() if v.dim() == 2 else v for k, v in sd.items()} for name, sd in m.items()}


def case_mods(case: Case) -> Dict[str, SD]:
    return mods(case.hidden, case.layers, case.S, case.F)


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Dict[str, torch.Tensor]:
    """fp32 inputs of a case: obs_cond ~ N(0,1), vla_n ~ U(-1,1), force ~ N(0,1) and a carried state 0.5 N(0,1); every batch row its own draw."""
    H, L, S, F, B, T = case
    g = synth.inputs_rng(((((H * 5 + L) * 17 + S) * 33 + F) * 64 + B) * 32 + T)
    t = _cases.T
    return dict(obs_cond=t(g.standard_normal((B, H), dtype=np.float32)),
                vla_n=t(g.uniform(-1, 1, (B, T, S)).astype(np.float32)),
                force=t(g.standard_normal((B, T, F), dtype=np.float32)),
                h0=t(0.5 * g.standard_normal((L, B, H), dtype=np.float32)),
                c0=t(0.5 * g.standard_normal((L, B, H), dtype=np.float32)))


def _gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _linear(x, w, b):
    return x @ w.T + b


def _planted(m: Dict[str, SD], layers: int, mistake: Optional[str]) -> Dict[str, SD]:
    """float64 copies of the weights, with one of MISTAKES planted."""
    m = {name: {k: v.double().clone() for k, v in sd.items()} for name, sd in m.items()}
    last = layers - 1
    lstm = m["lstm"]
    if mistake is None:
        pass
    elif mistake == "state_column":          # the last live column of the padded layer-0 input tile
        lstm["weight_ih_l0"][:, -1] = 0
    elif mistake == "force_column":          # the last live column of the one-k-step force tile
        m["force_encoder"]["0.weight"][:, -1] = 0
    elif mistake == "bias_hh":
        lstm[f"bias_hh_l{last}"].zero_()
    elif mistake == "head_row":              # the last stored row of the 16-row output tile
        m["output_head"]["4.weight"][-1] = 0
    elif mistake == "gates_f_o":
        for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            i, f, g, o = lstm[f"{k}_l{last}"].chunk(4, dim=0)
            lstm[f"{k}_l{last}"] = torch.cat((i, o, g, f), dim=0)
    else:
        raise ValueError(mistake)
    return m


def cell_stack(lstm: SD, x: torch.Tensor, h: torch.Tensor, c: torch.Tensor, layers: int):
    """One tick of `layers` LSTM cells in the dtype of its arguments: (h_top, h', c')."""
    h2, c2 = [], []
    for l in range(layers):
        z = _linear(x, lstm[f"weight_ih_l{l}"], lstm[f"bias_ih_l{l}"]) + _linear(h[l], lstm[f"weight_hh_l{l}"], lstm[f"bias_hh_l{l}"])
        i, f, g, o = z.chunk(4, dim=-1)
        cl = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
        x = torch.sigmoid(o) * torch.tanh(cl)
        h2.append(x)
        c2.append(cl)
    return x, torch.stack(h2), torch.stack(c2)


def reference(m: Dict[str, SD], obs_cond, vla_n, force, h0, c0, layers: int, mistake: Optional[str] = None):
    """(out [B,T,S], h [layers,B,H], c [layers,B,H]) in float64 after the T ticks of vla_n [B,T,S] / force [B,T,F] from the state (h0, c0)."""
    m = _planted(m, layers, mistake)
    fe, head = m["force_encoder"], m["output_head"]
    obs, vla, force = obs_cond.double(), vla_n.double(), force.double()
    h, c = h0.double(), c0.double()
    outs = []
    for t in range(vla.shape[1]):
        f = _linear(_gelu(_linear(force[:, t], fe["0.weight"], fe["0.bias"])), fe["2.weight"], fe["2.bias"])
        top, h, c = cell_stack(m["lstm"], torch.cat((f, vla[:, t]), dim=-1), h, c, layers)
        y = _linear(torch.cat((top, obs), dim=-1), head["0.weight"], head["0.bias"])
        mu = y.mean(dim=-1, keepdim=True)
        var = ((y - mu) ** 2).mean(dim=-1, keepdim=True)
        y = _gelu((y - mu) / torch.sqrt(var + 1e-5) * head["1.weight"] + head["1.bias"])
        outs.append(vla[:, t] + _linear(y, head["4.weight"], head["4.bias"]))
    return torch.stack(outs, dim=1), h, c


@functools.lru_cache(maxsize=None)
def case_reference(case: Case, weights: str = "fp32"):
    """reference() of a case, computed once: weights "fp32" as drawn, "bf16" rounded (the bf16 mode's bar then measures activation rounding
    only).  Callers leave the result unchanged."""
    m = case_mods(case)
    i = inputs(case)
    return reference(rounded(m) if weights == "bf16" else m, i["obs_cond"], i["vla_n"], i["force"], i["h0"], i["c0"], case.layers)


def max_err(got, ref) -> float:
    """max|got - ref| over (out, h, c) triples or single tensors, in float64; inf where `got` is not finite."""
    if isinstance(got, torch.Tensor):
        got, ref = (got,), (ref,)
    worst = 0.0
    for a, b in zip(got, ref):
        a = a.detach().cpu().double()
        assert a.shape == b.shape, (a.shape, b.shape)
        if not bool(torch.isfinite(a).all()):
            return float("inf")
        worst = max(worst, float((a - b.double()).abs().max()))
    return worst
