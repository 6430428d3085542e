"""Host side of the block-wise 8-bit AdamW state (csrc/vt_adam8.hip, `RdtTrainer(optimizer="adamw8bit")`): the two code tables, their
decision boundaries, thin wrappers of the stand-alone quantise / dequantise launches, and `Moments8`, the store a trainer holds.

The dynamic block-wise quantisation of Dettmers et al., "8-bit Optimizers via Block-wise Quantization", as DESIGN.md §8 states it (UNPINNED
against bitsandbytes, which this project does not depend on).  Two tables of 256 fp32 values, computed in fp64, sorted ascending and rounded
once to fp32: for decade i = 0 .. 6 the midpoints of n_i equal sub-intervals of [0.1, 1], times 10^(i - 6);
  T_s (signed, first moment):    n_i = 2^i,       those values, their negatives, 0 and 1   (0 is index 127; there is no -1)
  T_u (unsigned, second moment): n_i = 2^(i + 1), those values, 0 and 1                    (0 is index 0)
Boundaries B[j] = fp32(((double)T[j] + (double)T[j + 1]) / 2), j < 255; the code of x is the number of boundaries strictly below x: the
nearest table value, ties to the lower index.  A value is T[code] * absmax of its block of BLOCK consecutive elements."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib as L

BLOCK = 256              # elements per scale
MIN_8BIT_SIZE = 4096     # tensors below it keep fp32 moments (bitsandbytes' min_8bit_size)
ZERO_CODE_SIGNED, ZERO_CODE_UNSIGNED = 127, 0


def _decades(first_n: int) -> np.ndarray:
    vals = []
    for i in range(7):
        n = first_n << i
        vals.append((0.1 + 0.9 * (np.arange(n, dtype=np.float64) + 0.5) / n) * 10.0 ** (i - 6))
    return np.concatenate(vals)


def code_tables():
    """-> (T_s, T_u): float32 [256] each."""
    s, u = _decades(1), _decades(2)
    ts = np.sort(np.concatenate([-s, s, [0.0, 1.0]])).astype(np.float32)
    tu = np.sort(np.concatenate([u, [0.0, 1.0]])).astype(np.float32)
    assert ts.shape == tu.shape == (256,)
    return ts, tu


def boundaries(table: np.ndarray) -> np.ndarray:
    """float32 [255]: the midpoints of neighbouring table values, rounded once."""
    t = table.astype(np.float64)
    return ((t[:-1] + t[1:]) / 2).astype(np.float32)


def tables_buffer() -> np.ndarray:
    """float32 [1024] = T_s | T_u | B_s (+inf) | B_u (+inf): what vt_adamw8_ema_multi / vt_adam8_quantize / vt_adam8_dequantize read."""
    ts, tu = code_tables()
    inf = np.array([np.inf], dtype=np.float32)
    return np.concatenate([ts, tu, boundaries(ts), inf, boundaries(tu), inf])


def device_tables(device) -> torch.Tensor:
    return torch.from_numpy(tables_buffer()).to(device)


def nblocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def state_bytes(numels) -> int:
    """Bytes of AdamW state for tensors of these element counts: 2 codes + 2 scales per block, or 8 B per element below MIN_8BIT_SIZE."""
    return sum(2 * n + 8 * nblocks(n) if n >= MIN_8BIT_SIZE else 8 * n for n in numels)


def quantize(x: torch.Tensor, tables: torch.Tensor, signed: bool):
    """fp32 device tensor -> (codes uint8 [n], absmax fp32 [ceil(n / 256)]), one launch."""
    x = x.contiguous()
    n = x.numel()
    codes = torch.empty(n, dtype=torch.uint8, device=x.device)
    absmax = torch.empty(nblocks(n), dtype=torch.float32, device=x.device)
    L.check(L.lib().vt_adam8_quantize(L.ptr(x), L.ptr(codes), L.ptr(absmax), L.ptr(tables), int(signed), n, L.stream_ptr(x.device)), "vt_adam8_quantize")
    return codes, absmax


def dequantize(codes: torch.Tensor, absmax: torch.Tensor, tables: torch.Tensor, signed: bool) -> torch.Tensor:
    n = codes.numel()
    out = torch.empty(n, dtype=torch.float32, device=codes.device)
    L.check(L.lib().vt_adam8_dequantize(L.ptr(codes), L.ptr(absmax), L.ptr(tables), int(signed), L.ptr(out), n, L.stream_ptr(codes.device)),
            "vt_adam8_dequantize")
    return out


class Moments8:
    """The AdamW moments of a trainer's tensors in this format: uint8 codes `m` / `v` with fp32 scales `am` / `av` per BLOCK elements for a
    tensor of at least MIN_8BIT_SIZE elements, flat fp32 `m` / `v` for a smaller one.  The fp32 form with the same interface is
    vlatouch.rdt_train.Moments32.  Nothing here but `step` and `moments` launches, so a store on the CPU can zero, adopt, save and load.

    shapes: parameter name -> shape, in the order of the multi-tensor table's rows.  The state appears with `zero()` or `load()`; it is
    checkpoint/adam8.safetensors under the keys `m8.` / `v8.` / `am.` / `av.` (quantised) or `m.` / `v.` (fp32) + name, beside the two code
    tables, and `state_json` (the optimizer's name and the block size) in trainer_state.json."""
    state_json = dict(optimizer="adamw8bit", block=BLOCK)

    def __init__(self, shapes, device):
        self.numel = {k: math.prod(s) for k, s in shapes.items()}
        self.device = torch.device(device)
        self.m, self.v, self.am, self.av = {}, {}, {}, {}
        self._aux = self._tables = None

    def _spec(self, k):
        n = self.numel[k]
        if n < MIN_8BIT_SIZE:
            return (("m", torch.float32, n, 0), ("v", torch.float32, n, 0))
        return (("m8", torch.uint8, n, ZERO_CODE_SIGNED), ("v8", torch.uint8, n, ZERO_CODE_UNSIGNED),
                ("am", torch.float32, nblocks(n), 0), ("av", torch.float32, nblocks(n), 0))

    def _zeros(self):
        """Exactly zero moments in the file's layout: codes 127 / 0 with zero scales, or fp32 zeros for a small tensor."""
        return {f"{tag}.{k}": torch.full((cnt,), fill, dtype=dt, device=self.device) for k in self.numel for tag, dt, cnt, fill in self._spec(k)}

    def _state(self):
        """The live state under the file's keys (the tensors themselves, not copies)."""
        held = {"m8": self.m, "m": self.m, "v8": self.v, "v": self.v, "am": self.am, "av": self.av}
        return {f"{tag}.{k}": held[tag][k] for k in self.numel for tag, _, _, _ in self._spec(k)}

    def _adopt(self, st) -> None:
        """Take a state in the file's layout; every tensor is checked against the parameters' sizes before anything changes."""
        m, v, am, av = {}, {}, {}, {}
        for k in self.numel:
            for tag, dt, cnt, _ in self._spec(k):
                t = st.get(f"{tag}.{k}")
                if t is None or t.dtype != dt or t.numel() != cnt:
                    raise ValueError(f"adamw8bit state: {tag}.{k} missing or not {cnt} x {dt}")
                {"m8": m, "m": m, "v8": v, "v": v, "am": am, "av": av}[tag][k] = t.to(self.device).contiguous().reshape(cnt)
        self.m, self.v, self.am, self.av = m, v, am, av
        aux = [[am[k].data_ptr(), av[k].data_ptr()] if k in am else [0, 0] for k in self.numel]    # {am, av} per row of the table, a null pair where the
        self._aux = torch.tensor(aux, dtype=torch.int64).to(self.device)                           # moments are fp32; the state does not move: built once
        if self._tables is None:
            self._tables = device_tables(self.device)

    def zero(self) -> None:
        self._adopt(self._zeros())

    def columns(self, k):
        """The m / v addresses of tensor k's row of the multi-tensor table."""
        return self.m[k].data_ptr(), self.v[k].data_ptr()

    def step(self, table, ntensors, chunks, hyper, betas, eps, wd) -> None:
        """AdamW + EMA over a table whose m / v columns are `columns()` of every tensor, in the order of `shapes`: one launch."""
        L.check(L.lib().vt_adamw8_ema_multi(L.ptr(table), L.ptr(self._aux), L.ptr(self._tables), ntensors, chunks, L.ptr(hyper), betas[0], betas[1],
                                            eps, wd, L.stream_ptr(self.device)), "vt_adamw8_ema_multi")

    def moments(self, k):
        """(m, v) of tensor k dequantised: flat fp32 tensors, not views of the state."""
        if k not in self.am:
            return self.m[k].clone(), self.v[k].clone()
        return dequantize(self.m[k], self.am[k], self._tables, True), dequantize(self.v[k], self.av[k], self._tables, False)

    def nbytes(self) -> int:
        """Bytes of the state, held or, before it appears, counted from the shapes."""
        if self.m:
            return sum(t.numel() * t.element_size() for t in self._state().values())
        return state_bytes(self.numel.values())

    def save(self, path: str) -> None:
        from safetensors.torch import save_file
        st = {k: t.detach().cpu().contiguous() for k, t in (self._state() if self.m else self._zeros()).items()}
        st["table_signed"], st["table_unsigned"] = (torch.from_numpy(t) for t in code_tables())
        save_file(st, os.path.join(path, "checkpoint", "adam8.safetensors"))

    def load(self, path: str, state: dict) -> None:
        """Adopt what `save` wrote under `path`; `state` is its trainer_state.json.  Raises ValueError, leaving this store as it was, unless the
        block size, both code tables bit for bit and every tensor's size and dtype are this build's."""
        from safetensors.torch import load_file
        if state.get("block") != BLOCK:
            raise ValueError(f"checkpoint {path}: adamw8bit block size {state.get('block')!r}, this build has {BLOCK}")
        st = load_file(os.path.join(path, "checkpoint", "adam8.safetensors"))
        for key, want in zip(("table_signed", "table_unsigned"), code_tables()):
            got = st.pop(key, None)
            if got is None or got.dtype != torch.float32 or got.shape != (256,) or not torch.equal(got.view(torch.int32), torch.from_numpy(want).view(torch.int32)):
                raise ValueError(f"checkpoint {path}: {key} is not this build's code table")
        self._adopt(st)
