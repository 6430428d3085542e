"""Host side of the block-wise 8-bit AdamW state (csrc/vt_adam8.hip, `RdtTrainer(optimizer="adamw8bit")`): the two code tables, their
decision boundaries, and thin wrappers of the stand-alone quantise / dequantise launches.

The dynamic block-wise quantisation of Dettmers et al., "8-bit Optimizers via Block-wise Quantization", as DESIGN.md §8 states it (UNPINNED
against bitsandbytes, which this project does not depend on).  Two tables of 256 fp32 values, computed in fp64, sorted ascending and rounded
once to fp32: for decade i = 0 .. 6 the midpoints of n_i equal sub-intervals of [0.1, 1], times 10^(i - 6);
  T_s (signed, first moment):    n_i = 2^i,       those values, their negatives, 0 and 1   (0 is index 127; there is no -1)
  T_u (unsigned, second moment): n_i = 2^(i + 1), those values, 0 and 1                    (0 is index 0)
Boundaries B[j] = fp32(((double)T[j] + (double)T[j + 1]) / 2), j < 255; the code of x is the number of boundaries strictly below x: the
nearest table value, ties to the lower index.  A value is T[code] * absmax of its block of BLOCK consecutive elements."""
from __future__ import annotations

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
