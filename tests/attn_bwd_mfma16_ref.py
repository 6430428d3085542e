"""The fp16 statement of vt_attention_bwd_mfma (csrc/vt_attn_bwd.hip, half_t instantiation): tests/attn_bwd_mfma_ref.py's arithmetic with the
rounding swapped, the six shapes of the fp16 attention-backward tests and their fp64 / torch-fp16 references.

Inputs: fp16 values (held in fp32 here).  In fp32: S = scale q k^T, dP = do v^T (products of fp16 values are exact, the sums are fp32); per
row m, l, delta over the live keys; P = exp(S - m) / l and dS = P (dP - delta) are rounded ONCE to fp16, round to nearest even, NOT clamped
(beyond 65504: inf); dV = P^T do, dK = scale dS^T q, dQ = scale dS k are fp32 sums (the scale applied to the sums) rounded once to fp16.
A masked key gets zero dK and dV; a row whose keys are all masked gets zero dQ and contributes nothing."""
import torch

from tests import attn_bwd_mfma_ref as M

# (B, Nq, Nk, H, cross, masked): cross = q and packed kv buffers, else one packed qkv buffer; masked = the last 3 keys of batch row 0 and every
# key of batch row 1 are masked.  B * H runs from 2 * 3 to 2 * 32; (128, 257) is two key runs with a ragged tile, (67, 4374) the image
# cross-attention of the step, (1, 64) a single query row against exactly one key tile.
CASES = [
    (2, 5, 3, 3, True, False),
    (2, 67, 67, 32, False, False),
    (2, 67, 20, 32, True, True),
    (2, 128, 257, 3, True, False),
    (2, 67, 4374, 4, True, False),
    (2, 1, 64, 3, True, False),
]


def f16r(x):
    return x.half().float()


def statement(q, k, v, do, scale=0.125, mask=None):
    """-> dq, dk, dv (fp32 tensors holding fp16 values, inf where fp16 overflows) and the row statistics (m, 1 / l, delta), each [B, H, Nq]."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    B, Nk = k.shape[0], k.shape[1]
    live = torch.ones(B, Nk, dtype=torch.bool) if mask is None else mask
    lv = live[:, None, None, :]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    dp = torch.einsum("bihd,bjhd->bhij", do, v)
    m = s.masked_fill(~lv, float("-inf")).amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(lv, torch.exp(s - m), torch.zeros_like(s))
    l = e.sum(dim=-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    p = e * inv
    delta = (p * torch.where(lv, dp, torch.zeros_like(dp))).sum(dim=-1, keepdim=True)
    ds = torch.where(lv, p * (dp - delta), torch.zeros_like(p))
    p16, ds16 = f16r(p), f16r(ds)                                            # the one new rounding
    dv = torch.einsum("bhij,bihd->bjhd", p16, do)
    dk = torch.einsum("bhij,bihd->bjhd", ds16, q) * scale
    dq = torch.einsum("bhij,bjhd->bihd", ds16, k) * scale
    return f16r(dq), f16r(dk), f16r(dv), (m[..., 0], inv[..., 0], delta[..., 0])


def make_case(B, Nq, Nk, H, cross, masked, seed):
    """fp16-rounded inputs on packed buffers (strided views), as tests/attn_bwd_mfma_ref.py::make_case builds its bf16 ones.
    -> bufs, views(*bufs) -> (q, k, v), do, mask (or None)."""
    g = torch.Generator().manual_seed(seed)
    if cross:
        bufs = (torch.randn(B, Nq, H * 64, generator=g), torch.randn(B, Nk, 2 * H * 64, generator=g))
        views = lambda qb, kvb: (qb.view(B, Nq, H, 64), kvb.view(B, Nk, 2, H, 64)[:, :, 0], kvb.view(B, Nk, 2, H, 64)[:, :, 1])
    else:
        assert Nq == Nk
        bufs = (torch.randn(B, Nq, 3 * H * 64, generator=g),)
        views = lambda qkv: tuple(qkv.view(B, Nq, 3, H, 64)[:, :, i] for i in range(3))
    do = torch.randn(B, Nq, H, 64, generator=g)
    mask = None
    if masked:
        mask = torch.ones(B, Nk, dtype=torch.bool)
        mask[0, Nk - 3:] = False
        mask[1, :] = False
    return tuple(f16r(b) for b in bufs), views, f16r(do), mask


_REFS = {}


def refs(case):
    """(inputs of the case, fp64 gradients, torch's own fp16 CPU backward), computed once per process and shared; never modified."""
    if case not in _REFS:
        B, Nq, Nk, H, cross, masked = case
        bufs, views, do, mask = make_case(B, Nq, Nk, H, cross, masked, seed=Nk)
        _REFS[case] = ((bufs, views, do, mask), M.autograd_ref(bufs, views, do, mask, torch.float64), M.autograd_ref(bufs, views, do, mask, torch.float16))
    return _REFS[case]
