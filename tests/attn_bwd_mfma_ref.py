"""The statement of vt_attention_bwd_mfma (csrc/vt_attn_bwd.hip) in torch on the CPU, the case list of its tests and their fp64 / torch-bf16
references.

Inputs: bf16 values (held in fp32 here) q, do [B, Nq, H, 64] and k, v [B, Nk, H, 64], `scale`, an optional key mask [B, Nk] (True = live).  In fp32:
    S = scale q k^T, dP = do v^T            products of bf16 values are exact, the sums are fp32
    m = max_j S, l = sum_j exp(S - m), delta = sum_j P dP   over the live keys of the row
    P = exp(S - m) / l,  dS = P (dP - delta)
    P and dS are rounded ONCE to bf16, round to nearest even (they are MFMA operands): the one rounding the wave kernel does not have
    dV = P^T do,  dK = scale dS^T q,  dQ = scale dS k        fp32 sums, rounded once to bf16
The scale is applied AFTER the rounding of dS, to the fp32 sums of dK and dQ (the kernel multiplies its accumulators at the store).
A masked key gets zero dK and dV; a row whose keys are all masked gets zero dQ and contributes nothing."""
import torch

RUN_TILES, KEY_TILE = 4, 64          # csrc/vt_attn_bwd.hip: a workgroup owns a run of RUN_TILES tiles of KEY_TILE keys

# (B, Nq, Nk, H, cross): the kernel cases.  cross = q and packed kv buffers, else one packed qkv buffer (Nq == Nk)
KERNEL_CASES = [
    (2, 1, 1, 1, False),
    (2, 5, 3, 2, True),
    (2, 31, 63, 2, True), (2, 32, 64, 2, True), (2, 33, 65, 2, True),
    (2, 67, 67, 32, False),
    (2, 67, 130, 2, True),
    (1, 128, 257, 2, True),
    (2, 67, 1024, 2, True),
    (1, 67, 4374, 2, True),
    (1, 67, (2 * RUN_TILES + 1) * KEY_TILE + 5, 2, True),        # two full runs, one tile of a third, 5 keys of the next tile
]


def bf16r(x):
    return x.bfloat16().float()


def statement(q, k, v, do, scale=0.125, mask=None):
    """-> dq, dk, dv (fp32 tensors holding bf16 values) and the row statistics (m, 1 / l, delta), each [B, H, Nq]."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    B, Nk = k.shape[0], k.shape[1]
    live = torch.ones(B, Nk, dtype=torch.bool) if mask is None else mask
    lv = live[:, None, None, :]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    dp = torch.einsum("bihd,bjhd->bhij", do, v)
    m = s.masked_fill(~lv, float("-inf")).amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))               # a row without live keys: m = 0, 1 / l = 0
    e = torch.where(lv, torch.exp(s - m), torch.zeros_like(s))
    l = e.sum(dim=-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    p = e * inv
    delta = (p * torch.where(lv, dp, torch.zeros_like(dp))).sum(dim=-1, keepdim=True)
    ds = torch.where(lv, p * (dp - delta), torch.zeros_like(p))
    p16, ds16 = bf16r(p), bf16r(ds)                                          # the one new rounding
    dv = torch.einsum("bhij,bihd->bjhd", p16, do)
    dk = torch.einsum("bhij,bihd->bjhd", ds16, q) * scale
    dq = torch.einsum("bhij,bjhd->bihd", ds16, k) * scale
    return bf16r(dq), bf16r(dk), bf16r(dv), (m[..., 0], inv[..., 0], delta[..., 0])


def make_case(B, Nq, Nk, H, cross, seed, mask=None):
    """bf16-rounded inputs built as tests/test_gpu_rdt_train.py::_attn_case builds them (packed buffers, so the views are strided).
    -> bufs (fp32 holding bf16 values), views(*bufs) -> (q, k, v), do, mask."""
    g = torch.Generator().manual_seed(seed)
    if cross:
        bufs = (torch.randn(B, Nq, H * 64, generator=g), torch.randn(B, Nk, 2 * H * 64, generator=g))
        views = lambda qb, kvb: (qb.view(B, Nq, H, 64), kvb.view(B, Nk, 2, H, 64)[:, :, 0], kvb.view(B, Nk, 2, H, 64)[:, :, 1])
    else:
        assert Nq == Nk
        bufs = (torch.randn(B, Nq, 3 * H * 64, generator=g),)
        views = lambda qkv: tuple(qkv.view(B, Nq, 3, H, 64)[:, :, i] for i in range(3))
    do = torch.randn(B, Nq, H, 64, generator=g)
    return tuple(bf16r(b) for b in bufs), views, bf16r(do), mask


def _forward(q, k, v, mask, scale):
    s = (q.permute(0, 2, 1, 3) @ k.permute(0, 2, 3, 1)) * scale
    dead = None
    if mask is not None:
        dead = ~mask.any(dim=1)
        m = mask.clone()
        m[dead] = True                       # keep the softmax finite there; the output is zeroed below, so its gradients are 0
        s = s.masked_fill(~m[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    if dead is not None:
        o = o * (~dead)[:, None, None, None].to(o.dtype)
    return o


def autograd_ref(bufs, views, do, mask, dtype, scale=0.125):
    """Autograd through softmax(scale q k^T [+ mask]) v in `dtype` (torch.float64: the reference; torch.bfloat16: torch's own bf16 CPU
    backward, the yardstick of the 1.5 x bar) -> [dq, dk, dv] as float64."""
    with torch.enable_grad():                # other test modules switch autograd off process-wide
        leaves = [b.to(dtype).clone().requires_grad_(True) for b in bufs]
        q, k, v = views(*leaves)
        (_forward(q, k, v, mask, scale) * do.to(dtype)).sum().backward()
        return [views(*[l.grad for l in leaves])[i].double() for i in range(3)]


_REFS = {}


def refs(key, bufs, views, do, mask, scale=0.125):
    """(fp64 gradients, torch-bf16 gradients) of a case, computed once per process and shared."""
    if key not in _REFS:
        _REFS[key] = (autograd_ref(bufs, views, do, mask, torch.float64, scale), autograd_ref(bufs, views, do, mask, torch.bfloat16, scale))
    return _REFS[key]
