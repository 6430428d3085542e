"""vt_attention (csrc/vt_attn.hip) stated in torch float64 on the CPU, the inputs its tests run on, and the grid they walk.

`reference` is softmax(scale q k^T, masked keys at -inf) v per (batch, head) in fp64 from the stored fp32 / bf16 / fp16 values the kernel gets; a
row without a valid key is zero.  `reference_rounded_p` is the same with the probabilities exp(s - rowmax) rounded to the storage type before
P V and the output rounded once (the PackP step of the 16-bit kernels): the distance between the two is what the number format alone costs, and
the only thing a tolerance may be derived from.  (The kernels of vt_attn.hip add the fp32 probabilities into the row sum before they round
them; `sum_rounded=False` states that variant.)

The inputs are shaped so that a dropped, doubled or leaked key moves a row well past the bars:
  V    column 0 = 1 (the output is 1 wherever a row has a valid key); 1..4 = indicator of the key's tile (64 keys) mod 4; 5 / 6 = the sample's
       first / last key; 7 / 8 = the first / last key of the sample's last tile; the rest N(0, 1)
  q.k  needle: one key per query row 9 above the rest (by row: the first key, the last key, the first key of the second tile, a key inside the
       last tile); uniform: small q; ascending / descending: the score is a ramp over the key index from -10 to 10, stepped from tile to tile (the running maximum moves
       in every tile and the rescale runs each time / the maximum is in tile 0 and the rescale never runs again)
Heads of 80 and 96 carry 72 real columns: columns >= 72 are zero in q, k and v, as the models pack SigLIP's heads.

`route` restates the launcher's choice of kernel and wave count (vt_attn_launch) so that the grid's coverage can be checked without a GPU; the
library exports no query for it.  Written on its own: nothing here imports the product."""
import torch

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
REAL = {64: 64, 80: 72, 96: 72}                      # real head width behind the packed one
C_ONE, C_TILE, C_FIRST, C_LAST, C_LT_FIRST, C_LT_LAST, C_RAND = 0, 1, 5, 6, 7, 8, 9
KT = 64
NEEDLE, RAMP = 9.0, 10.0
REGIMES = ("needle", "uniform", "ascending", "descending")
MASKS = ("none", "trail", "lead", "holes", "first_tile", "middle_tile", "one_key", "sample")
QKV_LAYOUTS = ("fused3", "kvhalf", "sep")
O_LAYOUTS = ("compact", "stride8", "stride2")


def scale_of(hd):
    return REAL[hd] ** -0.5


def _scores(q, k, mask, scale):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    return s, torch.where(torch.isinf(m), torch.zeros_like(m), m)


def reference(q, k, v, mask, scale):
    """q [B, Nq, H, hd], k / v [B, Nk, H, hd] (any of the three dtypes), mask [B, Nk] bool (True = attend) or None -> [B, Nq, H, hd] float64."""
    s, m = _scores(q, k, mask, scale)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    p = torch.where(l > 0, p / l, torch.zeros_like(p))
    return torch.einsum("bhqk,bkhd->bqhd", p, v.double())


def reference_rounded_p(q, k, v, mask, scale, sum_rounded=True):
    """`reference` with exp(s - rowmax) rounded to the dtype of q before P V, the row sum taken from the rounded P (or, sum_rounded=False, from
    the unrounded one) and the output rounded once; float64 throughout otherwise."""
    dt = q.dtype
    s, m = _scores(q, k, mask, scale)
    p = torch.exp(s - m)
    pr = p.to(dt).double()
    l = (pr if sum_rounded else p).sum(-1)                                   # [B, H, Nq]
    o = torch.einsum("bhqk,bkhd->bqhd", pr, v.double())
    l = l.permute(0, 2, 1)[..., None]
    o = torch.where(l > 0, o / l, torch.zeros_like(o))
    return o.to(dt).double()


def needle_keys(Nk):
    """The four keys a needle row can point at."""
    t0 = (Nk - 1) // KT * KT
    return (0, Nk - 1, KT if Nk > KT else Nk // 2, t0 + (Nk - t0) // 2)


def needle_of_row(B, H, Nq):
    """[B, Nq, H] -> which of needle_keys the row points at."""
    return (torch.arange(Nq)[None, :, None] + torch.arange(B)[:, None, None] + torch.arange(H)[None, None, :]) % 4


def make_inputs(dname, B, H, Nq, Nk, hd, regime, seed):
    """-> q [B, Nq, H, hd], k, v [B, Nk, H, hd] in the dtype `dname`."""
    g = torch.Generator().manual_seed(seed)
    real, scale = REAL[hd], scale_of(hd)
    key = torch.arange(Nk)
    t0 = (Nk - 1) // KT * KT
    v = torch.randn(B, Nk, H, hd, generator=g)
    v[..., C_ONE] = 1.0
    v[..., C_TILE:C_TILE + 4] = (key[:, None] // KT % 4 == torch.arange(4)).float()[None, :, None, :]
    for col, where in ((C_FIRST, 0), (C_LAST, Nk - 1), (C_LT_FIRST, t0), (C_LT_LAST, Nk - 1)):
        v[..., col] = (key == where).float()[None, :, None]
    k = torch.zeros(B, Nk, H, hd)
    q = torch.zeros(B, Nq, H, hd)
    if regime == "uniform":
        k[..., :real] = torch.randn(B, Nk, H, real, generator=g)
        q[..., :real] = torch.randn(B, Nq, H, real, generator=g) * 0.05
    else:                                                # a small random background on channels < 56, the structure on channels 60 ..
        k[..., :56] = torch.randn(B, Nk, H, 56, generator=g)
        q[..., :56] = torch.randn(B, Nq, H, 56, generator=g) * (0.15 if regime == "needle" else 0.05)
        if regime == "needle":                           # channel 60 + j of q meets needle key j
            for j, l in enumerate(needle_keys(Nk)):
                k[:, l, :, 60 + j] = 1.0
            q[..., 60:64] = NEEDLE / scale * torch.nn.functional.one_hot(needle_of_row(B, H, Nq), 4).float()
        else:
            # half a step up inside a tile, the next tile starts the other half above: a ragged last tile of one key still moves the maximum
            ramp = -1.0 + 2.0 * (key // KT + 0.5 * (key % KT) / (KT - 1)) / ((Nk + KT - 1) // KT - 0.5)
            k[..., 60] = (ramp if regime == "ascending" else -ramp)[None, :, None]
            q[..., 60] = RAMP / scale
    v[..., real:] = 0.0
    dt = DT[dname]
    return q.to(dt), k.to(dt), v.to(dt)


def mask_ok(kind, B, Nk):
    """Whether the mask kind exists at this shape."""
    if kind == "first_tile":
        return Nk > KT
    if kind == "middle_tile":
        return Nk > 2 * KT
    if kind in ("trail", "lead", "holes", "one_key"):
        return Nk > 1
    if kind == "sample":
        return B >= 3
    return True


def make_mask(kind, B, Nk):
    """[B, Nk] bool (True = attend) or None.  Every sample keeps at least one key except the middle one of `sample`."""
    if kind == "none":
        return None
    assert mask_ok(kind, B, Nk), (kind, B, Nk)
    keep = torch.ones(B, Nk, dtype=torch.bool)
    n = min(max(1, Nk // 3), Nk - 1)
    if kind == "trail":
        keep[:, Nk - n:] = False
    elif kind == "lead":
        keep[:, :n] = False
    elif kind == "holes":                                # every third key, shifted by the sample
        keep = (torch.arange(Nk)[None, :] + torch.arange(B)[:, None]) % 3 != 1
    elif kind == "first_tile":
        keep[:, :KT] = False
    elif kind == "middle_tile":
        t = (Nk + KT - 1) // KT // 2
        keep[:, t * KT:(t + 1) * KT] = False
    elif kind == "one_key":                              # a single valid key, never the first
        keep[:] = False
        for b in range(B):
            keep[b, 1 + (b * 37 + Nk // 2) % (Nk - 1)] = True
    elif kind == "sample":                               # the middle sample fully masked, its neighbours fully valid
        keep[B // 2] = False
    return keep


# ---- the launcher's routing, restated (vt_attn_launch)
def block_waves(Nq, Nk):
    """Waves of an attn_kernel / attn16u_kernel block: fewest padded query rows, ties to fewer waves, except 8 over 4 at Nk >= 512."""
    nw, best = 4, 1 << 30
    for w in range(4, 9):
        padded = (Nq + 16 * w - 1) // (16 * w) * (16 * w)
        if padded < best or (padded == best and Nk >= 512 and w == 8):
            best, nw = padded, w
    return nw


def route(dname, hd, masked, Nq, Nk, o_rs, knob=1):
    """-> (kernel, G, waves): "attn" (attn_kernel), "attn16u" or "attn16g"; knob = the value of vt_tune(9, .)."""
    lo = dname != "f32" and not masked and o_rs % 4 == 0
    if lo and knob and Nq >= 128 and hd in (64, 80):
        need = (Nq + 15) // 16
        G = W = 0
        if knob in (3, 6):
            cost = None
            for w in range(4, 9):
                per = knob * w
                blocks = (need + per - 1) // per
                c = (blocks, blocks * per - need, 8 - w)
                if cost is None or c < cost:
                    cost, G, W = c, knob, w
        elif hd != 80 and need <= 24:
            G, W = 6, max(4, (need + 5) // 6)
        if G:
            return "attn16g", G, W
    return ("attn16u" if lo else "attn"), 1, block_waves(Nq, Nk)


def tile_class(Nk):
    """Key tiles, the ring of three stages behaves differently at 1, 2, 3 and 4 or more."""
    return min((Nk + KT - 1) // KT, 4)


# ---- the grid of tests/test_gpu_attention.py
# B, H, Nq, Nk.  Nq -> waves of a block: <= 64: 4; 67, 80: 5; 96: 6; 100: 7; 128: 4 (8 at Nk >= 512); 129: 5, two blocks; 257: 6, three blocks, the
# last partly filled; 370: 8 waves of 3 query groups under vt_tune(9, 3) (the only way to 8 waves below 512 keys).  Nk -> key tiles: 1, 7, 63, 64: 1;
# 65, 128: 2; 130, 192: 3; 193: 4; 257: 5; 577: 10
SHAPES = [
    (1, 1, 1, 257), (3, 3, 1, 577),                                      # DINOv2's CLS-only last block: Nq = 1, o_bs = o_rs
    (3, 1, 15, 1), (1, 3, 16, 7), (3, 3, 17, 65), (1, 3, 64, 130), (3, 1, 64, 193),
    (1, 1, 67, 63), (3, 3, 67, 128), (1, 3, 80, 192), (3, 1, 80, 257),
    (3, 3, 96, 64), (1, 1, 96, 65), (3, 1, 96, 130), (1, 3, 96, 577),
    (1, 3, 100, 7), (3, 1, 100, 128), (1, 1, 100, 192), (3, 3, 100, 193),
    (3, 1, 128, 63), (1, 3, 128, 577), (1, 1, 129, 130), (3, 3, 257, 257),
    (1, 1, 370, 64), (1, 3, 370, 128), (3, 1, 370, 192),
]
KNOBS = (0, 1, 3, 6)


def knobs_of(dname, hd, mask, Nq, o_layout):
    """The values of vt_tune(9, .) a case runs under."""
    return KNOBS if dname != "f32" and mask == "none" and Nq >= 128 and o_layout != "stride2" else (1,)


def o_row_stride(o_layout, H, hd):
    return H * hd + {"compact": 0, "stride8": 8, "stride2": 2}[o_layout]


def gpu_grid():
    """List of dict(dname, hd, B, H, Nq, Nk, mask, regime, qkv, o, km_pad, seed).  Not the full product: the 16-bit unmasked kernels see every shape
    at every head dimension; fp32 every shape once; every (mask, regime) pair occurs once per dtype on a shape that admits the mask, found from
    a strided start.  Layouts are dealt round-robin; Nq = 1 always writes the compact (CLS) output."""
    out = []

    def add(dname, hd, shape, mask, regime, qkv, o, km_pad):
        B, H, Nq, Nk = shape
        if Nq == 1:
            o = "compact"
        out.append(dict(dname=dname, hd=hd, B=B, H=H, Nq=Nq, Nk=Nk, mask=mask, regime=regime, qkv=qkv, o=o, km_pad=km_pad, seed=len(out)))

    for di, dname in enumerate(("bf16", "f16")):
        for hi, hd in enumerate((64, 80, 96)):
            for si, shape in enumerate(SHAPES):
                add(dname, hd, shape, "none", REGIMES[(si + hi + di) % 4], QKV_LAYOUTS[(si + hi) % 3], O_LAYOUTS[(si + di) % 2], False)
        for n, (si, hd) in enumerate(((8, 64), (22, 96), (13, 64), (5, 96))):              # o_rs % 4 != 0: back to attn_kernel
            add(dname, hd, SHAPES[si], "none", REGIMES[(n + di) % 4], QKV_LAYOUTS[n % 3], "stride2", False)
    for si, shape in enumerate(SHAPES):
        add("f32", (64, 96)[si % 2], shape, "none", REGIMES[si % 4], QKV_LAYOUTS[si % 3], O_LAYOUTS[si % 3], False)
    for di, dname in enumerate(DT):
        pairs = [(m, r) for m in MASKS[1:] for r in REGIMES]
        for pi, (mask, regime) in enumerate(pairs):
            si = (pi * 5 + di * 3) % len(SHAPES)
            while not mask_ok(mask, SHAPES[si][0], SHAPES[si][3]):
                si = (si + 1) % len(SHAPES)
            add(dname, (64, 96)[(pi + di) % 2], SHAPES[si], mask, regime, QKV_LAYOUTS[(pi + di) % 3], O_LAYOUTS[pi % 3], pi % 2 == 1)
    return out
