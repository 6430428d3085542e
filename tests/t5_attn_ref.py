"""t5_attn_kernel (csrc/vt_t5.hip, reached alone through vt_t5_attention) stated in torch float64 on the CPU, the inputs its tests run on, and
the grid they walk.  Follows tests/attn_ref.py, whose mask kinds it takes over.

`reference` is softmax(q k^T + rel_bias[bucket(j - i)][h], masked keys at -inf) v per (batch, head) in fp64 from the stored fp32 / bf16 values
the kernel gets: no 1/sqrt(d) scale, the bias of T5's relative-position buckets, a row without a valid key is zero.  `reference_rounded_p` is
the same with exp(s - rowmax) rounded to the storage type before P V, the row sum taken from the unrounded values (as the kernel adds its fp32
probabilities up before it rounds them) and the output rounded once: the distance between the two is what the number format alone costs.
`reference_f32_arithmetic` evaluates the same expression in torch float32 on the CPU: what fp32 products, sums and exp cost, which rounding
an fp64 P to fp32 does not show.

The inputs are shaped so that a dropped, doubled, leaked or shifted key moves a row well past the bars:
  V    column 0 = 1; 1..4 = indicator of the key's tile (64 keys) mod 4; 5 / 6 = the first / last key; 7..14 = one-hot of key % 8 (a shift by
       one key moves all the weight to another column); 15 = the ramp key / L; the rest N(0, 1)
  q.k  uniform: small q; ascending / descending: attn_ref's ramp over the key index from -10 to 10, stepped from tile to tile, at scale 1 (the
       running maximum moves in every tile / never again), under a small bias N(0, 0.1)
       bias_random: small q, rel_bias ~ N(0, 1), every bucket matters
       bias_needle: small q, rel_bias zero except one bucket per head at +12: the bucket of rel = 0, +1, -1, +max_exact (the first logarithmic
       bucket), -max_distance (the saturated last bucket) or +(L - 1), cycling over the heads from the case's seed
Nothing here imports the product except vlatouch.t5.bucket_table, host-only and pinned to HF by tests/test_t5_host.py."""
import torch

from tests import attn_ref as A
from vlatouch.t5 import bucket_table

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
KT, HD = 64, 64
C_ONE, C_TILE, C_FIRST, C_LAST, C_HOT, C_RAMP, C_RAND = 0, 1, 5, 6, 7, 15, 16
RAMP, NEEDLE = 10.0, 12.0
REGIMES = ("uniform", "ascending", "descending", "bias_random", "bias_needle")
BIAS_REGIMES = ("bias_random", "bias_needle")
MASKS = ("none", "trail", "lead", "holes", "first_tile", "middle_tile", "one_key", "per_sample")
BUCKETS = ((32, 128), (8, 16), (126, 1000))          # (num_buckets, max_distance): v1.1's, one that saturates at distance 16, a wide one
REL_SPAN = 1023
# Bars per (batch, head) slice: random columns max|out - ref| / max|ref|, structured columns max|out - ref|.  test_gpu_attention.py's bars for the
# same arithmetic (P rounded to the storage type, fp32 sums) are the ceiling; each is lowered to 3 x the format's own cost measured on the CPU
# over this grid (tests/test_t5_attn_ref_host.py::test_cost_of_the_number_formats_over_the_grid holds them to it and says what fp32's cost is).
ISSUE_BAR_REL = {"f32": 3e-5, "bf16": 1.5e-2}
ISSUE_BAR_ABS = {"f32": 3e-5, "bf16": 1e-2}
BAR_REL = {"f32": 3.7e-6, "bf16": 1.35e-2}
BAR_ABS = {"f32": 6.8e-6, "bf16": 9.3e-3}


def rel_buckets(L, num_buckets, max_distance):
    """[L, L] long: the bucket of rel = j - i at [i, j]."""
    tab = torch.from_numpy(bucket_table(num_buckets, max_distance)).long()
    rel = torch.arange(L)[None, :] - torch.arange(L)[:, None]
    return tab[rel + REL_SPAN]


def bucket_of(rel, num_buckets, max_distance):
    return int(bucket_table(num_buckets, max_distance)[max(-REL_SPAN, min(REL_SPAN, rel)) + REL_SPAN])


def last_bucket_from(num_buckets, max_distance):
    """The smallest distance whose bucket is the saturated last one."""
    tab = bucket_table(num_buckets, max_distance)
    return min(d for d in range(REL_SPAN + 1) if tab[REL_SPAN - d] == tab[0])


def _scores(q, k, rel_bias, buckets, mask):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) + rel_bias.double()[buckets].permute(2, 0, 1)[None]
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    return s, torch.where(torch.isinf(m), torch.zeros_like(m), m)


def reference(q, k, v, rel_bias, buckets, mask):
    """q, k, v [B, L, H, 64] (fp32 or bf16), rel_bias [num_buckets, H] fp32, buckets [L, L] long (rel_buckets), mask [B, L] bool (True = attend)
    or None -> [B, L, H, 64] float64."""
    s, m = _scores(q, k, rel_bias, buckets, mask)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    p = torch.where(l > 0, p / l, torch.zeros_like(p))
    return torch.einsum("bhqk,bkhd->bqhd", p, v.double())


def reference_rounded_p(q, k, v, rel_bias, buckets, mask):
    """`reference` with exp(s - rowmax) rounded to the dtype of q before P V, the row sum from the unrounded values, the output rounded once."""
    dt = q.dtype
    s, m = _scores(q, k, rel_bias, buckets, mask)
    p = torch.exp(s - m)
    l = p.sum(-1).permute(0, 2, 1)[..., None]
    o = torch.einsum("bhqk,bkhd->bqhd", p.to(dt).double(), v.double())
    o = torch.where(l > 0, o / l, torch.zeros_like(o))
    return o.to(dt).double()


def reference_f32_arithmetic(q, k, v, rel_bias, buckets, mask):
    """The same expression with every product, sum and exp in torch float32 on the CPU (P rounded to the dtype of q) -> float64."""
    dt = q.dtype
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) + rel_bias.float()[buckets].permute(2, 0, 1)[None]
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = p.sum(-1).permute(0, 2, 1)[..., None]
    o = torch.einsum("bhqk,bkhd->bqhd", p.to(dt).float(), v.float())
    o = torch.where(l > 0, o / l, torch.zeros_like(o))
    return o.to(dt).double()


def needle_rels(L, num_buckets, max_distance):
    """The relative positions a needle head can put its bucket on."""
    return (0, 1, -1, num_buckets // 2 // 2, -max_distance, L - 1)


def needle_bucket_of_head(H, L, num_buckets, max_distance, seed):
    """[H] -> the bucket that carries +12 in head h."""
    rels = needle_rels(L, num_buckets, max_distance)
    return [bucket_of(rels[(h + seed) % len(rels)], num_buckets, max_distance) for h in range(H)]


def make_inputs(dname, B, H, L, regime, num_buckets, max_distance, seed):
    """-> q, k, v [B, L, H, 64] in the dtype `dname`, rel_bias [num_buckets, H] fp32."""
    g = torch.Generator().manual_seed(seed)
    key = torch.arange(L)
    v = torch.randn(B, L, H, HD, generator=g)
    v[..., C_ONE] = 1.0
    v[..., C_TILE:C_TILE + 4] = (key[:, None] // KT % 4 == torch.arange(4)).float()[None, :, None, :]
    v[..., C_FIRST] = (key == 0).float()[None, :, None]
    v[..., C_LAST] = (key == L - 1).float()[None, :, None]
    v[..., C_HOT:C_HOT + 8] = (key[:, None] % 8 == torch.arange(8)).float()[None, :, None, :]
    v[..., C_RAMP] = (key.float() / L)[None, :, None]
    k = torch.zeros(B, L, H, HD)
    q = torch.zeros(B, L, H, HD)
    if regime in ("ascending", "descending"):            # attn_ref's construction at scale 1: background on channels < 56, the ramp on channel 60
        k[..., :56] = torch.randn(B, L, H, 56, generator=g)
        q[..., :56] = torch.randn(B, L, H, 56, generator=g) * 0.05
        ramp = -1.0 + 2.0 * (key // KT + 0.5 * (key % KT) / (KT - 1)) / ((L + KT - 1) // KT - 0.5)
        k[..., 60] = (ramp if regime == "ascending" else -ramp)[None, :, None]
        q[..., 60] = RAMP
    else:
        k[:] = torch.randn(B, L, H, HD, generator=g)
        q[:] = torch.randn(B, L, H, HD, generator=g) * 0.05
    if regime == "bias_random":
        rel_bias = torch.randn(num_buckets, H, generator=g)
    elif regime == "bias_needle":
        rel_bias = torch.zeros(num_buckets, H)
        for h, bk in enumerate(needle_bucket_of_head(H, L, num_buckets, max_distance, seed)):
            rel_bias[bk, h] = NEEDLE
    else:
        rel_bias = torch.randn(num_buckets, H, generator=g) * 0.1
    dt = DT[dname]
    return q.to(dt), k.to(dt), v.to(dt), rel_bias


def mask_ok(kind, B, L):
    if kind == "per_sample":
        return B >= 3 and L > 1
    return A.mask_ok(kind, B, L)


def make_mask(kind, B, L):
    """[B, L] bool (True = attend) or None; attn_ref's kinds that leave a key in every sample, and `per_sample`: valid lengths L, 1 and L // 2."""
    if kind == "per_sample":
        assert mask_ok(kind, B, L)
        lens = [(L, 1, max(1, L // 2))[b % 3] for b in range(B)]
        return torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    assert kind != "sample"
    return A.make_mask(kind, B, L)


# ---- the grid of tests/test_gpu_t5_kernels.py
# B, H, L.  L -> blocks of 64 query rows and key tiles: 1, 15, 16, 17: one block, partly filled waves; 63, 64, 65: the tile seam; 128, 129, 200: two and
# three blocks (and key tiles).  L = 1024 (B = 1, H = 2) fills relb's span completely.
SHAPES = [(3, 1, 1), (1, 3, 15), (3, 6, 16), (1, 1, 17), (3, 3, 63), (1, 6, 64), (3, 3, 65), (1, 1, 128), (3, 6, 129), (1, 3, 200), (3, 1, 200)]
LONG = (1, 2, 1024)
# where each bucket configuration meets both bias regimes: at lengths that reach its saturated last bucket (from distance 91, 6 and 898: last_bucket_from)
BUCKET_SHAPES = {(32, 128): ((3, 6, 129), (1, 3, 200)), (8, 16): ((1, 1, 17), (3, 3, 65)), (126, 1000): (LONG,)}


def gpu_grid():
    """List of dict(dname, B, H, L, mask, regime, num_buckets, max_distance, seed).  Per dtype: every shape once unmasked, regimes and bucket
    configurations dealt round-robin; every (mask, regime) pair once on a shape that admits the mask, found from a strided start; every bucket
    configuration under both bias regimes at lengths that reach its last bucket (L = 1024 is these two cases of (126, 1000))."""
    out = []

    def add(dname, shape, mask, regime, cfg):
        B, H, L = shape
        out.append(dict(dname=dname, B=B, H=H, L=L, mask=mask, regime=regime, num_buckets=cfg[0], max_distance=cfg[1], seed=len(out)))

    for di, dname in enumerate(DT):
        for si, shape in enumerate(SHAPES):
            add(dname, shape, "none", REGIMES[(si + di) % len(REGIMES)], BUCKETS[si % 3])
        pairs = [(m, r) for m in MASKS[1:] for r in REGIMES]
        for pi, (mask, regime) in enumerate(pairs):
            si = (pi * 5 + di * 3) % len(SHAPES)
            while not mask_ok(mask, SHAPES[si][0], SHAPES[si][2]):
                si = (si + 1) % len(SHAPES)
            add(dname, SHAPES[si], mask, regime, BUCKETS[(pi + di) % 3])
        for cfg, shapes in BUCKET_SHAPES.items():
            for shape in shapes:
                for regime in BIAS_REGIMES:
                    add(dname, shape, "none", regime, cfg)
    return out


def case_tensors(c):
    """-> q, k, v, rel_bias, buckets, keep of a grid case."""
    q, k, v, rel_bias = make_inputs(c["dname"], c["B"], c["H"], c["L"], c["regime"], c["num_buckets"], c["max_distance"], c["seed"])
    return q, k, v, rel_bias, rel_buckets(c["L"], c["num_buckets"], c["max_distance"]), make_mask(c["mask"], c["B"], c["L"])


def slice_errors(out, ref):
    """-> (worst over the (batch, head) slices of max|out - ref| / max|ref| on the random columns, worst absolute error of the structured ones)."""
    d = (out.double() - ref).abs()
    e_rel = d[..., C_RAND:].amax((1, 3)) / ref[..., C_RAND:].abs().amax((1, 3))
    e_abs = d[..., :C_RAND].amax((1, 3))
    return float(e_rel.max()), float(e_abs.max())
