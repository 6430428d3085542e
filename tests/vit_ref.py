"""The ViT driver vt_dino_forward (csrc/vt_models.hip) stated in float64 on the CPU, numpy and torch-double only, and the cases its tests walk.

`prepare` is the per-camera decision of the reference's DINOv2Encoder.forward (visual_encoder.py:65-106): numpy input is divided by 255, a batch
whose maximum exceeds 1 is divided by 255 (again), a batch whose mean is below 0.5 is left unnormalised.  `tokens` is the patch embedding (flatten
c*196 + i*14 + j, remainder res % 14 dropped, projection, bias, position rows, CLS row), `blocks` the HF DINOv2 block (GELU-erf or SwiGLU FFN,
LayerScale) or the SigLIP block (tanh-GELU, no LayerScale) and the final LayerNorm.  Position-embedding interpolation is not restated: the tests
pass the engine's own `pos_patch(grid)` rows to both sides.

Every function takes `acc` (the arithmetic type: float64 = the reference, float32 = what fp32 arithmetic of the same statement costs) and the
optional rounding points of the driver's 16-bit modes: `adt` rounds what the driver stores in its activation type (patches, normalised
activations, q|k|v, the attention probabilities the 16-bit attention kernels pack before P V (tests/attn_ref.py), attention output, FFN hidden),
`cdt` rounds the GEMM weights.  The residual stream, biases, norm gains and LayerScale stay unrounded, as in the driver.  The distance between
the float64 statement and one with rounding points and fp32 arithmetic is what the format alone costs: the only thing a bar is derived from.

`mut` names one deliberate error (MUTATIONS); the host test proves that each leaves the bars in at least one case of the grids.  Nothing here
imports the product's code; the synthetic weights come from vlatouch.synth's deterministic rule, as tests/cases.py takes them."""
import math

import numpy as np
import torch

AUTO, ON, OFF, RAW = 0, 1, 2, 3                    # norm_mode of vt_dino_forward (include/vlatouch.h)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PATCH = 14
DT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
PRECS = ("fp32", "bf16", "fp16")
MUTATIONS = ("swap_ij", "reverse_channels", "keep_remainder", "mean_le", "max_ge", "shift_pos", "cls_other_image", "layerscale_after_add")


def rnd(x: torch.Tensor, dt) -> torch.Tensor:
    """Round to the storage type `dt` through fp32 (the driver's kernels hold fp32 values when they store), keep the arithmetic type."""
    return x if dt is None else x.float().to(dt).to(x.dtype)


# ------------------------------------------------------------------------------------------------ statistics and the two decisions
def prepare(frames: np.ndarray, layout: str, pre_scale: float, norm_mode: int, mut: str = ""):
    """frames: one camera batch, uint8 or fp32, "nchw" [B,3,H,W] or "nhwc" [B,H,W,3]; pre_scale 1/255 where the caller passed numpy, else 1.
    -> (planar float64 pixels [B,3,H,W] as the patch embedding takes them, scale, norm flag, max, mean): the last four are the driver's flags."""
    x = np.asarray(frames).astype(np.float64)
    if layout == "nhwc":
        x = x.transpose(0, 3, 1, 2)
    inv = 1.0 / pre_scale
    div = float(round(inv)) if abs(inv - round(inv)) < 1e-4 * inv else inv          # 1/255 is a division by 255 in the reference
    mx = float(x.max()) / div
    big = mx >= 1.0 if mut == "max_ge" else mx > 1.0
    if norm_mode != RAW and big:
        div *= 255.0
    x = x / div
    mean = float(x.mean())
    if norm_mode == AUTO:
        norm = not (mean <= 0.5 if mut == "mean_le" else mean < 0.5)
    else:
        norm = norm_mode == ON
    if norm:
        x = (x - np.array(IMAGENET_MEAN).reshape(1, 3, 1, 1)) / np.array(IMAGENET_STD).reshape(1, 3, 1, 1)
    return np.ascontiguousarray(x), 1.0 / div, float(norm), mx, mean


# ------------------------------------------------------------------------------------------------ patch embedding
def _sd(sd, key, acc):
    return sd[key].detach().to(acc)


def is_siglip(sd) -> bool:
    return "embeddings.patch_embedding.weight" in sd


def tokens(sd, pixels, grid: int, pos, *, adt=None, cdt=None, acc=torch.float64, mut: str = "") -> torch.Tensor:
    """pixels [Bt,3,res,res] (prepare's), pos [grid*grid, D] position rows of the patch tokens -> the residual stream [Bt, N, D] the first block
    receives: CLS row (cls_token + position_embeddings[0, 0]; DINOv2 only) then the projected patches in row-major patch order."""
    x = torch.as_tensor(pixels).to(acc)
    Bt, _, res, _ = x.shape
    g = grid
    if mut == "keep_remainder" and res % PATCH:                     # the patch grid slid to the far edge: the remainder columns kept, the first dropped
        x = x[:, :, res - g * PATCH:, res - g * PATCH:]
    else:
        x = x[:, :, : g * PATCH, : g * PATCH]
    if mut == "reverse_channels":
        x = x.flip(1)
    p = x.reshape(Bt, 3, g, PATCH, g, PATCH)                        # b c py i px j
    p = p.permute(0, 2, 4, 1, 5, 3) if mut == "swap_ij" else p.permute(0, 2, 4, 1, 3, 5)
    p = rnd(p.reshape(Bt, g * g, 3 * PATCH * PATCH), adt)
    sig = is_siglip(sd)
    wk = "embeddings.patch_embedding" if sig else "embeddings.patch_embeddings.projection"
    w = rnd(_sd(sd, wk + ".weight", acc).reshape(-1, 3 * PATCH * PATCH), cdt)
    pos = torch.as_tensor(pos).detach().cpu().to(acc)
    if mut == "shift_pos":
        pos = pos.roll(1, 0)
    t = p @ w.T + _sd(sd, wk + ".bias", acc) + pos[None]
    if sig:
        return t
    cls = _sd(sd, "embeddings.cls_token", acc)[0, 0] + _sd(sd, "embeddings.position_embeddings", acc)[0, 0]
    return torch.cat((cls.expand(Bt, 1, -1), t), dim=1)


# ------------------------------------------------------------------------------------------------ transformer blocks
def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _attend(q, k, v, hd, adt):
    """softmax(q k^T hd^-0.5) v per [image, head]; the 16-bit kernels pack exp(s - max) before P V and sum the unrounded values (tests/attn_ref.py)."""
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return (rnd(p, adt) @ v) / p.sum(-1, keepdim=True)


def blocks(sd, tok, heads: int, *, pooled: bool = False, adt=None, cdt=None, acc=torch.float64, eps: float = 1e-6, mut: str = "") -> torch.Tensor:
    """tok [Bt, N, D] -> every token of the final LayerNorm [Bt, N, D], or (pooled, DINOv2) its CLS rows [Bt, D].  The pruned last block of the
    driver computes the same CLS rows: only a query, a projection and an FFN are left out for the rows nobody reads."""
    sig = is_siglip(sd)
    t = tok.to(acc)
    Bt, N, D = t.shape
    hd = D // heads
    lay = "encoder.layers" if sig else "encoder.layer"
    names = (dict(n1="layer_norm1", n2="layer_norm2", q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.out_proj") if sig else
             dict(n1="norm1", n2="norm2", q="attention.attention.query", k="attention.attention.key", v="attention.attention.value", o="attention.output.dense"))
    L = 0
    while f"{lay}.{L}.{names['n1']}.weight" in sd:
        L += 1
    for l in range(L):
        G = lambda k: _sd(sd, f"{lay}.{l}.{k}", acc)
        lin = lambda x, k: x @ rnd(G(k + ".weight"), cdt).T + G(k + ".bias")
        h = rnd(_ln(t, G(names["n1"] + ".weight"), G(names["n1"] + ".bias"), eps), adt)
        q, k, v = (rnd(lin(h, names[n]), adt).reshape(Bt, N, heads, hd).transpose(1, 2) for n in ("q", "k", "v"))      # [Bt, H, N, hd]
        a = _attend(q, k, v, hd, adt)
        if mut == "cls_other_image" and l == L - 1 and Bt > 1:      # the CLS query of image b reads image b + 1's keys and values
            a = torch.cat((_attend(q[:, :, :1], k.roll(-1, 0), v.roll(-1, 0), hd, adt), a[:, :, 1:]), dim=2)
        a = rnd(a.transpose(1, 2).reshape(Bt, N, D), adt)
        o = lin(a, names["o"])
        if sig:
            t = t + o
        elif mut == "layerscale_after_add":
            t = (o + t) * G("layer_scale1.lambda1")
        else:
            t = o * G("layer_scale1.lambda1") + t
        h = rnd(_ln(t, G(names["n2"] + ".weight"), G(names["n2"] + ".bias"), eps), adt)
        if f"{lay}.{l}.mlp.weights_in.weight" in sd:                # HF Dinov2SwiGLUFFN: x1, x2 = weights_in(h).chunk(2); weights_out(silu(x1) * x2)
            x1, x2 = rnd(lin(h, "mlp.weights_in"), adt).chunk(2, dim=-1)
            o = lin(rnd(x1 * torch.sigmoid(x1) * x2, adt), "mlp.weights_out")
        else:
            o = lin(rnd((_gelu_tanh if sig else _gelu_erf)(lin(h, "mlp.fc1")), adt), "mlp.fc2")
        if sig:
            t = t + o
        elif mut == "layerscale_after_add":
            t = (o + t) * G("layer_scale2.lambda1")
        else:
            t = o * G("layer_scale2.lambda1") + t
    fin = "post_layernorm" if sig else "layernorm"
    t = _ln(t, _sd(sd, fin + ".weight", acc), _sd(sd, fin + ".bias", acc), eps)
    return t[:, 0] if pooled else t


def row_err(out, ref) -> float:
    """The measure of every bar: per output row max|out - ref| / max|ref row|, the largest over the rows."""
    out = torch.as_tensor(out).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    out, ref = out.reshape(-1, out.shape[-1]), ref.reshape(-1, ref.shape[-1])
    if not bool(torch.isfinite(out).all()):
        return float("inf")
    return float(((out - ref).abs().amax(-1) / ref.abs().amax(-1)).max())


# ------------------------------------------------------------------------------------------------ frames
def frame(kind: str, shape, dtype, seed: int) -> np.ndarray:
    """A camera batch whose decisions are far from both thresholds (mean at least 0.05 from 0.5, maximum not within 0.05 of 1):
    bright / dark: mean 0.6 / 0.3 of full scale; fp32 "unit" kinds lie in [0, 0.9], fp32 "byte" kinds in [0, 255] (the /255 rule fires)."""
    g = np.random.Generator(np.random.PCG64(seed))
    lo, hi = (0.3, 0.9) if kind.startswith("bright") else (0.0, 0.6)
    u = lo + (hi - lo) * g.random(shape)
    if dtype == np.uint8:
        return np.clip(np.rint(u * 255.0), 0, 255).astype(np.uint8)
    return (u * (255.0 if kind.endswith("byte") else 1.0)).astype(np.float32)


def shape_of(layout: str, B: int, res: int):
    return (B, res, res, 3) if layout == "nhwc" else (B, 3, res, res)


# ------------------------------------------------------------------------------------------------ the grids
FRONT_MODELS = ((64, 1), (128, 2))                                   # (hidden, heads), one layer
FRONT_RES = (14, 28, 29, 42, 45)
FRONT_LAYOUTS = (("nchw", "f32"), ("nhwc", "f32"), ("nchw", "u8"), ("nhwc", "u8"))


def front_cases():
    """Every front-end case: resolution x layout x element type x B x (one camera | two cameras that decide differently).  Each runs once from
    an allocation's base and once from a base offset by one element (4 bytes fp32, 1 byte uint8) into a larger buffer."""
    out = []
    for res in FRONT_RES:
        for layout, et in FRONT_LAYOUTS:
            for B in (1, 3):
                for ncams in (1, 2):
                    i = len(out)
                    byte = et == "f32" and (i // 2) % 2 == 1           # fp32 frames alternate between [0, 0.9] and [0, 255] values
                    first = ("bright", "dark")[i % 2] + ("_byte" if byte else "")
                    second = ("dark", "bright")[i % 2] + ("_byte" if et == "f32" and not byte else "")
                    out.append(dict(res=res, layout=layout, et=et, B=B, kinds=(first, second)[:ncams], seed=100 + i))
    return out


def front_frames(c):
    dt = np.uint8 if c["et"] == "u8" else np.float32
    return [frame(k, shape_of(c["layout"], c["B"], c["res"]), dt, c["seed"] * 10 + n) for n, k in enumerate(c["kinds"])]


def dino_shapes_sd(hidden: int, layers: int, swiglu: bool = False, image_size: int = 56):
    """Synthetic HF Dinov2Model weights (vlatouch.synth's deterministic rule, imported lazily: data, not the code under test)."""
    from tests import cases
    from vlatouch import synth
    return cases.sd_torch(synth.dinov2_shapes(hidden, layers, image_size=image_size, swiglu=swiglu), prefix=f"vit-test-{hidden}-{layers}-{int(swiglu)}.")


def siglip_shapes_sd(image_size: int, hidden: int = 576, layers: int = 2, inter: int = 1072):
    from tests import cases
    from vlatouch import synth
    return cases.sd_torch(synth.siglip_shapes(hidden, layers, inter, image_size=image_size), prefix=f"vit-test-siglip-{image_size}.")


# DINOv2 block configs: name -> hidden, heads, layers, swiglu, precisions, [(res, ncams, B)]
BLOCK_CONFIGS = {
    "d128_l1": dict(hidden=128, heads=2, layers=1, swiglu=False, precs=PRECS, runs=[(28, 1, 1), (28, 1, 3), (28, 2, 3), (42, 1, 1), (42, 1, 3), (42, 2, 3)]),
    "d128_l2": dict(hidden=128, heads=2, layers=2, swiglu=False, precs=PRECS, runs=[(28, 1, 1), (28, 1, 3), (28, 2, 3), (42, 1, 1), (42, 1, 3), (42, 2, 3)]),
    "d256_packed": dict(hidden=256, heads=4, layers=2, swiglu=False, precs=("bf16", "fp16"), runs=[(28, 1, 13)]),        # Bt N = 13 x 5 = 65 rows
    "d512_splitk": dict(hidden=512, heads=8, layers=2, swiglu=False, precs=PRECS, runs=[(42, 1, 13)]),                    # 13 x 10 = 130 rows
    "d128_swiglu": dict(hidden=128, heads=2, layers=2, swiglu=True, precs=PRECS, runs=[(28, 1, 3)]),
}
SIGLIP_HEADS = 8
SIGLIP_RUNS = [(28, 1), (28, 3), (42, 1), (42, 3)]                   # (image size, B)


def block_frames(res: int, ncams: int, B: int, seed: int):
    """fp32 planar frames; with two cameras the first normalises and the second does not."""
    return [frame(("bright", "dark")[n % 2], (B, 3, res, res), np.float32, seed * 10 + n) for n in range(ncams)]


def siglip_pixels(B: int, res: int, seed: int, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> np.ndarray:
    """What SiglipImageProcessor hands the tower: (u8 / 255 - mean) / std, fp32.  ImageNet statistics reach (1 - 0.406) / 0.225 = 2.64."""
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.integers(0, 256, (B, 3, res, res)).astype(np.float64)
    u[0, :, 0, 0] = 255.0                                            # the largest value is present whatever the draw
    return ((u / 255.0 - np.array(mean).reshape(1, 3, 1, 1)) / np.array(std).reshape(1, 3, 1, 1)).astype(np.float32)


def pos_rows(sd, grid: int) -> torch.Tensor:
    """Position rows of the patch tokens for the CPU-side cost measurements, where no engine exists to ask (the GPU tests pass the engine's own
    `pos_patch(grid)`): the table's rows, resized as HF `interpolate_pos_encoding` does when the grid differs.  An input, not part of the statement."""
    if is_siglip(sd):
        return sd["embeddings.position_embedding.weight"].float()
    pp = sd["embeddings.position_embeddings"].float()[:, 1:]
    s = int(round(math.sqrt(pp.shape[1])))
    if grid != s:
        pp = torch.nn.functional.interpolate(pp.reshape(1, s, s, -1).permute(0, 3, 1, 2), size=(grid, grid), mode="bicubic", align_corners=False)
        pp = pp.permute(0, 2, 3, 1).reshape(1, grid * grid, -1)
    return pp[0].contiguous()


def dino_reference(sd, heads, frames_list, pos, norm_mode=AUTO, pre_scale=1.0, layout="nchw", **kw):
    """Frames of every camera -> (tokens after the front end [ncams*B, N, D], every token of the final LayerNorm) in the arithmetic of `kw`."""
    px = np.concatenate([prepare(f, layout, pre_scale, norm_mode)[0] for f in frames_list])
    res = px.shape[-1]
    t = tokens(sd, px, res // PATCH, pos, **kw)
    return t, blocks(sd, t, heads, **kw)


# ------------------------------------------------------------------------------------------------ decisions
def decision_cases():
    """name -> dict(frames, layout, pre_scale, mode, offset): one camera batch each; flags[0..2] must equal `prepare`'s.  `offset`: the frames
    start one element past an allocation's base.  Outside the named threshold cases the mean is at least 0.05 from 0.5 and the maximum 0.05 from 1."""
    f32, u8 = np.float32, np.uint8
    c = {}
    const = lambda v, dt, shape=(1, 3, 28, 28): np.full(shape, v, dtype=dt)
    case = lambda frames, layout="nchw", pre_scale=1.0, mode=AUTO, offset=False: dict(frames=frames, layout=layout, pre_scale=pre_scale, mode=mode, offset=offset)
    c["u8_127"] = case(const(127, u8))                                # 127 / 255 = 0.498: divided, not normalised
    c["u8_128"] = case(const(128, u8))                                # 128 / 255 = 0.502: divided, normalised
    c["f32_mean_half"] = case(const(0.5, f32))                        # every partial sum is exact: the mean is exactly 0.5 and `<` normalises
    x = frame("dark", (1, 3, 28, 28), f32, 1)
    x[0, 1, 13, 5] = 1.0
    c["f32_max_one"] = case(x)                                        # a maximum of exactly 1 is not `> 1`
    x = x.copy()
    x[0, 1, 13, 5] = np.nextafter(f32(1), f32(2))
    c["f32_max_next"] = case(x)                                       # one ulp above: divided
    g = np.random.Generator(np.random.PCG64(2))
    c["u8_zero_one"] = case((g.random((2, 28, 28, 3)) < 0.8).astype(u8), layout="nhwc")       # the reference does not divide a 0/1 frame; mean 0.8
    x = frame("bright", (1, 28, 28, 3), u8, 3)
    x[0, 27, 27, 2] = 255
    c["numpy_u8_255"] = case(x, layout="nhwc", pre_scale=1.0 / 255.0)  # 255 * fl(1/255) must round to 1.0: the scale stays 1/255
    for name, kind, mode in (("on_bright_byte", "bright_byte", ON), ("off_bright_byte", "bright_byte", OFF), ("raw_bright_byte", "bright_byte", RAW),
                             ("on_dark", "dark", ON), ("off_bright", "bright", OFF), ("raw_bright", "bright", RAW)):
        c[name] = case(frame(kind, (2, 3, 28, 28), f32, 4), mode=mode)
    x = frame("dark", (1, 3, 29, 29), f32, 5)                         # 2523 elements: 630 vectors and a tail of 3
    x.reshape(-1)[-1] = 200.0
    c["f32_tail_max"] = case(x)                                       # the only value above 1 lies in the tail
    x = frame("dark", (1, 29, 29, 3), u8, 6) // 153                   # 0 / 1 valued; 2523 bytes: 157 vectors and a tail of 11
    x.reshape(-1)[-1] = 2
    c["u8_tail_max"] = case(x, layout="nhwc")
    x = frame("dark", (1, 3, 28, 28), f32, 7)
    x.reshape(-1)[0] = 200.0
    c["f32_unaligned_max"] = case(x, offset=True)                     # unaligned base: the scalar walk alone
    x = frame("bright", (1, 28, 28, 3), u8, 8)
    c["u8_unaligned"] = case(x, layout="nhwc", offset=True)
    return c


LARGE = {"f32": (1, 3, 518, 518), "u8": (4, 518, 518, 3)}             # 804 972 floats and 3 219 888 bytes: 201 243 vectors of 16 bytes each


def large_case(et: str, where: str) -> np.ndarray:
    """A 0 / 1-valued frame (mean 0.25) whose only value above 1 is its first (`first`: the first vector) or last (`last`) element."""
    g = np.random.Generator(np.random.PCG64(9))
    x = (g.random(LARGE[et]) < 0.25).astype(np.uint8 if et == "u8" else np.float32)
    x.reshape(-1)[0 if where == "first" else -1] = 2
    return x


STAT_BLOCKS, STAT_THREADS = 256, 256                                  # vt_k_imgstats' launch: 256 blocks of 256 lanes, 16-byte vectors


def stat_walks(n: int, elem_bytes: int, aligned: bool):
    """Which of imgstat_partial_kernel's three walks a batch of n elements enters, and the longest per-lane chain of additions into `sm`."""
    V = 16 // elem_bytes
    stride = STAT_BLOCKS * STAT_THREADS
    nvec = n // V if aligned else 0
    walks = set()
    if nvec > 3 * stride:
        walks.add("unrolled")
    if nvec and (nvec <= 3 * stride or nvec % (4 * stride)):          # lanes left over after the unrolled rounds, or never unrolled
        walks.add("vector")
    if n - nvec * V:
        walks.add("scalar")
    chain = -(-nvec // stride) + -(-(n - nvec * V) // stride)
    return walks, chain


def mean_bound(n: int, elem_bytes: int, aligned: bool) -> float:
    """Bound on |flags[3] - mean| / mean|x| from the launch geometry alone: the additions an element can pass through are the in-vector sum (a
    tree of 2 levels for four floats, a run of 16 for sixteen bytes), the longest per-lane chain (one rounding per `sm +=`), 6 levels of the
    wave reduction and 2 of the four-wave fold; the fold of the 256 partials is in fp64; then the conversion to fp32, the product with the
    scale (2 roundings) and the scale's own two (fl(1/255), / 255).  Each rounding is at most 2^-24 of the running sum of |x|."""
    _, chain = stat_walks(n, elem_bytes, aligned)
    return ((2 if elem_bytes == 4 else 16) + chain + 6 + 2 + 2 + 2) * 2.0 ** -24


def patchify_path(layout: str, et: str, prec: str, res: int, aligned8: bool) -> str:
    """patchify_kernel's choice: two pixels per lane for planar fp32 -> 16-bit, even res, 8-byte-aligned base; one pixel otherwise."""
    return "two" if layout == "nchw" and et == "f32" and prec != "fp32" and res % 2 == 0 and aligned8 else "one"


def kpad(prec: str) -> int:
    """DinoEngine's K padding of the 588 patch columns: to 16 in fp32, to 64 in the 16-bit modes."""
    m = 16 if prec == "fp32" else 64
    return (588 + m - 1) // m * m


# The bars: 3 x the largest cost of a group (tests/test_vit_ref_host.py measures the costs on the CPU and holds these literals to them; the 3
# covers an accumulation order that differs from the CPU's).  A cost is the distance, in the measure of `row_err`, between the float64 statement
# and the same statement in fp32 arithmetic (fp32 mode) or with the 16-bit rounding points and fp32 arithmetic (bf16, fp16), the largest over the
# group's cases: front = front_cases() x FRONT_MODELS, dino = BLOCK_CONFIGS (every token), siglip = SIGLIP_RUNS with both pixel statistics.
COSTS = {
    ("front", "fp32"): 1.1e-6, ("front", "bf16"): 4.5e-3, ("front", "fp16"): 5.9e-4,
    ("dino", "fp32"): 8.5e-7, ("dino", "bf16"): 9.8e-3, ("dino", "fp16"): 1.5e-3,
    ("siglip", "fp32"): 8.6e-7, ("siglip", "bf16"): 6.8e-3, ("siglip", "fp16"): 8.7e-4,
}
BARS = {k: 3.0 * v for k, v in COSTS.items()}
