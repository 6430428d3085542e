"""CLIP vision tower with deep visual prompts (Octopi's tactile encoder, octopi_s/utils/encoder.py) and the heads around it.

`ClipEngine` packs an HF CLIPVisionModel state dict (plus the prompt-learning parameters VPT / VPT_shallow / VPT_gamma) for the ViT driver
(vt_dino_*, csrc/vt_models.hip) as its third variant: CLS token, no patch bias, pre_layrnorm, quick-GELU, no LayerScale, LayerNorm eps 1e-5,
pooler_output = post_layernorm(CLS row).  `TactileHeads` runs the video feature and the retrieval (csrc/vt_tactile_head.hip); `LinearHead`
the Adapter / PropertyClassifier / project Linears on vt_gemm / vt_mlp.  Weight packing (`clip_vision_sd`, `clip_pack`) is plain CPU code,
so its order can be checked without a GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import ops
from .engine import MlpEngine, RangeGuard, _Engine, _pad_to, _Workspace, precision_dtypes

SD = Mapping[str, torch.Tensor]
TOPK_MAX = 16                      # vt_tactile_head's output buffers (include/vlatouch.h)


def clip_vision_sd(sd: SD) -> Dict[str, torch.Tensor]:
    """The vision tower's keys of a checkpoint, relative to `vision_model.`: a `module.` prefix (DataParallel) is stripped, then
    `clip_model.vision_model.` (a ViFiCLIP file), `model.vision_model.` (a CLIPVisionEncoder file) or `vision_model.`; a dict that already
    is relative is returned as it is."""
    out = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    for pre in ("clip_model.vision_model.", "model.vision_model.", "vision_model."):
        if any(k.startswith(pre) for k in out):
            return {k[len(pre):]: v for k, v in out.items() if k.startswith(pre)}
    return out


def clip_depth(sd: SD, layers: int) -> int:
    """The prompt depth a relative state dict carries: 0 without `VPT`, else one past the last layer that owns a `VPT_shallow`."""
    if "VPT" not in sd:
        return 0
    return 1 + max([i for i in range(layers) if f"encoder.layers.{i}.VPT_shallow" in sd], default=0)


def clip_pack(sd: SD, *, heads: int, cdt: int, patch: int = 14, prompt_depth: Optional[int] = None) -> Tuple[List[str], List[torch.Tensor], dict]:
    """-> (names, CPU tensors in the driver's weight order, descriptor fields).  The order is vt_dino_create's: patch_w (K padded), patch bias
    (zeros: CLIP's conv has none), cls_pos0 = class_embedding + position_embedding[0]; per layer ln1, fused q|k|v, out_proj, ones (LayerScale
    slot), ln2, fc1, fc2, ones; post_layernorm; then pre_layrnorm and, with prompts, VPT, VPT_shallow_1 .. VPT_shallow_{P-1} and the gates
    sigmoid(VPT_gamma_i) as ONE fp32 array [layers] (0.5 where a layer has no gamma; never read there)."""
    sd = clip_vision_sd(sd)
    g = lambda k: sd[k].detach().float().cpu()
    wdt = L.torch_dtype(cdt)
    pw = g("embeddings.patch_embedding.weight")
    D = pw.shape[0]
    if D % heads or D // heads != 64:
        raise L.VtError(f"ClipEngine: hidden {D} / heads {heads}: the tower runs 64-wide heads only")
    kpad = _pad_to(3 * patch * patch, 16 if cdt == L.F32 else 64)
    layers = 0
    while f"encoder.layers.{layers}.layer_norm1.weight" in sd:
        layers += 1
    inter = g("encoder.layers.0.mlp.fc1.weight").shape[0]
    if inter % 64:
        raise L.VtError(f"ClipEngine: FFN width {inter} is not a multiple of 64")
    pos = g("embeddings.position_embedding.weight")
    grid = int(round(math.sqrt(pos.shape[0] - 1)))
    if grid * grid + 1 != pos.shape[0]:
        raise L.VtError(f"ClipEngine: position table of {pos.shape[0]} rows is not 1 + a square")
    P = clip_depth(sd, layers) if prompt_depth is None else (layers if prompt_depth == -1 else prompt_depth)
    if P < 0 or P > layers:
        raise L.VtError(f"ClipEngine: prompt_depth {prompt_depth} outside -1 .. {layers}")
    n_ctx = sd["VPT"].shape[0] if P else 0
    pwp = torch.zeros(D, kpad)
    pwp[:, : 3 * patch * patch] = pw.reshape(D, -1)
    ones = torch.ones(D)
    names = ["patch_w", "patch_b", "cls_pos0"]
    W: List[torch.Tensor] = [pwp.to(wdt), torch.zeros(D), g("embeddings.class_embedding") + pos[0]]
    for i in range(layers):
        p = f"encoder.layers.{i}"
        a = f"{p}.self_attn"
        qkv_w = torch.cat([g(f"{a}.q_proj.weight"), g(f"{a}.k_proj.weight"), g(f"{a}.v_proj.weight")], dim=0)
        qkv_b = torch.cat([g(f"{a}.q_proj.bias"), g(f"{a}.k_proj.bias"), g(f"{a}.v_proj.bias")], dim=0)
        names += [f"{i}.{n}" for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2")]
        W += [g(f"{p}.layer_norm1.weight"), g(f"{p}.layer_norm1.bias"), qkv_w.to(wdt), qkv_b, g(f"{a}.out_proj.weight").to(wdt), g(f"{a}.out_proj.bias"), ones,
              g(f"{p}.layer_norm2.weight"), g(f"{p}.layer_norm2.bias"), g(f"{p}.mlp.fc1.weight").to(wdt), g(f"{p}.mlp.fc1.bias"),
              g(f"{p}.mlp.fc2.weight").to(wdt), g(f"{p}.mlp.fc2.bias"), ones]
    names += ["lnf_w", "lnf_b", "pre_w", "pre_b"]
    W += [g("post_layernorm.weight"), g("post_layernorm.bias"), g("pre_layrnorm.weight"), g("pre_layrnorm.bias")]
    if P and n_ctx:
        names += ["VPT"] + [f"{i}.VPT_shallow" for i in range(1, P)] + ["gates"]
        gates = torch.full((layers,), 0.5)
        for i in range(layers):
            if f"encoder.layers.{i}.VPT_gamma" in sd:
                gates[i] = torch.sigmoid(g(f"encoder.layers.{i}.VPT_gamma").reshape(()))      # fp32, at load
        W += [g("VPT")] + [g(f"encoder.layers.{i}.VPT_shallow") for i in range(1, P)] + [gates]
    fields = dict(hidden=D, layers=layers, heads=heads, patch=patch, kpad=kpad, mlp_dim=inter, n_prompt=n_ctx if P else 0, prompt_depth=P if n_ctx else 0,
                  image_size=grid * patch, pos_patch=pos[1:].contiguous())
    return names, [w.contiguous() for w in W], fields


class ClipEngine(_Engine, RangeGuard):
    """HF CLIPVisionModel state dict (+ VPT / VPT_shallow / VPT_gamma) -> pooler_output [B, hidden]; with `out_all=True` post_layernorm of
    every row the last block carries ([B, 1 + grid^2 (+ n_ctx when the prompts run to the end), hidden]).  Frames are fp32, already
    CLIP-normalised, image_size x image_size (VT_IMGNORM_RAW); precisions fp32 / bf16 / fp16 with the fp32 residual stream."""

    def __init__(self, sd: SD, *, heads: int, precision: str = "fp32", device="cuda", patch: int = 14, eps: float = 1e-5,
                 prompt_depth: Optional[int] = None, out_all: bool = False):
        self.device = L.require_gpu(device)
        cdt, adt = precision_dtypes(precision)
        self.cdt, self.adt, self.precision = cdt, adt, precision
        self.weight_names, W, f = clip_pack(sd, heads=heads, cdt=cdt, patch=patch, prompt_depth=prompt_depth)
        self._pos = f.pop("pos_patch").to(self.device)
        self._weights = [w.to(self.device) for w in W]
        self.hidden, self.heads, self.patch, self.layers = f["hidden"], heads, patch, f["layers"]
        self.image_size, self.n_ctx, self.prompt_depth, self.out_all = f["image_size"], f["n_prompt"], f["prompt_depth"], bool(out_all)
        desc = L.DinoDesc()
        for k, v in f.items():
            setattr(desc, k, v)
        desc.cdt, desc.adt, desc.eps = cdt, adt, eps
        desc.act, desc.pre_ln, desc.out_all = L.ACT_QUICK_GELU, 1, int(self.out_all)
        self._create("dino", desc, self._weights, "vt_dino_create (clip)")
        self._packed = self._derive("vt_dino_packed_bytes", "vt_dino_set_packed")
        self._range_init(L.lib().vt_dino_set_range_flag, "vt_dino_set_range_flag")
        self._ws = _Workspace(self.device)
        self.last_flags: Optional[torch.Tensor] = None

    @property
    def tokens_out(self) -> int:
        """Rows per image of `forward_tokens`: the prompt rows are still there when they run to the last block."""
        return 1 + (self.image_size // self.patch) ** 2 + (self.n_ctx if self.prompt_depth == self.layers else 0)

    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values [B, 3, S, S] fp32 -> [B, hidden] ([B, tokens_out, hidden] with out_all)."""
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or pixel_values.shape[2] != pixel_values.shape[3]:
            raise ValueError(f"ClipEngine: expected [B, 3, S, S] frames, got {tuple(pixel_values.shape)}")
        B, res = pixel_values.shape[0], pixel_values.shape[2]
        if res != self.image_size:
            raise L.VtError(f"ClipEngine: {res}x{res} frames, the tower takes {self.image_size}x{self.image_size} only (CLIP's position table is never interpolated)")
        x = pixel_values.to(self.device, torch.float32).contiguous()
        shape = (B, self.tokens_out, self.hidden) if self.out_all else (B, self.hidden)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        flags = torch.empty(1, 4, dtype=torch.float32, device=self.device)
        lib = L.lib()
        ws = self._ws.get(lib.vt_dino_workspace_bytes(self._h, B, res))
        L.check(lib.vt_dino_forward(self._h, L.ptr_array([x]), 1, 0, 0, C.c_float(1.0), L.IMGNORM_RAW, B, res, L.ptr(self._pos), L.ptr(out),
                                    L.ptr(flags), L.ptr(ws), L.stream_ptr(self.device)), "vt_dino_forward (clip)")
        self.last_flags = flags
        return out

    def forward_tokens(self, pixel_values: torch.Tensor) -> torch.Tensor:
        if not self.out_all:
            raise L.VtError("ClipEngine.forward_tokens: build the engine with out_all=True (the pooled engine prunes its last block to the CLS query)")
        return self.forward(pixel_values)


class LinearHead:
    """nn.Sequential(Linear, GELU, Linear[, GELU, Linear]) on vt_mlp (keys '0.weight', '2.weight', ..), erf GELU, fp32 in; `residual=True` adds
    the input to the result in the last Linear's epilogue (Adapter: x + rfc(x))."""

    def __init__(self, sd: SD, *, precision: str = "fp32", device="cuda", residual: bool = False):
        self.mlp = MlpEngine(sd, act=L.ACT_GELU_ERF, precision=precision, device=device)
        self.device, self.residual = self.mlp.device, residual
        if self.mlp.in_pad != self.mlp.in_features:
            raise L.VtError("LinearHead: input width must be a multiple of 16")
        if residual and (len(self.mlp.W) != 2 or self.mlp.out_features != self.mlp.in_features):
            raise L.VtError("LinearHead: the residual form is Linear, GELU, Linear back to the input width")

    def _cast(self, x: torch.Tensor) -> torch.Tensor:
        adt = L.torch_dtype(self.mlp.adt)
        if x.dtype == adt:
            return x
        y = torch.empty(x.shape, dtype=adt, device=self.device)
        L.check(L.lib().vt_cast(L.ptr(x), L.dt_code(x.dtype), x.shape[1], L.ptr(y), self.mlp.adt, x.shape[1], x.shape[0], x.shape[1],
                                L.stream_ptr(self.device)), "vt_cast")
        return y

    def __call__(self, x: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        lead = x.shape[:-1]
        x = x.to(self.device, torch.float32).reshape(-1, x.shape[-1]).contiguous()
        xa = self._cast(x)
        if not self.residual:
            return self.mlp(xa, out_dtype).reshape(*lead, -1)
        h = ops.gemm(xa, self.mlp.W[0], self.mlp.b[0], act=L.ACT_GELU_ERF)
        return ops.gemm(h, self.mlp.W[1], self.mlp.b[1], residual=x, out_dtype=torch.float32).reshape(*lead, -1)


class TactileHeads:
    """Video feature (frame mean, L2: `video`) and retrieval against a bank of saved video features (cosine similarity, top-k; ties go to
    the lower index: `retrieve`), batched over videos that share the bank."""

    def __init__(self, device="cuda"):
        self.device = L.require_gpu(device)
        self.bank: Optional[torch.Tensor] = None
        self.bank_norm: Optional[torch.Tensor] = None
        self._bank_src = None                                        # (the caller's tensor, its version): the same tensor is not uploaded again

    def set_bank(self, saved_embeddings: torch.Tensor) -> None:
        """saved_embeddings [R, D]: uploaded once, with its row norms; handing in the same unmodified tensor again is free."""
        if self._bank_src is not None and self._bank_src[0] is saved_embeddings and self._bank_src[1] == saved_embeddings._version:
            return
        if saved_embeddings.dim() != 2 or saved_embeddings.shape[0] < 1 or saved_embeddings.shape[1] % 4:
            raise ValueError(f"TactileHeads: the bank must be [R >= 1, D % 4 == 0], got {tuple(saved_embeddings.shape)}")
        self.bank = saved_embeddings.to(self.device, torch.float32).contiguous()
        self.bank_norm = torch.empty(self.bank.shape[0], dtype=torch.float32, device=self.device)
        L.check(L.lib().vt_tactile_bank_norms(L.ptr(self.bank), self.bank.shape[0], self.bank.shape[1], L.ptr(self.bank_norm),
                                              L.stream_ptr(self.device)), "vt_tactile_bank_norms")
        self._bank_src = (saved_embeddings, saved_embeddings._version)

    def _pooled(self, pooled: torch.Tensor) -> torch.Tensor:
        if pooled.dim() != 3:
            raise ValueError(f"TactileHeads: pooled must be [b, l, D], got {tuple(pooled.shape)}")
        return pooled.to(self.device, torch.float32).contiguous()

    def video(self, pooled: torch.Tensor) -> torch.Tensor:
        """pooled [b, l, D] fp32 -> the video features [b, D], whether or not a bank is set."""
        pooled = self._pooled(pooled)
        b, l, D = pooled.shape
        video = torch.empty(b, D, dtype=torch.float32, device=self.device)
        L.check(L.lib().vt_tactile_head(L.ptr(pooled), b, l, D, None, None, 0, 0, L.ptr(video), None, None, None, L.stream_ptr(self.device)), "vt_tactile_head")
        return video

    def retrieve(self, pooled: torch.Tensor, k: int):
        """pooled [b, l, D] fp32 -> (video [b, D], sims [b, R], topk_idx [b, k] int32, topk_val [b, k]) against the bank of `set_bank`."""
        if self.bank is None:
            raise ValueError("TactileHeads.retrieve needs a bank (set_bank)")
        pooled = self._pooled(pooled)
        b, l, D = pooled.shape
        R = self.bank.shape[0]
        if self.bank.shape[1] != D:
            raise ValueError(f"TactileHeads: the bank is {self.bank.shape[1]} wide, the features {D}")
        if k < 0 or k > R or k > TOPK_MAX:
            raise ValueError(f"TactileHeads: k = {k} outside 0 .. min(R = {R}, {TOPK_MAX})")
        video = torch.empty(b, D, dtype=torch.float32, device=self.device)
        sims = torch.empty(b, R, dtype=torch.float32, device=self.device)
        idx = torch.empty(b, max(k, 1), dtype=torch.int32, device=self.device)
        val = torch.empty(b, max(k, 1), dtype=torch.float32, device=self.device)
        L.check(L.lib().vt_tactile_head(L.ptr(pooled), b, l, D, L.ptr(self.bank), L.ptr(self.bank_norm), R, k, L.ptr(video), L.ptr(sims), L.ptr(idx),
                                        L.ptr(val), L.stream_ptr(self.device)), "vt_tactile_head")
        return video, sims, idx[:, :k], val[:, :k]
