"""T5 v1.1 text encoder on the HIP engine (csrc/vt_t5.hip): HF T5EncoderModel with feed_forward_proj = "gated-gelu" — the encoder
that turns an instruction into RDT's lang_tokens (reference: models/multimodal_encoder/t5_encoder.py::T5Embedder).

* `bucket_table` — HF T5Attention._relative_position_bucket (bidirectional) for every relative position -1023 .. 1023, computed
  on the host in fp32 with HF's own formula; the kernel never evaluates `log` (a one-ulp difference flips the bucket at exact powers).
* `pack_plan` — host-only map from an HF state dict to the engine's weight slots (testable without a GPU).
* `T5Engine(sd, config, precision)` — packs the weights on the device (one tensor at a time) and runs `forward(ids, mask)`.
* `load_t5_encoder(path_or_name, precision, device)` — local HF directory or the local HF cache only; never fetches.
"""
from __future__ import annotations

import glob
import json
import math
import os
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from vlatouch import _lib as L
from vlatouch.engine import _Engine

MAX_LEN = 1024          # longest sequence of the attention kernel (RDT-1B's max_lang_cond_len)
REL_SPAN = MAX_LEN - 1  # bucket table covers rel = -REL_SPAN .. REL_SPAN

EMBED_KEYS = ("shared.weight", "encoder.embed_tokens.weight")


def t5_config(config) -> Dict:
    """Normalise an HF T5Config (object or dict) to the fields the engine needs; rejects anything but the v1.1 gated-gelu encoder."""
    c = config if isinstance(config, Mapping) else {k: getattr(config, k) for k in dir(config) if not k.startswith("_")}
    ffp = c.get("feed_forward_proj", "relu")
    if ffp != "gated-gelu":
        raise ValueError(f"T5 encoder: feed_forward_proj={ffp!r} is not supported; only T5 v1.1's 'gated-gelu' is built "
                         "(v1.0 ReLU FFNs are out of scope)")
    d_kv = int(c.get("d_kv", 64))
    if d_kv != 64:
        raise ValueError(f"T5 encoder: d_kv={d_kv} is not supported (the attention kernel is built for 64-wide heads)")
    return dict(vocab_size=int(c["vocab_size"]), d_model=int(c["d_model"]), d_kv=d_kv, d_ff=int(c["d_ff"]), num_heads=int(c["num_heads"]),
                num_layers=int(c["num_layers"]), relative_attention_num_buckets=int(c.get("relative_attention_num_buckets", 32)),
                relative_attention_max_distance=int(c.get("relative_attention_max_distance", 128)),
                layer_norm_epsilon=float(c.get("layer_norm_epsilon", 1e-6)), feed_forward_proj=ffp)


def relative_position_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """HF T5Attention._relative_position_bucket(rel, bidirectional=True, ...), restated operation for operation (fp32 log)."""
    buckets = torch.zeros_like(rel)
    num_buckets //= 2
    buckets += (rel > 0).to(torch.long) * num_buckets
    rel = torch.abs(rel)
    max_exact = num_buckets // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rel, large)


def bucket_table(num_buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    """int8 [2047]: the bucket of rel = j - i at index rel + 1023 (the layout vt_t5_forward reads)."""
    rel = torch.arange(-REL_SPAN, REL_SPAN + 1, dtype=torch.long)
    return relative_position_bucket(rel, num_buckets, max_distance).numpy().astype(np.int8)


def embed_key(keys) -> str:
    for k in EMBED_KEYS:
        if k in keys:
            return k
    raise KeyError(f"T5 state dict has no token embedding (expected one of {EMBED_KEYS})")


def pack_plan(cfg: Dict, keys) -> List[Tuple[str, List[str], str]]:
    """[(slot, source keys concatenated along dim 0, 'w' = weight dtype | 'f32')] in vt_t5_create's order.  Host-only."""
    keys = set(keys)
    a = "encoder.block.{}.layer.0.SelfAttention."
    f = "encoder.block.{}.layer.1.DenseReluDense."
    plan = [("shared", [embed_key(keys)], "w"), ("rel_bias", [a.format(0) + "relative_attention_bias.weight"], "f32")]
    for i in range(cfg["num_layers"]):
        plan += [(f"ln1.{i}", [f"encoder.block.{i}.layer.0.layer_norm.weight"], "f32"),
                 (f"qkv.{i}", [a.format(i) + n + ".weight" for n in ("q", "k", "v")], "w"),
                 (f"o.{i}", [a.format(i) + "o.weight"], "w"),
                 (f"ln2.{i}", [f"encoder.block.{i}.layer.1.layer_norm.weight"], "f32"),
                 (f"wi.{i}", [f.format(i) + "wi_0.weight", f.format(i) + "wi_1.weight"], "w"),
                 (f"wo.{i}", [f.format(i) + "wo.weight"], "w")]
    plan.append(("final_ln", ["encoder.final_layer_norm.weight"], "f32"))
    missing = [k for _, ks, _ in plan for k in ks if k not in keys]
    if missing:
        raise KeyError(f"T5 state dict lacks {len(missing)} encoder tensors, e.g. {missing[:3]}")
    return plan


def slot_shapes(cfg: Dict) -> Dict[str, Tuple[int, ...]]:
    """Packed shape of every slot of pack_plan (for checks)."""
    D, I, F, H = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"], cfg["num_heads"]
    s = {"shared": (cfg["vocab_size"], D), "rel_bias": (cfg["relative_attention_num_buckets"], H), "final_ln": (D,)}
    for i in range(cfg["num_layers"]):
        s.update({f"ln1.{i}": (D,), f"qkv.{i}": (3 * I, D), f"o.{i}": (D, I), f"ln2.{i}": (D,), f"wi.{i}": (2 * F, D), f"wo.{i}": (D, F)})
    return s


PRECISIONS = {"fp32": L.F32, "bf16": L.BF16}


class T5Engine(_Engine):
    """HF T5EncoderModel (v1.1, gated-gelu) on libvlatouch_hip.so.  `sd` maps HF keys to tensors (any device / dtype; values are read
    one at a time and moved to `device`, so a lazily loading mapping keeps the host footprint at one tensor)."""

    def __init__(self, sd: Mapping[str, torch.Tensor], config, precision: str = "bf16", device="cuda"):
        if precision not in PRECISIONS:
            raise ValueError(f"T5 precision {precision!r}: use 'fp32' or 'bf16' (T5 v1.1 overflows in fp16, which is not built)")
        self.cfg = t5_config(config)
        self.precision = precision
        self.device = L.require_gpu(device)
        code = PRECISIONS[precision]
        wdt = L.torch_dtype(code)
        want = slot_shapes(self.cfg)
        self.weights: List[torch.Tensor] = []
        for slot, ks, kind in pack_plan(self.cfg, sd.keys()):
            dt = wdt if kind == "w" else torch.float32
            parts = [sd[k].to(device=self.device, dtype=dt) for k in ks]
            w = (parts[0] if len(parts) == 1 else torch.cat(parts, 0)).contiguous()
            del parts
            if tuple(w.shape) != want[slot]:
                raise ValueError(f"T5 weight slot {slot} has shape {tuple(w.shape)}, expected {want[slot]}")
            self.weights.append(w)
        c = self.cfg
        self.desc = L.T5Desc(c["vocab_size"], c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"], c["num_layers"],
                             c["relative_attention_num_buckets"], c["relative_attention_max_distance"], c["layer_norm_epsilon"], code, code)
        self._create("t5", self.desc, self.weights)
        self.buckets = torch.from_numpy(bucket_table(c["relative_attention_num_buckets"], c["relative_attention_max_distance"])).to(self.device)
        self._ws: Optional[torch.Tensor] = None

    @property
    def d_model(self) -> int:
        return self.cfg["d_model"]

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, out_dtype=torch.float32) -> torch.Tensor:
        """input_ids [B, L] (or [L]) -> last_hidden_state [B, L, d_model] on the engine's device."""
        ids = input_ids.reshape(1, -1) if input_ids.dim() == 1 else input_ids
        B, Lq = ids.shape
        if Lq > MAX_LEN:
            raise ValueError(f"T5 encoder: sequence length {Lq} exceeds {MAX_LEN}")
        ids_h = np.ascontiguousarray(ids.detach().cpu().numpy().astype(np.int32))
        mask_h = None
        if attention_mask is not None:
            mask_h = np.ascontiguousarray((attention_mask.detach().reshape(B, Lq).cpu().numpy() != 0).astype(np.uint8))
        lib = L.lib()
        need = lib.vt_t5_workspace_bytes(self._h, B, Lq)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(B, Lq, self.d_model, dtype=out_dtype, device=self.device)
        L.check(lib.vt_t5_forward(self._h, ids_h.ctypes.data_as(L.C.c_void_p), None if mask_h is None else mask_h.ctypes.data_as(L.C.c_void_p),
                                  B, Lq, L.ptr(self.buckets), L.ptr(out), L.dt_code(out_dtype), L.ptr(self._ws), L.stream_ptr(self.device)),
                "vt_t5_forward")
        return out

    __call__ = forward


# ------------------------------------------------------------------ loading (local files only)
class _LazySafetensors(Mapping):
    """key -> tensor read on access from one or more .safetensors files (never the whole checkpoint in host memory)."""

    def __init__(self, files: List[str]):
        from safetensors import safe_open
        self._where: Dict[str, str] = {}
        self._open: Dict[str, object] = {}
        for f in files:
            h = safe_open(f, framework="pt")
            self._open[f] = h
            for k in h.keys():
                self._where[k] = f

    def __getitem__(self, k):
        return self._open[self._where[k]].get_tensor(k)

    def __iter__(self):
        return iter(self._where)

    def __len__(self):
        return len(self._where)


class _LazyBins(Mapping):
    def __init__(self, files: List[str]):
        self._sds = [torch.load(f, map_location="cpu", mmap=True, weights_only=True) for f in files]
        self._where = {k: i for i, sd in enumerate(self._sds) for k in sd}

    def __getitem__(self, k):
        return self._sds[self._where[k]][k]

    def __iter__(self):
        return iter(self._where)

    def __len__(self):
        return len(self._where)


def _shards(path: str, index_name: str) -> List[str]:
    idx = json.load(open(os.path.join(path, index_name)))
    return [os.path.join(path, f) for f in sorted(set(idx["weight_map"].values()))]


def local_state_dict(path: str) -> Mapping[str, torch.Tensor]:
    """The weights of a local HF directory: model.safetensors, its sharded form (model.safetensors.index.json), or pytorch_model*.bin."""
    if os.path.isfile(os.path.join(path, "model.safetensors")):
        return _LazySafetensors([os.path.join(path, "model.safetensors")])
    if os.path.isfile(os.path.join(path, "model.safetensors.index.json")):
        return _LazySafetensors(_shards(path, "model.safetensors.index.json"))
    if os.path.isfile(os.path.join(path, "pytorch_model.bin.index.json")):
        return _LazyBins(_shards(path, "pytorch_model.bin.index.json"))
    bins = sorted(glob.glob(os.path.join(path, "pytorch_model*.bin")))
    if bins:
        return _LazyBins(bins)
    raise FileNotFoundError(f"{path} holds no model.safetensors, model.safetensors.index.json or pytorch_model*.bin")


def hf_cache_dirs() -> List[str]:
    """The local HF hub cache directories, in HF's own order of precedence."""
    out = []
    for var in ("HF_HUB_CACHE", "HUGGINGFACE_HUB_CACHE"):
        if os.environ.get(var):
            out.append(os.environ[var])
    home = os.environ.get("HF_HOME") or os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "huggingface")
    out.append(os.path.join(home, "hub"))
    return out


def resolve_local(path_or_name: str, cache_dir: Optional[str] = None) -> str:
    """A local directory as given, or the snapshot of an HF repo id (e.g. google/t5-v1_1-xxl) in the local cache.  Never fetches."""
    if os.path.isdir(path_or_name):
        return path_or_name
    repo = "models--" + path_or_name.replace("/", "--")
    roots = ([cache_dir] if cache_dir else []) + hf_cache_dirs()
    for root in roots:
        d = os.path.join(root, repo)
        ref = os.path.join(d, "refs", "main")
        snaps = [os.path.join(d, "snapshots", open(ref).read().strip())] if os.path.isfile(ref) else []
        snaps += sorted(glob.glob(os.path.join(d, "snapshots", "*")))
        for s in snaps:
            if os.path.isfile(os.path.join(s, "config.json")):
                return s
    raise FileNotFoundError(
        f"no local copy of {path_or_name!r}: this loader never downloads. Place the checkpoint (config.json plus model.safetensors, its sharded "
        f"form with model.safetensors.index.json, or pytorch_model*.bin) in a directory and pass that directory, or put the HF snapshot under "
        f"{os.path.join(roots[0], repo, 'snapshots', '<revision>')}")


def load_t5_encoder(path_or_name: str, precision: str = "bf16", device="cuda", cache_dir: Optional[str] = None) -> T5Engine:
    """T5Engine from a local HF directory or a repo id found in the local HF cache (FileNotFoundError otherwise; no network)."""
    path = resolve_local(path_or_name, cache_dir)
    cfg = json.load(open(os.path.join(path, "config.json")))
    return T5Engine(local_state_dict(path), cfg, precision=precision, device=device)
