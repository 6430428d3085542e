"""Mirror of octopi/octopi_s/utils/encoder.py (the reference's planning-level tactile encoder): `CLIPVisionEncoder`, `ViFiCLIP`, `Adapter`,
`PropertyClassifier`, `load_encoder`, and beside them `TactileProjector` (the `project` module of llm.py:141-145) and `rag_topk` (the retrieval
of dataset.py:189-195).  The CLIP ViT-L/14 vision tower with deep visual prompts runs in the HIP engine (vlatouch.clip.ClipEngine), the video
feature and the retrieval in vt_tactile_head, the Linears on vt_gemm / vt_mlp.

Not built: the CLIP text tower (`ViFiCLIP.forward` with texts raises), the LLM, and the torchvision tensor-bicubic resize in front of the
encoder: frames arrive as `get_frames` returns them, fp32, CLIP-normalised, image_size x image_size.  There is no hub access: where the
reference downloads (`from_pretrained(use_clip)`), `use_clip` must be a local HF directory (config.json + model.safetensors /
pytorch_model.bin) or `state_dict=` must be given; VLATOUCH_SYNTH_WEIGHTS=1 gives the deterministic synthetic set."""
from __future__ import annotations

import json
import os
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from vlatouch import _lib as L
from vlatouch import synth
from vlatouch.clip import ClipEngine, LinearHead, TactileHeads, clip_vision_sd
from vlatouch.engine import AutoRange
from vlatouch.module import default_precision

_VIT_L14 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14)


def _strip_module(sd):
    return {k.replace("module.", ""): v for k, v in sd.items()}


def _load_local(path: str):
    cfg = dict(_VIT_L14)
    cj = os.path.join(path, "config.json")
    if os.path.isfile(cj):
        with open(cj) as f:
            c = json.load(f)
        c = c.get("vision_config", c)
        cfg.update({k: c[k] for k in cfg if k in c})
    st = os.path.join(path, "model.safetensors")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        return cfg, load_file(st)
    pt = os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(pt):
        return cfg, torch.load(pt, map_location="cpu", weights_only=True)
    return cfg, None


class ClipVisionTower:
    """`clip_model.vision_model` of the reference: the weights (HF CLIP vision keys relative to `vision_model.`, plus VPT / VPT_shallow /
    VPT_gamma) and the engine built from them.  `prompt_configs`: prompt_learning.yaml's num_context_vision, prompt_depth_vision, gate_prior;
    prompt parameters a checkpoint lacks are initialised as the reference's constructor does (0.02 x normal, gamma = gate_prior)."""

    def __init__(self, use_clip, prompt_configs: Optional[dict] = None, *, device="cuda", precision: Optional[str] = None,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, config: Optional[dict] = None):
        self.name = use_clip
        self._device = torch.device(device)
        self.precision = precision or default_precision()
        self.cfg = dict(_VIT_L14, **(config or {}))
        self.prompt_configs = dict(prompt_configs or {})
        sd = state_dict
        if sd is None and use_clip is not None and os.path.isdir(str(use_clip)):
            cfg, sd = _load_local(str(use_clip))
            self.cfg.update(cfg if config is None else {})
        if sd is None:
            if os.environ.get("VLATOUCH_SYNTH_WEIGHTS") == "1":
                c = self.cfg
                shapes = synth.clip_shapes(c["hidden_size"], c["num_hidden_layers"], c["intermediate_size"], c["image_size"], c["patch_size"],
                                           n_ctx=self.prompt_configs.get("num_context_vision", 0), prompt_depth=self.prompt_configs.get("prompt_depth_vision", 0))
                sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(shapes, prefix="clip.").items()}
            else:
                raise FileNotFoundError(
                    f"no CLIP weights for {use_clip!r}: pass state_dict=, point use_clip at a local HF directory, "
                    "or set VLATOUCH_SYNTH_WEIGHTS=1 for deterministic synthetic weights (no network access here)")
        self.sd = dict(clip_vision_sd(_strip_module(sd)))
        self.engine: Optional[ClipEngine] = None
        self._range: Optional[AutoRange] = None

    # ---- weights
    def load_state_dict(self, sd, strict: bool = False):
        """Overlay a checkpoint's vision keys (`module.` stripped; `clip_model.vision_model.` / `vision_model.` prefixes) and rebuild the engine
        at the next call.  Text-tower and logit-scale keys are ignored, as the reference ignores them with strict=False."""
        new = clip_vision_sd(_strip_module(sd))
        new = {k: v for k, v in new.items() if k in self.sd or "VPT" in k}
        self.sd.update(new)
        self.engine = None
        return sorted(new)

    def _complete_prompts(self):
        c, pc = self.cfg, self.prompt_configs
        if not pc:
            return None                                              # no prompt_learning.yaml: the depth is read off the checkpoint's keys
        layers, D = c["num_hidden_layers"], c["hidden_size"]
        P = pc.get("prompt_depth_vision", 0)
        P = layers if P == -1 else P
        n = pc.get("num_context_vision", 0) if P else 0
        if not (P and n):
            for k in [k for k in self.sd if "VPT" in k]:
                del self.sd[k]
            return 0
        init = lambda name: torch.from_numpy(synth.clip_prompt_init(name, n, D))
        self.sd.setdefault("VPT", init("VPT"))
        for i in range(layers):
            if 1 <= i < P:
                self.sd.setdefault(f"encoder.layers.{i}.VPT_shallow", init(f"{i}.VPT_shallow"))
            if i != layers - 1:
                self.sd.setdefault(f"encoder.layers.{i}.VPT_gamma", torch.tensor(float(pc.get("gate_prior", 0.0))))
        return P

    def _build(self, prec: str) -> ClipEngine:
        P = self._complete_prompts()
        return ClipEngine(self.sd, heads=self.cfg["num_attention_heads"], precision=prec, device=self._device, patch=self.cfg["patch_size"], prompt_depth=P)

    def _ensure(self):
        if self.engine is None:
            prec = self.precision
            if prec == "bf16":      # as for the other towers: IEEE fp16 storage (fp32 residual stream) by default, bf16 storage when the range guard fires
                prec = os.environ.get("VLATOUCH_CLIP_PRECISION") or "fp16"
                if "VLATOUCH_CLIP_PRECISION" not in os.environ:
                    self._range = AutoRange(f"ClipVisionTower({self.name})")
            self.engine = self._build(prec)

    @torch.no_grad()
    def pooler_output(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """[B, 3, S, S] fp32 -> [B, hidden] fp32."""
        self._ensure()
        out = self.engine.forward(pixel_values)
        rg = self._range
        if rg is not None and not rg.fell_back:
            bits = rg.after(self.engine, self.engine.adt == L.F16)
            if bits:
                rg.fall_back(bits)
                self.engine = self._build("bf16")
                out = self.engine.forward(pixel_values)
        return out

    @property
    def hidden_size(self) -> int:
        return self.cfg["hidden_size"]


def _frames_5d(frames: torch.Tensor):
    if frames.dim() != 5:
        raise ValueError(f"frames must be [b, l, c, h, w], got {tuple(frames.shape)}")
    b, l, c, h, w = frames.shape
    return b, l, frames.reshape(b * l, c, h, w)


class CLIPVisionEncoder:
    """encoder.py:426-438: frames [b, l, c, h, w] -> pooler_output per frame [b, l, D]."""

    def __init__(self, clip_model, **kw):
        self.model = clip_model if isinstance(clip_model, ClipVisionTower) else ClipVisionTower(clip_model, **kw)

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        b, l, x = _frames_5d(frames)
        return self.model.pooler_output(x).reshape(b, l, -1)

    __call__ = forward

    def eval(self):
        return self


class ViFiCLIP:
    """encoder.py:389-423: the video feature = mean of the frame features, L2-normalised.  `clip_model`: a ClipVisionTower (the vision half
    of the reference's CLIP model)."""

    def __init__(self, clip_model: ClipVisionTower, freeze_text_encoder: bool = True, use_positional_embeds: bool = True):
        self.clip_model = clip_model
        self.use_positional_embeds = use_positional_embeds
        self._heads: Optional[TactileHeads] = None

    @property
    def heads(self) -> TactileHeads:
        if self._heads is None:
            self._heads = TactileHeads(self.clip_model._device)
        return self._heads

    def load_state_dict(self, sd, strict: bool = False):
        return self.clip_model.load_state_dict(sd, strict)

    def frame_features(self, frames: torch.Tensor) -> torch.Tensor:
        b, l, x = _frames_5d(frames)
        return self.clip_model.pooler_output(x).reshape(b, l, -1)

    def forward(self, frames, texts=None, attention_masks=None):
        if texts is not None:
            raise NotImplementedError("ViFiCLIP: the CLIP text tower is not built; pass texts=None (video features only)")
        return self.heads.video(self.frame_features(frames)), None, None, None

    __call__ = forward

    def eval(self):
        return self


class _Head:
    _files = ()

    def load_state_dict(self, sd, strict: bool = True):
        sd = _strip_module(sd)
        missing = [k for k in self._keys if k not in sd]
        if strict and (missing or len(sd) != len(self._keys)):
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing {missing}, unexpected {sorted(set(sd) - set(self._keys))}")
        self._sd.update({k: v.detach().float().cpu() for k, v in sd.items() if k in self._keys})
        self._eng = None

    def state_dict(self):
        return dict(self._sd)

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self


def _synth_sd(prefix: str, shapes):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(shapes, prefix=prefix).items()}


class Adapter(_Head):
    """encoder.py:441-474: x + rfc(x), rfc = Linear(D, 512), GELU, Linear(512, D); `align` exists only when the sizes differ, which no caller
    in the reference asks for, and is refused here."""

    def __init__(self, input_size: int, output_size: int, residual_ratio: float = 0.5, *, device="cuda", precision: Optional[str] = None):
        if input_size != output_size:
            raise NotImplementedError("Adapter: input_size != output_size (the `align` branch) is not built")
        self.residual_ratio, self.device, self.precision = residual_ratio, device, precision or default_precision()
        shapes = synth.tactile_head_shapes(input_size)["adapter"]
        self._keys = list(shapes)
        # Until a file is loaded the weights are zero, so the module is the identity.  The reference's constructor draws trunc-normal weights of
        # std 1e-3 (biases 0) from torch's global generator: within 1e-3 of the identity, and not a stream that can be reproduced here.
        self._sd = {k: torch.zeros(s) for k, s in shapes.items()}
        self._eng = None

    def forward(self, vision_features: torch.Tensor) -> torch.Tensor:
        if self._eng is None:
            self._eng = LinearHead({"0.weight": self._sd["rfc.0.weight"], "0.bias": self._sd["rfc.0.bias"], "2.weight": self._sd["rfc.2.weight"],
                                    "2.bias": self._sd["rfc.2.bias"]}, precision=self.precision, device=self.device, residual=True)
        return self._eng(vision_features)

    __call__ = forward


class PropertyClassifier(_Head):
    """encoder.py:477-495: fc = Linear(D, 512), GELU, Linear(512, 256), GELU; [hardness_fc | roughness_fc] -> [B, 2]."""

    def __init__(self, input_size: int, *, device="cuda", precision: Optional[str] = None):
        self.device, self.precision = device, precision or default_precision()
        shapes = synth.tactile_head_shapes(input_size)["property_classifier"]
        self._keys = list(shapes)
        self._sd = {k: torch.zeros(s) for k, s in shapes.items()}
        self._eng = None

    def forward(self, vision_features: torch.Tensor) -> torch.Tensor:
        if self._eng is None:
            s = self._sd
            self._eng = LinearHead({"0.weight": s["fc.0.weight"], "0.bias": s["fc.0.bias"], "2.weight": s["fc.2.weight"], "2.bias": s["fc.2.bias"],
                                    "4.weight": torch.cat([s["hardness_fc.weight"], s["roughness_fc.weight"]], dim=0),
                                    "4.bias": torch.cat([s["hardness_fc.bias"], s["roughness_fc.bias"]], dim=0)}, precision=self.precision, device=self.device)
        return self._eng(vision_features)

    __call__ = forward


class TactileProjector(_Head):
    """llm.py:139-145, 171-175: project(encoder(frames)) -> [b, l, E] in the LLM's dtype: the tactile tokens spliced between the text
    embeddings.  `project` = Linear(D, E), GELU, Linear(E, E), loaded from project.pt."""

    def __init__(self, encoder: CLIPVisionEncoder, llm_embedding_size: int, *, dtype: torch.dtype = torch.bfloat16, device="cuda",
                 precision: Optional[str] = None):
        self.encoder, self.dtype, self.device, self.precision = encoder, dtype, device, precision or default_precision()
        shapes = synth.tactile_head_shapes(encoder.model.hidden_size, llm_embedding_size)["project"]
        self._keys = list(shapes)
        self._sd = {k: torch.zeros(s) for k, s in shapes.items()}
        self._eng = None

    def load(self, load_exp_path: str) -> bool:
        f = os.path.join(load_exp_path, "project.pt")
        if not os.path.exists(f):
            return False
        self.load_state_dict(torch.load(f, map_location="cpu", weights_only=True))
        return True

    def project(self, feats: torch.Tensor) -> torch.Tensor:
        if self._eng is None:
            self._eng = LinearHead(self._sd, precision=self.precision, device=self.device)
        return self._eng(feats, self.dtype)

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        return self.project(self.encoder(frames))

    __call__ = forward


def rag_topk(frames: torch.Tensor, vificlip: ViFiCLIP, saved_embeddings: torch.Tensor, k: int = 1):
    """dataset.py:189-195 batched: frames [b, l, c, h, w] (or one video [l, c, h, w]) -> (indices [b, k] int64, similarities [b, k]) of the
    saved video features nearest to each video; the caller maps the indices to object ids, as get_rag_tactile_paths does.  Ties go to the
    lower index.  The bank is kept on the device between calls that hand in the same tensor."""
    if frames.dim() == 4:
        frames = frames.unsqueeze(0)
    R = saved_embeddings.shape[0]
    if k < 1 or k > R or k > 16:
        raise ValueError(f"rag_topk: k = {k} outside 1 .. min(R = {R}, 16)")
    vificlip.heads.set_bank(saved_embeddings)                        # uploaded (with its row norms) only when the tensor is new or was modified
    _, _, idx, val = vificlip.heads.retrieve(vificlip.frame_features(frames), k)
    return idx.long(), val


def load_encoder(configs, device, *, precision: Optional[str] = None, state_dict=None, clip_config: Optional[dict] = None):
    """encoder.py:498-544: reads run.yaml, prompt_learning.yaml, tactile_vificlip.pt, the two adapter files and property_classifier.pt from the
    local `configs["load_exp_path"]` -> (tactile_vificlip, dotted_tactile_adapter, plain_tactile_adapter, property_classifier, load_exp_configs).
    A missing weight file warns with the reference's words and leaves the module at its initial weights."""
    import yaml
    path = configs["load_exp_path"]
    def read_yaml(name):
        with open(os.path.join(path, name), "r") as f:
            return yaml.safe_load(f)

    load_exp_configs = None if path is None else read_yaml("run.yaml")
    if "prompt_learning.yaml" in os.listdir(path):
        prompt_learning_configs = read_yaml("prompt_learning.yaml")
        use_clip = prompt_learning_configs["use_clip"]
    else:
        prompt_learning_configs, use_clip = None, configs["use_clip"]
    clip = ClipVisionTower(use_clip, prompt_learning_configs, device=device, precision=precision, state_dict=state_dict, config=clip_config)
    tactile_vificlip = ViFiCLIP(clip, freeze_text_encoder=True, use_positional_embeds=True)

    def load(module, fname, strict, ok, missing):
        f = os.path.join(path, fname)
        if os.path.exists(f):
            module.load_state_dict(torch.load(f, map_location="cpu", weights_only=True), strict=strict)
            print(ok)
        else:
            warnings.warn(missing)

    load(tactile_vificlip, "tactile_vificlip.pt", False, "Loaded tactile ViFi-CLIP!", "No trained tactile ViFi-CLIP model found!")
    D = load_exp_configs["dim_context_vision"]
    dotted = Adapter(D, D, load_exp_configs["residual_ratio"], device=device, precision=precision)
    load(dotted, "dotted_tactile_adapter.pt", True, "Loaded dotted tactile adapter!", "No trained dotted tactile adapter found!")
    plain = Adapter(D, D, load_exp_configs["residual_ratio"], device=device, precision=precision)
    load(plain, "plain_tactile_adapter.pt", True, "Loaded plain tactile adapter!", "No trained plain tactile adapter found!")
    prop = PropertyClassifier(D, device=device, precision=precision)
    load(prop, "property_classifier.pt", True, "Loaded property regression model!", "No trained property regression model found!")
    return tactile_vificlip, dotted, plain, prop, load_exp_configs
