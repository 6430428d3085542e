"""Seeded inputs and synthetic weights shared by tools/make_golden.py (which feeds them to the
imported reference) and the parity tests (which feed them to the oracle and the HIP path).
Only OUTPUTS are stored in tests/golden/*.npz; inputs and weights are regenerated from seeds.
"""
from __future__ import annotations

import os
import sys
from typing import Dict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vla-touch_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from vlatouch import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def T(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a))


def sd_torch(shapes, prefix="", salt="") -> Dict[str, torch.Tensor]:
    return {k: T(v) for k, v in synth.fill_state_dict(shapes, prefix, salt).items()}


# ------------------------------------------------------------------ weights
def si_net_sd(salt: str = "") -> Dict[str, torch.Tensor]:
    """InterpolantsConditionalUnet1D(10, 256) state dict.  salt="" = raw `net`, "ema" = shadow params."""
    return sd_torch(synth.si_net_shapes(10, 256), prefix="si.", salt=salt)


def dino_sd(size: str = "small") -> Dict[str, torch.Tensor]:
    c = synth.DINOV2_CONFIGS[size]
    name = size.split("-")[0]              # "giant-l4" = the first 4 blocks of giant: same tensor names, same weights
    return sd_torch(synth.dinov2_shapes(c["hidden"], c["layers"], swiglu=c.get("swiglu", False)), prefix=f"dinov2-{name}.")


def siglip_sd(name: str = "tiny") -> Dict[str, torch.Tensor]:
    return sd_torch(synth.siglip_shapes(**synth.SIGLIP_CONFIGS[name]), prefix=f"siglip-{name}.")


def siglip_pixels(B: int, res: int, seed: int = 8) -> torch.Tensor:
    """SiglipImageProcessor output range: (x/255 - 0.5) / 0.5 in [-1, 1]."""
    g = synth.inputs_rng(seed)
    return T((2.0 * g.random((B, 3, res, res), dtype=np.float32) - 1.0))


def state_encoder_sd(obs_dim: int) -> Dict[str, torch.Tensor]:
    return sd_torch(synth.state_encoder_shapes(obs_dim), prefix="state_encoder.")


def force_decoder_sd() -> Dict[str, torch.Tensor]:
    return sd_torch(synth.force_decoder_shapes(), prefix="force_decoder.")


def lstm_mods(latent: int = 384, hidden: int = 256, layers: int = 2) -> Dict[str, Dict[str, torch.Tensor]]:
    shp = synth.lstm_controller_shapes(latent, hidden=hidden, layers=layers)
    tag = "" if (hidden, layers) == (256, 2) else f"h{hidden}l{layers}."           # other widths / depths: their own deterministic weights
    return {m: sd_torch(s, prefix=f"lstm_ctrl.{tag}{m}.") for m, s in shp.items()}


RDT_TINY = dict(hidden=256, depth=4, heads=4, horizon=8, action_dim=128, lang_token_dim=96, img_token_dim=80,
                state_token_dim=128, max_lang_cond_len=16, img_cond_len=24)
RDT_WIDE = dict(hidden=2048, depth=2, heads=32, horizon=64, action_dim=128, lang_token_dim=128, img_token_dim=96,
                state_token_dim=128, max_lang_cond_len=32, img_cond_len=64)


def rdt_sd(cfg: dict, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    sd = sd_torch(synth.rdt_runner_shapes(**cfg), prefix=f"rdt{cfg['hidden']}.")
    return {k: v.to(dtype) for k, v in sd.items()}


def stats(kind: str = "nontrivial") -> Dict[str, torch.Tensor]:
    """Normalisation stats (controller_dataset.py:222-229).  'nontrivial' has a zero-range dim (9)."""
    if kind == "unit":
        z, o = torch.zeros(10), torch.ones(10)
        return dict(action_mins=z.clone(), action_maxs=o.clone(), vla_mins=z.clone(), vla_maxs=o.clone(),
                    action_range=o.clone(), vla_range=o.clone())
    g = synth.inputs_rng(77)
    amin = g.uniform(-1.0, -0.2, 10).astype(np.float32)
    amax = amin + g.uniform(0.5, 2.0, 10).astype(np.float32)
    vmin = g.uniform(-1.2, -0.1, 10).astype(np.float32)
    vmax = vmin + g.uniform(0.4, 2.5, 10).astype(np.float32)
    vmax[9] = vmin[9]            # zero range: exercises the <1e-6 guard (normalise only)
    d = dict(action_mins=amin, action_maxs=amax, vla_mins=vmin, vla_maxs=vmax,
             action_range=amax - amin, vla_range=vmax - vmin)
    return {k: T(v) for k, v in d.items()}


MODEL_ARGS = synth.MODEL_ARGS


def build_controller(cls, precision: str, device="cuda:0", size: str = "small", stats_kind: str = "nontrivial", **kw):
    """vlatouch.synth.build_controller with this module's normalisation statistics."""
    return synth.build_controller(cls, precision, device=device, size=size, stats=stats(stats_kind), **kw)


# ------------------------------------------------------------------ inputs
def unet_inputs(B: int, Tlen: int, seed: int = 1):
    g = synth.inputs_rng(seed)
    x = g.standard_normal((B, Tlen, 10), dtype=np.float32)
    cond = g.standard_normal((B, 256), dtype=np.float32)
    return T(x), T(cond)


def si_inputs(B: int, Tlen: int, steps: int = 10, seed: int = 2):
    g = synth.inputs_rng(seed)
    x0 = g.uniform(-1, 1, (B, Tlen, 10)).astype(np.float32)
    cond = g.standard_normal((B, 256), dtype=np.float32)
    z = g.standard_normal((steps, B, Tlen, 10), dtype=np.float32)
    return T(x0), T(cond), T(z)


def frames(B: int, res: int, kind: str, seed: int = 3):
    """kind: 'bright' (mean≈0.6 -> ImageNet-normalised branch), 'dark' (mean≈0.3 -> skipped),
    'uint8_bhwc' (0..255, BHWC), 'bthwc' (float 5-D [B,1,H,W,3], bright)."""
    g = synth.inputs_rng(seed)
    u = g.random((B, 3, res, res), dtype=np.float32)
    if kind == "bright":
        return T(0.2 + 0.8 * u)
    if kind == "dark":
        return T(0.6 * u)
    if kind == "uint8_bhwc":
        return T((255 * (0.2 + 0.8 * u)).astype(np.uint8).transpose(0, 2, 3, 1))
    if kind == "bthwc":
        return T((0.2 + 0.8 * u).transpose(0, 2, 3, 1)[:, None])
    raise ValueError(kind)


def predict_inputs(B: int, Tlen: int, res: int, seed: int = 4):
    g = synth.inputs_rng(seed)
    state = g.standard_normal((B, 10), dtype=np.float32)
    forces = g.standard_normal((B, 3), dtype=np.float32)
    vla = g.uniform(0, 1, (B, Tlen, 10)).astype(np.float32)
    cam1 = 0.2 + 0.8 * g.random((B, 3, res, res), dtype=np.float32)
    cam2 = 0.6 * g.random((B, 3, res, res), dtype=np.float32)         # second camera takes the 'dark' branch
    z = g.standard_normal((10, B, Tlen, 10), dtype=np.float32)
    return dict(state=T(state), forces=T(forces), vla=T(vla), cam1=T(cam1), cam2=T(cam2), z=T(z))


def synth_episode(seed: int, N: int, res: int = 28) -> Dict[str, np.ndarray]:
    """A synthetic episode in the reference's on-disk key layout (4_convert_to_hdf5.py; NPZ container, '/' for groups):
    the first 4 frames are static (exercises the first-motion trim), then a smooth pose walk."""
    g = synth.inputs_rng(seed)
    pos = np.zeros((N, 3))
    pos[4:] = np.cumsum(g.normal(0, 0.02, (N - 4, 3)), axis=0)
    pos += g.normal(0, 0.3, (1, 3))
    ang = np.zeros((N, 3))
    ang[4:] = np.cumsum(g.normal(0, 0.03, (N - 4, 3)), axis=0)
    half = ang / 2
    quat = np.stack([np.sin(half[:, 0]), np.sin(half[:, 1]) * 0.5, np.sin(half[:, 2]) * 0.25,
                     np.cos(half[:, 0])], axis=1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    grip = np.clip(128 + np.cumsum(g.normal(0, 6, N)), 0, 255)
    expert = None
    vla = g.normal(0, 0.2, (N, 64, 10))
    vla[:, :, :3] += pos[:, None, :]
    vla[:, :, -1] = np.clip(grip[:, None] + g.normal(0, 10, (N, 64)), 0, 255)
    return {
        "ee_poses": np.concatenate([pos, quat], axis=1).astype(np.float64),
        "gripper_pos": grip.astype(np.float64),
        "vla_action": vla.astype(np.float64),
        "gelsight_force/forces": g.normal(0, 1, (N, 3)).astype(np.float64),
        "gelsight_force/displacement": g.normal(0, 1, (N, 63, 2)).astype(np.float32),
        "camera1_resized": (255 * (0.2 + 0.8 * g.random((N, res, res, 3)))).astype(np.uint8),
        "camera2_resized": (255 * (0.6 * g.random((N, res, res, 3)))).astype(np.uint8),
    }


def lstm_inputs(B: int, Tlen: int, seed: int = 5, hidden: int = 256):
    g = synth.inputs_rng(seed)
    return dict(obs_cond=T(g.standard_normal((B, hidden), dtype=np.float32)),
                vla=T(g.uniform(0, 1, (B, Tlen, 10)).astype(np.float32)),
                forces=T(g.standard_normal((B, Tlen, 3), dtype=np.float32)))


def vt_kpos() -> torch.Tensor:
    """Position of key kk (0..63) inside a Vt row of the cached-condition tile stream (csrc/vt_kernels.h, vt_kpos)."""
    kk = torch.arange(64)
    return (kk & 32) | (((kk >> 2) & 3) << 3) | (((kk >> 4) & 1) << 2) | (kk & 3)


def kv_tile_stream(k: torch.Tensor, v: torch.Tensor, T: int, fill: float = 0.0) -> torch.Tensor:
    """The cached-condition tile stream of csrc/vt_attn_kvt.hip built in torch from row-major k, v [M, H, 64]: [H, T, 2, 64, 64] where
    tile(h, t) = [K: 64 rows x 64 d][Vt: 64 d x 64 rows, row kk at column vt_kpos(kk)] over the rows m = t * 64 + r; rows >= M hold `fill`."""
    M, H, D = k.shape
    assert v.shape == k.shape and D == 64 and T * 64 >= M
    pk = torch.full((T * 64, H, 64), fill, dtype=k.dtype, device=k.device)
    pv = torch.full((T * 64, H, 64), fill, dtype=v.dtype, device=v.device)
    pk[:M], pv[:M] = k, v
    kt = pk.reshape(T, 64, H, 64).permute(2, 0, 1, 3)                # [h, t, r, d]
    vt = torch.empty(H, T, 64, 64, dtype=v.dtype, device=v.device)  # [h, t, d, position]
    vt[..., vt_kpos().to(v.device)] = pv.reshape(T, 64, H, 64).permute(2, 0, 3, 1)
    return torch.stack([kt, vt], dim=2).contiguous()


def rdt_inputs(cfg: dict, B: int, lang_len: int, seed: int = 6, dtype=torch.float32):
    g = synth.inputs_rng(seed)
    D = cfg["hidden"]
    mask = np.ones((B, lang_len), dtype=bool)
    mask[0, lang_len - 3:] = False                                          # padded language tokens
    amask = np.zeros((B, 1, cfg["action_dim"]), dtype=np.float32)
    amask[:, :, :10] = 1.0
    d = dict(
        x=T(g.standard_normal((B, cfg["horizon"] + 1, D), dtype=np.float32)),
        lang_c=T(g.standard_normal((B, lang_len, D), dtype=np.float32)),
        img_c=T(g.standard_normal((B, cfg["img_cond_len"], D), dtype=np.float32)),
        lang_tokens=T(g.standard_normal((B, lang_len, cfg["lang_token_dim"]), dtype=np.float32)),
        img_tokens=T(g.standard_normal((B, cfg["img_cond_len"], cfg["img_token_dim"]), dtype=np.float32)),
        state_tokens=T(g.standard_normal((B, 1, cfg["state_token_dim"]), dtype=np.float32)),
        x_init=T(g.standard_normal((B, cfg["horizon"], cfg["action_dim"]), dtype=np.float32)),
        action_mask=T(amask),
    )
    d = {k: v.to(dtype) for k, v in d.items()}
    d["lang_mask"] = T(mask)
    d["freq"] = torch.full((B,), 10.0)
    d["t"] = torch.tensor([437])
    return d
