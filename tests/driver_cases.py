"""What the engines' host drivers (csrc/vt_unet.hip, vt_unet_fused.hip, vt_models.hip, vt_t5.hip, vt_lstm.hip, vt_rdt.hip) enqueue, as sha256
digests of the outputs: every engine at the smallest shapes that take each branch of its driver, through the engines' public surface only, so
that the same file runs on any version of the drivers.  tests/golden/g24_drivers_parent.json holds what the commit BEFORE the drivers' shared
host idioms (element size of a dtype code, the zeroed Linear parameter block, the workspace carver, the `create` preamble) moved into
csrc/vt_host.h gave on an MI355X (tools/make_golden_drivers_parent.py wrote it); tests/test_gpu_drivers_parent.py recomputes them.  That
refactor moved host code only, so every bit must be where it was.

Weights and inputs are tests/cases.py's.  One group per engine and configuration (`GROUPS`); a group builds its engine once:
  unet/<prec>       si_net_sd (v_net | s_net): fp32 and bf16_plain run the launch-per-op driver; bf16 (split-bf16 on fp32 storage) the fused one,
                    and at B = 1, T = 68 the launch-per-op driver again (the fused plan stops at 64 ticks).  forward with a scalar and with
                    per-sample times, a 2-step sample with injected noise (final state and trajectory), B = 2, T = 16
  dino/small/<prec> two cameras, B = 2, 28 px: uint8 NHWC (bright) and fp32 NCHW (bright | dark)
  dino/base/bf16    one camera, B = 1, 28 px: 5 token rows, so fc1 runs on the fragment-packed copy (vt_dino_packed_bytes > 0 is asserted)
  siglip/tiny/<prec> B = 2 at the position table's 56 px
  t5/tiny/<prec>    B = 2, L = 5, the second row padded after 3 tokens
  lstm/h256         one step and a 4-tick sequence, B = 3
  rdt/tiny/<dtype>/<rms> forward and a 2-step sample, B = 2, 12 language tokens, sample 0's last three padded (cases.rdt_inputs)
  rdt/wide/bf16     hidden 2048, packed weights.  B = 1: small-M tile and the split path; B = 8: register-staged generic tile; B = 32: the
                    weights-in-registers tile and the RMSNorm hand-off.  The route of the block's fc1 is asserted for each (`WIDE_ROUTES`)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from tests import cases
from tests.train16_cases import digest

GOLDEN_NAME = "g24_drivers_parent.json"
WIDE_ROUTES = OrderedDict([(1, "PWS"), (8, "REG"), (32, "PW")])       # batch -> kernel of a per-step Linear (fc1) on 67 * batch rows
LANG_LEN = 12


def _split_nets(sd, nets=("v_net", "s_net")):
    return [{k[len(n) + 1:]: v for k, v in sd.items() if k.startswith(n + ".")} for n in nets]


def _unet(out, key, dev, prec) -> None:
    from vlatouch.engine import UNetEngine
    eng = UNetEngine(_split_nets(cases.si_net_sd("")), precision=prec, device=dev)
    shapes = [(2, 16)] + ([(1, 68)] if prec == "bf16" else [])
    for B, T in shapes:
        x, cond = cases.unet_inputs(B, T)
        out[f"{key}/B{B}_T{T}/forward_scalar_t"] = digest(eng.forward(x, 0.3, cond))
        out[f"{key}/B{B}_T{T}/forward_sample_t"] = digest(eng.forward(x, torch.linspace(0.1, 0.9, B), cond))
        x0, c2, z = cases.si_inputs(B, T, steps=2)
        xT, traj = eng.sample(x0, c2, z, 2, 0.03, record=True)
        out[f"{key}/B{B}_T{T}/sample_xT"], out[f"{key}/B{B}_T{T}/sample_traj"] = digest(xT), digest(traj)


def _dino(out, key, dev, size, heads, prec) -> None:
    from vlatouch import _lib as L
    from vlatouch.engine import DinoEngine
    eng = DinoEngine(cases.dino_sd(size), heads=heads, precision=prec, device=dev)
    if size == "base":
        assert L.lib().vt_dino_packed_bytes(eng._h) > 0
        out[f"{key}/B1_fp32_nchw"] = digest(eng.forward([cases.frames(1, 28, "bright")], nhwc=False))
        return
    u8 = cases.frames(2, 28, "uint8_bhwc")
    out[f"{key}/B2_u8_nhwc"] = digest(eng.forward([u8, u8.flip(0)], nhwc=True))
    out[f"{key}/B2_fp32_nchw"] = digest(eng.forward([cases.frames(2, 28, "bright"), cases.frames(2, 28, "dark")], nhwc=False))


def _siglip(out, key, dev, prec) -> None:
    from vlatouch.engine import SiglipEngine
    from vlatouch import synth
    c = synth.SIGLIP_CONFIGS["tiny"]
    eng = SiglipEngine(cases.siglip_sd("tiny"), heads=c["heads"], precision=prec, device=dev)
    out[f"{key}/B2"] = digest(eng.forward(cases.siglip_pixels(2, c["image_size"])))


def _t5(out, key, dev, prec) -> None:
    from tests import t5_ref
    from vlatouch import synth
    from vlatouch import t5 as T5
    cfg = synth.t5_config("tiny")
    eng = T5.T5Engine(t5_ref.t5_sd("tiny"), cfg, precision=prec, device=dev)
    ids = torch.from_numpy(synth.inputs_rng(9).integers(0, cfg["vocab_size"], (2, 5)).astype(np.int64))
    mask = torch.ones(2, 5, dtype=torch.long)
    mask[1, 3:] = 0
    out[f"{key}/B2_L5_masked"] = digest(eng.forward(ids, mask))


def _lstm(out, key, dev) -> None:
    from vlatouch.engine import LstmEngine
    mods = cases.lstm_mods(hidden=256)
    eng = LstmEngine({k: mods[k] for k in ("force_encoder", "lstm", "output_head")}, hidden=256, precision="fp32", device=dev)
    li = cases.lstm_inputs(3, 4)
    h, c = torch.zeros(2, 3, 256, device=dev), torch.zeros(2, 3, 256, device=dev)
    out[f"{key}/step"] = digest(eng.step(li["obs_cond"], li["vla"][:, 0], li["forces"][:, 0], h, c))
    out[f"{key}/step_h"], out[f"{key}/step_c"] = digest(h), digest(c)
    out[f"{key}/sequence"] = digest(eng.sequence(li["obs_cond"], li["vla"], li["forces"], h, c))
    out[f"{key}/sequence_h"], out[f"{key}/sequence_c"] = digest(h), digest(c)


def _rdt_calls(out, key, eng, cfg, B) -> None:
    i = cases.rdt_inputs(cfg, B, LANG_LEN)
    out[f"{key}/B{B}/forward"] = digest(eng.forward(i["x"], i["freq"], i["t"], i["lang_c"], i["img_c"], i["lang_mask"]))
    out[f"{key}/B{B}/sample"] = digest(eng.sample(i["lang_tokens"], i["lang_mask"], i["img_tokens"], i["state_tokens"], i["action_mask"], i["freq"],
                                                  i["x_init"], num_inference_steps=2, return_fp32=True))


def _rdt_tiny(out, key, dev, dtype, rms) -> None:
    from vlatouch.rdt_engine import RdtEngine
    cfg = cases.RDT_TINY
    eng = RdtEngine(cases.rdt_sd(cfg), dtype=dtype, rms_mode=rms, device=dev, **cfg)
    _rdt_calls(out, key, eng, cfg, 2)


def _wide_route(B: int) -> str:
    """The kernel the router gives a block's fc1 on 67 * B rows, filled as the driver fills it (bf16, tanh-GELU, packed copy present)."""
    from vlatouch import _lib as L
    D = cases.RDT_WIDE["hidden"]
    p = L.GemmParams()
    p.A = p.W = p.C = p.Wp = p.bias = 4096
    p.M, p.N, p.K = (cases.RDT_WIDE["horizon"] + 3) * B, D, D
    p.lda = p.ldw = p.ldc = D
    p.groups = p.splitk = 1
    p.a_dtype = p.w_dtype = p.c_dtype = L.BF16
    p.act = L.ACT_GELU_TANH
    return L.ROUTE_NAMES[L.lib().vt_gemm_route_of(C.addressof(p))]


def _rdt_wide(out, key, dev) -> None:
    from vlatouch import _lib as L
    from vlatouch.rdt_engine import RdtEngine
    cfg = cases.RDT_WIDE
    eng = RdtEngine(cases.rdt_sd(cfg), dtype=torch.bfloat16, device=dev, **cfg)
    assert L.lib().vt_rdt_packed_bytes(eng._h) > 0
    for B, route in WIDE_ROUTES.items():
        assert _wide_route(B) == route, (B, _wide_route(B), route)
        _rdt_calls(out, key, eng, cfg, B)


GROUPS = OrderedDict()
for _p in ("fp32", "bf16_plain", "bf16"):
    GROUPS[f"unet/{_p}"] = (_unet, (_p,))
for _p in ("fp32", "bf16", "fp16"):
    GROUPS[f"dino/small/{_p}"] = (_dino, ("small", 6, _p))
GROUPS["dino/base/bf16"] = (_dino, ("base", 12, "bf16"))
for _p in ("fp32", "bf16"):
    GROUPS[f"siglip/tiny/{_p}"] = (_siglip, (_p,))
for _p in ("fp32", "bf16"):
    GROUPS[f"t5/tiny/{_p}"] = (_t5, (_p,))
GROUPS["lstm/h256"] = (_lstm, ())
for _n, _d in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
    for _r in ("meansq", "var"):
        GROUPS[f"rdt/tiny/{_n}/{_r}"] = (_rdt_tiny, (_d, _r))
GROUPS["rdt/wide/bf16"] = (_rdt_wide, ())


def driver_cases(dev, groups=None) -> "OrderedDict[str, str]":
    out = OrderedDict()
    with torch.no_grad():
        for key in (groups or GROUPS):
            fn, args = GROUPS[key]
            fn(out, key, dev, *args)
            torch.cuda.synchronize(dev)
    return out
