#!/usr/bin/env python
"""The reference's JPEG round trip of camera frames (vlatouch/jpegmap.py): Pillow on the host against csrc/vt_jpegmap.hip on one MI355X,
for the robot step's 6 frames of 480 x 640 (three smooth, three noise: libjpeg's time depends on the content, the kernel's does not).
  * `pillow_roundtrip_6_ms`: `jpeg_mapping` of the 6 frames, per content kind as well;
  * `vt_jpegmap_6_ms`: the C call alone on device-resident frames with a prepared table, back to back between two events, and
    `jpeg_mapping_device` as a caller sees it (table upload included, ending in a synchronise);
  * `preprocess_6`: `preprocess_images_device` (384 x 384 tower, bf16, pad + brightness check) without and with `jpeg=95`, from
    device-resident frames (events, back to back) and from host arrays (host clock, the copy included), and the CPU statement
    (Pillow mapping + `preprocess_images` + copy);
  * `step_b1`: `step()` at batch 1 from PIL frames (so400m tower + RDT-1B, synthetic weights) with `jpeg_mapping` off, on the device, with
    the mapping on the CPU in front of the device preprocessing, and with `device_preprocess=False` (mapping and preprocessing on the CPU).
Variants alternate inside every repeat, in this one process; medians over the repeats with min and max.  A machine without a GPU fails:
nothing here is measured on a CPU.  One JSON line.

    timeout -k 10 900 python tools/jpegmap_bench.py [--iters 20] [--repeats 7] [--no-step] > profiles/jpegmap_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vla-touch_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.preprocess_bench import ARGS, DEV  # noqa: E402


def host_once(fn, iters):
    """ms per call by the host clock, over `iters` calls that end in one synchronise each."""
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def event_once(fn, iters):
    """ms per call of `iters` back-to-back calls between two events: kernel time plus launch gaps."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, repeats, measure):
    """{name: fn} -> {name: {median, min, max}} of `measure(fn)`, the variants taking turns inside every repeat (after one warm-up each)."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ts[k].append(measure(fn))
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ts.items()}


def frames_6():
    g = np.random.default_rng(0)
    y, x = np.mgrid[0:480, 0:640]
    smooth = [np.clip(np.stack([(y * (0.3 + 0.1 * k) + x * 0.2), (x * 0.35 + 20 * k), (255 - y * 0.4 - x * 0.1)], axis=-1) + g.normal(0, 1.5, (480, 640, 3)),
                      0, 255).astype(np.uint8) for k in range(3)]
    noise = [g.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(3)]
    return smooth, noise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the step() comparison (it builds the so400m tower and RDT-1B)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpegmap_bench: needs an MI355X (nothing here is measured on a CPU)")
    import types
    import PIL
    from PIL import Image, features
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    from vlatouch import _lib
    from vlatouch.jpegmap import jpeg_mapped_pil, jpeg_mapping, jpeg_mapping_device, jpeg_table
    torch.set_grad_enabled(False)
    res = {"workload": "jpeg_round_trip_of_camera_frames", "frames": 6, "frame": [480, 640], "quality": 95, "order": "cv2", "pillow": PIL.__version__,
           "libjpeg_turbo": str(features.version("jpg")), "cpus": len(os.sched_getaffinity(0)), "iters": a.iters, "repeats": a.repeats,
           "cv2": "UNPINNED: not installed; the mapping is pinned to Pillow's libjpeg-turbo with the channel roles swapped"}
    smooth, noise = frames_6()
    arrs = smooth + noise
    dev = [torch.from_numpy(x).to(DEV) for x in arrs]

    # ---- the mapping alone
    items = [(t.data_ptr(), 480, 640, 3 * 640) for t in dev]
    arr, out_bytes, ws_bytes = jpeg_table(items)
    table = torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(DEV)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    L, st = _lib.lib(), _lib.stream_ptr(DEV)

    def c_call():
        _lib.check(L.vt_jpegmap(arr, _lib.ptr(table), 6, 95, _lib.JPEGMAP_CV2_ORDER, _lib.ptr(out), _lib.ptr(ws), ws_bytes, st), "vt_jpegmap")
    want = [jpeg_mapping(x) for x in arrs]
    got = jpeg_mapping_device(dev, out=out, workspace=ws)
    res["bit_identical_to_pillow"] = bool(all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(got, want)))
    res["changed_pixels_pct"] = {k: round(100 * float(np.mean([(w != x).any(axis=-1).mean() for w, x in zip(ws_, xs)])), 1)
                                 for k, ws_, xs in (("smooth", want[:3], smooth), ("noise", want[3:], noise))}
    res["pillow_roundtrip_6_ms"] = alternate({"all_6": lambda: [jpeg_mapping(x) for x in arrs], "smooth_3": lambda: [jpeg_mapping(x) for x in smooth],
                                              "noise_3": lambda: [jpeg_mapping(x) for x in noise]}, a.repeats, lambda fn: host_once(fn, max(3, a.iters // 4)))
    res["vt_jpegmap_6_ms"] = {
        "c_call_back_to_back": alternate({"v": c_call}, a.repeats, lambda fn: event_once(fn, 10 * a.iters))["v"],
        "jpeg_mapping_device_from_device_frames": alternate({"v": lambda: jpeg_mapping_device(dev, out=out, workspace=ws)}, a.repeats,
                                                            lambda fn: host_once(fn, a.iters))["v"],
        "jpeg_mapping_device_from_host_arrays": alternate({"v": lambda: jpeg_mapping_device(arrs, out=out, workspace=ws)}, a.repeats,
                                                          lambda fn: host_once(fn, a.iters))["v"],
        "bytes_moved": 6 * 480 * 640 * (3 + 1.5 + 1.5 + 3)}
    print("mapping", res["pillow_roundtrip_6_ms"], res["vt_jpegmap_6_ms"], file=sys.stderr, flush=True)

    # ---- in front of the SigLIP preprocessing
    vis = types.SimpleNamespace(config=types.SimpleNamespace(image_size=384), num_patches=729, hidden_size=1152, eval=lambda: None)
    pol = types.SimpleNamespace(eval=lambda: None)
    m = RoboticDiffusionTransformerModel(ARGS, device=DEV, dtype=torch.bfloat16, vision_model=vis, policy=pol)
    px = torch.empty(6, 3, 384, 384, dtype=torch.bfloat16, device=DEV)
    pil = [Image.fromarray(x) for x in arrs]
    cpu_statement = lambda: m.preprocess_images(jpeg_mapped_pil(pil, 95)).to(DEV, dtype=torch.bfloat16)      # noqa: E731
    same = bool(torch.equal(m.preprocess_images_device(dev, jpeg=95), cpu_statement()) and
                torch.equal(m.preprocess_images_device(arrs, jpeg=95), m.preprocess_images_device(want)))
    res["preprocess_6"] = {
        "bit_identical": same,
        "device_frames_back_to_back_ms": alternate({"plain": lambda: m.preprocess_images_device(dev, out=px),
                                                    "jpeg_95": lambda: m.preprocess_images_device(dev, out=px, jpeg=95)}, a.repeats,
                                                   lambda fn: event_once(fn, 10 * a.iters)),
        "from_host_arrays_ms": alternate({"plain": lambda: m.preprocess_images_device(arrs, out=px),
                                          "jpeg_95": lambda: m.preprocess_images_device(arrs, out=px, jpeg=95),
                                          "pillow_mapping_then_device": lambda: m.preprocess_images_device([jpeg_mapping(x) for x in arrs], out=px)},
                                         a.repeats, lambda fn: host_once(fn, max(3, a.iters // 2))),
        "cpu_statement_ms": alternate({"v": cpu_statement}, max(3, a.repeats // 2), lambda fn: host_once(fn, 3))["v"]}
    print("preprocess", res["preprocess_6"], file=sys.stderr, flush=True)

    if not a.no_step:
        from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
        from models.rdt_runner import RDTRunner
        from vlatouch import synth
        c = synth.SIGLIP_CONFIGS["so400m"]
        cfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                   image_size=c["image_size"], patch_size=14)
        ssd = synth.fill_state_dict_device(synth.siglip_shapes(**c), DEV, torch.float32, seed=9)
        tower = SiglipVisionTower("synthetic", None, device=DEV, precision="bf16", state_dict={k: v.cpu() for k, v in ssd.items()}, config=cfg)
        del ssd
        rcfg = {"rdt": {"hidden_size": 2048, "depth": 28, "num_heads": 32, "rms_norm": "meansq"}, "lang_adaptor": "mlp2x_gelu", "img_adaptor": "mlp2x_gelu",
                "state_adaptor": "mlp3x_gelu",
                "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "beta_schedule": "squaredcos_cap_v2",
                                    "prediction_type": "sample", "clip_sample": False}}
        shapes = dict(hidden=2048, depth=28, heads=32, horizon=64, action_dim=128, lang_token_dim=4096, img_token_dim=1152, state_token_dim=128,
                      max_lang_cond_len=1024, img_cond_len=4374)
        rdt = RDTRunner(action_dim=128, pred_horizon=64, config=rcfg, lang_token_dim=4096, img_token_dim=1152, state_token_dim=128,
                        max_lang_cond_len=1024, img_cond_len=4374, dtype=torch.bfloat16, device=DEV, init_weights=False)
        rdt.load_state_dict(synth.fill_state_dict_device(synth.rdt_runner_shapes(**shapes), DEV, torch.bfloat16, seed=7), assign=True)
        models = {sw: RoboticDiffusionTransformerModel(ARGS, device=DEV, dtype=torch.bfloat16, control_frequency=10, vision_model=tower, policy=rdt,
                                                       device_preprocess=sw) for sw in (False, True)}
        tg = torch.Generator().manual_seed(1)
        proprio, text = torch.randn(1, 10, generator=tg), torch.randn(1, 32, 4096, generator=tg).to(DEV, torch.bfloat16)
        variants = {"jpeg_mapping_off": lambda: models[True].step(proprio, pil, text),
                    "jpeg_mapping_on_device": lambda: models[True].step(proprio, pil, text, jpeg_mapping=True),
                    "pillow_mapping_then_device_preprocess": lambda: models[True].step(proprio, jpeg_mapped_pil(pil, 95), text),
                    "device_preprocess_off_jpeg_mapping_on_cpu": lambda: models[False].step(proprio, pil, text, jpeg_mapping=True)}
        outs = {}
        for k, fn in variants.items():
            torch.manual_seed(5)
            outs[k] = fn()
        stp = alternate(variants, a.repeats, lambda fn: host_once(fn, max(3, a.iters // 4)))
        stp["same_action_chunk_device_and_cpu_mapping"] = bool(torch.equal(outs["jpeg_mapping_on_device"], outs["pillow_mapping_then_device_preprocess"]) and
                                                               torch.equal(outs["jpeg_mapping_on_device"], outs["device_preprocess_off_jpeg_mapping_on_cpu"]))
        stp["mapping_changes_the_chunk"] = not bool(torch.equal(outs["jpeg_mapping_on_device"], outs["jpeg_mapping_off"]))
        stp.update(lang_len=32, rdt_steps=5)
        res["step_b1"] = stp
        print("step", stp, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
