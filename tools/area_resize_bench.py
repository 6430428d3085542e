#!/usr/bin/env python
"""The reference's zero pad + INTER_AREA resize of camera frames (vlatouch.imgprep.pad_and_resize_for_siglip): the numpy statement on the
host against csrc/vt_area.hip on one MI355X, for the robot step's 6 frames of 480 x 640 -> 384 x 384.
  * `statement_6_ms`: `pad_and_resize_for_siglip` of the 6 frames (cv2 is not installed: this is the numpy restatement, not cv2's own time);
  * `vt_area_resize_6_ms`: the C call alone on device-resident frames with a prepared table, back to back between two events, and
    `pad_and_resize_device` as a caller sees it (table upload included, ending in a synchronise), from device frames and from host arrays;
  * `preprocess_6`: `preprocess_images_device` (384 x 384 tower, bf16, pad + brightness check) from host arrays without `area`, with
    `area=384` and with `area=384, jpeg=95` (host clock, the copy included), and from device-resident frames (events, back to back);
  * `step_b1`: `step()` at batch 1 from PIL frames (so400m tower + RDT-1B, synthetic weights) with `pad_and_resize` on the device, through
    the CPU statement in front of the device preprocessing, with `device_preprocess=False`, and off;
  * `store`: tools/rdt_data_bench.py's synthetic store (`--episodes` episodes of `--steps` steps, two 480 x 640 cameras) without and with
    `pad_and_resize=384`: resident bytes, read-and-prepare and upload times (one run each: a load is not repeated).
Variants alternate inside every repeat, in this one process; medians over the repeats with min and max.  A machine without a GPU fails:
nothing here is measured on a CPU.  One JSON line.

    timeout -k 10 900 python tools/area_resize_bench.py [--iters 20] [--repeats 7] [--no-step] [--no-store] > profiles/area_resize_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vla-touch_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.jpegmap_bench import alternate, event_once, frames_6, host_once  # noqa: E402
from tools.preprocess_bench import ARGS, DEV  # noqa: E402

T = 384


def store_load(a, pad_and_resize):
    from tests import rdt_data_ref as R
    from vlatouch.rdt_data import EpisodeStore
    tmp = tempfile.mkdtemp(prefix="area_resize_bench_")
    try:
        from tools.rdt_data_bench import write_episodes
        write_episodes(tmp, a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = EpisodeStore(tmp, dataset_name=R.DATASET_NAME, dataset_names=R.DATASET_NAMES, control_freq=R.CONTROL_FREQ, device=DEV,
                             pad_and_resize=pad_and_resize)
        t1 = time.perf_counter()
        store.upload()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return {"read_and_prepare_s": round(t1 - t0, 3), "upload_s": round(t2 - t1, 3), "resident_bytes": store.resident_bytes,
                "host_frame_bytes": store.host_frame_bytes, "kept_episodes": len(store.episodes)}
    finally:
        shutil.rmtree(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the step() comparison (it builds the so400m tower and RDT-1B)")
    ap.add_argument("--no-store", action="store_true", help="skip the episode store (it writes and reads the synthetic episodes)")
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    a.height, a.width, a.lang_len, a.lang_dim = 480, 640, 32, 4096           # tools/rdt_data_bench.py's episode
    if not torch.cuda.is_available():
        raise SystemExit("area_resize_bench: needs an MI355X (nothing here is measured on a CPU)")
    import types
    from PIL import Image
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    from vlatouch import _lib
    from vlatouch.imgprep import area_table, pad_and_resize_device, pad_and_resize_for_siglip, pad_and_resize_pil
    torch.set_grad_enabled(False)
    res = {"workload": "zero_pad_and_area_resize_of_camera_frames", "frames": 6, "frame": [480, 640], "target": T, "cpus": len(os.sched_getaffinity(0)),
           "iters": a.iters, "repeats": a.repeats, "cv2": "UNPINNED: not installed; the statement is restated from OpenCV's resize.cpp"}
    smooth, noise = frames_6()
    arrs = smooth + noise
    dev = [torch.from_numpy(x).to(DEV) for x in arrs]

    # ---- the stage alone
    arr, out_bytes, taps = area_table([(t.data_ptr(), 480, 640, 3 * 640) for t in dev], T)
    table = torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(DEV)
    tabs = torch.from_numpy(taps).to(DEV)
    out = torch.empty((6, T, T, 3), dtype=torch.uint8, device=DEV)
    L, st = _lib.lib(), _lib.stream_ptr(DEV)

    def c_call():
        _lib.check(L.vt_area_resize(arr, _lib.ptr(table), 6, _lib.ptr(out), _lib.ptr(tabs), taps.size, st), "vt_area_resize")
    want = pad_and_resize_for_siglip(np.stack(arrs), T)
    res["bit_identical_to_the_statement"] = bool(np.array_equal(pad_and_resize_device(dev, T, out=out).cpu().numpy(), want))
    res["taps_per_output"] = int(arr[0].ntaps)
    res["statement_6_ms"] = alternate({"v": lambda: pad_and_resize_for_siglip(np.stack(arrs), T)}, a.repeats, lambda fn: host_once(fn, max(3, a.iters // 4)))["v"]
    res["vt_area_resize_6_ms"] = {
        "c_call_back_to_back": alternate({"v": c_call}, a.repeats, lambda fn: event_once(fn, 10 * a.iters))["v"],
        "pad_and_resize_device_from_device_frames": alternate({"v": lambda: pad_and_resize_device(dev, T, out=out)}, a.repeats,
                                                              lambda fn: host_once(fn, a.iters))["v"],
        "pad_and_resize_device_from_host_arrays": alternate({"v": lambda: pad_and_resize_device(arrs, T, out=out)}, a.repeats,
                                                            lambda fn: host_once(fn, a.iters))["v"],
        "bytes_read_at_most": 6 * 480 * 640 * 3, "bytes_written": 6 * T * T * 3}
    print("stage", res["statement_6_ms"], res["vt_area_resize_6_ms"], file=sys.stderr, flush=True)

    # ---- in front of the SigLIP preprocessing
    vis = types.SimpleNamespace(config=types.SimpleNamespace(image_size=384), num_patches=729, hidden_size=1152, eval=lambda: None)
    pol = types.SimpleNamespace(eval=lambda: None)
    m = RoboticDiffusionTransformerModel(ARGS, device=DEV, dtype=torch.bfloat16, vision_model=vis, policy=pol)
    px = torch.empty(6, 3, 384, 384, dtype=torch.bfloat16, device=DEV)
    pil = [Image.fromarray(x) for x in arrs]
    same = bool(torch.equal(m.preprocess_images_device(arrs, area=T), m.preprocess_images(pad_and_resize_pil(pil, T)).to(DEV, dtype=torch.bfloat16)) and
                torch.equal(m.preprocess_images_device(dev, area=T, jpeg=95), m.preprocess_images_device(list(want), jpeg=95)))
    res["preprocess_6"] = {
        "bit_identical": same,
        "from_host_arrays_ms": alternate({"plain": lambda: m.preprocess_images_device(arrs, out=px),
                                          "area_384": lambda: m.preprocess_images_device(arrs, out=px, area=T),
                                          "area_384_jpeg_95": lambda: m.preprocess_images_device(arrs, out=px, area=T, jpeg=95),
                                          "jpeg_95": lambda: m.preprocess_images_device(arrs, out=px, jpeg=95),
                                          "statement_then_device": lambda: m.preprocess_images_device(list(pad_and_resize_for_siglip(np.stack(arrs), T)), out=px)},
                                         a.repeats, lambda fn: host_once(fn, max(3, a.iters // 2))),
        "device_frames_back_to_back_ms": alternate({"plain": lambda: m.preprocess_images_device(dev, out=px),
                                                    "area_384": lambda: m.preprocess_images_device(dev, out=px, area=T),
                                                    "area_384_jpeg_95": lambda: m.preprocess_images_device(dev, out=px, area=T, jpeg=95),
                                                    "jpeg_95": lambda: m.preprocess_images_device(dev, out=px, jpeg=95)}, a.repeats,
                                                   lambda fn: event_once(fn, 10 * a.iters))}
    print("preprocess", res["preprocess_6"], file=sys.stderr, flush=True)

    if not a.no_store:
        res["store"] = {"episodes": a.episodes, "steps": a.steps, "cameras": 2, "raw": store_load(a, None)}
        print("store raw", res["store"]["raw"], file=sys.stderr, flush=True)
        res["store"]["pad_and_resize_384"] = store_load(a, T)
        res["store"]["frame_bytes_ratio"] = round(480 * 640 / (T * T), 4)
        print("store resized", res["store"]["pad_and_resize_384"], file=sys.stderr, flush=True)

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
        variants = {"pad_and_resize_off": lambda: models[True].step(proprio, pil, text),
                    "pad_and_resize_on_device": lambda: models[True].step(proprio, pil, text, pad_and_resize=True),
                    "statement_then_device_preprocess": lambda: models[True].step(proprio, pad_and_resize_pil(pil, T), text),
                    "device_preprocess_off_statement_on_cpu": lambda: models[False].step(proprio, pil, text, pad_and_resize=True)}
        outs = {}
        for k, fn in variants.items():
            torch.manual_seed(5)
            outs[k] = fn()
        stp = alternate(variants, a.repeats, lambda fn: host_once(fn, max(3, a.iters // 4)))
        stp["same_action_chunk_device_and_cpu_statement"] = bool(torch.equal(outs["pad_and_resize_on_device"], outs["statement_then_device_preprocess"]) and
                                                                 torch.equal(outs["pad_and_resize_on_device"], outs["device_preprocess_off_statement_on_cpu"]))
        stp["resize_changes_the_chunk"] = not bool(torch.equal(outs["pad_and_resize_on_device"], outs["pad_and_resize_off"]))
        stp.update(lang_len=32, rdt_steps=5)
        res["step_b1"] = stp
        print("step", stp, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
