#!/usr/bin/env python
"""Camera frames -> SigLIP pixel_values: the PIL path of `preprocess_images` against the device path (csrc/vt_imgprep.hip) on one
MI355X host, for (a) the robot step's 6 frames of 480 x 640 and (b) a labelling batch of 48 such frames (384 x 384 tower, bf16,
pad + brightness check on).  Per case: the CPU path's ms per call (PIL + the host-to-device copy, ending in a synchronise), the device
path from host frames (one copy of raw bytes included, ending in a synchronise), the device path from device-resident frames
(back-to-back calls between two events: kernel time plus launch gaps) and its bytes moved against the 6.3 TB/s copy ceiling.
Then the training-time colour jitter (`--image_aug`, tests/imgaug_ref.py / csrc/vt_colorjitter.hip) on the 6 frames, every frame jittered with all
four operations: the PIL chain followed by `preprocess_images` against one `DevicePreprocessor` call with `jitter=`, beside the unjittered
device call of the same run (key `c_jitter_6`).
Then the training-time corruption (tests/corrupt_ref.py / csrc/vt_corrupt.hip) on the 6 frames, every frame corrupted, the two costliest
blurs (median k = 11, motion k = 37) among them: one `DevicePreprocessor` call with `corrupt=` beside the call without it, alternated (key
`d_corrupt_6`), `vt_corrupt` alone on device frames back to back, and the numpy statement once, for scale.
Then `step()` at batch 1 from PIL frames (so400m tower + RDT-1B, synthetic weights) with `device_preprocess` off and on, alternated in
this process, with the spread of the repeats.  A machine without a GPU fails: nothing here is measured on a CPU.  One JSON line.

    timeout -k 10 900 python tools/preprocess_bench.py [--iters 20] [--repeats 7] [--no-step] > profiles/preprocess_bench.json
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

DEV = "cuda:0"
COPY_BW = 6.3e12
ARGS = {"common": {"img_history_size": 2, "num_cameras": 3, "state_dim": 128, "action_chunk_size": 64},
        "model": {"lang_token_dim": 4096, "img_token_dim": 1152, "state_token_dim": 128},
        "dataset": {"tokenizer_max_length": 1024, "image_aspect_ratio": "pad", "auto_adjust_image_brightness": True}}


def host_ms(fn, iters, warmup=2):
    """Host clock around calls that each end in a device synchronise: (median, min, max) ms."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def event_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="alternated off / on repeats of step()")
    ap.add_argument("--no-plain", action="store_true", help="skip the two plain legs (a, b)")
    ap.add_argument("--no-jitter", action="store_true", help="skip the colour-jitter leg")
    ap.add_argument("--no-corrupt", action="store_true", help="skip the corruption leg")
    ap.add_argument("--no-step", action="store_true", help="skip the step() comparison (it builds the so400m tower and RDT-1B)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: needs an MI355X (nothing here is measured on a CPU)")
    import types
    import PIL
    from PIL import Image
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    torch.set_grad_enabled(False)
    res = {"workload": "siglip_frame_preprocess", "tower_image_size": 384, "dtype": "bf16", "frame": [480, 640], "pillow": PIL.__version__,
           "cpus": len(os.sched_getaffinity(0)), "torch_threads": torch.get_num_threads()}
    vis = types.SimpleNamespace(config=types.SimpleNamespace(image_size=384), num_patches=729, hidden_size=1152, eval=lambda: None)
    pol = types.SimpleNamespace(eval=lambda: None)
    m = RoboticDiffusionTransformerModel(ARGS, device=DEV, dtype=torch.bfloat16, vision_model=vis, policy=pol)
    g = np.random.default_rng(0)
    for tag, n in () if a.no_plain else (("a_robot_step_6", 6), ("b_labelling_48", 48)):
        arrs = [(g.random((480, 640, 3)) * 256 * (0.2 if i % 5 == 4 else 1.0)).astype(np.uint8) for i in range(n)]       # every fifth frame is dark
        pil = [Image.fromarray(x) for x in arrs]
        dev = [torch.from_numpy(x).to(DEV) for x in arrs]
        out = torch.empty(n, 3, 384, 384, dtype=torch.bfloat16, device=DEV)
        want = m.preprocess_images(pil).to(DEV, torch.bfloat16)
        same = bool(torch.equal(m.preprocess_images_device(arrs), want) and torch.equal(m.preprocess_images_device(dev, out=out), want))
        it_cpu = max(3, a.iters // (4 if n > 6 else 1))
        cpu = host_ms(lambda: m.preprocess_images(pil).to(DEV, dtype=torch.bfloat16), it_cpu, warmup=1)
        hostf = host_ms(lambda: m.preprocess_images_device(arrs, out=out), a.iters)
        pilf = host_ms(lambda: m.preprocess_images_device(pil, out=out), a.iters)
        devf = host_ms(lambda: m.preprocess_images_device(dev, out=out), a.iters)
        gpu = event_ms(lambda: m.preprocess_images_device(dev, out=out), 10 * a.iters)
        moved = n * (480 * 640 * 3 + 3 * 384 * 384 * 2)
        r = {"n": n, "bit_identical": same,
             "cpu_path_ms": {"median": cpu[0], "min": cpu[1], "max": cpu[2], "iters": it_cpu},
             "device_path_from_host_arrays_ms": {"median": hostf[0], "min": hostf[1], "max": hostf[2]},
             "device_path_from_pil_ms": {"median": pilf[0], "min": pilf[1], "max": pilf[2]},
             "device_path_from_device_frames_ms": {"median": devf[0], "min": devf[1], "max": devf[2]},
             "device_frames_back_to_back_ms": gpu, "bytes_moved": moved,
             "gb_per_s": round(moved / gpu / 1e6, 1), "pct_of_6p3_tb_s_copy": round(100 * moved / (gpu * 1e-3) / COPY_BW, 2),
             "speedup_vs_cpu_path": round(cpu[0] / hostf[0], 1)}
        res[tag] = r
        print(tag, r, file=sys.stderr, flush=True)
    if not a.no_jitter:
        from tests import imgaug_ref
        from vlatouch.imgaug import color_jitter_params
        n = 6
        arrs = [(g.random((480, 640, 3)) * 256 * (0.2 if i % 5 == 4 else 1.0)).astype(np.uint8) for i in range(n)]
        pil = [Image.fromarray(x) for x in arrs]
        dev = [torch.from_numpy(x).to(DEV) for x in arrs]
        gen = torch.Generator().manual_seed(0)
        jit = [color_jitter_params(generator=gen) for _ in range(n)]          # all four operations on every frame
        out = torch.empty(n, 3, 384, 384, dtype=torch.bfloat16, device=DEV)
        proc = m.image_processor

        def host_chain():
            px = [imgaug_ref.train_image_chain(im, True, p, image_size=None, brightness=True, pad=True, processor=proc) for im, p in zip(pil, jit)]
            return torch.stack(px).to(DEV, dtype=torch.bfloat16)
        want = host_chain()
        same = bool(torch.equal(m.preprocess_images_device(arrs, jitter=jit), want) and torch.equal(m.preprocess_images_device(dev, out=out, jitter=jit), want))
        cpu = host_ms(host_chain, max(3, a.iters // 2), warmup=1)
        hostf = host_ms(lambda: m.preprocess_images_device(arrs, out=out, jitter=jit), a.iters)
        devf = host_ms(lambda: m.preprocess_images_device(dev, out=out, jitter=jit), a.iters)
        plainh = host_ms(lambda: m.preprocess_images_device(arrs, out=out), a.iters)
        plaind = host_ms(lambda: m.preprocess_images_device(dev, out=out), a.iters)
        gpu = event_ms(lambda: m.preprocess_images_device(dev, out=out, jitter=jit), 10 * a.iters)
        gpu_plain = event_ms(lambda: m.preprocess_images_device(dev, out=out), 10 * a.iters)
        r = {"n": n, "operations_per_frame": 4, "bit_identical": same,
             "host_chain_ms": {"median": cpu[0], "min": cpu[1], "max": cpu[2]},
             "device_jitter_from_host_arrays_ms": {"median": hostf[0], "min": hostf[1], "max": hostf[2]},
             "device_jitter_from_device_frames_ms": {"median": devf[0], "min": devf[1], "max": devf[2]},
             "device_unjittered_from_host_arrays_ms": {"median": plainh[0], "min": plainh[1], "max": plainh[2]},
             "device_unjittered_from_device_frames_ms": {"median": plaind[0], "min": plaind[1], "max": plaind[2]},
             "device_frames_back_to_back_ms": {"jitter": gpu, "unjittered": gpu_plain},
             "jitter_over_unjittered_from_host_arrays": round(hostf[0] / plainh[0], 2),
             "speedup_vs_host_chain": round(cpu[0] / hostf[0], 1)}
        res["c_jitter_6"] = r
        print("c_jitter_6", r, file=sys.stderr, flush=True)
    if not a.no_corrupt:
        import ctypes
        from tests import corrupt_ref
        from vlatouch import _lib
        from vlatouch.imgaug import CorruptParams, image_corrupt_device, pack_corrupt
        n = 6
        arrs = [(g.random((480, 640, 3)) * 256).astype(np.uint8) for i in range(n)]      # no dark frame: the lift, which precedes the corruption, stays out
        dev = [torch.from_numpy(x).to(DEV) for x in arrs]
        cor = [CorruptParams(True, "gaussian", 9.0, True, 11, blur="median", k=11),
               CorruptParams(False, "laplace", 6.0, False, 12, blur="motion", k=37, angle=37.0, direction=0.3),
               CorruptParams(True, "poisson", 11.0, True, 13, blur="gaussian", sigma=2.9),
               CorruptParams(False, "gaussian", 4.0, False, 14, blur="average", k=7),
               CorruptParams(True, "laplace", 12.0, True, 15, blur="motion", k=15, angle=200.0, direction=-0.7),
               CorruptParams(True, "poisson", 3.0, False, 16)]
        out = torch.empty(n, 3, 384, 384, dtype=torch.bfloat16, device=DEV)
        t0 = time.perf_counter()
        want = [corrupt_ref.image_corrupt_np(x, p) for x, p in zip(arrs, cor)]
        cpu_once = round((time.perf_counter() - t0) * 1e3, 1)
        got = image_corrupt_device(dev, cor)
        same = all(bool(torch.equal(t.cpu(), torch.from_numpy(w))) for t, w in zip(got, want))
        same = same and bool(torch.equal(m.preprocess_images_device(arrs, corrupt=cor), m.preprocess_images_device(want)))
        with_h, without_h, with_d, without_d = [], [], [], []
        for _ in range(a.repeats):                       # alternated in one process: the host is shared with other work
            without_h.append(host_ms(lambda: m.preprocess_images_device(arrs, out=out), a.iters)[0])
            with_h.append(host_ms(lambda: m.preprocess_images_device(arrs, out=out, corrupt=cor), a.iters)[0])
            without_d.append(host_ms(lambda: m.preprocess_images_device(dev, out=out), a.iters)[0])
            with_d.append(host_ms(lambda: m.preprocess_images_device(dev, out=out, corrupt=cor), a.iters)[0])
        spread = lambda ts: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

        def kernel_ms(idx):
            """vt_corrupt alone on the device frames `idx`, tables uploaded once, back-to-back launches between two events."""
            arr = (_lib.CorruptFrame * len(idx))()
            off = 0
            for f, i in zip(arr, idx):
                f.src, f.pitch, f.h, f.w, f.out_off = dev[i].data_ptr(), 3 * 640, 480, 640, off
                off += 480 * 640 * 3
            words = pack_corrupt(arr, [cor[i] for i in idx])
            fd = torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(DEV)
            td = torch.from_numpy(np.concatenate([words, np.zeros(1, dtype=np.uint32)]).view(np.uint8).copy()).to(DEV)
            buf = torch.empty(off, dtype=torch.uint8, device=DEV)
            L, st = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
            call = lambda: _lib.check(L.vt_corrupt(arr, _lib.ptr(fd), len(idx), ctypes.c_void_p(words.ctypes.data), _lib.ptr(td), words.size,
                                                   _lib.ptr(buf), st), "vt_corrupt")
            return event_ms(call, 10 * a.iters)
        r = {"n": n, "bit_identical": same, "blurs": [p.blur if p.blur != "median" and p.blur != "motion" else f"{p.blur} k={p.k}" for p in cor],
             "repeats": a.repeats,
             "device_corrupt_from_host_arrays_ms": spread(with_h), "device_uncorrupted_from_host_arrays_ms": spread(without_h),
             "device_corrupt_from_device_frames_ms": spread(with_d), "device_uncorrupted_from_device_frames_ms": spread(without_d),
             "corrupt_over_uncorrupted_from_host_arrays": round(statistics.median(with_h) / statistics.median(without_h), 2),
             "vt_corrupt_back_to_back_ms": {"all_6": kernel_ms(range(n)), "median_k11_alone": kernel_ms([0]), "motion_k37_alone": kernel_ms([1]),
                                            "noise_alone": kernel_ms([5])},
             "numpy_statement_once_ms": cpu_once}
        res["d_corrupt_6"] = r
        print("d_corrupt_6", r, file=sys.stderr, flush=True)
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
        arrs = [(g.random((480, 640, 3)) * 256).astype(np.uint8) for _ in range(6)]
        pil = [Image.fromarray(x) for x in arrs]
        tg = torch.Generator().manual_seed(1)
        proprio, text = torch.randn(1, 10, generator=tg), torch.randn(1, 32, 4096, generator=tg).to(DEV, torch.bfloat16)
        outs = {}
        for sw in (False, True):
            torch.manual_seed(5)
            outs[sw] = models[sw].step(proprio, pil, text)
        times = {False: [], True: []}
        for _ in range(a.repeats):                       # alternated in one process: the host is shared with other work
            for sw in (False, True):
                times[sw].append(host_ms(lambda: models[sw].step(proprio, pil, text), max(3, a.iters // 4), warmup=1)[0])
        st = {"same_action_chunk": bool(torch.equal(outs[False], outs[True])), "repeats": a.repeats, "lang_len": 32, "rdt_steps": 5}
        for sw, name in ((False, "device_preprocess_off_ms"), (True, "device_preprocess_on_ms")):
            st[name] = {"median": round(statistics.median(times[sw]), 3), "min": round(min(times[sw]), 3), "max": round(max(times[sw]), 3)}
        st["saved_ms"] = round(st["device_preprocess_off_ms"]["median"] - st["device_preprocess_on_ms"]["median"], 3)
        res["step_b1_from_pil"] = st
        print("step", st, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
