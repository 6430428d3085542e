#!/usr/bin/env python
"""Camera frames kept as JPEG in HBM (EpisodeStore(frames="jpeg"), vlatouch/jpegdec.py, csrc/vt_jpegdec.hip) against the store of decoded pixels
(frames="device", the path before that mode existed), on one MI355X -> profiles/jpeg_store_bench.json.

SYNTHETIC frames: by default 20 episodes of 300 steps, two cameras of 480 x 640 (a smooth image plus a window of one Gaussian noise field,
sigma 2 for camera1 and 6 for camera2, another window per step), written by Pillow at quality 95, and the always-missing third camera.  These
are not camera frames: the compression ratio of real recordings is NOT measured here.  The same recording is stored twice, as
`convert_episode_to_hdf5(..., images="jpeg")` and `images="decoded"` write it (uncompressed datasets, as tools/rdt_data_bench.py).
  * `load`: reading + preparing on the host and `upload()` of both stores (one run each), resident bytes, the JPEG bytes per frame;
  * `index`: vt_jpeg_index alone on one episode (both cameras), between events;
  * `decode_24`: vt_jpeg_decode alone for 24 frames of 480 x 640 with a prepared table, back to back between events, for index_interval 1, 2,
    4, 8 and one MCU row, with the entry bytes a frame costs at each;
  * `assemble_4`: draw + assemble of a micro-batch of 4 under both stores (host clock, ending in a synchronise);
  * unless --no-train: one loop iteration of tools/rdt_data_bench.py (assemble + prepare_batch through the so400m tower + train_step of the
    bf16 RDT-1B trainer, synthetic weights) under both stores.
Variants alternate inside every repeat, in this one process; medians of the repeats with min and max.  Nothing here is measured on a CPU.

    timeout -k 10 1100 python tools/jpeg_store_bench.py [--episodes 20] [--steps 300] [--repeats 7] [--no-train] [--out profiles/jpeg_store_bench.json]
"""
from __future__ import annotations

import argparse
import io
import json
import multiprocessing
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vla-touch_amd")]

import numpy as np  # noqa: E402

SIGMA = {1: 2.0, 2: 6.0}
_FIELDS: dict = {}


def _frame(a, e: int, cam: int, i: int) -> np.ndarray:
    """Step i of camera `cam` of episode e: a smooth image that drifts with i plus a window of the camera's noise field."""
    h, w = a.height, a.width
    if cam not in _FIELDS:
        _FIELDS[cam] = np.random.default_rng(cam).normal(0.0, SIGMA[cam], (h + 64, w + 64, 3)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    smooth = np.stack([128 + 90 * np.sin((x + 3 * i) / 97.0 + e), 128 + 90 * np.cos((y - 2 * i) / 71.0 + cam), 0.2 * x + 0.3 * y + (5 * i + 17 * e) % 64], axis=-1)
    oy, ox = (7 * i + e) % 64, (13 * i + 5 * e) % 64
    return np.clip(smooth + _FIELDS[cam][oy:oy + h, ox:ox + w], 0, 255).astype(np.uint8)


def _write_episode(job):
    """One episode both ways; returns the JPEG bytes of each camera."""
    from PIL import Image
    from vlatouch import h5lite
    a, e, d = job
    g = np.random.RandomState(e)
    n = a.steps
    pos, quat = np.cumsum(g.normal(scale=0.02, size=(n, 3)), axis=0), g.normal(size=(n, 4))
    pos[:3], quat[:3] = pos[0], quat[0]
    base = {"ee_poses": np.concatenate([pos, quat], axis=1), "gripper_pos": g.uniform(0, 255, n),
            "instruct_embeddings": g.normal(size=(1, a.lang_len, a.lang_dim)).astype(np.float32)}
    jp, dec, sizes = dict(base), dict(base), {}
    for cam in (1, 2):
        files = []
        for i in range(n):
            buf = io.BytesIO()
            Image.fromarray(_frame(a, e, cam, i)).save(buf, "JPEG", quality=95)
            files.append(buf.getvalue())
        name = f"camera{cam}"
        jp[name] = {f"{name}_jpeg": np.frombuffer(b"".join(files), np.uint8),
                    f"{name}_jpeg_offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)}
        dec[name] = {name: np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])}
        sizes[name] = sum(len(f) for f in files)
    h5lite.write_file(os.path.join(d, "jpeg", f"episode_{e}.h5"), jp, compression=None)
    h5lite.write_file(os.path.join(d, "decoded", f"episode_{e}.h5"), dec, compression=None)
    return sizes


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--lang-len", type=int, default=32)
    ap.add_argument("--lang-dim", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--workers", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--no-train", action="store_true", help="skip the loop iteration (it builds the so400m tower and the RDT-1B trainer)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_store_bench.json"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="jpeg_store_bench_")
    for sub in ("jpeg", "decoded"):
        os.makedirs(os.path.join(tmp, sub))
    try:
        t0 = time.perf_counter()
        with multiprocessing.Pool(a.workers) as pool:                 # before the GPU is touched: the workers are plain host processes
            sizes = pool.map(_write_episode, [(a, e, tmp) for e in range(a.episodes)])
        write_s = time.perf_counter() - t0
        run(a, tmp, sizes, write_s)
    finally:
        shutil.rmtree(tmp)


def run(a, tmp, sizes, write_s):
    import PIL
    import torch
    from tests import rdt_data_ref as R
    from vlatouch import _lib
    from vlatouch import jpegdec as D
    from vlatouch.rdt_data import EpisodeStore
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_store_bench: needs an MI355X (nothing here is measured on a CPU)")
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    B = a.batch
    nfr = a.episodes * a.steps
    rec = {"workload": "camera_frames_kept_as_jpeg_in_hbm", "synthetic_frames": True,
           "note": "synthetic frames (smooth image + Gaussian noise, sigma 2 / 6 per camera) at quality 95: the compression ratio of real recordings is not measured",
           "episodes": a.episodes, "steps": a.steps, "frame": [a.height, a.width, 3], "cameras": 2, "quality": 95, "pillow": PIL.__version__, "batch": B,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(dev), "write_fixture_s": round(write_s, 2),
           "jpeg_bytes_per_frame": {k: round(sum(s[k] for s in sizes) / nfr, 1) for k in sizes[0]}, "raw_bytes_per_frame": a.height * a.width * 3}
    kw = dict(dataset_name=R.DATASET_NAME, dataset_names=R.DATASET_NAMES, control_freq=R.CONTROL_FREQ, device=dev)
    torch.zeros(1, device=dev)
    stores, load = {}, {}
    for mode, sub in (("jpeg", "jpeg"), ("device", "decoded")):
        sync(); t0 = time.perf_counter()
        st = EpisodeStore(os.path.join(tmp, sub), frames=mode, **kw)
        t1 = time.perf_counter()
        st.upload()
        sync(); t2 = time.perf_counter()
        stores[mode] = st
        load[mode] = {"read_and_prepare_s": round(t1 - t0, 3), "upload_s": round(t2 - t1, 3), "resident_bytes": int(st.resident_bytes), "runs": 1}
    load["resident_ratio_device_over_jpeg"] = round(load["device"]["resident_bytes"] / load["jpeg"]["resident_bytes"], 2)
    load["jpeg_index_interval"] = D.DEFAULT_INDEX_INTERVAL
    rec["load"] = load
    print(json.dumps(load), flush=True)

    L, sp = _lib.lib(), _lib.stream_ptr(dev)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync(); e0.record()
        for _ in range(iters):
            fn()
        e1.record(); sync()
        return e0.elapsed_time(e1) / iters

    # ---- the index pass of one episode: both cameras' tables in one call
    jfs = [jf for jf in stores["jpeg"]._dev["frames"][0] if jf is not None]
    table = np.concatenate([jf.table for jf in jfs])
    tdev, status = torch.from_numpy(table).to(dev), torch.zeros(len(table), dtype=torch.int32, device=dev)
    index = lambda: _lib.check(L.vt_jpeg_index(table.ctypes.data, _lib.ptr(tdev), len(table), _lib.ptr(status), sp), "vt_jpeg_index")      # noqa: E731
    index()
    rec["index"] = {"frames": len(table), "vt_jpeg_index_ms": _stats([events(index, 3) for _ in range(a.repeats)]), "flagged": int(status.sum())}
    print(json.dumps(rec["index"]), flush=True)

    # ---- decode alone: 24 frames (12 steps of both cameras of episode 0), a prepared table per interval, alternated
    from vlatouch import h5lite
    with h5lite.File(os.path.join(tmp, "jpeg", "episode_0.h5")) as f:
        files = []
        for cam in ("camera1", "camera2"):
            data, off = f[cam][f"{cam}_jpeg"][...], f[cam][f"{cam}_jpeg_offsets"][...]
            files += [data[off[k]:off[k + 1]].tobytes() for k in range(100, 112)]
    want = torch.stack([torch.from_numpy(stores["device"]._dev["frames"][0][c][100:112].cpu().numpy()) for c in (0, 1)]).view(24, a.height, a.width, 3)
    out = torch.empty((24, a.height, a.width, 3), dtype=torch.uint8, device=dev)
    calls, dec = {}, {}
    for iv in (1, 2, 4, 8, "row"):
        jf = D.JpegFrames(files, dev, index_interval=iv)
        rows = jf.table.copy()
        rows[:, D.C_OUT_OFF] = np.arange(24) * out[0].numel()
        ws_bytes = int(L.vt_jpeg_workspace_bytes(rows.ctypes.data, 24))
        ws, rdev, st = torch.empty(ws_bytes, dtype=torch.uint8, device=dev), torch.from_numpy(rows).to(dev), torch.zeros(24, dtype=torch.int32, device=dev)

        def call(rows=rows, ws=ws, rdev=rdev, st=st, ws_bytes=ws_bytes, keep=jf):
            _lib.check(L.vt_jpeg_decode(rows.ctypes.data, _lib.ptr(rdev), 24, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.ptr(st), sp), "vt_jpeg_decode")
        out.zero_()
        call(); sync()
        dec[str(iv)] = {"mcus_per_entry": int(rows[0, D.C_INTERVAL]), "entry_bytes_per_frame": jf.index_bytes // 24, "workspace_bytes": ws_bytes,
                        "bit_identical_to_pillow": bool(torch.equal(out.cpu(), want))}
        calls[str(iv)] = call
    ts = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, fn in calls.items():
            ts[k].append(events(fn, a.iters))
    for k in calls:
        dec[k]["vt_jpeg_decode_24_ms"] = _stats(ts[k])
    dec["stream_bytes_per_frame"] = round(sum(len(f) for f in files) / 24, 1)
    rec["decode_24"] = dec
    print(json.dumps(dec), flush=True)
    del calls, ws, rdev

    # ---- a micro-batch of 4 under both stores
    draw = dict(cond_mask_prob=0.1, state_noise_snr=40, image_aug=True)
    rngs = lambda s: dict(np_rng=np.random.RandomState(s), rng=random.Random(s), generator=torch.Generator().manual_seed(s))      # noqa: E731
    r = {m: rngs(1) for m in stores}
    ts, same = {m: [] for m in stores}, True
    for k in range(2 + a.repeats):
        got = {}
        for m, st in stores.items():
            sync(); t0 = time.perf_counter()
            got[m] = st.assemble(st.draw(B, **r[m], **draw))
            sync()
            if k >= 2:
                ts[m].append(1e3 * (time.perf_counter() - t0))
        same = same and all((x is None) == (y is None) and (x is None or torch.equal(x, y))
                            for fa, fb in zip(got["jpeg"]["frames"], got["device"]["frames"]) for x, y in zip(fa, fb))
    rec["assemble_4"] = {"draw_and_assemble_ms": {m: _stats(v) for m, v in ts.items()}, "same_frames": bool(same),
                         "note": "host clock around draw + assemble, ending in a synchronise; frames='jpeg' decodes the valid frames of the batch here"}
    print(json.dumps(rec["assemble_4"]), flush=True)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)

    save()
    if not a.no_train:
        from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
        from models.rdt_runner import RDTRunner
        from vlatouch import synth
        from vlatouch.imgprep import DevicePreprocessor
        from vlatouch.rdt_train import prepare_batch
        c = synth.SIGLIP_CONFIGS["so400m"]
        vcfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                    image_size=c["image_size"], patch_size=14)
        ssd = synth.fill_state_dict_device(synth.siglip_shapes(**c), dev, torch.float32, seed=9)
        tower = SiglipVisionTower("synthetic", None, device=dev, precision="bf16", state_dict={k: v.cpu() for k, v in ssd.items()}, config=vcfg)
        del ssd
        pp = DevicePreprocessor(384, [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], dev, torch.bfloat16, pad=True, brightness=True, image_size=None)
        shapes = dict(hidden=2048, depth=a.depth, heads=32, horizon=64, action_dim=128, lang_token_dim=a.lang_dim, img_token_dim=1152, state_token_dim=128,
                      max_lang_cond_len=1024, img_cond_len=6 * 729)
        rcfg = {"rdt": {"hidden_size": 2048, "depth": a.depth, "num_heads": 32, "rms_norm": "meansq"}, "lang_adaptor": "mlp2x_gelu",
                "img_adaptor": "mlp2x_gelu", "state_adaptor": "mlp3x_gelu",
                "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "beta_schedule": "squaredcos_cap_v2", "prediction_type": "sample"}}
        runner = RDTRunner(action_dim=128, pred_horizon=64, config=rcfg, lang_token_dim=a.lang_dim, img_token_dim=1152, state_token_dim=128,
                           max_lang_cond_len=1024, img_cond_len=6 * 729, dtype=torch.bfloat16, device=dev, init_weights=False)
        runner.load_state_dict(synth.fill_state_dict_device(synth.rdt_runner_shapes(**shapes), dev, torch.float32, seed=7), assign=True)
        tr = runner.trainer(precision="bf16", lr=1e-4)
        r = {m: rngs(2) for m in stores}
        ts = {m: [] for m in stores}
        for k in range(1 + a.repeats):
            for m, st in stores.items():
                sync(); t0 = time.perf_counter()
                tr.train_step(**prepare_batch(st.assemble(st.draw(B, **r[m], **draw)), vision_encoder=tower, preprocessor=pp))
                sync()
                if k >= 1:
                    ts[m].append(1e3 * (time.perf_counter() - t0))
        s = {m: _stats(v) for m, v in ts.items()}
        rec["loop_iteration"] = {"ms": s, "depth": a.depth, "trainer_precision": "bf16", "tower": "so400m bf16, synthetic weights",
                                 "jpeg_median_inside_device_spread": bool(s["device"]["min"] <= s["jpeg"]["median"] <= s["device"]["max"]),
                                 "jpeg_minus_device_median_ms": round(s["jpeg"]["median"] - s["device"]["median"], 3),
                                 "peak_memory_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
                                 "note": "draw + assemble + prepare_batch + train_step, the two stores alternated in one process; the yardstick is the "
                                         "frames='device' leg"}
        print(json.dumps(rec["loop_iteration"]), flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
