#!/usr/bin/env python
"""Cost of feeding RDT fine-tuning from device-resident episodes (vlatouch.rdt_data.EpisodeStore) -> profiles/rdt_data_bench.json.

Synthetic episodes in the raw `episode_<n>.h5` layout (uncompressed, written to a temporary directory): by default 20 episodes of 300 steps,
two cameras of 480 x 640 and the always-missing third one (2 x 3 frame slots per sample), instructions of 32 x 4096, B = 4, H = 64, A = 128.
Device-synchronised wall times of
  * the load: reading and preparing the episodes on the host (`EpisodeStore(...)`), then `upload()`; the resident bytes;
  * one micro-batch on the device path: `draw` and `assemble` (with the reference recipe's cond_mask_prob 0.1, state_noise_snr 40, image_aug);
  * the same samples (same seeds) built by the host statement tests/rdt_data_ref.py from episodes already in host memory (no file read, which
    the reference repeats per sample) and copied up (arrays and the valid frames), in the same process, alternated with the device path;
  * unless --no-train: one `finetune` micro-batch (prepare_batch through the so400m tower + `train_step` of the bf16 RDT-1B trainer,
    synthetic weights) under each feed, alternated.
No bar is set; the file states what was measured and on how many runs.
    python tools/rdt_data_bench.py [--episodes 20] [--steps 300] [--repeats 20] [--no-train] [--out profiles/rdt_data_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vlatouch import h5lite, synth  # noqa: E402
from tests import rdt_data_ref as R  # noqa: E402


def _stats(ms):
    t = sorted(ms)
    n = len(t)
    return {"median": t[n // 2] if n % 2 else 0.5 * (t[n // 2 - 1] + t[n // 2]), "min": t[0], "max": t[-1], "n": n}


def write_episodes(d, a):
    g = np.random.RandomState(0)
    for e in range(a.episodes):
        n = a.steps
        pos = np.cumsum(g.normal(scale=0.02, size=(n, 3)), axis=0)
        quat = g.normal(size=(n, 4))
        pos[:3], quat[:3] = pos[0], quat[0]
        tree = {"ee_poses": np.concatenate([pos, quat], axis=1), "gripper_pos": g.uniform(0, 255, n),
                "instruct_embeddings": g.normal(size=(1, a.lang_len, a.lang_dim)).astype(np.float32)}
        base = g.randint(0, 256, (a.height + 64, a.width, 3)).astype(np.uint8)
        for cam in (1, 2):                                            # every frame another window of one noise image: cheap to make, not constant
            fr = np.stack([np.roll(base, 7 * i + cam, axis=1)[i % 64:i % 64 + a.height] for i in range(n)])
            tree[f"camera{cam}"] = {f"camera{cam}": fr}
        h5lite.write_file(os.path.join(d, f"episode_{e}.h5"), tree, compression=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--lang-len", type=int, default=32)
    ap.add_argument("--lang-dim", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train-repeats", type=int, default=5)
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--no-train", action="store_true", help="skip the finetune micro-batch (it builds the so400m tower and the RDT-1B trainer)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdt_data_bench.json"))
    a = ap.parse_args()
    from vlatouch.rdt_data import EpisodeStore
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    B = a.batch
    draw = dict(cond_mask_prob=0.1, state_noise_snr=40, image_aug=True)
    rngs = lambda s: dict(np_rng=np.random.RandomState(s), rng=random.Random(s), generator=torch.Generator().manual_seed(s))
    rec = {"episodes": a.episodes, "steps": a.steps, "frame": [a.height, a.width, 3], "cameras": 2, "frame_slots": 6, "lang": [a.lang_len, a.lang_dim],
           "batch": B, "horizon": 64, "state_dim": 128, "draw": draw, "device": torch.cuda.get_device_name(dev), "repeats": a.repeats}
    tmp = tempfile.mkdtemp(prefix="rdt_data_bench_")
    try:
        t0 = time.perf_counter()
        write_episodes(tmp, a)
        rec["write_fixture_s"] = time.perf_counter() - t0
        torch.zeros(1, device=dev)
        sync(); t0 = time.perf_counter()
        store = EpisodeStore(tmp, dataset_name=R.DATASET_NAME, dataset_names=R.DATASET_NAMES, control_freq=R.CONTROL_FREQ, device=dev)
        t1 = time.perf_counter()
        # the host statement shares the store's host arrays (one copy of the frames in host memory; the store lets go of its references in upload)
        ds = R.Dataset(paths=store.paths, horizon=64, with_frames=False)
        assert [e["path"] for e in ds.eps] == [e.path for e in store.episodes]
        for he, se in zip(ds.eps, store.episodes):
            he["cams"] = list(se.frames)
        t1b = time.perf_counter()
        store.upload()
        sync(); t2 = time.perf_counter()
        rec["load"] = {"read_and_prepare_s": t1 - t0, "upload_s": t2 - t1b, "resident_bytes": store.resident_bytes, "host_frame_bytes": store.host_frame_bytes,
                       "kept_episodes": len(store.episodes), "len": len(store), "runs": 1}
        print(json.dumps(rec["load"]), flush=True)
    finally:
        shutil.rmtree(tmp)

    def device_feed(r):
        t0 = time.perf_counter()
        plans = store.draw(B, **r, **draw)
        t1 = time.perf_counter()
        batch = store.assemble(plans)
        sync()
        return batch, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)

    def host_feed(r):
        t0 = time.perf_counter()
        batch = R.host_batch(ds, B, r["np_rng"], r["rng"], r["generator"], **draw)
        t1 = time.perf_counter()
        for k in ("states", "actions", "state_elem_mask", "state_norm", "lang_embeds", "lang_attn_mask", "ctrl_freqs"):
            batch[k] = batch[k].to(dev)
        up = [[None if f is None else torch.from_numpy(f).to(dev) for f in s] for s in batch["frames"]]
        sync()
        return batch, up, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)

    ra, rb = rngs(1), rngs(1)
    dd, da, hb, hc, same = [], [], [], [], True
    for k in range(3 + a.repeats):
        bd, t_draw, t_asm = device_feed(ra)
        bh, up, t_build, t_copy = host_feed(rb)
        same = same and all(torch.equal(bd[key], bh[key]) for key in ("actions", "state_elem_mask", "state_norm", "lang_embeds", "lang_attn_mask", "ctrl_freqs"))
        same = same and all((x is None) == (y is None) and (x is None or torch.equal(x, y)) for s, t in zip(bd["frames"], up) for x, y in zip(s, t))
        if k >= 3:
            dd.append(t_draw), da.append(t_asm), hb.append(t_build), hc.append(t_copy)
    rec["micro_batch"] = {"device_draw_ms": _stats(dd), "device_assemble_ms": _stats(da), "host_build_ms": _stats(hb), "host_copy_up_ms": _stats(hc),
                          "same_gathered_arrays_and_frames": bool(same),
                          "note": "alternated in one process, each timed between device synchronisations; the noised states are not compared (1 ulp); "
                                  "the host statement indexes episodes already read into host memory: its figure excludes the file read the reference "
                                  "repeats for every sample"}
    print(json.dumps(rec["micro_batch"]), flush=True)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)

    save()                                                            # the data-path figures stand even if the training part does not fit

    if not a.no_train:
        from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
        from models.rdt_runner import RDTRunner
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
        ra, rb = rngs(2), rngs(2)
        td, th = [], []
        for k in range(1 + a.train_repeats):
            sync(); t0 = time.perf_counter()
            tr.train_step(**prepare_batch(store.assemble(store.draw(B, **ra, **draw)), vision_encoder=tower, preprocessor=pp))
            sync(); t1 = time.perf_counter()
            tr.train_step(**prepare_batch(R.host_batch(ds, B, rb["np_rng"], rb["rng"], rb["generator"], **draw), vision_encoder=tower, preprocessor=pp))
            sync(); t2 = time.perf_counter()
            if k >= 1:
                td.append(1e3 * (t1 - t0)), th.append(1e3 * (t2 - t1))
        rec["finetune_micro_batch"] = {"device_feed_ms": _stats(td), "host_feed_ms": _stats(th), "depth": a.depth, "trainer_precision": "bf16",
                                       "tower": "so400m bf16, synthetic weights", "peak_memory_gib": torch.cuda.max_memory_allocated(dev) / 2 ** 30,
                                       "note": "draw + assemble (or the host statement) + prepare_batch + train_step, alternated in one process"}
        print(json.dumps(rec["finetune_micro_batch"]), flush=True)
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
