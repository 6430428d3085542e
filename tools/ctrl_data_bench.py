#!/usr/bin/env python
"""Cost of feeding controller training from device-resident episodes (vlatouch.ctrl_data.ControllerStore) -> profiles/ctrl_data_bench.json.

Synthetic episodes in the reference's `episode_<n>.h5` layout (LZF, written with vlatouch.h5lite to a temporary directory): by default 6
episodes of 60 steps, two cameras of 384 x 384, VLA chunks of 64 x 10; windows of 2 context frames and horizon 16, the reference's batch of
128, the controller's default encoder (dinov2-small, synthetic weights).  Device-synchronised wall times of
  * building the training store (read, encode every indexed frame with the normalisation off and on, byte sums) and its resident bytes;
  * `assemble` alone (the plan's upload and the vt_ctrl_batch call);
  * one loop iteration of `DiffusionControllerTrainer._train_epoch` under each feed, alternated in one process: the loader's next batch and
    `train_step` on it.  Host feed: `ControllerDataModule` (num_workers=0, every episode already decoded in the dataset's cache) through
    `ControllerDataset.__getitem__`, the collate, the frame upload and the frozen tower.  Store feed: `ControllerStoreModule` over the same
    data module.
The condition the store has to meet is stated in the result: the store-fed iteration is no slower than the host-fed one of the same process.
    python tools/ctrl_data_bench.py [--episodes 6] [--steps 60] [--res 384] [--batch 128] [--repeats 7] [--out profiles/ctrl_data_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
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


def _stats(ms):
    t = sorted(ms)
    n = len(t)
    return {"median": t[n // 2] if n % 2 else 0.5 * (t[n // 2 - 1] + t[n // 2]), "min": t[0], "max": t[-1], "n": n}


def write_episodes(d, a):
    g = np.random.RandomState(0)
    for e in range(a.episodes):
        n = a.steps
        ee = np.concatenate([np.cumsum(g.normal(scale=0.05, size=(n, 3)), axis=0), g.normal(size=(n, 4))], axis=1)
        vla = g.normal(size=(n, 64, 10))
        vla[:, :, -1] = g.uniform(0, 255, size=(n, 64))
        tree = {"ee_poses": ee, "gripper_pos": g.uniform(0, 255, n), "vla_action": vla, "gelsight_force": {"forces": g.normal(size=(n, 3))}}
        base = g.randint(0, 256, (a.res + 64, a.res, 3)).astype(np.uint8)
        for cam in (1, 2):                                            # every frame another window of one noise image: cheap to make, not constant
            tree[f"camera{cam}_resized"] = np.stack([np.roll(base, 7 * i + cam, axis=1)[i % 64:i % 64 + a.res] for i in range(n)])
        h5lite.write_file(os.path.join(d, f"episode_{e}.h5"), tree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=6)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--res", type=int, default=384)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--assemble-repeats", type=int, default=50)
    ap.add_argument("--precision", default="bf16", choices=("fp32", "bf16"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctrl_data_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    from residual_controller.bridge_controller import DiffusionController
    from residual_controller.bridge_train import DiffusionControllerTrainer
    from residual_controller.controller_dataset import ControllerDataModule
    from vlatouch.ctrl_data import ControllerStoreModule
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    B = a.batch
    rec = {"episodes": a.episodes, "steps": a.steps, "frame": [a.res, a.res, 3], "cameras": 2, "context_frames": 2, "horizon": a.horizon, "batch": B,
           "encoder": "dinov2-small, synthetic weights", "precision": a.precision, "device": torch.cuda.get_device_name(dev), "repeats": a.repeats}
    tmp = tempfile.mkdtemp(prefix="ctrl_data_bench_")
    try:
        t0 = time.perf_counter()
        write_episodes(tmp, a)
        rec["write_fixture_s"] = time.perf_counter() - t0
        np.random.seed(0)
        torch.manual_seed(0)
        dm = ControllerDataModule(tmp, batch_size=B, num_workers=0, context_frames=2, horizon=a.horizon, use_images=True, image_size=a.res)
        if len(dm.train_dataset) < B:
            raise SystemExit(f"{len(dm.train_dataset)} training windows are fewer than one batch of {B}: raise --episodes or --steps")
        ctrl = synth.build_controller(DiffusionController, a.precision, device=str(dev))
        torch.zeros(1, device=dev)
        sync()
        mod = ControllerStoreModule(dm, ctrl)
        rep = mod.train_store.report()
        rec["store"] = {"build_s": rep["build_seconds"], "resident_bytes": rep["resident_bytes"], "total_bytes": rep["total_bytes"], "rows": rep["rows"],
                        "frames_encoded": rep["frames_encoded"], "windows": len(mod.train_store), "files_skipped": len(rep["skipped"]),
                        "engine_rebuilds": rep["engine_rebuilds"], "validation_store_build_s": mod.val_store.report()["build_seconds"], "runs": 1}
        print(json.dumps(rec["store"]), flush=True)
        tr = DiffusionControllerTrainer(ctrl, mod, checkpoint_dir=os.path.join(tmp, "ck"), device=str(dev))
        kin = tr.trainer.mlp.kin

        # assemble alone
        g = torch.Generator().manual_seed(1)
        ta = []
        for k in range(3 + a.assemble_repeats):
            idx = torch.randperm(len(mod.train_store), generator=g)[:B]
            sync(); t0 = time.perf_counter()
            mod.train_store.assemble(idx, layout="bridge", kin=kin, use_force=tr.use_force)
            sync()
            if k >= 3:
                ta.append(1e3 * (time.perf_counter() - t0))
        rec["assemble_ms"] = _stats(ta)
        print(json.dumps({"assemble_ms": rec["assemble_ms"]}), flush=True)

        # one loop iteration under each feed, alternated
        def iteration(loader):
            sync(); t0 = time.perf_counter()
            batch = next(iter(loader))
            t1 = time.perf_counter()
            loss, _ = tr.train_step(batch)
            sync(); t2 = time.perf_counter()
            return 1e3 * (t2 - t0), 1e3 * (t1 - t0), float(loss)

        host_dl, store_dl = dm.train_dataloader(), mod.train_dataloader()
        th, ts, thb, tsb, finite = [], [], [], [], True
        for k in range(2 + a.repeats):                                # the first host iterations decode the episodes into the dataset's cache
            h = iteration(host_dl)
            s = iteration(store_dl)
            finite = finite and np.isfinite(h[2]) and np.isfinite(s[2])
            if k >= 2:
                th.append(h[0]), thb.append(h[1]), ts.append(s[0]), tsb.append(s[1])
        rec["train_iteration"] = {
            "host_feed_ms": _stats(th), "host_next_batch_ms": _stats(thb), "store_feed_ms": _stats(ts), "store_next_batch_ms": _stats(tsb),
            "losses_finite": bool(finite), "speedup_of_medians": _stats(th)["median"] / _stats(ts)["median"],
            "condition": "the store-fed iteration is no slower than the host-fed one of the same process (medians)",
            "condition_met": bool(_stats(ts)["median"] <= _stats(th)["median"]),
            "note": "next(iter(loader)) + train_step, timed between device synchronisations, the two feeds alternated in one process; host feed: "
                    "num_workers=0, episodes already decoded in the dataset's cache (no file read, no LZF decode in the timed iterations)"}
        print(json.dumps(rec["train_iteration"]), flush=True)
        rec["peak_memory_gib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    finally:
        shutil.rmtree(tmp)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
