#!/usr/bin/env python
"""Fixture episodes and golden results of the fine-tuning data path, captured from the reference's own code.

Writes tests/golden/episodes_raw/episode_<n>.h5 (vlatouch.h5lite, the raw layout of convert_episode_to_hdf5: ee_poses, gripper_pos,
instruct_embeddings, camera1/camera1, camera2/camera2 with 12 x 16 frames) and tests/golden/g19_rdt_data.npz.  Episodes (tests/rdt_data_ref):
  episode_2   40 steps, still for 3      kept          episode_3   31 steps                       dropped: short
  episode_10  32 steps, still for 1      late          episode_11  40 steps, never moves          dropped: still
  episode_12  57 steps, still for 5      kept          episode_20  40 steps, still for 10         late
  episode_21  45 steps, still for 2      kept
(the numbers order 2 < 3 < 10 < .. naturally, not as strings).  late: dropped at horizon 64, where first_idx - 1 >= N - 32 (a 32-step episode
always is: the reference's randint(0, 0) raises), and kept at horizon 8.  Quaternions are unnormalised and keep |sin(pitch)| <= 0.999 (asserted): the
reference's quaternion -> Euler -> matrix round trip loses accuracy near the gimbal pole, which is no property of the product.  Every frame
carries (episode number, camera, frame index) in the pixel the stand-in resize maps to the centre of the 384 x 384 image.

The reference runs through tools/ref_import.py with further stand-in MODULES: `h5py` whose File is h5lite.File, a `cv2` whose resize is a
nearest-neighbour pick (pixels are not recorded), `configs.state_vec` with the mapping scripts/franka_model_eef.py assumes,
`train.image_corrupt` (imgaug is absent; the stand-in marks the image), `torchvision.transforms` whose ColorJitter draws through
vlatouch.imgaug.color_jitter_params (UNPINNED to torchvision, as that function is) and marks the image, and an image processor that records,
per frame, whether it is the background, which frame it is and how it was augmented.  Legs:
  * `UnifiedVLADataset.parse_file` (instance made with __new__, its five attributes set) for 8 seeds per kept episode (`pf_*`), and with
    CHUNK_SIZE = 8 for the two late episodes (`pf8_*`);
  * `parse_file_state_only` for every file;
  * `process_hdf5_dataset` over the kept files (over all files the reference's loop retries an invalid index with a random one);
  * `VLAConsumerDataset(use_hdf5=True, use_precomp_lang_embed=True).__getitem__` + `DataCollatorForVLAConsumerDataset` in a temporary
    working directory holding configs/base.yaml, configs/*.json and data/datasets/mango_hdf5_gelsight/ with the kept, the short and the still
    episode (the two late episodes have a non-zero weight in the reference, whose randint then raises and whose loader silently draws again; the
    product drops it at load), 2 batches of 3 samples with cond_mask_prob 0.5, cam_ext_mask_prob 0.3, state_noise_snr 40, image_aug on;
  * `sixd_route_err`: the worst difference between the reference's 6-D rotation and the product's direct one on the fixture's quaternions.
    python tools/make_golden_rdt_data.py
"""
from __future__ import annotations

import json
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vla-touch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vlatouch import h5lite, imgaug, rdt_data  # noqa: E402
from tests import rdt_data_ref as R  # noqa: E402
import ref_import  # noqa: E402

OUT_DIR = R.FIXTURE_DIR
#            number, steps, still, lang length, expectation
EPISODES = [(2, 40, 3, 5, "kept"), (3, 31, 2, 4, rdt_data.DROP_SHORT), (10, 32, 1, 7, rdt_data.DROP_LATE), (11, 40, 40, 4, rdt_data.DROP_STILL),
            (12, 57, 5, 3, "kept"), (20, 40, 10, 6, rdt_data.DROP_LATE), (21, 45, 2, 7, "kept")]
LANG_DIM = 96
FRAME_H, FRAME_W, SIG_ROW, SIG_COL = 12, 16, 6, 8


def make_episode(number, n, still, lang_len):
    from scipy.spatial.transform import Rotation
    g = np.random.RandomState(1000 + number)
    pos = np.cumsum(g.normal(scale=0.02, size=(n, 3)), axis=0) + g.uniform(-0.5, 0.5, 3)
    euler = np.cumsum(g.normal(scale=0.05, size=(n, 3)), axis=0) + np.array([g.uniform(-3, 3), g.uniform(-1.0, 1.0), g.uniform(-3, 3)])
    euler[:, 1] = np.clip(euler[:, 1], -1.3, 1.3)
    quat = Rotation.from_euler("xyz", euler).as_quat() * g.uniform(0.5, 2.0, (n, 1)) * np.where(g.rand(n, 1) < 0.3, -1.0, 1.0)
    grip = np.clip(np.cumsum(g.normal(scale=8.0, size=n)) + 120.0, 0.0, 255.0)
    k = min(still, n)
    pos[:k], quat[:k], grip[:k] = pos[0], quat[0], grip[0]
    if k < n:
        pos[k:, 0] += 0.05                                             # the first moving step clears the 1e-2 threshold
    pitch = Rotation.from_quat(quat).as_euler("xyz")[:, 1]
    assert np.abs(np.sin(pitch)).max() <= 0.999, (number, np.abs(np.sin(pitch)).max())
    tree = {"ee_poses": np.concatenate([pos, quat], axis=1).astype(np.float64), "gripper_pos": grip.astype(np.float64),
            "instruct_embeddings": g.normal(size=(1, lang_len, LANG_DIM)).astype(np.float32)}
    yy, xx = np.mgrid[0:FRAME_H, 0:FRAME_W]
    for cam in (1, 2):
        fr = np.empty((n, FRAME_H, FRAME_W, 3), dtype=np.uint8)
        for i in range(n):
            fr[i, :, :, 0] = (40 * cam + 3 * i + 9 * xx) % 256
            fr[i, :, :, 1] = (5 * number + 7 * yy + i) % 256
            fr[i, :, :, 2] = (200 - 2 * i + 4 * (xx // 4)) % 256
            fr[i, SIG_ROW, SIG_COL] = (number, cam, i)
        tree[f"camera{cam}"] = {f"camera{cam}": fr}
    return tree


def write_fixtures():
    os.makedirs(OUT_DIR, exist_ok=True)
    for number, n, still, lang_len, _ in EPISODES:
        h5lite.write_file(os.path.join(OUT_DIR, f"episode_{number}.h5"), make_episode(number, n, still, lang_len), compression="lzf")


# ---------------------------------------------------------------------------------------------- stand-ins
def _nearest_resize(img, size, interpolation=None):
    w, h = size
    ys = np.floor((np.arange(h) + 0.5) * img.shape[0] / h).astype(np.int64)
    xs = np.floor((np.arange(w) + 0.5) * img.shape[1] / w).astype(np.int64)
    return img[ys][:, xs]


class _ColorJitter:
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.args = (brightness, contrast, saturation, hue)

    def __call__(self, image):
        out = image.copy()
        out.info = dict(image.info, jitter=imgaug.color_jitter_params(*self.args))
        return out


def _image_corrupt(image):
    out = image.copy()
    out.info = dict(image.info, corrupt=True)
    return out


class _Processor:
    """What __getitem__ reads of SiglipImageProcessor: image_mean, size, preprocess.  Records one row per frame."""
    image_mean = [0.5, 0.5, 0.5]
    size = {"height": 384, "width": 384}

    def __init__(self):
        self.rows = []

    def preprocess(self, image, return_tensors="pt"):
        a = np.asarray(image)
        assert a.shape == (384, 384, 3), a.shape
        background = bool((a == np.array([127, 127, 127], dtype=np.uint8)).all())
        p = image.info.get("jitter")
        self.rows.append(dict(background=background, sig=[-1, -1, -1] if background else [int(v) for v in a[192, 192]],
                              corrupt=bool(image.info.get("corrupt", False)), jittered=p is not None,
                              order=list(p.order) if p else [-1] * 4, factors=list(p.factors()) if p else [np.nan] * 4))
        return {"pixel_values": [torch.zeros(1)]}


def setup_reference():
    ref_import.setup()
    ref_import._stub("h5py", File=h5lite.File)
    ref_import._stub("cv2", resize=_nearest_resize, INTER_AREA=3)
    idx = {"eef_pos_x": 30, "eef_pos_y": 31, "eef_pos_z": 32, "right_gripper_open": 10}
    idx.update({f"eef_angle_{i}": 33 + i for i in range(6)})
    ref_import._stub("configs")
    ref_import._stub("configs.state_vec", STATE_VEC_IDX_MAPPING=idx)
    tv = sys.modules["torchvision"]
    tv.transforms = ref_import._stub("torchvision.transforms", ColorJitter=_ColorJitter, Resize=None)
    ref_import._stub("train.image_corrupt", image_corrupt=_image_corrupt)


def main():
    write_fixtures()
    paths = R.fixture_paths()
    names = [os.path.basename(p) for p in paths]
    assert names == [f"episode_{e[0]}.h5" for e in EPISODES], names
    expect = {f"episode_{e[0]}.h5": e[4] for e in EPISODES}
    kept = [p for p in paths if expect[os.path.basename(p)] == "kept"]
    setup_reference()
    from data.unified_vla_dataset_episode import UnifiedVLADataset
    from data.compute_dataset_stat_episode import process_hdf5_dataset
    from docs.test_6drot import convert_quaternion_to_orthod6d

    out = {"names": np.array(names), "expect": np.array([expect[n] for n in names])}
    ds = UnifiedVLADataset.__new__(UnifiedVLADataset)
    ds.DATASET_NAME, ds.CHUNK_SIZE, ds.IMG_HISORY_SIZE, ds.STATE_DIM, ds.file_paths = R.DATASET_NAME, 64, 2, 128, list(paths)

    # parse_file_state_only for every file, and the 6-D route difference
    lens, route = [], 0.0
    for p in paths:
        n = os.path.basename(p)[:-3]
        state, epi_len = ds.parse_file_state_only(p)
        lens.append(epi_len)
        if state is not None:
            out[f"so_{n}"] = state["state"]
        with h5lite.File(p) as f:
            q = np.asarray(f["ee_poses"][...])[:, 3:]
        route = max(route, float(np.abs(convert_quaternion_to_orthod6d(q) - rdt_data.quat_to_ortho6d(q)).max()))
    out["so_len"], out["sixd_route_err"] = np.array(lens), np.array(route)
    assert [l > 0 for l in lens] == [expect[n] != rdt_data.DROP_SHORT and expect[n] != rdt_data.DROP_STILL for n in names]

    # parse_file, seeded, per kept episode; the third kind of invalid episode raises in the reference's randint
    late = [p for p in paths if expect[os.path.basename(p)] == rdt_data.DROP_LATE]
    for p, tag, chunk in [(p, "pf", 64) for p in kept] + [(p, "pf8", 8) for p in late]:
        n = os.path.basename(p)[:-3]
        rows = []
        ds.CHUNK_SIZE = chunk
        for seed in R.G19_PARSE_SEEDS:
            np.random.seed(seed)
            s, num = ds.parse_file(p)
            assert s["cam_left_wrist"].shape == (2, 0, 0, 0) and (s["cam_high_mask"] == s["cam_right_wrist_mask"]).all()
            rows.append(s)
        for key in ("state", "actions", "state_std", "state_mean", "state_norm", "state_indicator", "cam_high_mask"):
            out[f"{tag}_{n}_{key}"] = np.stack([r[key] for r in rows])
        out[f"{tag}_{n}_step_id"] = np.array([r["meta"]["step_id"] for r in rows])
        out[f"{tag}_{n}_steps"] = np.array(num)
    ds.CHUNK_SIZE = 64
    for p in late:
        try:
            np.random.seed(0)
            ds.parse_file(p)
        except ValueError:
            pass
        else:
            raise AssertionError(f"{p}: the reference's randint was expected to raise")

    # process_hdf5_dataset over the kept files
    ds.file_paths = list(kept)
    ds.episode_sample_weights = np.ones(len(kept)) / len(kept)
    stat = process_hdf5_dataset(ds)
    for key in ("state_mean", "state_std", "state_min", "state_max"):
        out[f"stat_{key}"] = np.array(stat[key])

    # __getitem__ + collator in a working directory of their own
    from train.dataset import VLAConsumerDataset, DataCollatorForVLAConsumerDataset
    cwd, tmp = os.getcwd(), tempfile.mkdtemp(prefix="g19_")
    try:
        os.makedirs(os.path.join(tmp, "configs"))
        data_dir = os.path.join(tmp, "data", "datasets", f"{R.DATASET_NAME}_hdf5_gelsight")
        os.makedirs(data_dir)
        for p in paths:
            if p not in late:
                shutil.copy(p, data_dir)
        with open(os.path.join(tmp, "configs", "base.yaml"), "w") as f:
            f.write("common:\n  action_chunk_size: 64\n  img_history_size: 2\n  state_dim: 128\n  num_cameras: 3\n")
        for name, obj in (("dataset_control_freq.json", {R.DATASET_NAME: R.CONTROL_FREQ}), ("finetune_datasets.json", R.DATASET_NAMES),
                          ("dataset_stat.json", {R.DATASET_NAME: stat})):
            with open(os.path.join(tmp, "configs", name), "w") as f:
                json.dump(obj, f)
        os.chdir(tmp)
        proc = _Processor()
        cfg = {"buf_path": None, "buf_num_chunks": 0, "buf_chunk_size": 0, "tokenizer_max_length": 32, "image_aspect_ratio": "pad"}
        vla = VLAConsumerDataset(config=cfg, tokenizer=None, image_processor=proc, num_cameras=3, img_history_size=2, dataset_type="finetune",
                                 use_hdf5=True, use_precomp_lang_embed=True, **R.G19_KW)
        out["gi_len"], out["gi_weights"] = np.array(len(vla)), np.asarray(vla.hdf5_dataset.episode_sample_weights)
        out["gi_files"] = np.array([os.path.basename(p) for p in vla.hdf5_dataset.file_paths])
        collator = DataCollatorForVLAConsumerDataset(None)
        for seed in R.G19_SEEDS:
            np.random.seed(seed), random.seed(seed), torch.manual_seed(seed)
            proc.rows = []
            batch = collator([vla[0] for _ in range(R.G19_B)])
            assert len(proc.rows) == R.G19_B * 6
            for key in ("states", "actions", "state_elem_mask", "state_norm", "ctrl_freqs", "lang_embeds", "lang_attn_mask"):
                out[f"gi_{seed}_{key}"] = batch[key].numpy()
            out[f"gi_{seed}_data_indices"] = np.array(batch["data_indices"])
            for key in ("background", "sig", "corrupt", "jittered", "order", "factors"):
                out[f"gi_{seed}_fr_{key}"] = np.array([r[key] for r in proc.rows]).reshape(R.G19_B, 6, *np.shape(proc.rows[0][key]))
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    dst = R.GOLDEN
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({os.path.getsize(dst)} bytes), sixd_route_err = {route:.3e}")
    for p in paths:
        print(f"  {os.path.basename(p)}: {os.path.getsize(p)} bytes, {expect[os.path.basename(p)]}")


if __name__ == "__main__":
    main()
