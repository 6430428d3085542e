"""The reference's fine-tuning data path restated in fp64 numpy, one sample at a time as the reference does it, independent of
vlatouch.rdt_data: UnifiedVLADataset.parse_file / parse_file_state_only / get_item (data/unified_vla_dataset_episode.py),
compute_dataset_stat_episode.process_hdf5_dataset, VLAConsumerDataset.__getitem__ and DataCollatorForVLAConsumerDataset
(train/dataset.py).  Pinned to the reference's own code by tests/golden/g19_rdt_data.npz (tools/make_golden_rdt_data.py).

Two things differ from the reference on purpose, as in the product: an image is kept as the raw frame (the frame index and whether it is
the background are what is stated; the pixels go through the device preprocessor), and the 6-D rotation is computed from the quaternion
directly (here through the full rotation matrix, another expression than the product's)."""
from __future__ import annotations

import os
import re
from typing import Dict, List, Optional

import numpy as np
import torch

from vlatouch import h5lite

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "episodes_raw")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_rdt_data.npz")
STATE_INDICES = [30, 31, 32] + [33 + i for i in range(6)] + [10]
DATASET_NAME, DATASET_NAMES, CONTROL_FREQ = "mango", ["other", "mango"], 25
CAMERAS = ("camera1", "camera2", None)                    # cam_high, cam_right_wrist, the empty cam_left_wrist: __getitem__'s order
# the golden's __getitem__ runs: seeds (numpy, random and torch seeded alike) and samples per collated batch
G19_SEEDS, G19_B = (3, 11), 3
G19_KW = dict(cond_mask_prob=0.5, cam_ext_mask_prob=0.3, state_noise_snr=40, image_aug=True)
G19_PARSE_SEEDS = tuple(range(8))


def fixture_paths() -> List[str]:
    num = lambda f: int(re.search(r"episode_(\d+)", f).group(1))
    return [os.path.join(FIXTURE_DIR, f) for f in sorted((f for f in os.listdir(FIXTURE_DIR) if f.endswith(".h5")), key=num)]


def rotation_matrix(quat: np.ndarray) -> np.ndarray:
    """xyzw quaternions [N, 4] -> rotation matrices [N, 3, 3] (the homogeneous form: squares on the diagonal, as scipy's as_matrix)."""
    q = np.asarray(quat, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    m = np.empty((q.shape[0], 3, 3))
    m[:, 0, 0], m[:, 1, 1], m[:, 2, 2] = x * x - y * y - z * z + w * w, -x * x + y * y - z * z + w * w, -x * x - y * y + z * z + w * w
    m[:, 1, 0], m[:, 0, 1] = 2 * (x * y + z * w), 2 * (x * y - z * w)
    m[:, 2, 0], m[:, 0, 2] = 2 * (x * z - y * w), 2 * (x * z + y * w)
    m[:, 2, 1], m[:, 1, 2] = 2 * (y * z + x * w), 2 * (y * z - x * w)
    return m


def load_episode(path: str, with_frames: bool = True) -> dict:
    """with_frames=False leaves `cams` as [None] * 3 for the caller to fill (a caller that already holds the frames)."""
    with h5lite.File(path) as f:
        ee, grip = np.asarray(f["ee_poses"][...], dtype=np.float64), np.asarray(f["gripper_pos"][...], dtype=np.float64)
        m = rotation_matrix(ee[:, 3:])
        sixd = m[:, :, :2].transpose(0, 2, 1).reshape(m.shape[0], -1)          # compute_ortho6d_from_rotation_matrix
        cams = []
        for c in CAMERAS:
            cams.append(np.asarray(f[c][c][...]) if with_frames and c is not None and c in f else None)
        return {"path": path, "qpos_raw": np.concatenate((ee[:, :3], sixd, grip.reshape(-1, 1)), axis=-1),
                "lang": np.asarray(f["instruct_embeddings"][...])[0], "cams": cams}


def fill_in_state(values: np.ndarray, state_dim: int = 128) -> np.ndarray:
    uni = np.zeros(values.shape[:-1] + (state_dim,))
    uni[..., STATE_INDICES] = values
    return uni


def first_idx_of(qpos_raw: np.ndarray) -> Optional[int]:
    idx = np.where(np.any(np.abs(qpos_raw - qpos_raw[0:1]) > 1e-2, axis=1))[0]
    return int(idx[0]) if len(idx) > 0 else None


def parse_file(ep: dict, np_rng, horizon: int = 64, hist: int = 2) -> Optional[dict]:
    """parse_file on a loaded episode -> the sample (images as frame indices per slot), or None for an invalid episode.  Raises ValueError
    where the reference's randint does (first_idx - 1 >= N - int(horizon / 2))."""
    qpos = ep["qpos_raw"]
    n = qpos.shape[0]
    if n < 32:
        return None
    first = first_idx_of(qpos)
    if first is None:
        return None
    step_id = int(np_rng.randint(first - 1, n - int(horizon / 2)))
    action_id = step_id + 2
    qpos = qpos / np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 255]])
    actions = qpos[action_id:action_id + horizon]
    if actions.shape[0] < horizon:
        actions = np.concatenate([actions, np.tile(actions[-1:], (horizon - actions.shape[0], 1))], axis=0)
    state_std = np.std(qpos, axis=0)
    valid_len = min(step_id - (first - 1) + 1, hist)
    got = list(range(max(step_id - hist + 1, 0), step_id + 1))                 # parse_img's slice, padded in front with its first frame
    return {"step_id": step_id, "n_steps": n, "first_idx": first, "state": fill_in_state(qpos[step_id:step_id + 1]),
            "state_std": fill_in_state(state_std), "state_mean": fill_in_state(np.mean(qpos, axis=0)),
            "state_norm": fill_in_state(np.sqrt(np.mean(qpos ** 2, axis=0))), "actions": fill_in_state(actions),
            "state_indicator": fill_in_state(np.ones_like(state_std)), "cam_mask": np.array([False] * (hist - valid_len) + [True] * valid_len),
            "frame_idx": [got[0]] * (hist - len(got)) + got, "lang": ep["lang"]}


def state_only(ep: dict):
    """parse_file_state_only -> (state [len, 128] | None, len)."""
    qpos = ep["qpos_raw"]
    if qpos.shape[0] < 32:
        return None, 0
    first = first_idx_of(qpos)
    if first is None:
        return None, 0
    state = fill_in_state((qpos / np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 255]]))[first - 1:])
    return state, len(state)


def dataset_stat(eps: List[dict]) -> dict:
    """process_hdf5_dataset over valid episodes."""
    EPS = 1e-8
    acc = None
    for ep in eps:
        s, _ = state_only(ep)
        z = s.copy()
        z[np.abs(s) <= EPS] = 0
        cur = [np.sum(np.abs(s) > EPS, axis=0).astype(np.float64), np.sum(s, axis=0), np.sum(z, axis=0), np.sum(z ** 2, axis=0), s.shape[0],
               np.max(s, axis=0), np.min(s, axis=0)]
        if acc is None:
            acc = cur
        else:
            acc = [acc[0] + cur[0], acc[1] + cur[1], acc[2] + cur[2], acc[3] + cur[3], acc[4] + cur[4], np.maximum(acc[5], cur[5]), np.minimum(acc[6], cur[6])]
    nz, ssum, zsum, zsq, cnt, smax, smin = acc
    nz = np.maximum(nz, np.ones_like(nz))
    return {"state_mean": ssum / cnt, "state_std": np.sqrt(np.maximum(zsq / nz - (zsum / cnt) ** 2 * (cnt / nz), np.zeros_like(zsq))),
            "state_min": smin, "state_max": smax}


class Dataset:
    """The valid episodes of a file list with the reference's sampling weights (an invalid file has weight 0 there, which leaves the choice
    among the others unchanged), for one horizon."""

    def __init__(self, paths=None, horizon: int = 64, hist: int = 2, with_frames: bool = True):
        self.horizon, self.hist = horizon, hist
        eps = [load_episode(p, with_frames) for p in (fixture_paths() if paths is None else paths)]
        self.eps = []
        for ep in eps:
            _, n = state_only(ep)
            if n > 0 and first_idx_of(ep["qpos_raw"]) - 1 < ep["qpos_raw"].shape[0] - int(horizon / 2):
                ep["len"] = n
                self.eps.append(ep)
        lens = np.array([ep["len"] for ep in self.eps])
        self.total, self.weights = int(np.sum(lens)), lens / np.sum(lens)
        self.stat = dataset_stat(self.eps)

    def getitem(self, np_rng, rng, generator=None, *, cond_mask_prob=0.1, cam_ext_mask_prob=-1.0, state_noise_snr=None, image_aug=False) -> dict:
        """get_item + __getitem__ for one sample: fp64 arrays, `frames` (the raw frame or None per slot and camera, slot-major), `frame_ref`
        ((camera, frame index) or None), `jitter` (ColorJitterParams or None per frame)."""
        from vlatouch.imgaug import color_jitter_params
        e = int(np_rng.choice(len(self.eps), p=self.weights))
        ep = self.eps[e]
        res = parse_file(ep, np_rng, self.horizon, self.hist)
        d = {"episode": e, "step_id": res["step_id"], "data_idx": DATASET_NAMES.index(DATASET_NAME)}
        d["ctrl_freq"] = CONTROL_FREQ if rng.random() > cond_mask_prob else 0
        states = res["state"]
        if state_noise_snr is not None:
            states = states + np_rng.normal(0.0, res["state_std"] / np.sqrt(10 ** (state_noise_snr / 10)), states.shape)
        ds_mean = np.tile(self.stat["state_mean"][None], (states.shape[0], 1))
        d["states"] = states if rng.random() > cond_mask_prob else ds_mean
        d["actions"] = res["actions"]
        d["state_elem_mask"] = res["state_indicator"] if rng.random() > cond_mask_prob else np.zeros_like(res["state_indicator"])
        d["state_norm"] = res["state_norm"]
        mask_probs = [cond_mask_prob] * len(CAMERAS)
        if cam_ext_mask_prob >= 0.0:
            mask_probs[0] = cam_ext_mask_prob
        frames, frame_ref = [], []
        for i in range(self.hist):
            for j in range(len(CAMERAS)):
                if res["cam_mask"][i] and ep["cams"][j] is not None and rng.random() > mask_probs[j]:
                    frames.append(ep["cams"][j][res["frame_idx"][i]])
                    frame_ref.append((j, res["frame_idx"][i]))
                else:
                    frames.append(None)
                    frame_ref.append(None)
        jitter = []
        for f in frames:
            p = None
            if f is not None and image_aug and rng.random() > 0.5:
                if rng.choice(["corrput_only", "color_only", "both"]) != "corrput_only":
                    p = color_jitter_params(generator=generator)
            jitter.append(p)
        d["frames"], d["frame_ref"], d["jitter"], d["lang_embed"] = frames, frame_ref, jitter, res["lang"]
        return d


def collate(instances: List[dict]) -> Dict[str, object]:
    """DataCollatorForVLAConsumerDataset on precomputed language embeddings (fp64 tensors, as the reference's), with frames / jitter as B lists."""
    out = {k: torch.stack([torch.from_numpy(np.asarray(i[k])) for i in instances], dim=0) for k in ("states", "actions", "state_elem_mask", "state_norm")}
    out["data_indices"] = [i["data_idx"] for i in instances]
    out["ctrl_freqs"] = torch.tensor([i["ctrl_freq"] for i in instances])
    lang = [torch.from_numpy(np.asarray(i["lang_embed"])) for i in instances]
    out["lang_embeds"] = torch.nn.utils.rnn.pad_sequence(lang, batch_first=True, padding_value=0)
    mask = torch.zeros(out["lang_embeds"].shape[0], out["lang_embeds"].shape[1], dtype=torch.bool)
    for i, l in enumerate(lang):
        mask[i, :l.shape[0]] = True
    out["lang_attn_mask"] = mask
    out["frames"] = [i["frames"] for i in instances]
    out["jitter"] = [i["jitter"] for i in instances]
    return out


def host_batch(ds: Dataset, B: int, np_rng, rng, generator=None, **kw) -> Dict[str, object]:
    """One micro-batch assembled on the host: the collated mapping with the fp64 arrays rounded once to fp32."""
    out = collate([ds.getitem(np_rng, rng, generator, **kw) for _ in range(B)])
    for k in ("states", "actions", "state_elem_mask", "state_norm", "lang_embeds"):
        out[k] = out[k].to(torch.float32)
    return out
