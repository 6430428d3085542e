"""Fine-tuning micro-batches drawn from device-resident episodes: what feeds `vlatouch.rdt_train.finetune`.

Replaces the reference's data path for `episode_*.h5` files (VLAConsumerDataset -> UnifiedVLADataset -> DataCollatorForVLAConsumerDataset):
  * `UnifiedVLADataset.parse_file` / `parse_file_state_only` (data/unified_vla_dataset_episode.py:250-495) re-read an episode for every
    sample; `EpisodeStore` reads every episode once, derives `qpos`, `first_idx` and the per-episode statistics on the host in fp64 and keeps
    them, the instruction embeddings and the camera frames on the device;
  * `compute_dataset_stat_episode.process_hdf5_dataset` is `EpisodeStore.dataset_stat`;
  * the random decisions of `get_item`, `parse_file` and `VLAConsumerDataset.__getitem__` (train/dataset.py:300-442) are `EpisodeStore.draw`,
    which consumes numpy's, `random`'s and torch's streams in the reference's order and returns small host records (`SamplePlan`);
  * the sample's arrays and the collator's stacks (train/dataset.py:460-533) are one vt_rdt_batch call (csrc/vt_rdt_data.hip) in
    `EpisodeStore.assemble`, whose result is the mapping `prepare_batch` / `sample_eval` take, with raw `frames`, `jitter` and `corrupt`.

Only precomputed instruction embeddings are built (`instruct_embeddings[0]`, the reference's use_precomp_lang_embed); `input_ids` and the
instruction masking draw are not.  Deviations from the reference are listed in INTEGRATION.md.  Everything except `upload` / `assemble` /
`batches` works without a GPU.
"""
from __future__ import annotations

import ctypes as C
import fnmatch
import os
import re
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import h5lite
from .imgaug import draw_image_aug

MIN_STEPS = 32                      # parse_file: "we drop too-short episodes"
STILL_EPS = 1e-2                    # parse_file: the first step whose qpos moved more than this from the first one
DROP_SHORT = "fewer than 32 steps"
DROP_STILL = "no step moves more than 1e-2 away from the first"
DROP_LATE = "first_idx - 1 >= N - int(horizon / 2): no step can be drawn"
# configs/state_vec.py as scripts/franka_model_eef.py assumes it: eef_pos x y z, eef_angle_0..5, right_gripper_open
DEFAULT_STATE_INDICES = (30, 31, 32, 33, 34, 35, 36, 37, 38, 10)
MASK_FREQ, MASK_STATE, MASK_ELEM, NOISE = 1, 2, 4, 8      # VT_RDT_* of include/vlatouch.h


def episode_number(path: str) -> int:
    m = re.search(r"episode_(\d+)", os.path.basename(path))
    return int(m.group(1)) if m else 0


def quat_to_ortho6d(quat: np.ndarray) -> np.ndarray:
    """xyzw quaternions [N, 4] -> the first two columns of their rotation matrices [N, 6] (column 0, then column 1), in fp64.  The
    reference (docs/test_6drot.py:110-116) reaches the same matrix through scipy's quaternion -> Euler -> matrix round trip."""
    q = np.asarray(quat, dtype=np.float64)
    x, y, z, w = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    c0 = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)], axis=1)
    c1 = np.stack([2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)], axis=1)
    return np.concatenate([c0, c1], axis=1)


def episode_qpos(ee_poses: np.ndarray, gripper_pos: np.ndarray) -> np.ndarray:
    """converted_ee_pose_with_gripper: [N, 10] = position | 6-D rotation | gripper (raw, not yet divided by 255)."""
    ee = np.asarray(ee_poses, dtype=np.float64)
    return np.concatenate([ee[:, :3], quat_to_ortho6d(ee[:, 3:]), np.asarray(gripper_pos, dtype=np.float64).reshape(-1, 1)], axis=-1)


def first_moving_index(qpos_raw: np.ndarray) -> Optional[int]:
    """parse_file:303-312, on qpos before the gripper is rescaled; None when the episode never moves."""
    idx = np.where(np.any(np.abs(qpos_raw - qpos_raw[0:1]) > STILL_EPS, axis=1))[0]
    return int(idx[0]) if len(idx) else None


class SamplePlan:
    """The random decisions of one sample.  episode: index among the store's kept episodes; step_id and action_id = step_id + 2; ctrl_masked /
    state_masked / elem_masked: the three condition masks; frame_idx [hist] and slot_valid [hist]: the frame each history slot shows and
    whether parse_file marks it valid; frame_valid [hist * cameras] (slot-major): valid, present and not masked, i.e. not the background;
    noise: the standard-normal draws at the state indices [S] or None, and noise_snr, the SNR in dB they are scaled for; jitter
    [hist * cameras]: ColorJitterParams or None per frame; corrupt [hist * cameras]: CorruptParams or None per frame."""
    __slots__ = ("episode", "step_id", "action_id", "ctrl_masked", "state_masked", "elem_masked", "frame_idx", "slot_valid", "frame_valid", "noise",
                 "noise_snr", "jitter", "corrupt")

    def __init__(self, episode, step_id, ctrl_masked, state_masked, elem_masked, frame_idx, slot_valid, frame_valid, noise=None, jitter=None,
                 action_id=None, noise_snr=None, corrupt=None):
        self.episode, self.step_id = int(episode), int(step_id)
        self.action_id = self.step_id + 2 if action_id is None else int(action_id)
        self.ctrl_masked, self.state_masked, self.elem_masked = bool(ctrl_masked), bool(state_masked), bool(elem_masked)
        self.frame_idx, self.slot_valid, self.frame_valid = list(frame_idx), list(slot_valid), list(frame_valid)
        self.noise = None if noise is None else np.asarray(noise, dtype=np.float64)
        self.noise_snr = None if noise is None else noise_snr
        self.jitter = [None] * len(self.frame_valid) if jitter is None else list(jitter)
        self.corrupt = [None] * len(self.frame_valid) if corrupt is None else list(corrupt)

    def flags(self) -> int:
        return (MASK_FREQ * self.ctrl_masked | MASK_STATE * self.state_masked | MASK_ELEM * self.elem_masked | NOISE * (self.noise is not None))

    def __repr__(self):
        return (f"SamplePlan(episode={self.episode}, step_id={self.step_id}, masked=(ctrl {self.ctrl_masked}, state {self.state_masked}, "
                f"elem {self.elem_masked}), frame_idx={self.frame_idx}, frame_valid={self.frame_valid}, noise={self.noise is not None})")


class _JpegCamera:
    """A camera's frames under frames="jpeg", on the host until upload(): the files' bytes and the one size and sampling they share."""
    __slots__ = ("files", "shape", "sampling", "nbytes")

    def __init__(self, files, h, w, sampling):
        self.files, self.shape, self.sampling = files, (len(files), h, w, 3), sampling
        self.nbytes = sum(len(f) for f in files)


class _Episode:
    __slots__ = ("path", "qpos", "first_idx", "stats", "lang", "frames", "has_cam")      # frames: host arrays until upload() moves them


class EpisodeStore:
    """paths_or_dir: a directory of `episode_<n>.h5` files or a sequence of paths, ordered by <n>.  dataset_name / dataset_names: this
    dataset and the list its index is looked up in (configs/finetune_datasets.json); control_freq: its frequency, or a mapping name ->
    frequency (configs/dataset_control_freq.json).  horizon = action_chunk_size, img_history_size and state_dim as configs/base.yaml.
    cameras: per camera slot a top-level key (a group `c` holding the array `c`, or a plain array dataset) or None for the always-missing
    camera; the order is the reference's (camera1, camera2, the missing left wrist).  frames="device" keeps the frames in HBM, at most
    `max_device_bytes` of them: episodes are taken whole, in order, and the first one that does not fit and every one after it stay in pinned
    host memory; frames="host" keeps all of them there.  Host frames reach the preprocessor as host arrays, which it stages and uploads in one
    copy per call (the staging copy is a host memcpy, so the store's pinning saves no copy, it only locks the pages).
    pad_and_resize: None, or the target size of the reference's `pad_and_resize_for_siglip` (vlatouch.imgprep; parse_file applies it to every
    frame it reads, data/unified_vla_dataset_episode.py:382-397): `upload` then resizes every camera frame once on the card
    (csrc/vt_area.hip), in chunks, and the store keeps the target x target frames, on the device or in pinned host memory as above;
    `max_device_bytes` counts the resized size, and `assemble` hands out the resized frames, so jitter and corruption act on them as
    train/dataset.py does.  The stage precedes every random decision: `dataset_stat` and the draws are the same with and without it.
    frames="jpeg" reads episode files written by `convert_episode_to_hdf5(..., images="jpeg")` (a camera group holds `<camera>_jpeg` and
    `<camera>_jpeg_offsets`) and keeps every camera as JPEG bitstreams in HBM, one `vlatouch.jpegdec.JpegFrames` per episode and camera;
    all frames of a camera must share size and sampling.  `assemble` decodes exactly the frames its plans mark valid, in one vt_jpeg_decode
    call per micro-batch (csrc/vt_jpegdec.hip, bit-identical to the Pillow decode the other modes store), and hands out views of that
    buffer; with pad_and_resize the decoded frames go through `pad_and_resize_device` in the same call (decoded at full size, resized per
    batch).  `max_device_bytes` counts the compressed size, and there is no pinned-host spill in this mode: an episode past the cap raises.
    jpeg_index_interval: the `index_interval` of the `JpegFrames`.  Everything that works without a GPU is the same as for a store of the
    decoded files."""

    def __init__(self, paths_or_dir, *, dataset_name: str, dataset_names: Sequence[str], control_freq, horizon: int = 64, img_history_size: int = 2,
                 state_dim: int = 128, state_indices: Optional[Sequence[int]] = None, cameras: Sequence[Optional[str]] = ("camera1", "camera2", None),
                 device="cuda", frames: str = "device", max_device_bytes: Optional[int] = None, pad_and_resize: Optional[int] = None,
                 jpeg_index_interval=None):
        if int(horizon) != horizon or horizon < 4:
            raise ValueError(f"EpisodeStore: horizon must be an integer >= 4, got {horizon!r} (below 4 the last drawable step has an empty action chunk)")
        if int(img_history_size) != img_history_size or img_history_size < 1:
            raise ValueError(f"EpisodeStore: img_history_size must be an integer >= 1, got {img_history_size!r}")
        idx = tuple(int(i) for i in (DEFAULT_STATE_INDICES if state_indices is None else state_indices))
        if len(idx) != 10 or len(set(idx)) != 10 or min(idx) < 0 or max(idx) >= state_dim:
            raise ValueError(f"EpisodeStore: state_indices must be 10 distinct columns of the {state_dim}-wide unified vector, got {idx}")
        if frames not in ("device", "host", "jpeg"):
            raise ValueError(f"EpisodeStore: frames must be 'device', 'host' or 'jpeg', got {frames!r}")
        self.jpeg_index_interval = jpeg_index_interval
        if max_device_bytes is not None and max_device_bytes < 0:
            raise ValueError("EpisodeStore: max_device_bytes must be >= 0")
        if pad_and_resize is not None and (isinstance(pad_and_resize, bool) or int(pad_and_resize) != pad_and_resize or pad_and_resize < 1):
            raise ValueError(f"EpisodeStore: pad_and_resize must be None or a positive target size, got {pad_and_resize!r}")
        self.pad_and_resize = None if pad_and_resize is None else int(pad_and_resize)
        dataset_names = list(dataset_names)
        if dataset_name not in dataset_names:
            raise ValueError(f"EpisodeStore: dataset_name {dataset_name!r} is not in dataset_names {dataset_names}")
        freq = control_freq[dataset_name] if hasattr(control_freq, "keys") else control_freq
        if int(freq) != freq or freq < 1:
            raise ValueError(f"EpisodeStore: control_freq must be a positive integer, got {freq!r}")
        if not cameras:
            raise ValueError("EpisodeStore: at least one camera slot is needed")
        self.dataset_name, self.dataset_names, self.data_idx, self.control_freq = dataset_name, dataset_names, dataset_names.index(dataset_name), int(freq)
        self.horizon, self.hist, self.state_dim, self.state_indices = int(horizon), int(img_history_size), int(state_dim), idx
        self.cameras, self.frames_mode, self.max_device_bytes = tuple(cameras), frames, max_device_bytes
        self.device = torch.device(device)
        if isinstance(paths_or_dir, (str, os.PathLike)):
            d = os.fspath(paths_or_dir)
            paths = [os.path.join(d, f) for f in fnmatch.filter(sorted(os.listdir(d)), "*.h5")]
        else:
            paths = [os.fspath(p) for p in paths_or_dir]
        self.paths = sorted(paths, key=episode_number)                 # natural_sort_filenames: stable, by the number alone
        self.report: Dict[str, str] = {}                               # dropped file -> reason
        self.episodes: List[_Episode] = []
        for p in self.paths:
            self._load(p)
        if not self.episodes:
            raise ValueError(f"EpisodeStore: no usable episode among {len(self.paths)} files: {self.report}")
        self.lengths = np.array([e.qpos.shape[0] - (e.first_idx - 1) for e in self.episodes])
        self.weights = self.lengths / np.sum(self.lengths)             # UnifiedVLADataset.episode_sample_weights
        self._stat = None
        self._dev = None                                                # the device tables, built by upload()
        self.resident_bytes = 0                                         # device bytes of tables and frames after upload()
        self.host_frame_bytes = 0                                       # frame bytes that stayed in pinned host memory

    # ---- loading
    def _camera(self, f, key):
        if key is None or key not in f:
            return None
        node = f[key]
        if isinstance(node, h5lite.Group):
            if self.frames_mode == "jpeg":
                return self._jpeg_camera(node, key)
            if key not in node:
                return None
            node = node[key]
        if self.frames_mode == "jpeg":
            raise ValueError(f"EpisodeStore: frames='jpeg' needs camera {key!r} as a group holding {key}_jpeg and {key}_jpeg_offsets "
                             "(convert_episode_to_hdf5(..., images='jpeg'))")
        a = np.asarray(node[...])
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise ValueError(f"EpisodeStore: camera {key!r} must be uint8 [N, H, W, 3], got {a.dtype} {a.shape}")
        if self.pad_and_resize is not None:
            from .imgprep import area_scale
            area_scale(max(a.shape[1], a.shape[2]), self.pad_and_resize)      # refuses, by name, a frame smaller than the target
        return a

    def _jpeg_camera(self, group, key):
        """The two datasets `convert_episode_to_hdf5(..., images="jpeg")` writes -> a `_JpegCamera`; headers are parsed, nothing is decoded."""
        from .jpegdec import SAMPLING_NAMES, parse_jpeg
        if f"{key}_jpeg" not in group or f"{key}_jpeg_offsets" not in group:
            if key in group:
                raise ValueError(f"EpisodeStore: camera {key!r} holds decoded pixels; frames='jpeg' reads files converted with images='jpeg'")
            return None
        data, off = np.asarray(group[f"{key}_jpeg"][...]), np.asarray(group[f"{key}_jpeg_offsets"][...])
        if data.dtype != np.uint8 or data.ndim != 1 or off.dtype != np.int64 or off.ndim != 1 or len(off) < 2 or off[0] != 0 or \
                off[-1] != len(data) or np.any(np.diff(off) <= 0):
            raise ValueError(f"EpisodeStore: camera {key!r}: {key}_jpeg must be uint8 [bytes] and {key}_jpeg_offsets int64 [N + 1], rising from 0 to its length")
        files = [data[off[k]:off[k + 1]].tobytes() for k in range(len(off) - 1)]
        kinds = {(r.h, r.w, r.sampling) for r in (parse_jpeg(f, k, header_only=True) for k, f in enumerate(files))}
        if len(kinds) > 1:
            raise ValueError(f"EpisodeStore: camera {key!r}: its frames differ in size or sampling: "
                             f"{sorted((h, w, SAMPLING_NAMES[s]) for h, w, s in kinds)}")
        (h, w, samp), = kinds
        if self.pad_and_resize is not None:
            from .imgprep import area_scale
            area_scale(max(h, w), self.pad_and_resize)
        return _JpegCamera(files, h, w, samp)

    def _load(self, path: str) -> None:
        with h5lite.File(path) as f:
            raw = episode_qpos(f["ee_poses"][...], f["gripper_pos"][...])
            n = raw.shape[0]
            name = os.path.basename(path)
            if n < MIN_STEPS:
                self.report[name] = DROP_SHORT
                return
            first = first_moving_index(raw)
            if first is None:
                self.report[name] = DROP_STILL
                return
            if first - 1 >= n - int(self.horizon / 2):
                self.report[name] = DROP_LATE
                return
            ep = _Episode()
            ep.path, ep.first_idx = path, first
            ep.qpos = qpos = raw / np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 255]])
            ep.stats = np.stack([np.std(qpos, axis=0), np.mean(qpos, axis=0), np.sqrt(np.mean(qpos ** 2, axis=0))])
            lang = np.asarray(f["instruct_embeddings"][...])[0]
            if lang.ndim != 2 or lang.shape[0] < 1:
                raise ValueError(f"EpisodeStore: {name}: instruct_embeddings[0] must be [L, D], got {lang.shape}")
            ep.lang = np.ascontiguousarray(lang, dtype=np.float32)
            ep.frames = [self._camera(f, c) for c in self.cameras]
            ep.has_cam = [a is not None for a in ep.frames]
            for c, a in zip(self.cameras, ep.frames):
                if a is not None and a.shape[0] < n:
                    raise ValueError(f"EpisodeStore: {name}: camera {c!r} has {a.shape[0]} frames for {n} steps")
            if self.episodes and ep.lang.shape[1] != self.episodes[0].lang.shape[1]:
                raise ValueError(f"EpisodeStore: {name}: instruction embedding width {ep.lang.shape[1]} differs from the first episode's")
            self.episodes.append(ep)

    def __len__(self) -> int:
        """UnifiedVLADataset.get_totol_episode_lengths: what VLAConsumerDataset.__len__ returns."""
        return int(np.sum(self.lengths))

    # ---- statistics
    def fill_in_state(self, values: np.ndarray) -> np.ndarray:
        uni = np.zeros(values.shape[:-1] + (self.state_dim,))
        uni[..., list(self.state_indices)] = values
        return uni

    def dataset_stat(self) -> dict:
        """compute_dataset_stat_episode.process_hdf5_dataset over the kept episodes, in order: the dict that file writes under the dataset's name."""
        if self._stat is not None:
            return self._stat
        EPS = 1e-8
        state_sum = state_sum_sq = z_state_sum = z_state_sum_sq = 0
        state_cnt, nz_state_cnt, state_max, state_min = 0, None, None, None
        for ep in self.episodes:
            states = self.fill_in_state(ep.qpos[ep.first_idx - 1:])
            z_states = states.copy()
            z_states[np.abs(states) <= EPS] = 0
            if nz_state_cnt is None:
                nz_state_cnt = np.zeros(states.shape[1])
            nz_state_cnt += np.sum(np.abs(states) > EPS, axis=0)
            state_sum += np.sum(states, axis=0)
            state_sum_sq += np.sum(states ** 2, axis=0)
            z_state_sum += np.sum(z_states, axis=0)
            z_state_sum_sq += np.sum(z_states ** 2, axis=0)
            state_cnt += states.shape[0]
            if state_max is None:
                state_max, state_min = np.max(states, axis=0), np.min(states, axis=0)
            else:
                state_max, state_min = np.maximum(state_max, np.max(states, axis=0)), np.minimum(state_min, np.min(states, axis=0))
        nz_state_cnt = np.maximum(nz_state_cnt, np.ones_like(nz_state_cnt))
        self._stat = {
            "dataset_name": self.dataset_name,
            "state_mean": (state_sum / state_cnt).tolist(),
            "state_std": np.sqrt(np.maximum((z_state_sum_sq / nz_state_cnt) - (z_state_sum / state_cnt) ** 2 * (state_cnt / nz_state_cnt),
                                            np.zeros_like(state_sum_sq))).tolist(),
            "state_min": state_min.tolist(),
            "state_max": state_max.tolist(),
        }
        return self._stat

    # ---- the draws
    def draw(self, B: int, *, np_rng, rng, generator: Optional[torch.Generator] = None, cond_mask_prob: float = 0.1, cam_ext_mask_prob: float = -1.0,
             state_noise_snr: Optional[float] = None, image_aug: bool = False, image_corrupt: bool = False, corrupt_rng=None) -> List[SamplePlan]:
        """B samples' decisions, one sample after the other, from np_rng (numpy's legacy interface: `np.random` or a RandomState), rng (`random`
        or a random.Random) and generator (torch; None = the global one), each consumed as the reference consumes its global stream:
        get_item's choice(p=weights), parse_file's randint(first_idx - 1, N - int(horizon / 2)), then __getitem__'s random() for ctrl_freq,
        normal(0, 1, (1, state_dim)) when state_noise_snr is set (all state_dim draws; the reference's normal(0, scale, shape) equals scale
        times these), random() for the state, random() for the element mask, one random() per frame that is valid and present (against
        cam_ext_mask_prob for camera 0 when that is >= 0, else cond_mask_prob) in slot-major order, and the augmentation draws
        (vlatouch.imgaug.draw_image_aug) when image_aug.  image_corrupt (only with image_aug): the frames whose augmentation type asks for
        it also get corruption parameters, drawn from corrupt_rng (a numpy `Generator`) alone, so every other decision and the three
        streams above are the same with and without it."""
        if int(B) != B or B < 1:
            raise ValueError(f"draw: B must be an integer >= 1, got {B!r}")
        if image_corrupt and not image_aug:
            raise ValueError("draw: image_corrupt needs image_aug (the corruption is one of the augmentation types)")
        if image_corrupt and corrupt_rng is None:
            raise ValueError("draw: image_corrupt needs a corrupt_rng (a numpy Generator)")
        ncam, hist = len(self.cameras), self.hist
        mask_probs = [cond_mask_prob] * ncam
        if cam_ext_mask_prob >= 0.0:
            mask_probs[0] = cam_ext_mask_prob
        plans = []
        for _ in range(B):
            e = int(np_rng.choice(len(self.episodes), p=self.weights))
            ep = self.episodes[e]
            n = ep.qpos.shape[0]
            step = int(np_rng.randint(ep.first_idx - 1, n - int(self.horizon / 2)))
            ctrl_masked = not (rng.random() > cond_mask_prob)
            noise = None
            if state_noise_snr is not None:
                noise = np.asarray(np_rng.normal(0.0, 1.0, (1, self.state_dim)))[0, list(self.state_indices)]
            state_masked = not (rng.random() > cond_mask_prob)
            elem_masked = not (rng.random() > cond_mask_prob)
            valid_len = min(step - (ep.first_idx - 1) + 1, hist)
            slot_valid = [i >= hist - valid_len for i in range(hist)]
            frame_idx = [max(step - hist + 1 + i, 0) for i in range(hist)]
            frame_valid = []
            for i in range(hist):
                for j in range(ncam):
                    frame_valid.append(bool(slot_valid[i] and ep.has_cam[j] and rng.random() > mask_probs[j]))
            jitter = corrupt = None
            if image_aug and image_corrupt:
                jitter, corrupt = draw_image_aug(frame_valid, rng=rng, generator=generator, corrupt_rng=corrupt_rng)
            elif image_aug:
                jitter = draw_image_aug(frame_valid, rng=rng, generator=generator)
            plans.append(SamplePlan(e, step, ctrl_masked, state_masked, elem_masked, frame_idx, slot_valid, frame_valid, noise, jitter,
                                    noise_snr=state_noise_snr, corrupt=corrupt))
        return plans

    def check_plans(self, plans: Sequence[SamplePlan]) -> None:
        """Refuse a plan that does not fit the tables, on the host, before anything is launched."""
        if len(plans) < 1:
            raise ValueError("assemble: no plans")
        nfr = self.hist * len(self.cameras)
        snrs: dict = {}
        for k, p in enumerate(plans):
            if not 0 <= p.episode < len(self.episodes):
                raise ValueError(f"assemble: plan {k}: episode {p.episode} is not one of the {len(self.episodes)} kept episodes")
            ep = self.episodes[p.episode]
            n = ep.qpos.shape[0]
            lo, hi = ep.first_idx - 1, n - int(self.horizon / 2)
            if not lo <= p.step_id < hi:
                raise ValueError(f"assemble: plan {k}: step_id {p.step_id} is outside [{lo}, {hi}) of episode {p.episode} ({n} steps)")
            if p.action_id != p.step_id + 2 or p.action_id > n - 1:
                raise ValueError(f"assemble: plan {k}: action_id {p.action_id} must be step_id + 2 = {p.step_id + 2} and a row of the episode")
            if p.noise is not None and p.noise.shape != (len(self.state_indices),):
                raise ValueError(f"assemble: plan {k}: noise must hold {len(self.state_indices)} draws, got {p.noise.shape}")
            if p.noise is not None and (p.noise_snr is None or p.noise_snr != snrs.setdefault("snr", p.noise_snr)):
                raise ValueError(f"assemble: plan {k}: noise draws need a noise_snr, the same for every noised plan of a batch (got {p.noise_snr!r})")
            if len(p.frame_idx) != self.hist or len(p.frame_valid) != nfr or len(p.jitter) != nfr or len(p.corrupt) != nfr:
                raise ValueError(f"assemble: plan {k}: {self.hist} frame indices and {nfr} frame flags / jitter / corrupt entries expected")
            for q, c in enumerate(p.corrupt):
                if c is not None and not p.frame_valid[q]:
                    raise ValueError(f"assemble: plan {k}: frame {q} is missing and cannot be corrupted")
            for i, fi in enumerate(p.frame_idx):
                if not 0 <= fi < n:
                    raise ValueError(f"assemble: plan {k}: frame index {fi} of slot {i} is outside the episode")
            for q, v in enumerate(p.frame_valid):
                if v and not ep.has_cam[q % len(self.cameras)]:
                    raise ValueError(f"assemble: plan {k}: frame {q} is marked valid but episode {p.episode} has no camera {q % len(self.cameras)}")

    # ---- the device half
    def upload(self) -> "EpisodeStore":
        """Build the device tables and move the frames (once; `assemble` calls it)."""
        if self._dev is not None:
            return self
        dev = L.require_gpu(self.device)
        eps = self.episodes
        S = len(self.state_indices)
        i32 = lambda a: torch.tensor(a, dtype=torch.int32).to(dev)
        col_map = np.full(self.state_dim, -1, dtype=np.int32)
        col_map[list(self.state_indices)] = np.arange(S, dtype=np.int32)
        mean = np.asarray(self.dataset_stat()["state_mean"], dtype=np.float64)[list(self.state_indices)]
        d = {
            "qpos": torch.from_numpy(np.ascontiguousarray(np.concatenate([e.qpos for e in eps], axis=0))).to(dev),
            "ep_off": i32(np.concatenate([[0], np.cumsum([e.qpos.shape[0] for e in eps])])),
            "stats": torch.from_numpy(np.ascontiguousarray(np.stack([e.stats for e in eps]))).to(dev),
            "mean": torch.from_numpy(np.ascontiguousarray(mean)).to(dev),
            "col_map": torch.from_numpy(col_map).to(dev),
            "lang": torch.from_numpy(np.ascontiguousarray(np.concatenate([e.lang for e in eps], axis=0))).to(dev),
            "lang_off": i32(np.concatenate([[0], np.cumsum([e.lang.shape[0] for e in eps])])),
        }
        self.resident_bytes = sum(t.numel() * t.element_size() for t in d.values())
        if self.frames_mode == "jpeg":
            d["frames"] = self._upload_jpeg(dev)
            self._dev = d
            return self
        budget = 0 if self.frames_mode == "host" else self.max_device_bytes
        frames = []
        T = self.pad_and_resize
        kept = (lambda a: a.nbytes) if T is None else (lambda a: a.shape[0] * 3 * T * T)      # the bytes the store keeps of a camera's frames
        for e in eps:                                                  # decided per episode, in order: the first one past the cap and all after it stay on the host
            need = sum(kept(a) for a in e.frames if a is not None)
            if budget is not None:
                budget = budget - need if need <= budget else -1      # -1: the cap is reached, nothing more goes to the device
            per_cam = []
            for a in e.frames:
                if a is None:
                    per_cam.append(None)
                elif T is not None:
                    on_dev = budget is None or budget >= 0
                    t = self._resized(a, T, dev, on_dev)
                    if on_dev:
                        per_cam.append(t)
                        self.resident_bytes += kept(a)
                    else:
                        per_cam.append(t.numpy())
                        d.setdefault("pinned", []).append(t)
                        self.host_frame_bytes += kept(a)
                elif budget is None or budget >= 0:
                    per_cam.append(torch.from_numpy(a).to(dev))
                    self.resident_bytes += a.nbytes
                else:
                    # Pinned as a resident host store should be; note that DevicePreprocessor still copies each host frame into its own pinned
                    # staging buffer before its one upload, so the pinning saves no copy today: it only keeps the pages locked.
                    pinned = torch.from_numpy(a).pin_memory()
                    per_cam.append(pinned.numpy())
                    d.setdefault("pinned", []).append(pinned)
                    self.host_frame_bytes += a.nbytes
            frames.append(per_cam)
            e.frames = None                                            # the host copies are not kept
        d["frames"] = frames
        self._dev = d
        return self

    def _upload_jpeg(self, dev) -> list:
        """One `JpegFrames` per episode and camera; resident_bytes counts what each keeps (streams + index + tables)."""
        from .jpegdec import DEFAULT_INDEX_INTERVAL, JpegFrames
        iv = DEFAULT_INDEX_INTERVAL if self.jpeg_index_interval is None else self.jpeg_index_interval
        frames, used = [], 0
        for k, e in enumerate(self.episodes):
            per_cam = []
            for c, a in zip(self.cameras, e.frames):
                if a is None:
                    per_cam.append(None)
                    continue
                try:
                    jf = JpegFrames(a.files, dev, iv)
                except ValueError as err:
                    raise ValueError(f"EpisodeStore: {os.path.basename(e.path)}, camera {c!r}: {err}") from None
                used += jf.nbytes
                if self.max_device_bytes is not None and used > self.max_device_bytes:
                    raise ValueError(f"EpisodeStore: episode {k} ({os.path.basename(e.path)}) brings the compressed frames to {used} bytes, past "
                                     f"max_device_bytes = {self.max_device_bytes}; frames='jpeg' has no pinned-host spill")
                per_cam.append(jf)
            frames.append(per_cam)
            e.frames = None
        self.resident_bytes += used
        return frames

    def _decoded_frames(self, plans) -> list:
        """frames="jpeg": the frames the plans mark valid, decoded in one vt_jpeg_decode call (and resized in one vt_area_resize call under
        pad_and_resize) -> B lists of hist * cameras entries, views of that call's buffer or None."""
        from .jpegdec import decode_many
        ncam, jfs = len(self.cameras), self._dev["frames"]
        where = [(k, q) for k, p in enumerate(plans) for q, v in enumerate(p.frame_valid) if v]
        res = [[None] * len(p.frame_valid) for p in plans]
        if not where:
            return res
        got = decode_many([(jfs[plans[k].episode][q % ncam], plans[k].frame_idx[q // ncam]) for k, q in where])
        if self.pad_and_resize is not None:
            from .imgprep import pad_and_resize_device
            got = pad_and_resize_device(got, self.pad_and_resize)
        for (k, q), t in zip(where, got):
            res[k][q] = t
        return res

    @staticmethod
    def _resized(a: np.ndarray, T: int, dev, on_dev: bool) -> torch.Tensor:
        """`pad_and_resize_for_siglip` of a camera's frames [N, H, W, 3] on the card, in chunks of at most 64 MiB of raw frames -> uint8
        [N, T, T, 3], on the device or (on_dev False) in pinned host memory."""
        from .imgprep import pad_and_resize_device
        n = a.shape[0]
        out = torch.empty((n, T, T, 3), dtype=torch.uint8, device=dev) if on_dev else torch.empty((n, T, T, 3), dtype=torch.uint8).pin_memory()
        chunk = max(1, (64 << 20) // max(1, a[0].nbytes))
        for i in range(0, n, chunk):
            raw = torch.from_numpy(a[i:i + chunk]).to(dev)
            got = pad_and_resize_device(list(raw), T, out=out[i:i + chunk] if on_dev else None)
            if not on_dev:
                out[i:i + chunk].copy_(got)
        return out

    def assemble(self, plans: Sequence[SamplePlan]) -> dict:
        """plans -> the collator's mapping on the device: states [B, 1, A], actions [B, H, A], state_elem_mask [B, A], state_norm [B, A] (fp32),
        ctrl_freqs [B] int64, data_indices (list), lang_embeds [B, Lmax, D] zero padded, lang_attn_mask [B, Lmax] bool, frames (B lists of
        hist * cameras entries, slot-major: a uint8 [H, W, 3] view into the resident episode (frames="jpeg": into the buffer this call
        decoded), a host array for an episode kept in pinned memory, or None for the background), jitter (B lists, or None when no plan carries any) and, where a plan carries any, corrupt."""
        plans = list(plans)
        self.check_plans(plans)
        snr = next((p.noise_snr for p in plans if p.noise is not None), None)
        noise_div = float(np.sqrt(10 ** (snr / 10))) if snr is not None else 1.0      # train/dataset.py:332
        self.upload()
        d, dev = self._dev, self.device
        B, S, A, H = len(plans), len(self.state_indices), self.state_dim, self.horizon
        D = self.episodes[0].lang.shape[1]
        Lmax = max(self.episodes[p.episode].lang.shape[0] for p in plans)
        buf = np.zeros(16 * B + 8 * B * S, dtype=np.uint8)
        hdr, z = buf[:16 * B].view(np.int32).reshape(B, 4), buf[16 * B:].view(np.float64).reshape(B, S)
        for k, p in enumerate(plans):
            hdr[k, :3] = (p.episode, p.step_id, p.flags())
            if p.noise is not None:
                z[k] = p.noise
        plan_dev = torch.from_numpy(buf).to(dev)                       # the call's one upload
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = {"states": f32(B, 1, A), "actions": f32(B, H, A), "state_elem_mask": f32(B, A), "state_norm": f32(B, A),
               "ctrl_freqs": torch.empty(B, dtype=torch.int64, device=dev), "lang_embeds": f32(B, Lmax, D),
               "lang_attn_mask": torch.empty((B, Lmax), dtype=torch.bool, device=dev)}
        L.check(L.lib().vt_rdt_batch(L.ptr(d["qpos"]), L.ptr(d["ep_off"]), L.ptr(d["stats"]), L.ptr(d["mean"]), L.ptr(d["col_map"]), L.ptr(d["lang"]),
                                     L.ptr(d["lang_off"]), len(self.episodes), S, A, H, D, Lmax, self.control_freq, C.c_double(noise_div),
                                     L.ptr(plan_dev), B, L.ptr(out["states"]), L.ptr(out["actions"]), L.ptr(out["state_elem_mask"]),
                                     L.ptr(out["state_norm"]), L.ptr(out["ctrl_freqs"]), L.ptr(out["lang_embeds"]), L.ptr(out["lang_attn_mask"]),
                                     L.stream_ptr(dev)), "vt_rdt_batch")
        ncam = len(self.cameras)
        out["data_indices"] = [self.data_idx] * B
        out["frames"] = self._decoded_frames(plans) if self.frames_mode == "jpeg" else [[d["frames"][p.episode][q % ncam][p.frame_idx[q // ncam]] if v else None for q, v in enumerate(p.frame_valid)] for p in plans]
        out["jitter"] = [list(p.jitter) for p in plans] if any(j is not None for p in plans for j in p.jitter) else None
        if any(c is not None for p in plans for c in p.corrupt):
            out["corrupt"] = [list(p.corrupt) for p in plans]
        return out

    def plan_batches(self, batch_size: int, rank: int = 0, world_size: int = 1, **draw_kwargs) -> Iterator[List[SamplePlan]]:
        """The plans of `batches`, on the host: an endless iterator of draw(batch_size, **draw_kwargs).  With world_size = W > 1 it yields
        micro-batches rank, rank + W, ... of that one-process stream (the round-robin of accelerate's default batch sharding): the other
        ranks' decisions are drawn, so that every rank's random streams stay those of the one-process run, and dropped.  The ranks must
        seed np_rng, rng and the generator alike."""
        if int(world_size) != world_size or world_size < 1 or int(rank) != rank or not 0 <= rank < world_size:
            raise ValueError(f"plan_batches: rank must be in [0, world_size), got rank={rank!r}, world_size={world_size!r}")
        i = 0
        while True:
            plans = self.draw(batch_size, **draw_kwargs)
            if i % world_size == rank:
                yield plans
            i += 1

    def batches(self, batch_size: int, rank: int = 0, world_size: int = 1, **draw_kwargs) -> Iterator[dict]:
        """An endless iterator of micro-batches: plan_batches(batch_size, rank, world_size, **draw_kwargs) then assemble, which only this
        rank's micro-batches reach.  A W-rank run with gradient_accumulation_steps k so consumes exactly the samples of a one-rank run with
        k W.  A sample loader is the same call with cond_mask_prob=0, state_noise_snr=None, image_aug=False."""
        for plans in self.plan_batches(batch_size, rank, world_size, **draw_kwargs):
            yield self.assemble(plans)
