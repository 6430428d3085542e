"""Controller-training batches drawn from device-resident episodes: what feeds `DiffusionControllerTrainer.train` / `LSTMControllerTrainer.train`
without the per-step host work of `ControllerDataset.__getitem__` and without running the frozen DINOv2 tower again every step.

`ControllerStore` reads every episode of a `ControllerDataset` once (one episode alive at a time), derives the pose table on the host in fp64
as `vlatouch.eval.make_sample` does, encodes every frame an indexed window can show ONCE through the controller's own `DINOv2Encoder` and
keeps on the device: `pose10`, `vla`, `forces`, `ep_off`, the CLS features `feat` and the frames' byte sums `pix_sum`.  The frames themselves
are dropped after encoding.  `assemble` turns a list of dataset indices into the mapping `_prepare_batch_for_diffusion` / `_prepare_batch`
return, with one upload of the plan and one `vt_ctrl_batch` call (csrc/vt_ctrl_data.hip).

The reference's encoder decides whether to apply the ImageNet normalisation from the mean of the WHOLE call's batch (visual_encoder.py:78,100),
so a frame's feature depends on the frames it shares a batch with.  The store therefore keeps both features of every frame (mode 0: off,
mode 1: on) and the kernel takes the reference's decision per batch and camera from the exact byte sums: normalise iff
2 * sum_b pix_sum[frame_b] >= 255 * B * P (`norm_decision` states it in NumPy).  It differs from the encoder's fp32 mean only when the batch
mean is within fp32 rounding of 0.5.  What else differs from the dataset path: the store hands the encoder uint8 frames, read as
u8 * (1/255), where the dataset hands over float32(u8) / 255: at most 1 ulp per pixel before the patch rounding.

`loader` yields `StoreBatch` objects in the order, and with the random draws, of `torch.utils.data.DataLoader(dataset, batch_size,
shuffle=..., drop_last=...)`; `ControllerStoreModule` wraps a `ControllerDataModule` so that the two trainers take it unchanged.
Everything except the device build and `assemble` works without a GPU (`build=False`).
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from . import _lib as L

LAYOUTS = {"bridge": 0, "lstm": 1}      # VT_CTRL_BRIDGE / VT_CTRL_LSTM of include/vlatouch.h
PADDING_FACTOR = 1.4                     # normalize_actions' default, which both trainers use
SKIP_NO_WINDOW = "no window is indexed in this file"
CAMERAS = ("camera1_resized", "camera2_resized")


def norm_decision(pix_sums, bytes_per_frame: int) -> bool:
    """The batch's ImageNet-normalisation decision from its frames' byte sums, in whole numbers: mean(u8 / 255) >= 0.5."""
    sums = [int(s) for s in np.asarray(pix_sums).reshape(-1)]
    return 2 * sum(sums) >= 255 * len(sums) * int(bytes_per_frame)


class StoreBatch:
    """What a store loader yields in place of a collated dict: the store and the dataset indices [B] (int64, on the host)."""
    __slots__ = ("store", "index")

    def __init__(self, store: "ControllerStore", index: torch.Tensor):
        self.store, self.index = store, index

    def __len__(self) -> int:
        return int(self.index.shape[0])


class StoreLoader:
    """DataLoader(dataset, batch_size, shuffle, drop_last) without a `generator`, restated: per epoch the DataLoader takes one int64
    `random_()` from torch's global generator (its base seed); a RandomSampler then takes one more as the seed of a fresh generator, whose
    `randperm(n)` is the epoch's order."""

    def __init__(self, store: "ControllerStore", batch_size: int, shuffle: bool, drop_last: bool):
        if int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f"StoreLoader: batch_size must be an integer >= 1, got {batch_size!r}")
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), bool(shuffle), bool(drop_last)

    def __len__(self) -> int:
        n = len(self.store)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self) -> Iterator[StoreBatch]:
        torch.empty((), dtype=torch.int64).random_()                   # the DataLoader iterator's base seed: drawn, not used
        return self._batches()

    def _batches(self) -> Iterator[StoreBatch]:
        n, bs = len(self.store), self.batch_size
        if self.shuffle:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            g = torch.Generator()
            g.manual_seed(seed)
            order = torch.randperm(n, generator=g)
        else:
            order = torch.arange(n)
        for i in range(0, n, bs):
            idx = order[i:i + bs]
            if self.drop_last and idx.shape[0] < bs:
                return
            yield StoreBatch(self.store, idx)


class ControllerStore:
    """dataset: a `ControllerDataset` (`use_images=False` is enough): the store takes its `file_paths`, `episode_indices`, `context_frames`,
    `horizon` and `stats`, so store index i is dataset index i.  encoder: the controller's `image_encoder`; `assemble` refuses a controller
    whose encoder is another object.  stats: other statistics than the dataset's own (a validation store normalises with the training
    files').  encode_chunk: frames per camera and encoder call; chunks never span two episodes.  max_device_bytes: the build raises when the
    tables need more (nothing can stay behind: a batch may touch every table).  build=False leaves the device half to the first `assemble`."""

    def __init__(self, dataset, encoder, *, encode_chunk: int = 64, max_device_bytes: Optional[int] = None, stats=None, device=None,
                 build: bool = True):
        if int(encode_chunk) != encode_chunk or encode_chunk < 1:
            raise ValueError(f"ControllerStore: encode_chunk must be an integer >= 1, got {encode_chunk!r}")
        if max_device_bytes is not None and max_device_bytes < 0:
            raise ValueError("ControllerStore: max_device_bytes must be >= 0")
        self.file_paths = list(dataset.file_paths)
        self.episode_indices = [(int(e), int(s)) for e, s in dataset.episode_indices]
        self.context_frames, self.horizon = int(dataset.context_frames), int(dataset.horizon)
        if self.context_frames < 1 or self.horizon < 1:
            raise ValueError(f"ControllerStore: context_frames and horizon must be >= 1, got {self.context_frames}, {self.horizon}")
        self.stats = dataset.stats if stats is None else stats
        if self.stats is None:
            raise ValueError("ControllerStore: the dataset has no statistics (no episode file)")
        self.encoder, self.encode_chunk, self.max_device_bytes = encoder, int(encode_chunk), max_device_bytes
        self.device = torch.device(device if device is not None else getattr(encoder, "device", "cuda"))
        self._index = np.asarray(self.episode_indices, dtype=np.int32).reshape(-1, 2)
        self._dev: Optional[Dict[str, torch.Tensor]] = None
        self._report: dict = {}
        if build:
            self.upload()

    def __len__(self) -> int:
        return len(self.episode_indices)

    # ---- the device half
    def _stats_table(self) -> np.ndarray:
        """[4][10] fp32 = expert mins | expert maxs | vla mins | vla maxs, rounded as `normalize_actions` passes them to the kernel."""
        rows = []
        for k in ("action_mins", "action_maxs", "vla_mins", "vla_maxs"):
            v = self.stats[k]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            rows.append(v.astype(np.float32).reshape(10))
        return np.ascontiguousarray(np.stack(rows))

    def _encode(self, cams, rows, feat, pix, P) -> None:
        """One episode's used frames through the encoder, `encode_chunk` at a time, with the normalisation off and on; and their byte sums."""
        dev, lib = self.device, L.lib()
        for i in range(0, len(rows), self.encode_chunk):
            sel = rows[i:i + self.encode_chunk]
            # NumPy uint8 frames take the encoder's `u8 * (1/255)` path whatever the chunk's maximum (a torch tensor would be left unscaled when
            # its maximum is <= 1, e.g. a chunk of black frames with one stray count)
            chunk = [np.ascontiguousarray(c[sel]) for c in cams]
            where = torch.as_tensor(sel, dtype=torch.int64, device=dev)
            for mode, norm_mode in ((0, L.IMGNORM_OFF), (1, L.IMGNORM_ON)):
                f = self.encoder.forward_many(chunk, norm_mode=norm_mode)          # [2, n, dv]
                feat[:, where, mode] = f
            for c in range(2):
                frames = torch.from_numpy(chunk[c]).to(dev)
                sums = torch.empty(len(sel), dtype=torch.int64, device=dev)        # the kernel's uint64; a frame's sum is far below 2^63
                L.check(lib.vt_ctrl_pixsum(L.ptr(frames), C.c_longlong(P), len(sel), L.ptr(sums), L.stream_ptr(dev)), "vt_ctrl_pixsum")
                pix[c, where] = sums

    def _pass(self) -> dict:
        """Every file once, one episode alive at a time -> the tables (device tensors) of this pass."""
        from . import eval as ev
        dev = self.device
        cf, h = self.context_frames, self.horizon
        dv = int(self.encoder.hidden_size)
        starts_of: Dict[int, list] = {}
        for e, s in self.episode_indices:
            starts_of.setdefault(e, []).append(s)
        pose, vla, forces, feats, pixs, n_rows = [], [], [], [], [], []
        skipped, shape, encoded = {}, None, 0
        for e, path in enumerate(self.file_paths):
            if e not in starts_of:
                skipped[path] = SKIP_NO_WINDOW
                n_rows.append(0)
                continue
            ep = ev.load_episode(path, images=True)
            p10 = ev.converted_ee_pose_with_gripper(ep)                # fp64, gripper not divided
            n = p10.shape[0]
            va = np.array(ep["vla_action"], dtype=np.float64)
            fo = np.asarray(ep["gelsight_force/forces"])
            if va.ndim != 3 or va.shape[0] < n or va.shape[2] != 10 or va.shape[1] < h:
                raise ValueError(f"ControllerStore: {path}: vla_action must be [>= {n}, >= {h}, 10], got {va.shape}")
            if fo.ndim != 2 or fo.shape[0] < n:
                raise ValueError(f"ControllerStore: {path}: forces must be [>= {n}, Fd], got {fo.shape}")
            if max(starts_of[e]) + cf + h > n or min(starts_of[e]) < 0:
                raise ValueError(f"ControllerStore: {path}: an indexed window leaves the episode's {n} frames")
            cams = []
            for k in CAMERAS:
                if k not in ep:
                    raise ValueError(f"ControllerStore: {path}: no {k!r} stream")
                a = np.asarray(ep[k])
                if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[0] < n or a.shape[1] != a.shape[2]:
                    raise ValueError(f"ControllerStore: {path}: {k!r} must be square uint8 frames [>= {n}, R, R, 3], got {a.dtype} {a.shape}")
                if shape is None:
                    shape = a.shape[1:]
                if a.shape[1:] != shape:
                    raise ValueError(f"ControllerStore: {path}: {k!r} frames are {a.shape[1:]}, earlier ones {shape} (a batch has one frame size)")
                cams.append(a)
            pose.append(p10)
            vla.append(va[:n])
            forces.append(np.asarray(fo[:n], dtype=np.float32))
            n_rows.append(n)
            feat = torch.zeros(2, n, 2, dv, dtype=torch.float32, device=dev)
            pix = torch.zeros(2, n, dtype=torch.int64, device=dev)
            used = sorted({s + cf - 1 for s in starts_of[e]})
            self._encode(cams, used, feat, pix, int(np.prod(shape)))
            encoded += len(used)
            feats.append(feat)
            pixs.append(pix)
            del ep, cams
        if not pose:
            raise ValueError(f"ControllerStore: no window in any of {len(self.file_paths)} files")
        hv, fd = {v.shape[1] for v in vla}, {f.shape[1] for f in forces}
        if len(hv) != 1 or len(fd) != 1:
            raise ValueError(f"ControllerStore: the files disagree on the VLA chunk length {sorted(hv)} or the force width {sorted(fd)}")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d = {
            "pose10": up(np.concatenate(pose, axis=0)),
            "vla": up(np.concatenate(vla, axis=0)),
            "forces": up(np.concatenate(forces, axis=0)),
            "ep_off": up(np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int32)),
            "feat": torch.cat(feats, dim=1).contiguous(),
            "pix_sum": torch.cat(pixs, dim=1).contiguous(),
            "stats": up(self._stats_table()),
        }
        self._n_rows = np.asarray(n_rows, dtype=np.int64)
        self._bytes_per_frame = int(np.prod(shape))
        self._frame_shape = tuple(int(x) for x in shape)
        self._report = {"skipped": skipped, "episodes": len(pose), "rows": int(sum(n_rows)), "frames_encoded": encoded}
        return d

    def upload(self) -> "ControllerStore":
        """Build the device tables (once; the constructor calls it unless build=False, and `assemble` does otherwise)."""
        if self._dev is not None:
            return self
        if self.encoder is None:
            raise ValueError("ControllerStore: an encoder is needed to build the feature table")
        self.device = L.require_gpu(self.device)
        t0 = time.perf_counter()
        rebuilt = 0
        while True:
            engine = self.encoder.engine
            d = self._pass()
            if self.encoder.engine is engine:
                break
            # the encoder's range guard rebuilt its engine in bf16 part-way: every chunk again, so that one store never mixes two precisions
            rebuilt += 1
            del d
            if rebuilt > 2:
                raise RuntimeError("ControllerStore: the encoder keeps rebuilding its engine")
        torch.cuda.synchronize(self.device)
        per_table = {k: int(t.numel() * t.element_size()) for k, t in d.items()}
        total = sum(per_table.values())
        if self.max_device_bytes is not None and total > self.max_device_bytes:
            del d
            raise ValueError(f"ControllerStore: the tables need {total} bytes on the device, max_device_bytes allows {self.max_device_bytes}")
        self._dev = d
        self._report.update({"resident_bytes": per_table, "total_bytes": total, "build_seconds": time.perf_counter() - t0,
                             "engine_rebuilds": rebuilt})
        return self

    def report(self) -> dict:
        """Resident bytes per table and in total, the build time, the files skipped (path -> reason), rows and frames encoded."""
        return dict(self._report)

    def check_index(self, index) -> np.ndarray:
        """Refuse an index that does not fit the tables, on the host, before anything is launched.  Returns the plan [B][2] int32."""
        idx = index.detach().cpu().numpy() if isinstance(index, torch.Tensor) else np.asarray(index)
        if idx.ndim != 1 or idx.shape[0] < 1 or idx.dtype.kind not in "iu":
            raise ValueError(f"assemble: index must be a 1-D integer tensor or list with at least one entry, got {idx.dtype} {idx.shape}")
        if idx.min() < 0 or idx.max() >= len(self):
            raise ValueError(f"assemble: index {int(idx.min() if idx.min() < 0 else idx.max())} is outside the store's {len(self)} windows")
        plan = np.ascontiguousarray(self._index[idx.astype(np.int64)])
        if self._dev is not None:
            n = self._n_rows[plan[:, 0]]
            bad = np.nonzero((plan[:, 1] < 0) | (plan[:, 1] + self.context_frames + self.horizon > n))[0]
            if len(bad):
                k = int(bad[0])
                raise ValueError(f"assemble: entry {k}: window start {int(plan[k, 1])} leaves episode {int(plan[k, 0])} ({int(n[k])} frames)")
        return plan

    def assemble(self, index, *, layout: str, kin: int, use_force: bool = True) -> Dict[str, torch.Tensor]:
        """index [B] (int64 tensor or list of store indices) -> the trainer's mapping on the device.  layout "bridge": obs_in [B, kin],
        expert_act, vla_act [B, h, 10], forces [B, h, Fd], current_force [B, Fd]; layout "lstm": obs_in (no force columns), expert_act,
        vla_act, forces (rows cf - 1 .. cf + h - 2).  Both carry norm_flags [2], the two cameras' normalisation decisions (1.0 = on).
        One upload (the plan) and one vt_ctrl_batch call; no host read, no synchronisation."""
        if layout not in LAYOUTS:
            raise ValueError(f"assemble: layout must be 'bridge' or 'lstm', got {layout!r}")
        self.upload()
        plan = self.check_index(index)
        d, dev = self._dev, self.device
        B, h = plan.shape[0], self.horizon
        dv, fd, hv = d["feat"].shape[3], d["forces"].shape[1], d["vla"].shape[1]
        fdo = fd if (layout == "bridge" and use_force) else 0
        if int(kin) < 2 * dv + 10 + fdo:
            raise ValueError(f"assemble: kin = {kin} is smaller than the observation row 2 * {dv} + 10 + {fdo}")
        plan_dev = torch.from_numpy(plan).to(dev)                      # the call's one upload
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = {"obs_in": f32(B, int(kin)), "expert_act": f32(B, h, 10), "vla_act": f32(B, h, 10), "forces": f32(B, h, fd)}
        if layout == "bridge":
            out["current_force"] = f32(B, fd)
        out["norm_flags"] = f32(2)
        L.check(L.lib().vt_ctrl_batch(L.ptr(d["pose10"]), L.ptr(d["vla"]), L.ptr(d["forces"]), L.ptr(d["ep_off"]), L.ptr(d["feat"]), L.ptr(d["pix_sum"]),
                                      len(self.file_paths), C.c_longlong(d["pose10"].shape[0]), hv, fd, dv, C.c_longlong(self._bytes_per_frame),
                                      L.ptr(d["stats"]), C.c_float(PADDING_FACTOR), self.context_frames, h, LAYOUTS[layout], int(bool(use_force)),
                                      L.ptr(plan_dev), B, L.ptr(out["obs_in"]), int(kin), L.ptr(out["expert_act"]), L.ptr(out["vla_act"]),
                                      L.ptr(out["forces"]), L.ptr(out.get("current_force")), L.ptr(out["norm_flags"]), L.stream_ptr(dev)),
                "vt_ctrl_batch")
        return out

    def assemble_for(self, controller, index, *, layout: str, kin: int, use_force: bool = True, context_frames: Optional[int] = None):
        """`assemble` for a trainer: refuses a controller whose `image_encoder` is not the object the features were encoded with, and a
        window length other than the one the trainer slices with."""
        if getattr(controller, "image_encoder", None) is not self.encoder:
            raise ValueError("ControllerStore: the features were encoded with another encoder object than this controller's image_encoder")
        if context_frames is not None and int(context_frames) != self.context_frames:
            raise ValueError(f"ControllerStore: the store's windows have context_frames = {self.context_frames}, the trainer uses {context_frames}")
        return self.assemble(index, layout=layout, kin=kin, use_force=use_force)

    def loader(self, batch_size: int, shuffle: bool, drop_last: bool) -> StoreLoader:
        return StoreLoader(self, batch_size, shuffle, drop_last)


class ControllerStoreModule:
    """A `ControllerDataModule` fed from stores: the same files, the same (already made) train / validation split and the same `stats`,
    which both stores normalise with.  `DiffusionControllerTrainer(ctrl, module)` / `LSTMControllerTrainer(ctrl, module)` and their
    `.train(module, ...)` take it in place of the data module."""

    def __init__(self, data_module, controller, **store_kw):
        self.data_module = data_module
        self.batch_size = data_module.batch_size
        self.stats = data_module.stats
        self.train_dataset, self.val_dataset = data_module.train_dataset, data_module.val_dataset
        encoder = getattr(controller, "image_encoder", None)
        self.train_store = ControllerStore(self.train_dataset, encoder, stats=self.stats, **store_kw)
        self.val_store = ControllerStore(self.val_dataset, encoder, stats=self.stats, **store_kw)

    def train_dataloader(self) -> StoreLoader:
        return self.train_store.loader(self.batch_size, shuffle=True, drop_last=True)

    def val_dataloader(self) -> StoreLoader:
        return self.val_store.loader(self.batch_size, shuffle=False, drop_last=False)
