"""Camera frames -> SigLIP `pixel_values` on the device (csrc/vt_imgprep.hip), bit-identical to the PIL path of
`scripts.franka_model_eef.RoboticDiffusionTransformerModel.preprocess_images(...).to(device, dtype)`.

Host side of the feature:
  * `resample_coeffs(in, out, filter)`: PIL's 8-bit resampler restated — per output index the first input index, the tap count and
    the taps in 22-bit fixed point, computed in double exactly as Pillow's `precompute_coeffs` / `normalize_coeffs_8bpc` do
    (src/libImaging/Resample.c).  Cached per geometry, on the host and on the device.
  * `norm_table(mean, std, dtype)`: the 256 possible outputs of a channel, built with the very expressions of
    `SiglipPreprocessor.preprocess` and torch's own cast, so the kernel only looks up.
  * `FrameStager`: frames of any accepted kind -> one pinned staging buffer -> one host-to-device copy of raw bytes; device-resident
    frames (pitched views included) are used in place.  `DevicePreprocessor` owns one, `jpeg_mapping_device` one per device.
  * `DevicePreprocessor`: the stager's frames -> a list of stages, each one driver call (`_JpegStage`, `_ResampleStage` for the pre-resize
    and for the main pass, `_JitterStage`, `_CorruptStage`, `_AreaStage`), planned in one loop that carves the workspace and launched in one loop.
    With frames of an already-seen geometry at already-seen addresses the call allocates nothing (given `out=`), copies nothing and
    never synchronises, so it can be captured in a graph together with the tower.
  * `jitter=`: the training-time ColorJitter (vlatouch/imgaug.py, csrc/vt_colorjitter.hip) between the `image_size` pre-resize and the
    pad, where the reference's dataset applies it (train/dataset.py:373-409): Resize -> lift -> jitter -> pad -> resize -> normalise.
  * `corrupt=`: the training-time corruption (`image_corrupt`: noise and blur; vlatouch/imgaug.py, csrc/vt_corrupt.hip) directly behind the
    jitter, as the reference orders it: Resize -> lift -> jitter -> corruption -> pad -> resize -> normalise.
  * `jpeg=`: the reference's cv2 JPEG round trip of the raw frames (vlatouch/jpegmap.py, csrc/vt_jpegmap.hip) ahead of all of the above,
    where the robot loop and the labeller apply it: JPEG -> Resize -> lift -> jitter -> pad -> resize -> normalise.
  * `area=`: the reference's `pad_and_resize_for_siglip` (below; csrc/vt_area.hip) ahead of the JPEG mapping, where every consumer of the
    reference applies it to the raw camera frame: area -> JPEG -> Resize -> lift -> jitter -> pad -> resize -> normalise.

`pad_and_resize_for_siglip(images, target_size)` is the CPU statement of that first stage (scripts/utils_eef.py:5-77: a zero pad to a centred
square, then `cv2.resize(..., interpolation=cv2.INTER_AREA)`), in numpy; `pad_and_resize_device` gives the same bytes from the kernel.
UNPINNED against cv2, which is not available where this was written.  It is restated from OpenCV 4.x modules/imgproc/src/resize.cpp, and
these parts rest on reading that source alone: that `resize` takes INTER_AREA with scale >= 1 to `resizeAreaFast_` when the fp64 scale is
within DBL_EPSILON of an integer and to `resizeArea_<uchar, float>` with `computeResizeAreaTab` otherwise; the fast form's `(s + 2) >> 2`
for a factor of 2 and `saturate_cast<uchar>(s * (1.f / area))` for the others; the table's 1e-3 thresholds and `cellWidth`; the loop order of
the fractional form (buf over the horizontal taps per source row, sum over the rows) in fp32 without fused multiply-adds; and that
`saturate_cast<uchar>(float)` rounds to nearest-even.  A build of cv2 that dispatches the call to another back end (IPP, OpenCL, a HAL) may
differ.  What is checked here is independent of cv2: known answers of the cell sums, and the exact fp64 box integral of the padded canvas.
A frame smaller than the target (scale < 1) takes cv2 to its fixed-point bilinear emulation, which is not built: the statement and the
device refuse it.

All launches go to the current stream; the staging buffers are reused from call to call on the assumption that calls are issued in
stream order (the pinned buffer itself is guarded by an event).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .imgaug import OP_NONE, TABLE_WORDS_MAX, ColorJitterParams, corrupt_list, pack_corrupt
from .jpegmap import jpeg_table

BILINEAR, BICUBIC = 1, 2
_SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}
PRECISION_BITS = 22
TILE_ROWS = 16          # output rows of a kernel tile (kTR in csrc/vt_imgprep.hip)
FUSED_ROWS = 128        # most intermediate rows the fused kernel holds; beyond it the two-launch form runs


def _filter(x: np.ndarray, filt: int) -> np.ndarray:
    x = np.abs(x)
    if filt == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


_coeff_cache: dict = {}


def resample_coeffs(in_size: int, out_size: int, filt: int = BICUBIC) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds [out, 2] int32 = (xmin, count), taps [out, ksize] int32) of PIL's resize of an 8-bit axis from in_size to out_size."""
    key = (int(in_size), int(out_size), int(filt))
    hit = _coeff_cache.get(key)
    if hit is not None:
        return hit
    in_size, out_size = key[0], key[1]
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_coeffs: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = _SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int) truncates toward zero, as astype does
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):                                                     # the sum runs over the taps in order, as in C
        valid = t < xmax
        wt = np.where(valid, _filter((t + xmin - center + 0.5) * ss, filt), 0.0)
        w[:, t] = wt
        ww = ww + wt
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, (-0.5 + w * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    _coeff_cache[key] = (bounds, kk)
    return bounds, kk


def tile_rows_max(bounds: np.ndarray) -> int:
    """Most input rows a TILE_ROWS-row output tile reads (the LDS rows of the fused kernel)."""
    out = bounds.shape[0]
    y0 = np.arange(0, out, TILE_ROWS)
    y1 = np.minimum(y0 + TILE_ROWS - 1, out - 1)
    return int((bounds[y1, 0] + bounds[y1, 1] - bounds[y0, 0]).max())


def norm_table(image_mean, image_std, dtype: torch.dtype = torch.float32, rescale_factor: float = 1 / 255.0) -> torch.Tensor:
    """[3, 256]: channel c of a byte v after SiglipPreprocessor.preprocess and `.to(dtype)`."""
    x = np.arange(256, dtype=np.uint8).reshape(256, 1).repeat(3, axis=1)
    x = np.asarray(x, dtype=np.float32) * np.float32(rescale_factor)
    x = (x - np.asarray(image_mean, dtype=np.float32)) / np.asarray(image_std, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(dtype)


# ---- the zero pad and area resize of the raw frames
DBL_EPSILON = float(np.finfo(np.float64).eps)
AREA_MAX_ISCALE = 2048      # VT_AREA_MAX_ISCALE: the cell sum of the integer form is an int


def area_scale(m: int, target: int) -> Tuple[float, int, bool]:
    """cv2.resize's (scale, iscale, fast) of an axis m -> target, in fp64 as it computes them; refuses what is not built."""
    if int(target) != target or target < 1 or m < 1:
        raise ValueError(f"pad_and_resize_for_siglip: sizes must be positive integers, got {m} -> {target!r}")
    inv = float(np.float64(target) / np.float64(m))
    scale = 1.0 / inv
    iscale = int(scale)
    if scale < 1.0:
        raise ValueError(f"pad_and_resize_for_siglip: a frame of side {m} is smaller than the target {target}: cv2's bilinear up-scale "
                         "emulation is not built")
    fast = abs(scale - iscale) < DBL_EPSILON
    if fast and iscale > AREA_MAX_ISCALE:
        raise ValueError(f"pad_and_resize_for_siglip: a reduction by {iscale} (at most {AREA_MAX_ISCALE})")
    return scale, iscale, fast


_area_cache: dict = {}


def area_taps(m: int, target: int) -> Tuple[np.ndarray, np.ndarray]:
    """computeResizeAreaTab of an axis m -> target (fractional scale >= 1): (source index [K, target] int32, weight [K, target] float32),
    per output its taps in the table's order, the shorter lists padded to the longest K with (0, 0.0).  Cached per (m, target)."""
    key = (int(m), int(target))
    hit = _area_cache.get(key)
    if hit is not None:
        return hit
    m, target = key
    scale, _, fast = area_scale(m, target)
    if fast:
        raise ValueError(f"area_taps: {m} -> {target} is an integer scale and has no tap table")
    taps = []
    for dx in range(target):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, m - fsx1)
        sx1, sx2 = math.ceil(fsx1), min(math.floor(fsx2), m - 1)
        sx1 = min(sx1, sx2)
        t = []
        if sx1 - fsx1 > 1e-3:
            t.append((sx1 - 1, np.float32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            t.append((sx, np.float32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            t.append((sx2, np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        taps.append(t)
    K = max(1, max(len(t) for t in taps))
    idx, wgt = np.zeros((K, target), dtype=np.int32), np.zeros((K, target), dtype=np.float32)
    for dx, t in enumerate(taps):
        for k, (si, a) in enumerate(t):
            idx[k, dx], wgt[k, dx] = si, a
    _area_cache[key] = (idx, wgt)
    return idx, wgt


def _area_one(img: np.ndarray, target: int) -> np.ndarray:
    H, W = img.shape[:2]
    m = max(H, W)
    _, k, fast = area_scale(m, target)
    canvas = np.zeros((m, m, 3), dtype=np.uint8)
    top, left = (m - H) // 2, (m - W) // 2
    canvas[top:top + H, left:left + W] = img
    if fast:
        if k == 1:
            return canvas
        s = canvas.reshape(target, k, target, k, 3).sum(axis=(1, 3), dtype=np.int64)
        if k == 2:
            return ((s + 2) >> 2).astype(np.uint8)
        v = s.astype(np.float32) * (np.float32(1.0) / np.float32(k * k))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    idx, wgt = area_taps(m, target)
    S = canvas.astype(np.float32)
    buf = np.zeros((m, target, 3), dtype=np.float32)               # every source row's horizontal pass; fp32 products and sums, each rounded
    for k in range(idx.shape[0]):
        buf = buf + S[:, idx[k], :] * wgt[k][None, :, None]
    total = wgt[0][:, None, None] * buf[idx[0]]
    for k in range(1, idx.shape[0]):
        total = total + wgt[k][:, None, None] * buf[idx[k]]
    return np.clip(np.rint(total), 0, 255).astype(np.uint8)


def pad_and_resize_for_siglip(images, target_size: int = 384) -> np.ndarray:
    """The reference's `pad_and_resize_for_siglip` / `pad_and_resize_for_siglip_batch` (scripts/utils_eef.py:5-77): one uint8 [H, W, 3] frame
    or a batch [n, H, W, 3] -> uint8 [.., target, target, 3]: the frame on a centred square of zeros, rows from (m - H) // 2 and columns from
    (m - W) // 2 with m = max(H, W), then cv2's INTER_AREA resize as the module docstring states it (UNPINNED against cv2)."""
    a = np.asarray(images)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3 or min(a.shape) < 1:
        raise ValueError(f"pad_and_resize_for_siglip: frames must be uint8 [H, W, 3] or [n, H, W, 3], got {a.dtype} {a.shape}")
    target = int(target_size)
    area_scale(max(a.shape[-3], a.shape[-2]), target_size)
    if a.ndim == 3:
        return _area_one(a, target)
    return np.stack([_area_one(f, target) for f in a], axis=0)


def area_size(flag, tower_size: int) -> Optional[int]:
    """The `pad_and_resize=` argument of the callers (step, encode_frames, label_episode) -> None or a target: False / None is off, True is
    the tower's size, an integer is that size."""
    if flag is None or flag is False:
        return None
    if flag is True:
        return int(tower_size)
    if int(flag) != flag or flag < 1:
        raise ValueError(f"pad_and_resize must be False, True or a positive target size, got {flag!r}")
    return int(flag)


def pad_and_resize_pil(images: Sequence, target: Optional[int]) -> list:
    """The CPU route of the callers: every frame that exists -> a PIL image of `pad_and_resize_for_siglip(frame, target)`; all as given
    when `target` is None."""
    from PIL import Image
    if target is None:
        return list(images)
    rgb = lambda im: np.asarray(im if not isinstance(im, Image.Image) or im.mode == "RGB" else im.convert("RGB"))
    return [None if im is None else Image.fromarray(pad_and_resize_for_siglip(rgb(im), target)) for im in images]


def area_table(items, target: int, align: int = 1):
    """[(ptr, h, w, pitch), ...] -> (the `vt_area_frame` table with out_off, ntaps and the table offsets set, output bytes, the tap tables'
    bytes as one uint8 array): the table builder of the area stage, for `pad_and_resize_device` below and for the preprocessor's stage list
    alike.  Frame k is written at k * stride, stride = 3 * target^2 rounded up to `align`; frames of one canvas side share one table, which
    serves both axes."""
    arr = (_lib.AreaFrame * len(items))()
    tabs, offs = [], {}
    stride = (3 * target * target + align - 1) // align * align
    for k, (ptr, h, w, pitch) in enumerate(items):
        m = max(h, w)
        try:
            _, _, fast = area_scale(m, target)
        except ValueError as e:
            raise _lib.VtError(f"frame {k} of {h} x {w}: {e}") from None
        f = arr[k]
        f.src, f.h, f.w, f.pitch, f.out_off, f.target = ptr, h, w, pitch, k * stride, target
        if fast:
            continue
        if m not in offs:
            idx, wgt = area_taps(m, target)
            rec = np.empty(idx.shape, dtype=[("si", np.int32), ("alpha", np.float32)])
            rec["si"], rec["alpha"] = idx, wgt
            offs[m] = (sum(t.size for t in tabs), idx.shape[0])
            tabs.append(rec.view(np.uint8).reshape(-1))
        f.tab_x = f.tab_y = offs[m][0]
        f.ntaps = offs[m][1]
    return arr, len(items) * stride, (np.concatenate(tabs) if tabs else np.zeros(0, dtype=np.uint8))


def _align(v: int, a: int) -> int:
    return (v + a - 1) // a * a


_SIZING_BASE = 4096     # the drivers size only tables whose sources are set: where a plan is sized before there is a workspace, it stands at this address


class FrameStager:
    """Frames of every accepted kind -> (ptr, h, w, pitch) on one device: PIL images, uint8 [H, W, 3] arrays and host tensors go through one
    pinned buffer (guarded by an event) and up in one copy, 16 bytes apart; device tensors, pitched views included, are used in place."""

    def __init__(self, device):
        self.device = _lib.require_gpu(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._pinned: Optional[torch.Tensor] = None
        self._pinned_free: Optional[torch.cuda.Event] = None
        self._upload: Optional[torch.Tensor] = None

    def gather(self, images: Sequence, missing=None):
        """-> per frame (ptr, h, w, pitch), or `missing` for a None entry, plus the tensors that must stay alive until the launches are queued."""
        from PIL import Image
        items, host, keep = [], [], []
        for im in images:
            if im is None:
                items.append(missing)
                continue
            if isinstance(im, torch.Tensor) and im.is_cuda:
                if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                    raise _lib.VtError(f"device frame must be uint8 [H, W, 3], got {im.dtype} {tuple(im.shape)}")
                if im.device != self.device:
                    raise _lib.VtError(f"device frame lives on {im.device}, the preprocessor on {self.device}")
                h, w = int(im.shape[0]), int(im.shape[1])
                if not (im.stride(2) == 1 and im.stride(1) == 3 and (h == 1 or im.stride(0) >= 3 * w)):
                    im = im.contiguous()          # an exotic view: one device copy (allocates)
                keep.append(im)
                items.append((im.data_ptr(), h, w, int(im.stride(0)) if h > 1 else 3 * w))
                continue
            if isinstance(im, Image.Image):
                a = np.asarray(im if im.mode == "RGB" else im.convert("RGB"))
            elif isinstance(im, torch.Tensor):
                a = im.numpy()
            else:
                a = np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise _lib.VtError(f"frame must be uint8 [H, W, 3], got {a.dtype} {a.shape}")
            host.append((len(items), a))
            items.append(None)
        if host:
            offs, total = [], 0
            for _, a in host:
                offs.append(total)
                total = _align(total + a.size, 16)
            if self._pinned is None or self._pinned.numel() < total:
                self._pinned = torch.empty(_align(total * 3 // 2, 4096), dtype=torch.uint8).pin_memory()
                self._upload = torch.empty(self._pinned.numel(), dtype=torch.uint8, device=self.device)
                self._pinned_free = None
            if self._pinned_free is not None:
                self._pinned_free.synchronize()           # the previous call's copy has left the pinned buffer (waits for that copy only)
            pin = self._pinned.numpy()
            for (_, a), o in zip(host, offs):
                pin[o:o + a.size] = a.reshape(-1)
            self._upload[:total].copy_(self._pinned[:total], non_blocking=True)
            self._pinned_free = torch.cuda.Event()
            self._pinned_free.record(torch.cuda.current_stream(self.device))
            base = self._upload.data_ptr()
            for (i, a), o in zip(host, offs):
                items[i] = (base + o, int(a.shape[0]), int(a.shape[1]), 3 * int(a.shape[1]))
        return items, keep

    def to_device(self, arr) -> torch.Tensor:
        """A ctypes table's bytes on the device."""
        return torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(self.device)


# ---- the stages of a call.  Each kind answers the same two questions:
#   plan(items) -> (output bytes, scratch bytes, [(frame index, offset in the output, h, w), ...]): builds `self.table` over the incoming items
#       (ptr, h, w, pitch), None for a frame that is missing; the list names the tight uint8 frames it writes, which the next stage reads
#   launch(wp, st, out, jitter, quality, corrupt): enqueues on stream `st`, workspace at address `wp`, with this call's arguments
# `_plan` places the output at `out_off` and the scratch at `ws_off` of the workspace and, once there is a workspace, calls bind().
class _Stage:
    def bind(self, stager: FrameStager) -> None:
        self.dev = stager.to_device(self.table)


class _AreaStage(_Stage):
    """The zero pad and area resize of the raw frames `idx` (those that exist; a missing frame stays the fill image) to `target`.  The
    records and, 16 bytes aligned behind them, the tap tables go up once with the plan: the call stays as capturable as the plain one."""

    def __init__(self, idx, target: int):
        self.idx, self.target = idx, target

    def plan(self, items):
        self.table, out_bytes, self.taps = area_table([items[i] for i in self.idx], self.target, 16)
        self.rec_bytes = _align(C.sizeof(self.table), 16)
        return out_bytes, 0, [(i, f.out_off, self.target, self.target) for i, f in zip(self.idx, self.table)]

    def bind(self, stager: FrameStager) -> None:
        host = np.zeros(self.rec_bytes + self.taps.size, dtype=np.uint8)
        host[:C.sizeof(self.table)] = np.frombuffer(self.table, dtype=np.uint8)
        host[self.rec_bytes:] = self.taps
        self.dev = torch.from_numpy(host).to(stager.device)

    def launch(self, wp, st, out, jitter, quality, corrupt):
        _lib.check(_lib.lib().vt_area_resize(self.table, _lib.ptr(self.dev), len(self.idx), C.c_void_p(wp + self.out_off),
                                             C.c_void_p(self.dev.data_ptr() + self.rec_bytes) if self.taps.size else None, self.taps.size, st),
                   "vt_area_resize")


class _JpegStage(_Stage):
    """The JPEG round trip of the frames `idx` (those that exist; a missing frame's fill is not mapped), vlatouch/jpegmap.py."""

    def __init__(self, idx):
        self.idx = idx

    def plan(self, items):
        self.table, out_bytes, ws_bytes = jpeg_table([items[i] for i in self.idx])
        return out_bytes, ws_bytes, [(i, f.out_off, f.h, f.w) for i, f in zip(self.idx, self.table)]

    def launch(self, wp, st, out, jitter, quality, corrupt):
        _lib.check(_lib.lib().vt_jpegmap(self.table, _lib.ptr(self.dev), len(self.idx), quality, _lib.JPEGMAP_CV2_ORDER, C.c_void_p(wp + self.out_off),
                                         C.c_void_p(wp + self.ws_off), self.ws_bytes, st), "vt_jpegmap")


class _ResampleStage(_Stage):
    """One vt_imgprep call of preprocessor `pp`: the uint8 pre-resize into the workspace (`final` False), or the main pass into `out`."""

    def __init__(self, pp, flags: int, final: bool):
        self.pp, self.flags, self.final = pp, flags, final
        self.S, self.filt, self.what = (pp.S, BICUBIC, "vt_imgprep") if final else (0, BILINEAR, "vt_imgprep (pre-resize)")

    def plan(self, items):
        n = len(items)
        self.table = arr = (_lib.ImgprepFrame * n)()
        off, outputs = 0, []
        for i, it in enumerate(items):
            if it is None:
                continue
            ptr, h, w, pitch = it
            oh, ow = (self.S, self.S) if self.final else self.pp._resized(h, w)
            ih, iw = (max(h, w), max(h, w)) if self.flags & _lib.IMGPREP_PAD else (h, w)
            if ih > 100 * iw and oh < ih:
                # recent Pillow resizes such a sliver vertically first (Image.resize), older ones do not: there is no single result to match
                raise _lib.VtError(f"frame of {h} x {w} resized without padding: more than 100 times taller than wide is not supported "
                                   "on the device (use preprocess_images)")
            th, kh, _ = self.pp._table(iw, ow, self.filt)
            tv, kv, rows = self.pp._table(ih, oh, self.filt)
            f = arr[i]
            f.src, f.pitch, f.h, f.w, f.out_h, f.out_w = ptr, pitch, h, w, oh, ow
            f.coef_h = th.data_ptr() if th is not None else None
            f.coef_v = tv.data_ptr() if tv is not None else None
            f.ksize_h, f.ksize_v, f.rows_max = kh, kv, rows
            f.out_off = off
            outputs.append((i, off, oh, ow))
            off += _align(oh * ow * 3, 16)
        L = _lib.lib()
        ws_bytes = int(L.vt_imgprep_workspace_bytes(arr, n, self.S, self.flags))
        if ws_bytes == 0:
            raise _lib.VtError("vt_imgprep_workspace_bytes: " + L.vt_last_error().decode())
        return (0, ws_bytes, []) if self.final else (off, ws_bytes, outputs)

    def launch(self, wp, st, out, jitter, quality, corrupt):
        lut, fill, dst = (_lib.ptr(self.pp.lut), self.pp.fill, _lib.ptr(out)) if self.final else (None, 0, C.c_void_p(wp + self.out_off))
        _lib.check(_lib.lib().vt_imgprep(self.table, _lib.ptr(self.dev), len(self.table), self.S, lut, fill, self.flags, dst,
                                         C.c_void_p(wp + self.ws_off), self.ws_bytes, st), self.what)


class _JitterStage(_Stage):
    """ColorJitter (vlatouch/imgaug.py): every frame that exists goes through it, an unjittered one with an empty operation list.  With `lift`
    the stage also takes the brightness-lift decision, on the frame before the jitter, so the stage behind it runs without IMGPREP_BRIGHT and
    no frame is lifted twice.  The table is this call's: the cached geometry with the call's parameters, through a pinned buffer."""

    def __init__(self, lift: bool):
        self.flags = _lib.COLORJITTER_LIFT if lift else 0
        self.free: Optional[torch.cuda.Event] = None

    def plan(self, items):
        self.idx = [i for i, it in enumerate(items) if it is not None]
        self.table = (_lib.ColorJitterFrame * len(self.idx))()
        off = 0
        for f, i in zip(self.table, self.idx):
            f.src, f.h, f.w, f.pitch = items[i]
            f.out_off = off
            f.order[:] = [OP_NONE] * 4
            f.brightness = f.contrast = f.saturation = 1.0
            off += _align(3 * f.h * f.w, 16)
        return off, int(_lib.lib().vt_colorjitter_workspace_bytes(len(self.idx))), [(i, f.out_off, f.h, f.w) for i, f in zip(self.idx, self.table)]

    def bind(self, stager: FrameStager) -> None:
        self.pin = torch.empty(C.sizeof(self.table), dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(C.sizeof(self.table), dtype=torch.uint8, device=stager.device)

    def launch(self, wp, st, out, jitter, quality, corrupt):
        arr = type(self.table).from_buffer_copy(self.table)
        for f, i in zip(arr, self.idx):
            if jitter is not None and jitter[i] is not None:      # no jitter list: the stage is here for the lift ahead of a corruption
                jitter[i].fill_record(f)
        if self.free is not None:
            self.free.synchronize()                                     # the previous call's copy has left the pinned table
        self.pin.numpy()[:] = np.frombuffer(arr, dtype=np.uint8)
        self.dev.copy_(self.pin, non_blocking=True)
        self.free = torch.cuda.Event()
        self.free.record(torch.cuda.current_stream(self.dev.device))
        _lib.check(_lib.lib().vt_colorjitter(arr, _lib.ptr(self.dev), len(self.idx), self.flags, C.c_void_p(wp + self.out_off),
                                             C.c_void_p(wp + self.ws_off), self.ws_bytes, st), "vt_colorjitter")


class _CorruptStage(_Stage):
    """The corruption (vlatouch/imgaug.py, csrc/vt_corrupt.hip) directly behind the jitter: every frame that exists goes through it, an
    uncorrupted one as a copy.  Records and tables are this call's: one pinned buffer holds the frame table and, behind it, room for
    `TABLE_WORDS_MAX` words per frame, and goes up in one copy."""

    def __init__(self):
        self.free: Optional[torch.cuda.Event] = None

    def plan(self, items):
        self.idx = [i for i, it in enumerate(items) if it is not None]
        self.table = (_lib.CorruptFrame * len(self.idx))()
        off = 0
        for f, i in zip(self.table, self.idx):
            f.src, f.h, f.w, f.pitch = items[i]
            f.out_off = off
            off += _align(3 * f.h * f.w, 16)
        self.rec_bytes = _align(C.sizeof(self.table), 16)
        return off, 0, [(i, f.out_off, f.h, f.w) for i, f in zip(self.idx, self.table)]

    def bind(self, stager: FrameStager) -> None:
        nbytes = self.rec_bytes + 4 * TABLE_WORDS_MAX * len(self.idx)
        self.pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=stager.device)

    def launch(self, wp, st, out, jitter, quality, corrupt):
        arr = type(self.table).from_buffer_copy(self.table)
        words = pack_corrupt(arr, [corrupt[i] for i in self.idx])
        if self.free is not None:
            self.free.synchronize()                                     # the previous call's copy has left the pinned buffer
        pin, used = self.pin.numpy(), self.rec_bytes + 4 * words.size
        pin[:C.sizeof(arr)] = np.frombuffer(arr, dtype=np.uint8)
        pin[self.rec_bytes:used] = words.view(np.uint8)
        self.dev[:used].copy_(self.pin[:used], non_blocking=True)
        self.free = torch.cuda.Event()
        self.free.record(torch.cuda.current_stream(self.dev.device))
        _lib.check(_lib.lib().vt_corrupt(arr, _lib.ptr(self.dev), len(self.idx), words.ctypes.data if words.size else None,
                                         C.c_void_p(self.dev.data_ptr() + self.rec_bytes), words.size, C.c_void_p(wp + self.out_off), st),
                   "vt_corrupt")


class DevicePreprocessor:
    """`preprocess_images` of one model configuration on one device.  image_size / pad / brightness as in the wrapper."""

    def __init__(self, size: int, image_mean, image_std, device, dtype: torch.dtype = torch.float32, *, pad: bool = True,
                 brightness: bool = False, image_size=None, rescale_factor: float = 1 / 255.0):
        self.stager = FrameStager(device)
        self.device = self.stager.device
        if dtype not in (torch.float32, torch.bfloat16):
            raise _lib.VtError(f"DevicePreprocessor: fp32 or bf16 output, got {dtype}")
        self.S, self.dtype, self.pad, self.brightness, self.image_size = int(size), dtype, bool(pad), bool(brightness), image_size
        self.mean255 = tuple(int(x * 255) for x in image_mean)
        self.fill = self.mean255[0] | self.mean255[1] << 8 | self.mean255[2] << 16
        self.lut = norm_table(image_mean, image_std, dtype, rescale_factor).to(self.device)
        self.flags = (_lib.IMGPREP_PAD if self.pad else 0) | (_lib.IMGPREP_BRIGHT if self.brightness else 0) | \
                     (_lib.IMGPREP_OUT_BF16 if dtype == torch.bfloat16 else 0)
        self.force_two_pass = False           # tests: run the two-launch form where the fused one would do
        # a missing frame is the S x S fill image; the kernel writes it directly (item None) unless a pre-resize or a brightness lift could
        # touch it: then it is a frame like the others, the background image
        self._bg = self._missing = None
        if image_size is not None or (self.brightness and sum(self.mean255) / (255.0 * 3) <= 0.15):
            bg = np.ones((self.S, self.S, 3), dtype=np.uint8) * np.array(self.mean255, dtype=np.uint8).reshape(1, 1, 3)
            self._bg = torch.from_numpy(bg).to(self.device)
            self._missing = (self._bg.data_ptr(), self.S, self.S, 3 * self.S)
        self._tables: dict = {}               # (in, out, filter) -> (device int32 table, ksize, rows_max)
        self._plans: dict = {}
        self._ws: Optional[torch.Tensor] = None
        self._keepalive: list = []

    # ---- tables
    def _table(self, in_size: int, out_size: int, filt: int):
        if in_size == out_size:
            return None, 0, TILE_ROWS
        key = (in_size, out_size, filt)
        hit = self._tables.get(key)
        if hit is None:
            b, k = resample_coeffs(in_size, out_size, filt)
            flat = np.concatenate([b.reshape(-1), k.reshape(-1)]).astype(np.int32)
            hit = (torch.from_numpy(flat).to(self.device), int(k.shape[1]), tile_rows_max(b))
            self._tables[key] = hit
        return hit

    def _resized(self, h: int, w: int) -> Tuple[int, int]:
        sz = self.image_size
        if isinstance(sz, int):                           # transforms.Resize(int): shorter side -> sz
            return (max(1, int(sz * h / w)), sz) if w <= h else (sz, max(1, int(sz * w / h)))
        return int(sz[0]), int(sz[1])

    # ---- planning: everything that depends only on geometry and addresses
    def _stages(self, jit: bool, jpeg_idx: Optional[tuple], cor: bool = False, area: Optional[tuple] = None) -> list:
        """The chain of one call, as the reference orders it: area -> JPEG -> Resize -> (lift and) jitter -> corruption -> pad, resize,
        normalise.  The lift precedes the corruption: with `brightness`, a corrupting call runs the jitter stage even where no frame is
        jittered.  `area`: None or (target, the indices of the frames that exist)."""
        stages = []
        if area and area[1]:
            stages.append(_AreaStage(area[1], area[0]))
        if jpeg_idx:
            stages.append(_JpegStage(jpeg_idx))
        if self.image_size is not None:
            stages.append(_ResampleStage(self, _lib.IMGPREP_OUT_U8, final=False))
        flags = self.flags | (_lib.IMGPREP_TWO_PASS if self.force_two_pass else 0)
        if jit or (cor and self.brightness):
            stages.append(_JitterStage(self.brightness))
            flags &= ~_lib.IMGPREP_BRIGHT
        if cor:
            stages.append(_CorruptStage())
        stages.append(_ResampleStage(self, flags, final=True))
        return stages

    def _plan(self, items, ws_ptr: Optional[int], jit: bool = False, jpeg_idx: Optional[tuple] = None, cor: bool = False,
              area: Optional[tuple] = None):
        key = (tuple(items), ws_ptr, self.force_two_pass, jit, jpeg_idx, cor, area)
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        if len(self._plans) >= 64:                        # plans a captured graph reads (their device tables) are never dropped
            self._plans = {k: v for k, v in self._plans.items() if v.get("captured")}
        base = ws_ptr if ws_ptr is not None else _SIZING_BASE
        stages, off = self._stages(jit, jpeg_idx, cor, area), 0
        for st in stages:                                 # the workspace, carved: per stage its output, then its scratch, each 256-byte aligned
            out_bytes, st.ws_bytes, outputs = st.plan(items)
            st.out_off, st.ws_off = off, off + _align(out_bytes, 256)
            items = list(items)
            for i, rel, h, w in outputs:
                items[i] = (base + off + rel, h, w, 3 * w)
            off = st.ws_off + _align(st.ws_bytes, 256)
            if ws_ptr is not None:
                st.bind(self.stager)
        plan = self._plans[key] = {"stages": stages, "ws_bytes": stages[-1].ws_off + stages[-1].ws_bytes}
        return plan

    @staticmethod
    def _jitter_list(images: Sequence, jitter):
        """`jitter` checked against the frames -> the per-frame list, or None where no frame is jittered."""
        if jitter is None:
            return None
        jitter = list(jitter)
        if len(jitter) != len(images):
            raise _lib.VtError(f"jitter has {len(jitter)} entries for {len(images)} frames")
        for i, (im, p) in enumerate(zip(images, jitter)):
            if p is None:
                continue
            if not isinstance(p, ColorJitterParams):
                raise _lib.VtError(f"jitter entry {i} must be None or a ColorJitterParams, got {type(p).__name__}")
            if im is None:
                raise _lib.VtError(f"jitter entry {i} belongs to a missing frame (the reference never augments an invalid image)")
        return jitter if any(p is not None for p in jitter) else None

    @staticmethod
    def _jpeg_idx(images: Sequence, jpeg):
        """`jpeg` checked -> (quality, the indices of the frames that exist) or (None, None)."""
        if jpeg is None:
            return None, None
        if isinstance(jpeg, bool) or not isinstance(jpeg, (int, np.integer)) or not 1 <= int(jpeg) <= 100:
            raise _lib.VtError(f"jpeg must be None or a quality in 1..100, got {jpeg!r}")
        return int(jpeg), tuple(i for i, im in enumerate(images) if im is not None)

    @staticmethod
    def _area_idx(images: Sequence, area):
        """`area` checked -> (target, the indices of the frames that exist) or None."""
        if area is None:
            return None
        if isinstance(area, bool) or not isinstance(area, (int, np.integer)) or int(area) < 1:
            raise _lib.VtError(f"area must be None or a positive target size, got {area!r}")
        return int(area), tuple(i for i, im in enumerate(images) if im is not None)

    def workspace_bytes(self, images: Sequence, jitter=None, jpeg=None, corrupt=None, area=None) -> int:
        """Bytes of workspace a call on these frames needs (geometry only, plus whether any frame is jittered, JPEG-mapped, corrupted or
        area-resized)."""
        jit = self._jitter_list(images, jitter) is not None
        cor = corrupt_list(images, corrupt, _lib.VtError) is not None
        items, _ = self.stager.gather(images, self._missing)
        return self._plan(items, None, jit, self._jpeg_idx(images, jpeg)[1], cor, self._area_idx(images, area))["ws_bytes"]

    @torch.no_grad()
    def __call__(self, images: Sequence, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, jitter=None,
                 jpeg=None, corrupt=None, area=None) -> torch.Tensor:
        """-> pixel_values [n, 3, S, S].  `jitter`: None, or one entry per frame, each None or a `ColorJitterParams` (never on a missing
        frame).  Without it, or with every entry None, the call is the unjittered one: same launches, same bits, capturable in a graph.
        A call that jitters writes its parameters into a device table through a pinned buffer and waits for the previous such copy, so
        it is not capturable in a graph.
        `jpeg`: None, or the quality of the reference's cv2 JPEG round trip (vlatouch/jpegmap.py, order "cv2"), applied to every frame
        that exists before anything else.  Its table is cached with the plan: the call stays as capturable as the plain one.
        `corrupt`: None, or one entry per frame, each None or a `CorruptParams` (never on a missing frame): the training-time corruption
        (vlatouch/imgaug.py), directly behind the jitter.  Without it, or with every entry None, the call is the one without it.  Like
        a jittering call it uploads this call's tables through a pinned buffer, so it is not capturable in a graph.
        `area`: None, or the target size of the reference's `pad_and_resize_for_siglip` (zero pad to a square, cv2's INTER_AREA resize),
        applied to every frame that exists before anything else, the JPEG mapping included; a missing frame stays the fill image.  Its
        records and tap tables are cached with the plan: the call stays as capturable as the plain one."""
        n = len(images)
        if n < 1:
            raise _lib.VtError("DevicePreprocessor: no frames")
        S = self.S
        jitter = self._jitter_list(images, jitter)
        jit = jitter is not None
        quality, jpeg_idx = self._jpeg_idx(images, jpeg)
        corrupt = corrupt_list(images, corrupt, _lib.VtError)
        cor = corrupt is not None
        area = self._area_idx(images, area)
        if jit and torch.cuda.is_current_stream_capturing():
            raise _lib.VtError("DevicePreprocessor: a call with jitter= cannot be captured in a graph")
        if cor and torch.cuda.is_current_stream_capturing():
            raise _lib.VtError("DevicePreprocessor: a call with corrupt= cannot be captured in a graph")
        with torch.cuda.device(self.device):
            items, keep = self.stager.gather(images, self._missing)
            if workspace is None:
                need = self._plan(items, None, jit, jpeg_idx, cor, area)["ws_bytes"]
                if self._ws is None or self._ws.numel() < need:
                    if self._ws is not None and any(v.get("captured") for v in self._plans.values()):
                        self._keepalive.append(self._ws)          # a captured graph still works in the old one
                    self._ws = torch.empty(_align(need * 3 // 2, 4096), dtype=torch.uint8, device=self.device)
                workspace = self._ws
            elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != self.device:
                raise _lib.VtError("workspace must be a contiguous uint8 tensor on the preprocessor's device")
            plan = self._plan(items, workspace.data_ptr(), jit, jpeg_idx, cor, area)
            if torch.cuda.is_current_stream_capturing():
                plan["captured"] = True
            if workspace.numel() < plan["ws_bytes"]:
                raise _lib.VtError(f"workspace of {workspace.numel()} bytes, {plan['ws_bytes']} needed")
            if out is None:
                out = torch.empty((n, 3, S, S), dtype=self.dtype, device=self.device)
            elif out.shape != (n, 3, S, S) or out.dtype != self.dtype or not out.is_contiguous() or out.device != self.device:
                raise _lib.VtError(f"out must be a contiguous {self.dtype} [{n}, 3, {S}, {S}] tensor on {self.device}")
            wp, st = workspace.data_ptr(), _lib.stream_ptr(self.device)
            for stage in plan["stages"]:
                stage.launch(wp, st, out, jitter, quality, corrupt)
        return out


@torch.no_grad()
def pad_and_resize_device(frames: Sequence, target_size: int = 384, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """`pad_and_resize_for_siglip` of every frame on the card (csrc/vt_area.hip), bit for bit: per frame a PIL image, uint8 [H, W, 3] array or
    uint8 tensor (host or device, pitched views included), of mixed sizes; a `None` entry gives the canvas with nothing on it, all zeros.
    Returns uint8 [n, target, target, 3] on the device: `out` (contiguous, of that shape) or a new tensor.  `device`: where to run when no
    frame is a device tensor (default: the current one).  One launch, on the current stream."""
    from .jpegmap import _stager
    frames = list(frames)
    target = area_size(target_size, 0)
    if target is None or not frames:
        raise _lib.VtError(f"pad_and_resize_device: a target size and at least one frame are needed, got {target_size!r} and {len(frames)} frames")
    if device is None:
        device = next((f.device for f in frames if isinstance(f, torch.Tensor) and f.is_cuda), "cuda")
    st = _stager(device)
    idx = [i for i, f in enumerate(frames) if f is not None]
    shape = (len(frames), target, target, 3)
    with torch.cuda.device(st.device):
        items, _keep = st.gather([frames[i] for i in idx])       # _keep: contiguous copies of exotic views, alive until the launch is queued
        arr, _, taps = area_table(items, target) if idx else (None, 0, None)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=st.device)
        elif out.shape != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != st.device:
            raise _lib.VtError(f"out must be a contiguous uint8 {list(shape)} tensor on {st.device}")
        if len(idx) < len(frames):
            out.zero_()
        if idx:
            per = 3 * target * target
            for f, i in zip(arr, idx):
                f.out_off = i * per
            dev, tabs = st.to_device(arr), (torch.from_numpy(taps).to(st.device) if taps.size else None)
            _lib.check(_lib.lib().vt_area_resize(arr, _lib.ptr(dev), len(idx), _lib.ptr(out), _lib.ptr(tabs) if tabs is not None else None,
                                                 taps.size, _lib.stream_ptr(st.device)), "vt_area_resize")
    return out
