"""The reference's JPEG round trip of camera frames: `cv2.imencode('.jpg', frame)` -> `cv2.imdecode` before the policy sees a frame, "to
align with training" (residual_controller/frank_inference_eef.py:84-87,131-132; data/create_controller_dataset_episode.py:54-62).

  * `jpeg_mapping(img, quality, order)`: the CPU statement, through Pillow, whose libjpeg-turbo is the library cv2 wraps.
  * `jpeg_mapping_device(frames, ...)`: the same pixels from csrc/vt_jpegmap.hip, bit for bit, for frames of every kind
    `preprocess_images_device` takes, gathered by a `FrameStager` of its own.  The SigLIP path reaches the kernel through the JPEG stage of
    `DevicePreprocessor.__call__(..., jpeg=quality)`, which builds its table with `jpeg_table` as this function does; this function
    serves consumers of the mapped frames themselves (the DINOv2 controller path reads the same frames on the robot).

`order="cv2"`: channel 0 of the array plays blue's role, as cv2 treats whatever array it is given (the reference hands it RGB frames), i.e.
`pil(img[..., ::-1])[..., ::-1]`.  `order="rgb"`: Pillow on the array as given.

UNPINNED against cv2, which is not available where this was written: that `imencode('.jpg', a)` + `imdecode` is libjpeg with
jpeg_set_defaults (quality 95, 4:2:0, islow DCT) and a default decompress (fancy up-sampling), the array read as BGR, rests on reading
OpenCV's grfmt_jpeg.cpp.  The mapping is pinned to Pillow's libjpeg-turbo with the channel roles swapped.  Decoding stored JPEG files (the
entropy coder in front of this file's inverse half) is vlatouch/jpegdec.py.
"""
from __future__ import annotations

import ctypes as C
import io
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

ORDERS = ("cv2", "rgb")


def _check(quality, order) -> int:
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg quality must be an integer in 1..100, got {quality!r}")
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    return int(quality)


def jpeg_mapping(img, quality: int = 95, order: str = "cv2") -> np.ndarray:
    """uint8 [H, W, 3] array or RGB PIL image -> the frame after a JPEG round trip at `quality`, uint8 [H, W, 3]."""
    from PIL import Image
    quality = _check(quality, order)
    a = np.asarray(img if not isinstance(img, Image.Image) or img.mode == "RGB" else img.convert("RGB"))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"frame must be uint8 [H, W, 3], got {a.dtype} {a.shape}")
    if order == "cv2":
        a = a[..., ::-1]
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a)).save(buf, "JPEG", quality=quality)
    buf.seek(0)
    out = np.asarray(Image.open(buf).convert("RGB"))
    return np.ascontiguousarray(out[..., ::-1] if order == "cv2" else out)


def jpeg_quality(flag) -> Optional[int]:
    """The `jpeg_mapping=` argument of the callers (step, encode_frames, label_episode) -> None or a quality: False / None is off, True
    is cv2's default quality 95, an integer is that quality."""
    if flag is None or flag is False:
        return None
    return 95 if flag is True else _check(flag, "cv2")


def jpeg_mapped_pil(images: Sequence, quality: Optional[int]) -> list:
    """The CPU route of the callers: every frame that exists -> a PIL image of `jpeg_mapping(frame, quality)`; all as given when
    `quality` is None."""
    from PIL import Image
    if quality is None:
        return list(images)
    return [None if im is None else Image.fromarray(jpeg_mapping(im, quality)) for im in images]


_stagers: dict = {}


def _stager(device):
    """One `FrameStager` per device (host frames up in one copy, device views in place); a new one holds no memory until it gathers."""
    st = _stagers.get(device)                 # the keys are devices with their index stated, as a frame's `.device` is
    if st is None:
        from .imgprep import FrameStager
        st = FrameStager(device)
        st = _stagers.setdefault(st.device, st)
    return st


def jpeg_table(items):
    """[(ptr, h, w, pitch), ...] -> (the `vt_jpegmap_frame` table with out_off and ws_off set, output bytes, workspace bytes): the table
    builder of the JPEG stage, for `jpeg_mapping_device` below and for the preprocessor's stage list (vlatouch/imgprep.py) alike."""
    arr = (_lib.JpegmapFrame * len(items))()
    off = 0
    for k, (ptr, h, w, pitch) in enumerate(items):
        f = arr[k]
        f.src, f.h, f.w, f.pitch, f.out_off = ptr, h, w, pitch, off
        off += (3 * h * w + 15) // 16 * 16
    L = _lib.lib()
    ws = int(L.vt_jpegmap_workspace_bytes(arr, len(items)))
    if ws == 0:
        raise _lib.VtError("vt_jpegmap_workspace_bytes: " + L.vt_last_error().decode())
    return arr, off, ws


@torch.no_grad()
def jpeg_mapping_device(frames: Sequence, quality: int = 95, order: str = "cv2", out: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None, device=None) -> List[Optional[torch.Tensor]]:
    """`jpeg_mapping` of every frame on the card: per frame a PIL image, uint8 [H, W, 3] array, or uint8 tensor (host or device, pitched
    views included); `None` entries stay `None`.  Returns device uint8 [H, W, 3] tensors, views of `out` (a contiguous uint8 device tensor
    of enough bytes; allocated when None).  `workspace`: likewise, the kernel's scratch.  `device`: where to run when no frame is a device
    tensor (default: the current one).  Launches go to the current stream."""
    quality = _check(quality, order)
    frames = list(frames)
    if device is None:
        device = next((f.device for f in frames if isinstance(f, torch.Tensor) and f.is_cuda), "cuda")
    st = _stager(device)
    idx = [i for i, f in enumerate(frames) if f is not None]
    res: List[Optional[torch.Tensor]] = [None] * len(frames)
    if not idx:
        return res
    with torch.cuda.device(st.device):
        items, _keep = st.gather([frames[i] for i in idx])       # _keep: contiguous copies of exotic views, alive until the launch is queued
        arr, out_bytes, ws_bytes = jpeg_table(items)
        for name, t, need in (("out", out, out_bytes), ("workspace", workspace, ws_bytes)):
            if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.device != st.device or t.numel() < need):
                raise _lib.VtError(f"{name} must be a contiguous uint8 tensor of at least {need} bytes on {st.device}")
        if out is None:
            out = torch.empty(out_bytes, dtype=torch.uint8, device=st.device)
        if workspace is None:
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=st.device)
        dev = st.to_device(arr)
        _lib.check(_lib.lib().vt_jpegmap(arr, _lib.ptr(dev), len(idx), quality, _lib.JPEGMAP_CV2_ORDER if order == "cv2" else 0,
                                         _lib.ptr(out), _lib.ptr(workspace), ws_bytes, _lib.stream_ptr(st.device)), "vt_jpegmap")
    flat = out.view(-1)
    for k, i in enumerate(idx):
        f = arr[k]
        res[i] = flat[f.out_off:f.out_off + 3 * f.h * f.w].view(f.h, f.w, 3)
    return res
