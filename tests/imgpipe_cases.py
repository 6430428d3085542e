"""The camera-frame chain's grid: every subset of the stages of `DevicePreprocessor` (JPEG map, `image_size` pre-resize, colour jitter, the
main pass in its fused and its two-launch form) on one set of frames of every input kind.  Shared by tests/test_gpu_imgpipe.py and
tools/make_golden_imgpipe_ws_parent.py, which recorded tests/golden/g26_imgpipe_ws_parent.json from a build of the commit before the
preprocessor's plan became a list of stages: the workspace layout is not supposed to move.  Needs a GPU (the preprocessor has no other route)."""
import itertools
from collections import OrderedDict

import numpy as np
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)

GOLDEN_NAME = "g26_imgpipe_ws_parent.json"
S = 64
# (jpeg, image_size, jitter, force_two_pass)
COMBOS = list(itertools.product((None, 95), (None, 40), (False, True), (False, True)))
JPEG_TABLE_GEOS = ((480, 640), (19, 21), (1, 1))
BIG = (1080, 1920)       # -> 64: a 16-row tile reads more rows than the fused kernel holds (FUSED_ROWS), whatever is asked for


def combo_id(c) -> str:
    jpeg, image_size, jit, force = c
    return f"jpeg{jpeg}-size{image_size}-{'jitter' if jit else 'plain'}-{'two_pass' if force else 'fused'}"


def preprocessor(image_size, dev, force_two_pass=False):
    from vlatouch.imgprep import DevicePreprocessor
    pp = DevicePreprocessor(S, (0.5,) * 3, (0.5,) * 3, dev, pad=True, brightness=True, image_size=image_size)
    pp.force_two_pass = force_two_pass
    return pp


def frames(dev):
    """-> (the five frames, the device tensors used in place with their host copies): a 48 x 64 host array, a dark one that takes the lift, a
    missing frame, a 30 x 50 device tensor, and a pitched device view (rows 300 bytes apart, 70 pixels wide, odd start address)."""
    g = np.random.default_rng(26)
    host = g.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    dark = (g.integers(0, 256, (48, 64, 3)) // 8).astype(np.uint8)
    small_host = g.integers(0, 256, (30, 50, 3), dtype=np.uint8)
    big_host = g.integers(0, 256, (60, 100, 3), dtype=np.uint8)
    small, big = torch.from_numpy(small_host).to(dev), torch.from_numpy(big_host).to(dev)
    pitched = big[5:50, 11:81, :]
    assert not pitched.is_contiguous() and pitched.data_ptr() % 2 == 1
    return [host, dark, None, small, pitched], [(small, small_host), (big, big_host)]


def jitter_list():
    """Two parameter sets that hold contrast (one on the dark frame: the contrast mean of the lifted pixels), the missing frame's None, and one
    frame that exists and is not jittered."""
    from vlatouch.imgaug import ColorJitterParams
    a = ColorJitterParams((1, 0, 3, 2), 1.2, 0.8, 1.3, 0.02)
    b = ColorJitterParams((3, 2, 1, 0), 0.9, 1.3, 0.7, -0.03)
    return [a, b, None, None, a]


def workspace_sizes(dev="cuda:0") -> "OrderedDict[str, int]":
    from vlatouch.jpegmap import jpeg_table
    out = OrderedDict()
    fr, _ = frames(dev)
    for c in COMBOS:
        jpeg, image_size, jit, force = c
        out[combo_id(c)] = int(preprocessor(image_size, dev, force).workspace_bytes(fr, jitter_list() if jit else None, jpeg))
    big = [torch.zeros((*BIG, 3), dtype=torch.uint8, device=dev)]
    for name, kw in (("plain", {}), ("jpeg95", {"jpeg": 95}), ("jitter", {"jitter": jitter_list()[:1]})):
        out[f"big_{BIG[0]}x{BIG[1]}-{name}"] = int(preprocessor(None, dev).workspace_bytes(big, **kw))
    for h, w in JPEG_TABLE_GEOS:
        _, out_bytes, ws_bytes = jpeg_table([(4096, h, w, 3 * w)])      # a fake source: sizing never dereferences it
        out[f"jpeg_table_{h}x{w}-out"], out[f"jpeg_table_{h}x{w}-workspace"] = int(out_bytes), int(ws_bytes)
    return out
