#!/usr/bin/env python
"""tests/golden/g27_jpeg_streams.npz: a handful of baseline JPEG streams with their Pillow-decoded pixels, so that restart markers and the
decoder's arithmetic stay pinned where the installed Pillow writes other bytes (or no DRI at all).  Frames: tests/jpeg_ref.make_frame, 19 x 21
noise and 48 x 64 gradient at quality 90, written by Pillow in each mode of tests/jpegdec_ref.MODES (default, optimize, 4:4:4,
restart_marker_blocks=3, restart_marker_rows=1).  Keys: `s_<h>x<w>_<mode>` the file's bytes, `p_<h>x<w>_<mode>` uint8 [h, w, 3].
    python tools/make_jpeg_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import jpeg_ref as J  # noqa: E402
from tests import jpegdec_ref as R  # noqa: E402

FRAMES = (("noise", 19, 21), ("gradient", 48, 64))
QUALITY = 90


def main():
    import PIL
    out = {}
    for kind, h, w in FRAMES:
        for mode in R.MODES:
            b = R.encode(J.make_frame(kind, h, w), QUALITY, mode)
            assert (b"\xff\xdd" in b) == mode.startswith("restart"), f"this Pillow ({PIL.__version__}) writes no DRI for {mode}"
            out[f"s_{h}x{w}_{mode}"] = np.frombuffer(b, np.uint8)
            out[f"p_{h}x{w}_{mode}"] = R.pillow_decode(b)
    path = os.path.join(ROOT, "tests", "golden", "g27_jpeg_streams.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
