#!/usr/bin/env python
"""Golden results of the JPEG round trip of camera frames (vlatouch/jpegmap.py, csrc/vt_jpegmap.hip), made with Pillow's libjpeg-turbo,
the library cv2 wraps: `Image.save(buf, "JPEG", quality=q)` + `Image.open` of every small test frame of tests/jpeg_ref.py (SHAPES x
CONTENTS) at qualities 95 and 75, in both channel orders ("cv2": the array's channel 0 plays blue's role, i.e. the round trip of
img[..., ::-1], flipped back).  cv2 itself is absent here, so its encoder defaults (quality 95, 4:2:0, islow DCT, fancy up-sampling on
decode) stay UNPINNED; the golden pins the arithmetic of the library.

Stored in tests/golden/g25_jpegmap.npz: `in_<kind>_<h>x<w>` (the input, so a change of the generator shows) and
`out_<kind>_<h>x<w>_q<quality>_<order>`, plus `pillow` and `libjpeg_turbo`, the versions that made them.
    python tools/make_golden_jpegmap.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_ref as J  # noqa: E402


def main() -> None:
    import PIL
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the golden is defined by libjpeg-turbo"
    data = {"pillow": np.array(PIL.__version__), "libjpeg_turbo": np.array(str(features.version("jpg")))}
    for h, w in J.SHAPES:
        for kind in J.CONTENTS:
            a = J.make_frame(kind, h, w)
            data[f"in_{kind}_{h}x{w}"] = a
            for q in J.GOLDEN_QUALITIES:
                for order in J.ORDERS:
                    data[f"out_{kind}_{h}x{w}_q{q}_{order}"] = J.pillow_roundtrip(a, q, order)
    path = os.path.join(ROOT, "tests", "golden", "g25_jpegmap.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(data)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
