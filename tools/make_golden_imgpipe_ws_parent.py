#!/usr/bin/env python
"""tests/golden/g26_imgpipe_ws_parent.json: `DevicePreprocessor.workspace_bytes` on the grid of tests/imgpipe_cases.py (every subset of the
JPEG, pre-resize, jitter and main stages, the 1080 x 1920 -> 64 geometry beyond the fused kernel's bound) and `jpeg_table`'s sizes, taken from a
build of the commit BEFORE the preprocessor's plan became a list of stages.  Needs an MI355X (the preprocessor has no CPU route).
tests/test_gpu_imgpipe.py compares the current planner with it byte for byte, so the file is regenerated only on purpose, from a checkout of
that commit with this tool and tests/imgpipe_cases.py copied in:
    python tools/make_golden_imgpipe_ws_parent.py [output.json]"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv) -> None:
    from vlatouch import _lib as L
    from tests import imgpipe_cases as K
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", K.GOLDEN_NAME)
    sizes = K.workspace_sizes()
    with open(out, "w") as f:
        json.dump({"csrc_sha16": L.csrc_sha16(), "bytes": sizes}, f, indent=0)
        f.write("\n")
    print(f"{len(sizes)} numbers -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
