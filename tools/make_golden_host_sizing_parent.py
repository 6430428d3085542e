#!/usr/bin/env python
"""tests/golden/g24_host_sizing_parent.json: what the host drivers size (weight counts, workspaces, derived weight copies, the fused U-Net plan)
on the grid of tests/host_sizing_cases.py, taken from a build of the commit BEFORE the drivers' carver, element-size table and `create`
preamble moved into csrc/vt_host.h.  Needs no GPU.  tests/test_host_sizing_parent.py compares the current drivers with it byte for byte, so the
file is regenerated only on purpose, from a checkout of that commit with this tool and tests/host_sizing_cases.py copied in:
    python tools/make_golden_host_sizing_parent.py [output.json]"""
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
    from tests import host_sizing_cases as K
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", K.GOLDEN_NAME)
    sizes = K.sizing()
    with open(out, "w") as f:
        json.dump({"csrc_sha16": L.csrc_sha16(), "bytes": sizes}, f, indent=0)
        f.write("\n")
    print(f"{len(sizes)} numbers -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
