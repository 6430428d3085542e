#!/usr/bin/env python
"""tests/golden/g24_drivers_parent.json: sha256 digests of what the engines give on the cases of tests/driver_cases.py (U-Net forward and sampler
on both drivers, DINOv2 / SigLIP, T5, LSTM, RDT forward and sample), taken on an MI355X from a tree whose vlatouch/ and csrc/ were those of the
commit BEFORE the host drivers' shared idioms moved into csrc/vt_host.h.  tests/test_gpu_drivers_parent.py compares the current drivers with
it, so the file is regenerated only on purpose, from a checkout of that commit with this tool and tests/driver_cases.py copied in:
    python tools/make_golden_drivers_parent.py [output.json]
Run it twice, in two processes, and keep only the groups whose digests agree: a case that differs between two runs of one build is no referee
(`--keep-equal a.json b.json out.json` merges two such files and names what it dropped).  The cases use the engines' public surface only, so
they run on that commit unchanged.  `csrc_sha16` records which kernel sources the library the digests came from was built of."""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def keep_equal(a_path: str, b_path: str, out: str) -> None:
    a, b = json.load(open(a_path)), json.load(open(b_path))
    assert a["csrc_sha16"] == b["csrc_sha16"] and list(a["sha256"]) == list(b["sha256"])
    unstable = [k for k in a["sha256"] if a["sha256"][k] != b["sha256"][k]]
    a["sha256"] = {k: v for k, v in a["sha256"].items() if k not in unstable}
    with open(out, "w") as f:
        json.dump(a, f, indent=1)
        f.write("\n")
    print(f"{len(a['sha256'])} digests -> {out}; differing between the two runs (dropped): {unstable or 'none'}")


def main(argv) -> None:
    if argv and argv[0] == "--keep-equal":
        return keep_equal(*argv[1:4])
    from vlatouch import _lib as L
    from tests import driver_cases as K
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", K.GOLDEN_NAME)
    digests = K.driver_cases("cuda:0")
    with open(out, "w") as f:
        json.dump({"csrc_sha16": L.csrc_sha16(), "sha256": digests}, f, indent=1)
        f.write("\n")
    print(f"{len(digests)} digests -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
