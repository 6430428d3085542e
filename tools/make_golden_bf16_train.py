#!/usr/bin/env python
"""tests/golden/g20_bf16_train_kernels.json: sha256 digests of what the bf16 RDT training kernels give on the two saved cases of
tests/train16_cases.py, taken on an MI355X from a library built at the commit BEFORE those kernels became templates on the 16-bit type (the
commit before the fp16 training mode).  The fp16 kernel test compares the current build with it, so the file is regenerated only on purpose:
build that commit's csrc/ into a library of its own and point VLATOUCH_LIB at it,
    VLATOUCH_LIB=/path/to/that/libvlatouch_hip.so python tools/make_golden_bf16_train.py [output.json]
(that library lacks the entry points added since: `--skip-missing` drops them from the binding table for this run).

`--cases parent` writes tests/golden/g22_train_kernels_parent.json instead: the second set of tests/train16_cases.py (fp32 and fp16
instantiations, vt_sample_metrics, the multi-tensor table kernels), taken the same way from a library built at the commit BEFORE the dtype
dispatch and the chunk walk of those kernels were each stated once.  That commit exports every symbol, so no `--skip-missing`."""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv) -> None:
    import ctypes as C

    from vlatouch import _lib as L
    from tests import train16_cases as K
    args = [a for a in argv if a != "--skip-missing"]
    which = "bf16"
    if "--cases" in args:
        i = args.index("--cases")
        which = args[i + 1]
        del args[i:i + 2]
    name, cases = {"bf16": (K.GOLDEN_NAME, K.bf16_saved_cases), "parent": (K.PARENT_GOLDEN_NAME, K.parent_cases)}[which]
    if "--skip-missing" in argv:
        raw = C.CDLL(L.LIB_PATH)
        for name in [n for n in L.SIGNATURES if not hasattr(raw, n)]:
            print(f"not exported by {L.LIB_PATH}: {name}")
            del L.SIGNATURES[name]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", name)
    digests = cases("cuda:0")
    with open(out, "w") as f:
        json.dump({"library": os.path.basename(L.LIB_PATH), "sha256": digests}, f, indent=1)
        f.write("\n")
    print(f"{len(digests)} digests -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
