#!/usr/bin/env python
"""tests/golden/g26_gemm_launch_parent.json: sha256 digests of what the GEMM family's launchers enqueue on the cases of tests/gemm_launch_cases.py
(one case per template instantiation of the PWS / PW / PPK / PT / PP / GLDS / F32R launchers), taken on an MI355X from a tree whose csrc/ was that of
the commit BEFORE the family's tile order, DMA staging and launch table were stated once (csrc/vt_gemm_tile.h, vt_gemm_route.h).
tests/test_gpu_gemm_launch_parent.py compares the current launchers with it, so the file is regenerated only on purpose, from a checkout of that commit
with this tool and tests/gemm_launch_cases.py copied in:
    python tools/make_golden_gemm_launch_parent.py [output.json]
Run it twice, in two processes, and keep only the digests that agree: a case that differs between two runs of one build is no referee
(`--keep-equal a.json b.json out.json` merges two such files and names what it dropped).  Every kernel here is deterministic, so none should be.
The fp64 comparisons of the cases are printed and asserted here too.  `csrc_sha16` records which kernel sources the library was built of."""
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
    from tests import gemm_launch_cases as K
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", K.GOLDEN_NAME)
    res = K.gemm_launch_cases("cuda:0")
    for k, (err, bar) in res.err.items():
        print(f"{k}: {err:.3e} (bar {bar:.0e})")
    with open(out, "w") as f:
        json.dump({"csrc_sha16": L.csrc_sha16(), "sha256": res.sha}, f, indent=1)
        f.write("\n")
    print(f"{len(res.sha)} digests -> {out}")
    bad = {k: v for k, v in res.err.items() if not v[0] < v[1]}
    assert not bad, bad


if __name__ == "__main__":
    main(sys.argv[1:])
