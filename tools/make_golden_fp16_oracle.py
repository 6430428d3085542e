#!/usr/bin/env python
"""tests/golden/g21_fp16_oracle_errors.json: what the oracle run in fp16 on the CPU under the static loss scale 1024 reaches against fp64 autograd
(tests/rdt_train16_ref.py), per tensor and over all parameters, on `RDT_TINY` (B 3, 12 language tokens) and `RDT_WIDE` (B 2, 20): the e_ref of
tests/test_gpu_rdt_train_fp16.py::test_gradients_fp16.  Recorded because torch's fp16 matmul on a CPU without native half arithmetic takes
over a minute for `RDT_WIDE`; tests/test_loss_scale_host.py recomputes the `RDT_TINY` half against it.
    python tools/make_golden_fp16_oracle.py"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    from tests import rdt_train16_ref as R16
    out = {"loss_scale": R16.ORACLE_SCALE}
    for name in ("tiny", "wide"):
        out[name] = R16.oracle_errors_fresh(name)
        print(name, out[name]["total_error"] / out[name]["grad_norm"])
    with open(os.path.join(ROOT, "tests", "golden", R16.ORACLE_GOLDEN), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
