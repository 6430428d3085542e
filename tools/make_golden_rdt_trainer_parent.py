#!/usr/bin/env python
"""tests/golden/g23_rdt_trainer_parent.json: sha256 digests of what `RdtTrainer` gives on the seven runs of tests/rdt_trainer_cases.py (loss
and every gradient of one get_loss; every parameter, EMA shadow and AdamW moment, the norm, the counters and the fp16 scaler's trajectory after
a few train_steps), taken on an MI355X from a tree whose vlatouch/ and csrc/ were those of the commit BEFORE get_loss was cut into stages and
the ways of closing an accumulation window became one.  tests/test_gpu_rdt_trainer_parent.py compares the current trainer with it, so the file
is regenerated only on purpose, from a checkout of that commit with this tool and tests/rdt_trainer_cases.py copied in:
    python tools/make_golden_rdt_trainer_parent.py [output.json]
The cases use the trainer's public surface only, so they run on that commit unchanged.  `csrc_sha16` records which kernel sources the
library the digests came from was built of."""
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
    from tests import rdt_trainer_cases as K
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", K.GOLDEN_NAME)
    digests = K.trainer_cases("cuda:0")
    with open(out, "w") as f:
        json.dump({"csrc_sha16": L.csrc_sha16(), "sha256": digests}, f, indent=1)
        f.write("\n")
    print(f"{len(digests)} digests -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
