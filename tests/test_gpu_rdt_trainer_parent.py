"""`RdtTrainer` after `get_loss` was cut into stages (inputs, a forward that returns the tape, the loss, a backward that consumes it; one
block forward / backward; the attention sub-block the two attentions share stated once) and `optimizer_step` / `ema_step` got one way of
closing a window: sha256 for sha256 what the trainer of the commit before gave on an MI355X (tests/golden/g23_rdt_trainer_parent.json,
written by tools/make_golden_rdt_trainer_parent.py and never regenerated to make this pass).  The cases are tests/rdt_trainer_cases.py's:
loss, every gradient, parameter, EMA shadow and moment, the norm, the counters and the fp16 scaler's trajectory on seven small runs that
between them take every branch of the forward, the backward and the step.  The grouped trainer is covered through
tests/test_gpu_rdt_dp.py, which pins it bit for bit to the one-process trainer with a window of two."""
import json
import os

import pytest

from tests import cases
from tests import rdt_trainer_cases as K

pytestmark = pytest.mark.gpu


def test_results_are_the_parents():
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        want = json.load(f)["sha256"]
    got = K.trainer_cases("cuda:0")
    assert list(got) == list(want)
    diff = K.differing(want, got)
    assert not diff, diff
