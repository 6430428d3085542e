"""The RDT training kernels after their dtype dispatch (DISPATCH_T, csrc/vt_common.h) and their walk over a chunk of the multi-tensor table
(mt_chunk / mt_walk, csrc/vt_optim.h) were each stated once: sha256 for sha256 what a library built from the commit before gave on an MI355X
(tests/golden/g22_train_kernels_parent.json, written by tools/make_golden_bf16_train.py --cases parent and never regenerated to make this
pass).  The cases are tests/train16_cases.py's second set: the element-wise and attention-backward kernels on fp32 and fp16 operands,
vt_mse_loss_scaled, the typed column sum / add / column copy at fp32, vt_sample_metrics in the three dtypes, and the eight table kernels
over tensors of 1 .. 3 * 4096 + 5 elements, 16-byte aligned and not, digests taken over whole buffers with their guard words."""
import json
import os

import pytest

from tests import cases
from tests import train16_cases as K

pytestmark = pytest.mark.gpu


def test_results_are_the_parents():
    with open(os.path.join(cases.GOLDEN, K.PARENT_GOLDEN_NAME)) as f:
        want = json.load(f)["sha256"]
    got = K.parent_cases("cuda:0")
    assert list(got) == list(want)
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, diff
