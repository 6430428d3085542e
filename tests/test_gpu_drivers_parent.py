"""The host drivers after their shared idioms moved into csrc/vt_host.h (CK, the element size of a dtype code, the workspace carver, the `create`
checks and weight cursor), the zeroed Linear block into csrc/vt_gemm.h, and the engines' handle protocol into one base class: sha256 for
sha256 what the drivers of the commit before enqueued on an MI355X (tests/golden/g24_drivers_parent.json, written by
tools/make_golden_drivers_parent.py and never regenerated to make this pass).  The cases are tests/driver_cases.py's: every engine at the
smallest shapes that take each branch of its driver.  Before recording, the cases ran twice in separate processes on that commit; all 51
digests agreed between the two runs, so none was dropped.  One test per group, so that a difference names its driver."""
import json
import os

import pytest

from tests import cases
from tests import driver_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        return json.load(f)["sha256"]


def test_the_record_holds_every_case(want):
    assert sorted({k for k in want for g in K.GROUPS if k.startswith(g + "/")}) == sorted(want)
    assert all(any(k.startswith(g + "/") for k in want) for g in K.GROUPS)


@pytest.mark.parametrize("group", list(K.GROUPS))
def test_outputs_are_the_parents(want, group):
    got = K.driver_cases("cuda:0", [group])
    exp = {k: v for k, v in want.items() if k.startswith(group + "/")}
    assert list(got) == list(exp)
    diff = [k for k in exp if got[k] != exp[k]]
    assert not diff, diff
