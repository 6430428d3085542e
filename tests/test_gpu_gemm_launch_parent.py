"""The GEMM family's launchers after their shared host idioms (the (a_dtype, c16) dispatch, the tile counts, the 256-square family's 32-bit offset
limit) were stated once, and the kernels after their tile order and DMA staging moved into csrc/vt_gemm_tile.h: sha256 for sha256 what the commit
before enqueued on an MI355X (tests/golden/g26_gemm_launch_parent.json, written by tools/make_golden_gemm_launch_parent.py and never regenerated to
make this pass), and every output against an fp64 product computed on the device.  The cases are tests/gemm_launch_cases.py's: one per template
instantiation a launcher can choose, at the smallest shape that routes there.  Before recording, the cases ran twice in separate processes on that
commit; all digests agreed between the two runs, so none was dropped.  One test per route, so that a difference names its launcher.  Each fp64 figure is
printed before it is asserted (pytest -s / -rP shows them)."""
import json
import os

import pytest

from tests import cases
from tests import gemm_launch_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        return json.load(f)["sha256"]


def test_the_record_holds_every_route(want):
    assert sorted({k for k in want for r in K.ROUTES if k.startswith(r + "/")}) == sorted(want)
    assert all(any(k.startswith(r + "/") for k in want) for r in K.ROUTES)


@pytest.mark.parametrize("route", list(K.ROUTES))
def test_launches_are_the_parents(want, route):
    res = K.gemm_launch_cases("cuda:0", [route])
    for k, (err, bar) in res.err.items():
        print(f"[gemm_launch] {k}: {err:.3e} (bar {bar:.0e})")
    exp = {k: v for k, v in want.items() if k.startswith(route + "/")}
    assert list(res.sha) == list(exp)
    diff = [k for k in exp if res.sha[k] != exp[k]]
    assert not diff, diff
    bad = {k: v for k, v in res.err.items() if not v[0] < v[1]}          # a NaN fails here too
    assert not bad, bad
