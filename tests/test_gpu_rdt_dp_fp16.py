"""Data-parallel fp16 fine-tuning: two ranks sharing cuda:0 over gloo run tests/_dp_train16_worker.py, which states each scenario.  Rank 1
gets a non-finite micro-batch: both ranks skip and stay bit-equal (fp32 and bf16 exchange); a clean step is bit-equal to one process with
k = 2; ranks that disagree on loss_scale all raise."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_rdt_dp import ROOT, _env, _free_port

pytestmark = pytest.mark.gpu
SCENARIOS = ("skip_fp32_exchange", "skip_bf16_exchange", "exact_k2", "disagreement")


@pytest.fixture(scope="module")
def two_ranks():
    """Both ranks' output after all scenarios; the parent kills both children on its time limit."""
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, "-m", "tests._dp_train16_worker", str(r), port], cwd=ROOT, env=_env(), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for r, o in enumerate(outs):
        print(f"---- rank {r}\n" + "\n".join(l for l in o.splitlines() if l.startswith("DP_")))
    return procs, outs


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_two_ranks_fp16(two_ranks, scenario):
    procs, outs = two_ranks
    for r, o in enumerate(outs):
        assert any(l.startswith(f"DP_OK {scenario} ") for l in o.splitlines()), f"rank {r} did not pass {scenario!r} (exit {procs[r].returncode}):\n{o[-3000:]}"


def test_both_ranks_end_clean(two_ranks):
    procs, outs = two_ranks
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
