"""The host half of data-parallel RDT fine-tuning: the per-rank plan stream of `EpisodeStore.plan_batches`, the `comm_dtype` keyword,
and the bf16 exchange's host statement (tests/rdt_dp_ref.py) against a real two-process gloo
all-reduce of bf16 CPU tensors.  No GPU."""
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import rdt_data_ref as D
from tests import rdt_dp_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 12


def _store():
    from vlatouch.rdt_data import EpisodeStore
    return EpisodeStore(D.FIXTURE_DIR, dataset_name=D.DATASET_NAME, dataset_names=D.DATASET_NAMES, control_freq={D.DATASET_NAME: D.CONTROL_FREQ})


def _stream(store, seed, **kw):
    """plan_batches with the three random streams (numpy, random, torch) seeded by `seed`, every decision drawn (D.G19_KW)."""
    return store.plan_batches(3, np_rng=np.random.RandomState(seed), rng=random.Random(seed), generator=torch.Generator().manual_seed(seed),
                              **D.G19_KW, **kw)


@pytest.mark.parametrize("world", [2, 3])
def test_plan_batches_of_a_rank_are_every_wth_of_the_one_process_stream(world):
    """12 rounds of W ranks: rank r's plans equal plans r, r + W, ... of the ungrouped stream, field by field; the ranks' streams together are
    the ungrouped stream and share nothing."""
    store = _store()
    one = _stream(store, 11)
    want = [[P.plan_fields(p) for p in next(one)] for _ in range(ROUNDS * world)]
    assert len({tuple(b) for b in want}) == len(want), "the stream must not repeat itself, or the test shows nothing"
    assert any(f[9] is not None for b in want for f in b) and any(j is not None for b in want for f in b for j in f[11]), "noise and jitter are drawn"
    for r in range(world):
        it = _stream(store, 11, rank=r, world_size=world)
        for n in range(ROUNDS):
            got = [P.plan_fields(p) for p in next(it)]
            assert got == want[r + n * world], (world, r, n)
    assert [P.plan_fields(p) for p in next(store.plan_batches(3, np_rng=np.random.RandomState(11), rng=random.Random(11),
                                                                generator=torch.Generator().manual_seed(11), **D.G19_KW))] == want[0]


def test_plan_batches_refuses_a_rank_outside_the_world():
    store = _store()
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            next(store.plan_batches(3, rank=rank, world_size=world, np_rng=np.random.RandomState(0), rng=random.Random(0)))


def test_unknown_comm_dtype_is_refused_before_anything_is_built():
    from vlatouch.rdt_train import COMM_DTYPES, RdtTrainer
    assert COMM_DTYPES == ("fp32", "bf16")
    for bad in ("fp16", "float32", None):
        with pytest.raises(ValueError, match="comm_dtype"):
            RdtTrainer({}, heads=2, horizon=8, action_dim=16, comm_dtype=bad)
    with pytest.raises(ValueError, match="comm_bucket_bytes"):
        RdtTrainer({}, heads=2, horizon=8, action_dim=16, comm_bucket_bytes=0)


def test_statement_rounds_ties_to_even_and_adds_once():
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    bits = lambda t: t.view(torch.int16).tolist()
    assert bits(P.bf16_rne(f(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20))) == bits(f(1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7).bfloat16())
    # 1 + 2^-7 and 2^-8 are bf16 values; their sum 1 + 3 * 2^-8 is a tie and goes to the even neighbour 1 + 2^-6
    assert bits(P.bf16_exchange(f(1 + 2.0 ** -7), f(2.0 ** -8))) == bits(f(1 + 2.0 ** -6).bfloat16())
    # the operand is rounded first (1 + 2^-8 -> 1), then 257 is the tie between 256 and 258 and goes to 256; the fp32 sum would round to 258
    assert bits(P.bf16_exchange(f(256.0), f(1.0 + 2.0 ** -8))) == bits(f(256.0).bfloat16())
    assert bits(P.bf16_rne(f(256.0) + f(1.0 + 2.0 ** -8))) == bits(f(258.0).bfloat16())


def test_statement_against_gloo_s_two_rank_bf16_all_reduce(tmp_path):
    """bf16(bf16(a) + bf16(b)) of tests/rdt_dp_ref.py, bit for bit, against what two gloo ranks leave after all_reduce(SUM) of their bf16 CPU
    tensors: 200 000 values of mixed magnitude with exact ties among them."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    out = str(tmp_path / "sum.pt")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, "-m", "tests._dp_train_worker", "hostsum", str(r), port, out], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
    got = torch.load(out)
    a, b = P.mixed_values(200_000, 500), P.mixed_values(200_000, 501)
    want = P.bf16_exchange(a, b)
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    assert got.view(torch.int16).equal(want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    fp32_sum = a + b
    assert int((want.float() != fp32_sum).sum()) > 100_000, "the exchange must differ from the fp32 sum, or the test shows nothing"
