"""Data-parallel RDT fine-tuning on the device (vlatouch/rdt_train.py with `process_group=`; vt_grad_fold_pack_multi and vt_grad_unpack_multi
of csrc/vt_train_rdt.hip).

Kernel level, one process, the harness of tests/test_gpu_rdt_accum.py (guarded tensors at aligned and unaligned bases, its sizes): the packed
value of every real element is bit-equal to torch's `.to(bfloat16)` of what vt_grad_accum_multi leaves on a copy of the same inputs, the
padding is zero, nothing else changes, two runs agree; the unpacked accumulators are bit-equal to `comm.float()`.  One departure, with its
reason: torch has no single bf16 encoding of NaN (its CPU conversion gives 0xFFFF where c10's round_to_nearest_even gives 0x7FC0), so where
the fp32 value is NaN the packed element is held to the header's own statement, 0x7FC0, and to being NaN where torch's is.

Trainer level: two ranks sharing cuda:0 over gloo and one rank over RCCL run tests/_dp_train_worker.py, which states what each scenario
asserts; the ranks are started once per module and every test below reads its scenario's line."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from tests.test_gpu_rdt_accum import DEV, GUARD, NAN, SENTINEL, SIZES, _Guarded, _L, _sp, _table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096
BF16_NAN = 0x7FC0


# ------------------------------------------------------------------------------------------------ kernels as units
def _special(x: torch.Tensor, gen) -> torch.Tensor:
    """Sprinkle +-inf, NaN, fp32 subnormals and exact bf16 ties (1 + 2^-8 and odd multiples of 2^-8 above a power of two) into x."""
    n = x.numel()
    pool = torch.tensor([float("inf"), float("-inf"), NAN, 1e-40, -3e-42, 2.0 ** -140, 1 + 2.0 ** -8, -(1 + 3 * 2.0 ** -8), (1 + 5 * 2.0 ** -8) * 2.0 ** -9,
                         (1 + 255 * 2.0 ** -8) * 2.0 ** 7, 2.0 ** -126 * (1 + 2.0 ** -8)])
    pick = torch.rand(n, generator=gen) < 0.15
    return torch.where(pick, pool[torch.randint(0, pool.numel(), (n,), generator=gen)], x)


class _Comm:
    """[8 sentinel bf16 | total elements | GUARD sentinel bf16] on the device: the exchange buffer, 16-byte aligned, with guards."""

    def __init__(self, total: int, fill: torch.Tensor):
        self.total = total
        self.buf = torch.cat([torch.full((8,), SENTINEL).bfloat16(), fill.bfloat16(), torch.full((GUARD,), SENTINEL).bfloat16()]).to(DEV)
        self.ptr = self.buf.data_ptr() + 16
        assert self.ptr % 16 == 0

    def bits(self):
        return self.buf[8:8 + self.total].cpu().view(torch.int16)

    def guards_intact(self):
        b, s = self.buf.cpu().float(), float(torch.tensor(SENTINEL).bfloat16())
        return bool((b[:8] == s).all()) and bool((b[8 + self.total:] == s).all())


def _same_bits(x: torch.Tensor, want: torch.Tensor) -> bool:
    return x.view(torch.int32).equal(want.view(torch.int32))


@pytest.mark.parametrize("pre", [4, 5], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_grad_fold_pack_multi_is_the_rounded_fold(k, pre):
    """k micro-batches: the first k - 1 are folded by vt_grad_accum_multi, the k-th by vt_grad_fold_pack_multi into a NaN-filled bf16 buffer
    and, on a copy of the accumulators, by vt_grad_accum_multi.  See the module docstring for what is compared."""
    L, lib = _L(), _L().lib()
    gen = torch.Generator().manual_seed(900 + 10 * k + pre)
    fresh_host = [[_special(torch.randn(n, generator=gen) * 10 ** float(torch.randint(-3, 3, (1,), generator=gen)), gen) for n in SIZES] for _ in range(k)]
    if k == 1:
        fresh_host[0][4][:3] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)])      # scale 1: these ties reach the rounding as they are
    others_host = [torch.randn(n, generator=gen) for n in SIZES]
    scale = 1.0 / k
    starts, chunk0 = [], 0
    for n in SIZES:
        starts.append(chunk0 * CHUNK)
        chunk0 += (n + CHUNK - 1) // CHUNK
    total = chunk0 * CHUNK

    def run():
        acc = [_Guarded(torch.full((n,), NAN), pre) for n in SIZES]
        p, m, v = ([_Guarded(x, pre) for x in others_host] for _ in range(3))
        tab, chunks = _table(p, acc, m, v, [None] * len(SIZES), SIZES)
        assert chunks * CHUNK == total
        fresh = [[_Guarded(x, pre) for x in gs] for gs in fresh_host]
        ptrs = [torch.tensor([x.ptr for x in fresh[j]], dtype=torch.int64).to(DEV) for j in range(k)]
        for j in range(k - 1):
            L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(ptrs[j]), len(SIZES), chunks, scale, int(j > 0), _sp()), "vt_grad_accum_multi")
        torch.cuda.synchronize()
        before = [a.values() for a in acc]
        comm = _Comm(total, torch.full((total,), NAN))
        L.check(lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(ptrs[k - 1]), len(SIZES), chunks, scale, int(k > 1), comm.ptr, _sp()), "vt_grad_fold_pack_multi")
        torch.cuda.synchronize()
        for what, xs in (("acc", acc), ("p", p), ("m", m), ("v", v)) + tuple((f"fresh{j}", fresh[j]) for j in range(k)):
            for x in xs:
                assert x.guards_intact(), ("guard words", what, x.n)
        assert comm.guards_intact(), "guard words of the bf16 buffer"
        for a, want in zip(acc, before):
            assert _same_bits(a.values(), want), ("the accumulator was written", a.n)
        for j in range(k):
            for x, want in zip(fresh[j], fresh_host[j]):
                assert _same_bits(x.values(), want), ("fresh gradient changed", x.n)
        for xs in (p, m, v):
            for x, want in zip(xs, others_host):
                assert torch.equal(x.values(), want), ("p / m / v changed", x.n)
        # the reference: the same last fold by vt_grad_accum_multi on the accumulators themselves, rounded by torch on the device
        L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(ptrs[k - 1]), len(SIZES), chunks, scale, int(k > 1), _sp()), "vt_grad_accum_multi")
        torch.cuda.synchronize()
        folded = [a.buf[a.pre:a.pre + a.n] for a in acc]
        return comm.bits(), [f.cpu() for f in folded], [f.to(torch.bfloat16).cpu().view(torch.int16) for f in folded]

    (got, folded, want), (again, _, _) = run(), run()
    assert got.equal(again), "two runs differ"
    specials = 0
    for i, n in enumerate(SIZES):
        real = got[starts[i]:starts[i] + n]
        nan = torch.isnan(folded[i])
        assert real[~nan].equal(want[i][~nan]), (n, int((real[~nan] != want[i][~nan]).sum()))
        assert bool((real[nan].to(torch.int32) & 0xFFFF == BF16_NAN).all()), ("a NaN must be packed as 0x7FC0", n)
        assert bool(torch.isnan(want[i][nan].view(torch.bfloat16).float()).all())
        pad = got[starts[i] + n:starts[i] + (n + CHUNK - 1) // CHUNK * CHUNK]
        assert bool((pad == 0).all()), ("padding must be zero", n, int((pad != 0).sum()))
        specials += int(nan.sum()) + int(torch.isinf(folded[i]).sum()) + int(((folded[i] != 0) & (folded[i].abs() < 2.0 ** -126)).sum())
    assert specials > 100, "NaN, inf and subnormal values must reach the rounding"
    pads = torch.ones(total, dtype=torch.bool)
    for i, n in enumerate(SIZES):
        pads[starts[i]:starts[i] + n] = False
    assert not bool(torch.isnan(got.view(torch.bfloat16).float()[pads]).any()), "no NaN of the fill may be left in the padding"
    if k == 1:
        t = got[starts[4]:starts[4] + 3].view(torch.bfloat16).float().tolist()
        assert t == [1.0, 1 + 2.0 ** -6, -1.0], ("ties go to the even neighbour", t)


@pytest.mark.parametrize("pre", [4, 5], ids=["aligned", "unaligned"])
def test_grad_unpack_multi_widens_the_real_elements_only(pre):
    """A bf16 buffer of values everywhere (the padding holds junk on purpose) into NaN-filled accumulators: every accumulator bit-equal to
    comm.float() over its n elements; the buffer, p / m / v and every guard word unchanged; twice, bit-equal."""
    L, lib = _L(), _L().lib()
    gen = torch.Generator().manual_seed(950 + pre)
    starts, chunk0 = [], 0
    for n in SIZES:
        starts.append(chunk0 * CHUNK)
        chunk0 += (n + CHUNK - 1) // CHUNK
    total = chunk0 * CHUNK
    fill = _special(torch.randn(total, generator=gen) * 10.0 ** torch.randint(-3, 3, (total,), generator=gen).float(), gen)
    others_host = [torch.randn(n, generator=gen) for n in SIZES]

    def run():
        acc = [_Guarded(torch.full((n,), NAN), pre) for n in SIZES]
        p, m, v = ([_Guarded(x, pre) for x in others_host] for _ in range(3))
        tab, chunks = _table(p, acc, m, v, [None] * len(SIZES), SIZES)
        comm = _Comm(total, fill)
        before = comm.bits()
        L.check(lib.vt_grad_unpack_multi(L.ptr(tab), comm.ptr, len(SIZES), chunks, _sp()), "vt_grad_unpack_multi")
        torch.cuda.synchronize()
        for what, xs in (("acc", acc), ("p", p), ("m", m), ("v", v)):
            for x in xs:
                assert x.guards_intact(), ("guard words", what, x.n)
        assert comm.guards_intact() and comm.bits().equal(before), "the bf16 buffer, its padding included, must be untouched"
        for xs in (p, m, v):
            for x, want in zip(xs, others_host):
                assert torch.equal(x.values(), want), ("p / m / v changed", x.n)
        return [a.values() for a in acc], before

    (got, bits), (again, _) = run(), run()
    wide = bits.view(torch.bfloat16).float()
    for i, n in enumerate(SIZES):
        assert _same_bits(got[i], again[i]), ("two runs differ", n)
        assert _same_bits(got[i], wide[starts[i]:starts[i] + n]), ("acc != float(comm)", n)


def test_exchange_kernels_refuse_bad_arguments():
    L, lib = _L(), _L().lib()
    t = torch.zeros(CHUNK, device=DEV)
    cols = [[_Guarded(torch.zeros(5), 4)] for _ in range(4)]
    tab, chunks = _table(*cols, [None], [5])
    comm = torch.zeros(CHUNK + 8, dtype=torch.bfloat16, device=DEV)
    ptrs = torch.tensor([t.data_ptr()], dtype=torch.int64).to(DEV)
    assert lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(ptrs), 1, chunks, 1.0, 0, None, _sp()) != 0
    assert lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(ptrs), 1, chunks, 0.0, 0, L.ptr(comm), _sp()) != 0
    assert lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(ptrs), 1, chunks, 1.0, 0, comm.data_ptr() + 2, _sp()) != 0      # not 16-byte aligned
    assert lib.vt_grad_unpack_multi(L.ptr(tab), None, 1, chunks, _sp()) != 0
    assert lib.vt_grad_unpack_multi(L.ptr(tab), comm.data_ptr() + 2, 1, chunks, _sp()) != 0
    assert lib.vt_grad_unpack_multi(L.ptr(tab), L.ptr(comm), 0, chunks, _sp()) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the trainer, over gloo and over RCCL
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _env():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return env


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    """Both ranks' output after all scenarios; the parent kills both children on its time limit."""
    port, tmp = _free_port(), str(tmp_path_factory.mktemp("dp"))
    procs = [subprocess.Popen([sys.executable, "-m", "tests._dp_train_worker", "gloo", str(r), port, tmp], cwd=ROOT, env=_env(),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for r, o in enumerate(outs):
        print(f"---- rank {r}\n" + "\n".join(l for l in o.splitlines() if l.startswith("DP_")))
    return procs, outs


def _ok(two_ranks, scenario):
    procs, outs = two_ranks
    for r, o in enumerate(outs):
        assert any(l.startswith(f"DP_OK {scenario} ") for l in o.splitlines()), f"rank {r} did not pass {scenario!r} (exit {procs[r].returncode}):\n{o[-3000:]}"


def test_rank_0_s_parameters_are_broadcast_at_construction(two_ranks):
    _ok(two_ranks, "broadcast")


def test_ranks_that_disagree_all_raise(two_ranks):
    _ok(two_ranks, "disagreement")


def test_two_ranks_fp32_exchange_is_bit_equal_to_one_process_with_k2(two_ranks):
    _ok(two_ranks, "exact_adamw")


def test_two_ranks_adamw8bit_is_bit_equal_to_one_process_with_k2(two_ranks):
    _ok(two_ranks, "exact_adamw8bit")


def test_two_ranks_k2_against_one_process_k4(two_ranks):
    _ok(two_ranks, "accumulated")


def test_two_ranks_bf16_exchange_is_the_host_statement(two_ranks):
    _ok(two_ranks, "bf16_exchange")


def test_two_ranks_resume_is_exact_with_one_set_of_files(two_ranks):
    _ok(two_ranks, "resume")


def test_two_ranks_sample_eval_is_reduced_over_the_group(two_ranks):
    _ok(two_ranks, "evaluation")


def test_both_ranks_end_clean(two_ranks):
    procs, outs = two_ranks
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"


def test_rccl_world_size_one_exchanges():
    """The "nccl" (= RCCL) backend, world size 1 on cuda:0: the grouped trainer with the fp32 exchange is bit-equal after two steps to the ungrouped
    one with the same k (k = 1 and 2), and with the bf16 exchange its gradients are the bf16 rounding of the ungrouped ones."""
    p = subprocess.run([sys.executable, "-m", "tests._dp_train_worker", "nccl", _free_port()], cwd=ROOT, env=_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    for scenario in ("nccl_fp32_exchange", "nccl_bf16_exchange"):
        assert f"DP_OK {scenario}" in p.stdout, p.stdout[-2000:]
