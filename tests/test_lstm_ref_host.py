"""tests/lstm_ref.py held to two independent statements on the CPU (torch.nn.LSTM in float64; the fp32 oracle), its planted mistakes shown to
move the result by a multiple of every bar of tests/test_gpu_lstm.py, and its grid shown to name every instantiation of lstm_seq_kernel.

Measured: the cell stack equals torch.nn.LSTM exactly; the smallest planted-mistake shift is 1.06e-1 (the zeroed state column at
h256l2-s10f3-b16t1, one tick), 3.5 x the bf16 bar; the saturated case's oracle is 1.9e-6 from float64."""
import pytest
import torch

from oracle import controller as oc
from tests import lstm_ref as R

torch.set_grad_enabled(False)

ORACLE_BAR = 3e-6            # fp32 oracle against float64 (measured over the grid: at most 2.1e-6, h384l3-s16f32-b19t5)
# the pairs vt_lstm_create accepts, written out: hidden 128 / 256 with 1..4 layers, 384 with 1..3 (csrc/vt_lstm.hip)
ACCEPTED = [(128, 1), (128, 2), (128, 3), (128, 4), (256, 1), (256, 2), (256, 3), (256, 4), (384, 1), (384, 2), (384, 3)]
REFUSED = [(384, 4), (64, 2), (200, 2), (512, 2), (256, 0), (256, 5)]


def oracle_fp32(m, i, layers):
    h, c, outs = i["h0"].clone(), i["c0"].clone(), []
    for t in range(i["vla_n"].shape[1]):
        o, h, c = oc.lstm_step(m, i["obs_cond"], i["vla_n"][:, t], i["force"][:, t], h, c, layers)
        outs.append(o)
    return torch.stack(outs, dim=1), h, c


@pytest.mark.parametrize("hidden,layers", [(128, 3), (256, 4)])
def test_cell_stack_equals_torch_lstm_fp64(hidden, layers):
    case = R.Case(hidden, layers, 10, 3, 19, 5)
    sd, i = R.case_mods(case)["lstm"], R.inputs(case)
    net = torch.nn.LSTM(hidden // 2 + case.S, hidden, num_layers=layers, batch_first=True).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    x = torch.randn(case.B, case.T, hidden // 2 + case.S, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    want, (hn, cn) = net(x, (i["h0"].double(), i["c0"].double()))
    sd64 = {k: v.double() for k, v in sd.items()}
    h, c, tops = i["h0"].double(), i["c0"].double(), []
    for t in range(case.T):
        top, h, c = R.cell_stack(sd64, x[:, t], h, c, layers)
        tops.append(top)
    err = R.max_err((torch.stack(tops, dim=1), h, c), (want, hn, cn))
    print(f"lstm-ref cell stack h{hidden}l{layers}: max|ref - nn.LSTM| = {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_reference_equals_fp32_oracle(case):
    got = oracle_fp32(R.case_mods(case), R.inputs(case), case.layers)
    err = R.max_err(got, R.case_reference(case))
    print(f"lstm-ref oracle {case.id}: max|oracle fp32 - fp64| = {err:.2e}")
    assert err < ORACLE_BAR


def test_saturated_case_oracle_within_bar():
    """The saturated-gate case of tests/test_gpu_lstm.py is one the fp32 oracle itself resolves: otherwise the kernel's fp32 bar would be asking
    for more than fp32 holds."""
    case, i = R.SATURATED, R.inputs(R.SATURATED)
    m = R.scaled(R.case_mods(case), R.SATURATED_SCALE)
    ref = R.reference(m, i["obs_cond"], i["vla_n"], i["force"], i["h0"], i["c0"], case.layers)
    err = R.max_err(oracle_fp32(m, i, case.layers), ref)
    z = i["h0"][0].double() @ m["lstm"]["weight_hh_l0"].double().T
    print(f"lstm-ref saturated x{R.SATURATED_SCALE:g}: max|oracle fp32 - fp64| = {err:.2e}; |h0 W_hh^T| reaches {float(z.abs().max()):.1f}")
    assert err < ORACLE_BAR


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_planted_mistakes_move_the_result(case):
    """Each of MISTAKES shifts (out, h, c) by at least 10 x the fp32 and x3 bars and 3 x the bf16 bar: a kernel that made it could not pass."""
    i, ref = R.inputs(case), R.case_reference(case)
    need = max(10 * R.BARS["fp32"], 10 * R.BARS["x3"], 3 * R.BARS["bf16"])
    shifts = {}
    for mistake in R.MISTAKES:
        got = R.reference(R.case_mods(case), i["obs_cond"], i["vla_n"], i["force"], i["h0"], i["c0"], case.layers, mistake)
        shifts[mistake] = R.max_err(got, ref)
    worst = min(shifts, key=shifts.get)
    print(f"lstm-ref mistakes {case.id}: smallest shift {shifts[worst]:.2e} ({worst})")
    assert shifts[worst] >= need, shifts


def test_grid_names_every_instantiation():
    pairs = {(c.hidden, c.layers) for c in R.CASES}
    assert pairs == set(ACCEPTED) and not pairs & set(REFUSED)
    assert sorted((c.hidden, c.layers) for c in R.PAIR_CASES) == ACCEPTED            # each once, at the common (S, F, B, T)
    assert all((c.S, c.F, c.B, c.T) == (10, 3, 19, 5) for c in R.PAIR_CASES)
    assert len(R.WIDTH_CASES) == 9 and {(c.S, c.F) for c in R.WIDTH_CASES} == {(16, 32), (1, 1), (7, 17)}
    assert [(c.B, c.T) for c in R.BLOCK_CASES] == [(16, 1), (17, 5)]
    assert len(set(R.CASES)) == len(R.CASES) == 22 and R.MODES == ("fp32", "x3", "bf16")
    for c in R.CASES:                                                               # every batch row distinct
        i = R.inputs(c)
        for k in ("obs_cond", "vla_n", "force"):
            rows = i[k].reshape(c.B, -1)
            assert len({tuple(r.tolist()) for r in rows}) == c.B, (c, k)
