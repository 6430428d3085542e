"""CPU: the fp64 sampler reference of tests/si_sample_ref.py, which tests/test_gpu_si_sampler.py holds the kernels to.

(a) it reproduces the trajectories captured from the reference (tests/golden/g2_si_*), at the bar test_oracle_golden.py uses;
(b) on float64 nets it agrees with oracle/interpolant.py;
(c) its closed form for constant nets equals the integration through the (constant-output) networks;
(d) the GPU sweep has the power it claims: every planted mistake moves the fp64 result by at least ten times the bar the GPU test asserts,
    in at least one case of the sweep.  A condition on the sweep's inputs: if it fails, the inputs change, not the factor."""
import functools

import numpy as np
import pytest
import torch

from oracle import interpolant as oi, unet1d as ou
from tests import cases, si_sample_ref as ref
from tests.test_oracle_golden import DIRECTION_CASES, SCHEDULE_CASES

torch.set_grad_enabled(False)
G = lambda n: np.load(f"{cases.GOLDEN}/{n}.npz")
GPU_BAR = 2e-4          # the widest bar of the GPU sweep (split-bf16 engine); the fp32 engine's is 1e-4


@functools.lru_cache(maxsize=None)
def production_sd64():
    return {k: v.double() for k, v in cases.si_net_sd("ema").items()}


GOLDEN_CASES = ([("traj_T16", "vs", 10, ref.GAMMAS[0], ref.EPSILONS[0], 1.0, "forward")] +
                [(tag, sde, 8, gt, et, 1.0, "forward") for tag, sde, gt, et in SCHEDULE_CASES] +
                [(tag, sde, 8, ref.GAMMAS[0], ref.EPSILONS[0], sw, direction) for tag, sde, sw, direction in DIRECTION_CASES])


@pytest.mark.parametrize("tag,sde,steps,gt,et,sw,direction", GOLDEN_CASES)
def test_sample64_reproduces_reference_trajectories(tag, sde, steps, gt, et, sw, direction):
    g = G(f"g2_si_{tag}")
    x0, cond, _ = cases.si_inputs(2, 16)
    traj = ref.sample64(production_sd64(), ref.net_names(sde), x0, cond, torch.from_numpy(g["z"]), steps, 0.03, gt, et, sde, direction, sw)
    assert traj.dtype == torch.float64 and traj.shape == g["traj"].shape
    want = g["traj"].astype(np.float64)
    e = np.abs(traj.numpy() - want)
    print(f"{tag}: max abs err {e.max():.3e}, max rel {np.max(e / np.maximum(1.0, np.abs(want))):.3e}")
    assert np.all(e <= 5e-5 * np.maximum(1.0, np.abs(want))), (tag, float(e.max()))


def test_float64_state_dict_gives_float64_forward():
    sd = ref.sweep_sd()
    x0, cond, _ = ref.inputs(2, 8, 10, 1)
    t = torch.full((2,), 0.3)
    y32 = ou.unet_forward(sd, "v_net.", x0, t, cond, n_down=2)
    y64 = ou.unet_forward({k: v.double() for k, v in sd.items()}, "v_net.", x0, t, cond, n_down=2)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    e = float((y32.double() - y64).abs().max())
    assert 0.0 < e < 2e-5 * max(1.0, float(y64.abs().max())), e


@functools.lru_cache(maxsize=None)
def sweep_sd64():
    return {k: v.double() for k, v in ref.sweep_sd().items()}


@functools.lru_cache(maxsize=None)
def sweep_traj(case, mistake=None, beta_max=ref.SWEEP_BETA):
    gt, et, sde, direction = case
    x0, cond, z = ref.inputs(ref.SWEEP_B, ref.SWEEP_T, 10, ref.SWEEP_STEPS)
    return ref.sample64(sweep_sd64(), ref.net_names(sde), x0, cond, z, ref.SWEEP_STEPS, beta_max, gt, et, sde, direction, ref.SWEEP_WEIGHT, mistake=mistake)


def step_scale(traj):
    """max(1, max |traj[k]|) per state, shaped to broadcast against the trajectory."""
    return traj.abs().flatten(1).max(dim=1).values.clamp(min=1.0)[:, None, None, None]


@pytest.fixture
def exact_sqrt(monkeypatch):
    """torch's CPU float32 sqrt is one ulp off on some inputs, and not on the same ones on every machine; eps = 1 - sqrt(t) at t = 0.999 turns
    that ulp into 1e-4 of the coefficient.  The oracle's schedules get the correctly rounded root (the float64 root, rounded once) that
    sample64 and the kernels' host code use."""
    real = torch.sqrt
    monkeypatch.setattr(torch, "sqrt", lambda x: real(x.double()).float() if x.dtype == torch.float32 else real(x))


@pytest.mark.parametrize("case", ref.SWEEP, ids=ref.case_id)
def test_sample64_agrees_with_oracle_on_float64_nets(case, exact_sqrt):
    gt, et, sde, direction = case
    sd = sweep_sd64()
    first, score = ref.net_names(sde)
    x0, cond, z = ref.inputs(ref.SWEEP_B, ref.SWEEP_T, 10, ref.SWEEP_STEPS)
    a = lambda x, t, c: ou.unet_forward(sd, first + ".", x, t, c, n_down=2)
    s = lambda x, t, c: ou.unet_forward(sd, score + ".", x, t, c, n_down=2)
    fn = oi.sde_bs if sde == "bs" else oi.sde_vs
    _, xs = fn(a, s, x0.double(), cond.double(), z.double(), ref.SWEEP_STEPS, ref.SWEEP_BETA, gt, et, ref.SWEEP_WEIGHT, direction)
    want = torch.stack(xs)
    got = sweep_traj(case)
    assert want.dtype == torch.float64 and got.dtype == torch.float64
    rel = float(((got - want).abs() / step_scale(want)).max())
    assert rel <= 1e-6, (case, rel)


CLOSED_FORM_EXTRA = [(ref.SWEEP[13], 1, 7, 1, 8), (ref.SWEEP[13], 65, 16, 1, 8), (ref.SWEEP[46], 64, 10, 3, 64)]


@pytest.mark.parametrize("case,steps,dim,B,T", [(c, ref.SWEEP_STEPS, 10, ref.SWEEP_B, ref.SWEEP_T) for c in ref.SWEEP[::7]] + CLOSED_FORM_EXTRA)
def test_closed_form_equals_integration_through_constant_nets(case, steps, dim, B, T):
    gt, et, sde, direction = case
    sd = ref.constant_sd(dim)
    nets = ref.net_names(sde)
    v, s = ref.constants(sd, nets)
    assert len(set(v.tolist() + s.tolist())) == 2 * dim
    x0, cond, z = ref.constant_inputs(B, T, dim, steps)
    args = (steps, ref.SWEEP_BETA, gt, et, sde, direction, ref.SWEEP_WEIGHT)
    cf, M = ref.closed_form64(v, s, x0, z, *args)
    through = ref.sample64(sd, nets, x0, cond, z, *args)
    assert cf.shape == through.shape == (steps + 1, B, T, dim) and M.shape == (steps, B, T, dim)
    assert torch.equal(cf[0], x0.double())
    assert float(((cf - through).abs() / step_scale(cf)).max()) <= 1e-12
    # each state stays within the magnitude sum of the step that made it
    assert bool((cf[1:].abs() <= M * (1 + 1e-12)).all())
    det, _ = ref.closed_form64(v, s, x0, None, *args)
    det_through = ref.sample64(sd, nets, x0, cond, None, *args)
    assert float(((det - det_through).abs() / step_scale(det)).max()) <= 1e-12
    if et != "0":
        assert not torch.equal(det, cf)


def applies(mistake, case):
    """The cases in which a mistake can show at all."""
    gt, et, sde, direction = case
    return {"net_time": direction == "backward", "eps_in_b": direction == "backward" and sde == "vs", "noise_eps": direction == "backward",
            "sign": direction == "backward", "gdg_for_bs": sde == "bs"}.get(mistake, True)


@pytest.mark.parametrize("mistake", ref.MISTAKES[:8])
def test_sweep_shows_planted_mistake(mistake):
    """(d): the mistake moves a state of the fp64 trajectory by >= 10 x the GPU bar relative to max(1, scale_k) in at least one sweep case."""
    worst = 0.0
    for case in ref.SWEEP:
        if not applies(mistake, case):
            continue
        good, bad = sweep_traj(case), sweep_traj(case, mistake)
        worst = max(worst, float(((bad - good).abs() / step_scale(good)).max()))
        if worst >= 10 * GPU_BAR:
            break
    print(f"{mistake}: shift {worst:.3e} (needed {10 * GPU_BAR:.1e}) at {ref.case_id(case)}")
    assert worst >= 10 * GPU_BAR, (mistake, worst)


def test_update_only_test_shows_the_gamma_constant():
    """(d), ninth mistake: sqrt(2) for the literal 1.4142 in gamma_inv moves the closed form by >= 10 x the rounding bound of the update-only
    GPU test at some element of some sweep case (the sweep against the networks, at 1e-4 relative, cannot see it).  The constant moves gamma_inv
    by sqrt(2) / 1.4142 - 1 = 9.59e-6 and the bound is 16 * 2^-24 = 9.54e-7 of the step's magnitude sum, so the ratio cannot exceed 10.06: it
    takes an element whose first step is all score term, which is what constant_inputs and constant_sd's channel 0 provide (10.10 measured)."""
    worst = 0.0
    for case in ref.SWEEP:
        gt, et, sde, direction = case
        v, s = ref.constants(ref.constant_sd(10), ref.net_names(sde))
        x0, _, z = ref.constant_inputs(ref.SWEEP_B, ref.SWEEP_T, 10, ref.SWEEP_STEPS)
        args = (ref.SWEEP_STEPS, ref.SWEEP_BETA, gt, et, sde, direction, ref.SWEEP_WEIGHT)
        good, M = ref.closed_form64(v, s, x0, z, *args)
        bad, _ = ref.closed_form64(v, s, x0, z, *args, mistake="sqrt2")
        worst = max(worst, float(((bad - good).abs()[1:] / ref.rounding_bound(M)[1:]).max()))
    print(f"sqrt2: largest shift / bound {worst:.1f}")
    assert worst >= 10.0, worst
