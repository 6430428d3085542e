"""GPU: the stochastic-interpolant sampler (vt_si_sample_ex) against the fp64 reference of tests/si_sample_ref.py on every gamma and epsilon
schedule, both integrators and both directions, under all three drivers: the fp32 engine (launch per op, sde_update_kernel), the split-bf16
engine launch per op, and the split-bf16 engine on the fused path (csrc/vt_uconv.hip ufinal_kernel's own Euler–Maruyama update, the VtSdeCoef
table and the per-step FiLM rows of csrc/vt_unet_fused.hip).

  * the sweep: trajectories through a small U-Net pair against sample64, per state k within tol * max(1, max |traj64[k]|),
    tol = 1e-4 (fp32) / 2e-4 (split-bf16, either driver); tests/test_si_sample_ref_host.py proves that these cases and bars would catch a wrong
    backward sign, eps at the wrong time, gdg kept for 'bs', a dropped score weight, the nets at the wrong time and a neighbouring step's FiLM
    row or noise slice;
  * the update alone: nets that return constants exactly, against closed_form64 element-wise within 16 * 2^-24 * (sum of the steps' magnitude
    sums), incl. 1 / 64 / 65 steps (65 leaves the fused path's 64-entry tables and must fall back) and input_dim 7 / 10 / 16.

Worst e_k / max(1, scale_k) measured on the MI355X over the sweep and its extra shapes, weights and widths (bar in brackets):
    fp32 engine                      1.3e-6  [1e-4]   (g0-e0-vs-backward, B 3, T 8)
    split-bf16, launch per op        2.2e-5  [2e-4]   (g2-e2-vs-backward, B 2, T 64; 1.9e-5 over the 60 sweep cases)
    split-bf16, fused                2.1e-5  [2e-4]   (g2-e2-vs-backward, B 2, T 64; 1.8e-5 over the 60 sweep cases)
    fused against launch per op      1.4e-5  [2e-4]
No case needed a bar of its own.  The update alone reaches 0.16 of its rounding bound, the same figure under all three drivers.

The reference evaluates the step coefficients on numpy float32 scalars, not with torch: torch's CPU float32 sqrt is one ulp off on some inputs
(which ones depends on the machine), and for eps = 1 - sqrt(t) at t = 0.999 that ulp is 1.2e-4 of eps: twice the rounding bound of the update.
"""
import functools

import pytest
import torch

from tests import si_sample_ref as ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL = {"fp32": 1e-4, "bf16-ops": 2e-4, "bf16-fused": 2e-4}
DRIVERS = ("fp32", "bf16-ops", "bf16-fused")
# one backward velocity-score and one forward drift-score case on non-default schedules, for the shapes, widths, weights and step counts
PROBES = [("(1-t)^2(2t)^0.5", "1-sqrt(t)", "vs", "backward"), ("(2t(t-1))^0.5", "1-t^2", "bs", "forward")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    """(constant?, input_dim, sde, precision) -> UNetEngine over (v_net | b_net, s_net) of the small U-Net, each built once for the module."""
    from vlatouch.engine import UNetEngine
    built = {}

    def get(const, dim, sde, prec):
        key = (const, dim, sde, prec)
        if key not in built:
            sd = ref.constant_sd(dim) if const else ref.sweep_sd(dim)
            built[key] = UNetEngine(ref.split_nets(sd, ref.net_names(sde)), input_dim=dim, global_cond_dim=ref.NET_COND, down_dims=ref.NET_DIMS,
                                    kernel_size=ref.NET_K, precision=prec, device=dev)
        return built[key]

    for sde in ("vs", "bs"):
        for prec in ("fp32", "bf16"):
            get(False, 10, sde, prec)
    return get


def run_drivers(engines, const, dim, case, x0, cond, z, n_steps, beta_max, score_weight, fused_expected=1):
    """The sampler under the three drivers -> {driver: (xT, traj)} on the host."""
    from vlatouch import _lib as L
    lib = L.lib()
    gt, et, sde, direction = case
    kw = dict(record=True, gamma_type=ref.GAMMAS.index(gt), epsilon_type=ref.EPSILONS.index(et), sde_type=("vs", "bs").index(sde),
              backward=direction == "backward", score_weight=score_weight)
    B, T, _ = x0.shape
    out = {}
    e32, e16 = engines(const, dim, sde, "fp32"), engines(const, dim, sde, "bf16")
    assert e32._fused is None and e16._fused is not None, "only the split-bf16 engine carries the fused weight stream"
    assert lib.vt_unet_fused_covers(e32._h, B, T, n_steps) == 0
    xT, traj = e32.sample(x0, cond, z, n_steps, beta_max, **kw)
    out["fp32"] = (xT.cpu(), traj.cpu())
    try:
        for on, name in ((0, "bf16-ops"), (1, "bf16-fused")):
            lib.vt_tune(7, on)
            assert lib.vt_unet_fused_covers(e16._h, B, T, n_steps) == (fused_expected if on else 0), (name, B, T, n_steps)
            xT, traj = e16.sample(x0, cond, z, n_steps, beta_max, **kw)
            out[name] = (xT.cpu(), traj.cpu())
    finally:
        lib.vt_tune(7, 1)
    return out


@functools.lru_cache(maxsize=None)
def reference(dim, B, T, n_steps, case, beta_max, score_weight, noise):
    gt, et, sde, direction = case
    x0, cond, z = ref.inputs(B, T, dim, n_steps)
    traj = ref.sample64(ref.sweep_sd(dim), ref.net_names(sde), x0, cond, z if noise else None, n_steps, beta_max, gt, et, sde, direction, score_weight)
    return x0, cond, (z if noise else None), traj


def check_against_fp64(engines, dim, B, T, n_steps, case, beta_max=ref.SWEEP_BETA, score_weight=ref.SWEEP_WEIGHT, noise=True):
    x0, cond, z, want = reference(dim, B, T, n_steps, case, beta_max, score_weight, noise)
    got = run_drivers(engines, False, dim, case, x0, cond, z, n_steps, beta_max, score_weight)
    scale = want.abs().flatten(1).max(dim=1).values.clamp(min=1.0)
    assert bool(torch.isfinite(want).all())
    rel = {}
    for name in DRIVERS:
        xT, traj = got[name]
        assert traj.shape == want.shape and traj.dtype == torch.float32
        assert torch.equal(traj[0], x0), name
        assert torch.equal(xT, traj[-1]), name
        rel[name] = (traj.double() - want).abs().flatten(1).max(dim=1).values / scale
        print(f"SI_ERR {name} {float(rel[name].max()):.3e} {ref.case_id(case)} dim{dim} B{B} T{T} w{score_weight} noise{int(noise)}")
    between = (got["bf16-fused"][1].double() - got["bf16-ops"][1].double()).abs().flatten(1).max(dim=1).values / scale
    print(f"SI_ERR fused-vs-ops {float(between.max()):.3e} {ref.case_id(case)}")
    for name in DRIVERS:
        assert bool((rel[name] <= TOL[name]).all()), (name, ref.case_id(case), rel[name].tolist())
    assert bool((between <= 2e-4).all()), (ref.case_id(case), between.tolist())
    return got


@pytest.mark.parametrize("case", ref.SWEEP, ids=ref.case_id)
def test_sweep_against_fp64(engines, case):
    check_against_fp64(engines, 10, ref.SWEEP_B, ref.SWEEP_T, ref.SWEEP_STEPS, case)


@pytest.mark.parametrize("case", PROBES, ids=ref.case_id)
@pytest.mark.parametrize("weight", [1.0, 1.3])
def test_score_weights_against_fp64(engines, case, weight):
    check_against_fp64(engines, 10, ref.SWEEP_B, ref.SWEEP_T, ref.SWEEP_STEPS, case, score_weight=weight)


@pytest.mark.parametrize("case", PROBES, ids=ref.case_id)
def test_deterministic_path_against_fp64(engines, case):
    det = check_against_fp64(engines, 10, ref.SWEEP_B, ref.SWEEP_T, ref.SWEEP_STEPS, case, noise=False)
    x0, cond, z, _ = reference(10, ref.SWEEP_B, ref.SWEEP_T, ref.SWEEP_STEPS, case, ref.SWEEP_BETA, ref.SWEEP_WEIGHT, True)
    noisy = run_drivers(engines, False, 10, case, x0, cond, z, ref.SWEEP_STEPS, ref.SWEEP_BETA, ref.SWEEP_WEIGHT)
    for name in DRIVERS:
        assert not torch.equal(noisy[name][0], det[name][0]), name


@pytest.mark.parametrize("case", PROBES, ids=ref.case_id)
@pytest.mark.parametrize("B,T", [(1, 8), (5, 48), (33, 16), (2, 64)])
def test_shapes_against_fp64(engines, case, B, T):
    check_against_fp64(engines, 10, B, T, ref.SWEEP_STEPS, case)


@pytest.mark.parametrize("case", PROBES, ids=ref.case_id)
@pytest.mark.parametrize("dim", [7, 16])
def test_input_widths_against_fp64(engines, case, dim):
    check_against_fp64(engines, dim, ref.SWEEP_B, ref.SWEEP_T, ref.SWEEP_STEPS, case)


# ------------------------------------------------------------------------------------------------------------ the update alone, to rounding
def check_update_to_rounding(engines, dim, B, T, n_steps, case):
    gt, et, sde, direction = case
    v, s = ref.constants(ref.constant_sd(dim), ref.net_names(sde))
    x0, cond, z = ref.constant_inputs(B, T, dim, n_steps)
    want, M = ref.closed_form64(v, s, x0, z, n_steps, ref.SWEEP_BETA, gt, et, sde, direction, ref.SWEEP_WEIGHT)
    bound = ref.rounding_bound(M)
    fused_expected = 1 if n_steps <= 64 else 0         # the fused path's coefficient and time tables hold 64 steps: beyond, the launch-per-op driver
    got = run_drivers(engines, True, dim, case, x0, cond, z, n_steps, ref.SWEEP_BETA, ref.SWEEP_WEIGHT, fused_expected)
    worst = {}
    for name in DRIVERS:
        xT, traj = got[name]
        assert torch.equal(traj[0], x0) and torch.equal(xT, traj[-1]), name
        err = (traj.double() - want).abs()
        worst[name] = float((err[1:] / bound[1:]).max())
        print(f"SI_ULP {name} {worst[name]:.3f} of the bound, {ref.case_id(case)} dim{dim} B{B} T{T} n{n_steps}")
    for name in DRIVERS:
        assert worst[name] <= 1.0, (name, ref.case_id(case), worst[name])


@pytest.mark.parametrize("case", ref.SWEEP, ids=ref.case_id)
def test_update_alone_to_rounding(engines, case):
    check_update_to_rounding(engines, 10, ref.SWEEP_B, ref.SWEEP_T, ref.SWEEP_STEPS, case)


@pytest.mark.parametrize("case", PROBES, ids=ref.case_id)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [8, 64])
@pytest.mark.parametrize("dim", [7, 10, 16])
@pytest.mark.parametrize("n_steps", [1, 64, 65])
def test_update_alone_step_counts_widths_and_shapes(engines, case, n_steps, dim, T, B):
    check_update_to_rounding(engines, dim, B, T, n_steps, case)
