"""fp64 reference of the stochastic-interpolant sampler (test infrastructure, no test in here).

`sample64` integrates the reference's Euler–Maruyama loop (bridge_model.py:281-387) with both nets and the update in float64.  The scalar
coefficients of a step are evaluated in float32 exactly where the reference rounds them (schedules :59-101 on fp32 scalars, the literal
1.4142, t clipped to [1e-3, 1 - 1e-3], gamma_inv clamped to 200, `dot_gamma * gamma`, `score_weight * eps`, `delta_t * sqrt(2 eps)`, the fp32
`beta_max` and `delta_t` a scalar takes in a product with an fp32 tensor) and then promoted: those rounding points are the specification the
kernels' host-side coefficient table (csrc/vt_unet.hip, si_schedule) is held to.

`closed_form64` is the same loop for nets whose outputs are constants, with no network evaluation, plus the per-step magnitude sum the
rounding bound of the update-only GPU test is built from.

`mistake=` plants one deviation (MISTAKES) a sampler could have; the host tests prove that the GPU sweep's inputs make each of them visible.
"""
from __future__ import annotations

import functools
import itertools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import interpolant as oi, unet1d as ou
from tests import cases
from vlatouch import synth

GAMMAS = ("2^0.5*t(t-1)", "(2t(t-1))^0.5", "(1-t)^2(2t)^0.5")          # position = the engine's gamma_type code
EPSILONS = ("1-t", "t(t-1)", "1-sqrt(t)", "1-t^2", "0")                 # position = the engine's epsilon_type code
MISTAKES = ("net_time",      # nets evaluated at t instead of 1 - t when backward
            "film_row",      # the FiLM / time row of step k + 1
            "eps_in_b",      # the epsilon inside b taken at 1 - t (bridge_model.py:369 takes it at t)
            "gdg_for_bs",    # gamma_dot * gamma kept for the drift-score integrator
            "weight",        # the score weight dropped
            "noise_eps",     # the noise scale from eps(t) instead of eps(1 - t)
            "sign",          # the backward sign
            "noise_slice",   # the noise slice of step k - 1
            "sqrt2")         # sqrt(2) in place of the literal 1.4142 in gamma_inv

# the GPU sweep: every schedule, integrator and direction
SWEEP = list(itertools.product(GAMMAS, EPSILONS, ("vs", "bs"), ("forward", "backward")))
SWEEP_B, SWEEP_T, SWEEP_STEPS, SWEEP_WEIGHT, SWEEP_BETA = 3, 8, 4, 0.7, 0.03
NET_DIMS, NET_K, NET_COND = (64, 128), 3, 64


def case_id(c) -> str:
    return f"g{GAMMAS.index(c[0])}-e{EPSILONS.index(c[1])}-{c[2]}-{c[3]}"


# ------------------------------------------------------------------------------------------------------------ nets and inputs of the sweep
@functools.lru_cache(maxsize=None)
def sweep_sd(input_dim: int = 10) -> Dict[str, torch.Tensor]:
    """fp32 state dict (b_net, v_net, s_net) of the small U-Net: two levels, kernel 3, 64 condition features."""
    shapes = synth.si_net_shapes(input_dim, NET_COND, down_dims=NET_DIMS, k=NET_K)
    return cases.sd_torch(shapes, prefix=f"si-sweep-{input_dim}.")


@functools.lru_cache(maxsize=None)
def constant_sd(input_dim: int = 10) -> Dict[str, torch.Tensor]:
    """sweep_sd with final_conv.1.weight = 0 and distinct fp32 constants as its bias: every driver returns exactly those constants."""
    sd = dict(sweep_sd(input_dim))
    for i, net in enumerate(("b_net", "v_net", "s_net")):
        sd[f"{net}.final_conv.1.weight"] = torch.zeros_like(sd[f"{net}.final_conv.1.weight"])
        d = torch.arange(input_dim, dtype=torch.float32)
        # channel 0 of the drift and velocity nets is tiny and the score's constants are the largest: with constant_inputs' tiny element the
        # score term is then all of that element's first step, which is what lets the rounding bound see gamma_inv's constant
        sd[f"{net}.final_conv.1.bias"] = ((1.5 * 2.0 ** -11, -2.0 ** -11, 2.3)[i] + (0.043 + 0.011 * i) * d * (1.0 - 2.0 * ((d + i) % 2))).float()
    return sd


def constants(sd: Dict[str, torch.Tensor], nets: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
    return tuple(sd[f"{n}.final_conv.1.bias"].double() for n in nets)


def net_names(sde: str) -> Tuple[str, str]:
    return ("b_net" if sde == "bs" else "v_net", "s_net")


def split_nets(sd: Dict[str, torch.Tensor], nets: Sequence[str]) -> List[Dict[str, torch.Tensor]]:
    return [{k[len(n) + 1:]: v for k, v in sd.items() if k.startswith(n + ".")} for n in nets]


def inputs(B: int, T: int, dim: int, n_steps: int, seed: int = 41):
    """x0 in [-1, 1] (normalised actions), cond ~ N(0, 1), z[k] ~ N(0, 1): fp32 values, what the GPU is given."""
    g = synth.inputs_rng(seed)
    x0 = g.uniform(-1, 1, (B, T, dim)).astype(np.float32)
    cond = g.standard_normal((B, NET_COND), dtype=np.float32)
    z = g.standard_normal((n_steps, B, T, dim), dtype=np.float32)
    return cases.T(x0), cases.T(cond), cases.T(z)


def constant_inputs(B: int, T: int, dim: int, n_steps: int):
    """Inputs of the update-only tests: `inputs` with one element, (0, 0, 0), whose state and noise are tiny next to the score term."""
    x0, cond, z = inputs(B, T, dim, n_steps, seed=43)
    x0[0, 0, 0] = 2.0 ** -14
    z[:, 0, 0, 0] *= 2.0 ** -10
    return x0, cond, z


# ------------------------------------------------------------------------------------------------------------ coefficients of one step
# The schedules of bridge_model.py:59-101 in its operation order, on numpy float32 scalars: every operation, the square roots included, is
# correctly rounded (torch's CPU float32 sqrt is one ulp off on some inputs, differently from machine to machine, and eps = 1 - sqrt(t) at
# t = 0.999 turns that ulp into 1e-4 of the coefficient).  Python numbers enter as float32, as they do in a product with an fp32 tensor.
_f = np.float32
_ONE, _TWO, _TINY = _f(1.0), _f(2.0), _f(1e-4)


def _epsilon32(t, kind: str):
    if kind == "t(t-1)":
        return t * (_ONE - t)
    if kind == "1-t":
        return (_ONE - t) * _ONE
    if kind == "1-sqrt(t)":
        return _ONE - np.sqrt(t)
    if kind == "1-t^2":
        return _ONE - t * t
    if kind == "0":
        return t * _f(0.0)
    raise NotImplementedError(kind)


def _gamma32(t, kind: str, r2):
    """(gamma, gamma_dot, gamma_inv clamped to [0, 200]) with the constant as an argument (the `sqrt2` mistake replaces it in gamma_inv)."""
    lit = _f(1.4142)
    if kind == "(2t(t-1))^0.5":
        g, gd = lit * np.sqrt(t * (_ONE - t)), (_ONE - _TWO * t) / np.sqrt(_TWO * (t - t * t) + _TINY)
        gi = _ONE / (r2 * np.sqrt(t * (_ONE - t) + _TINY))
    elif kind == "2^0.5*t(t-1)":
        g, gd = lit * t * (_ONE - t), lit * (_ONE - _TWO * t)
        gi = _ONE / (r2 * t * (_ONE - t) + _TINY)
    elif kind == "(1-t)^2(2t)^0.5":
        sq = (_ONE - t) * (_ONE - t)
        g = lit * sq * np.sqrt(t)
        gd = lit * (_TWO * (t - _ONE) * np.sqrt(t) + sq / (_TWO * np.sqrt(t + _TINY)))
        gi = _ONE / (r2 * sq * np.sqrt(t) + _TINY)
    else:
        raise NotImplementedError(kind)
    return g, gd, min(max(gi, _f(0.0)), _f(oi.GAMMA_INV_MAX))


def step_times(k: int, n_steps: int, direction: str):
    """(t, the time the nets and the gamma schedules see) of step k = 1 .. n_steps as float32 scalars (bridge_model.py:347-361)."""
    t = min(max(_f(k / n_steps), _f(oi.T_MIN)), _f(1.0 - oi.T_MIN))
    return t, (_ONE - t if direction == "backward" else t)


def step_coef(k: int, n_steps: int, beta_max: float, gamma: str, epsilon: str, sde: str, direction: str, score_weight: float,
              mistake: Optional[str] = None) -> Dict[str, float]:
    """The scalars of step k, each rounded to fp32 where the reference rounds it, as Python floats (exact promotions)."""
    assert direction in ("forward", "backward") and sde in ("vs", "bs") and mistake in (None,) + MISTAKES
    dt = _f(float(1.0 / n_steps))                                         # bridge_model.py:270; n_steps = int(1 / delta_t) (:335)
    t, tn = step_times(k, n_steps, direction)
    g, gd, gi = _gamma32(tn, gamma, _f(math.sqrt(2.0)) if mistake == "sqrt2" else _f(1.4142))
    gdg = gd * g if (sde == "vs" or mistake == "gdg_for_bs") else _f(0.0)
    eps_t = _epsilon32(tn if mistake == "eps_in_b" else t, epsilon)       # :369 reads t_tensor in both directions
    eps_n = _epsilon32(tn, epsilon)
    noise_scale = dt * np.sqrt(_TWO * (_epsilon32(t, epsilon) if mistake == "noise_eps" else eps_n))
    score_eps = _f(1.0 if mistake == "weight" else score_weight) * eps_n
    out = dict(dt=dt, gi=gi, gdg=gdg, eps_t=eps_t, noise_scale=noise_scale, score_eps=score_eps, d=_f(beta_max))
    assert all(type(v) is np.float32 for v in out.values()), out
    return {name: float(v) for name, v in out.items()}


def _integrate(net_fn, x0, z, n_steps, beta_max, gamma, epsilon, sde, direction, score_weight, mistake):
    x = x0.double()
    traj, mags = [x], []
    for k in range(1, n_steps + 1):
        c = step_coef(k, n_steps, beta_max, gamma, epsilon, sde, direction, score_weight, mistake)
        t, tn = step_times(min(k + 1, n_steps) if mistake == "film_row" else k, n_steps, direction)
        v, s = net_fn(x, torch.tensor([t if mistake == "net_time" else tn], dtype=torch.float32))
        sv = s * c["gi"]
        b = v - c["gdg"] * sv * c["eps_t"]
        if direction == "backward" and mistake != "sign":
            xn = x - (b - c["score_eps"] * sv) * c["dt"]
        else:
            xn = x + (b + c["score_eps"] * sv) * c["dt"]
        mag = x.abs() + c["dt"] * (v.abs() + (abs(c["gdg"] * c["eps_t"]) + abs(c["score_eps"])) * sv.abs())
        if z is not None:
            zk = z[max(k - 2, 0) if mistake == "noise_slice" else k - 1].double()
            xn = xn + c["noise_scale"] * (c["d"] * zk)
            mag = mag + (c["noise_scale"] * c["d"] * zk).abs()
        x = xn
        traj.append(x)
        mags.append(mag + torch.zeros_like(x))
    return torch.stack(traj), torch.stack(mags)


def sample64(sd, nets, x0, cond, z, n_steps, beta_max, gamma, epsilon, sde, direction, score_weight, mistake=None) -> torch.Tensor:
    """The n_steps + 1 states in float64.  `sd` holds the nets under the prefixes `nets` = (first, score); z = None is the deterministic path."""
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items() if k.startswith(tuple(n + "." for n in nets))}
        n_down = len({k.split(".")[2] for k in sd64 if k.startswith(f"{nets[0]}.down_modules.")})
        cond64 = cond.double()

        def net_fn(x, t32):
            tt = t32.expand(x.shape[0])
            return tuple(ou.unet_forward(sd64, f"{n}.", x, tt, cond64, n_down=n_down) for n in nets)

        return _integrate(net_fn, x0, z, n_steps, beta_max, gamma, epsilon, sde, direction, score_weight, mistake)[0]


def closed_form64(v, s, x0, z, n_steps, beta_max, gamma, epsilon, sde, direction, score_weight, mistake=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(the n_steps + 1 states, M[n_steps]) for nets that return the constants v[d], s[d].  M[k-1] is the element-wise magnitude sum of step k:
    |x_{k-1}| + dt (|v| + (|gdg eps_t| + |score_eps|) |s gamma_inv|) + |noise_scale d z_k|."""
    v64, s64 = v.double(), s.double()
    return _integrate(lambda x, t32: (v64.expand_as(x), s64.expand_as(x)), x0, z, n_steps, beta_max, gamma, epsilon, sde, direction, score_weight, mistake)


def rounding_bound(M: torch.Tensor) -> torch.Tensor:
    """Element-wise bound on |x_fp32 - x_64| after each step for an update computed in fp32 from exact net outputs: the update is about ten
    fp32 operations on intermediates bounded by M (with or without contraction), and 16 * 2^-24 per step also leaves room for one-ulp
    differences in the host-evaluated coefficients.  Row 0 (the initial state) is zero."""
    return torch.cat([torch.zeros_like(M[:1]), 16.0 * 2.0 ** -24 * torch.cumsum(M, dim=0)])
