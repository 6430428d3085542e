"""Reference side of the controller-training tests: the interpolant controller's training loss (three conditional 1-D U-Nets + the
observation MLP, VLA/residual_controller/bridge/bridge_model.py:73-91, 103-258, bridge/networks/conditional_unet_1D.py:7-247,
bridge_controller.py:42-48), the LSTM residual head's (lstm_step_controller.py:176-211, 321-337) and the optimizer loop around them
(torch.optim.AdamW + torch_ema, bridge_train.py:49-58, 312-334), restated with plain functional torch on the CPU in any dtype.  fp64 is the
yardstick, an fp32 run of the same code gives the error the reference's own arithmetic has.  tests/test_train_host.py pins the fp64
statement to the goldens recorded from the reference itself (g13_train, g13_train_interpolants, g14_train_lstm)."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Callable, Dict, Optional, Sequence, Union

import torch
import torch.nn.functional as F

GAMMAS = ("2^0.5*t(t-1)", "(2t(t-1))^0.5", "(1-t)^2(2t)^0.5")
INTERPOLANTS = ("linear", "power3", "power4", "reverse_power3", "reverse_power4", "gaussian_encode_decode", "reverse_linear")
SD = Dict[str, torch.Tensor]


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """|a - ref| / |ref| over the whole tensor (fp64); a zero reference demands an exactly zero `a`."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    n = float(ref.norm())
    if n == 0.0:
        return 0.0 if float(a.abs().max()) == 0.0 else float("inf")
    return float((a - ref).norm()) / n


def max_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| / max |ref| (fp64); a zero reference demands an exactly zero `a`."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    m = float(ref.abs().max())
    if m == 0.0:
        return 0.0 if float(a.abs().max()) == 0.0 else float("inf")
    return float((a - ref).abs().max()) / m


def leaf_sd(sd: SD, dtype) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())


def _grads(leaves) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, (torch.zeros_like(v) if v.grad is None else v.grad).double()) for k, v in leaves.items())


# ---------------------------------------------------------------------------------------------- the interpolant and its loss targets
def clip_t(t: torch.Tensor, t_min: float = 0.001) -> torch.Tensor:
    """torch.clip(t, t_min, 1 - t_min) on the fp32 draw, as the reference does it (bridge_model.py:184, 252)."""
    return torch.clip(t.float(), t_min, 1.0 - t_min)


def si_targets(x0, x1, z, t, gamma_type: str, interpolant_type: str, t_min: float = 0.001, dtype=torch.float64):
    """q_sample + the three loss targets (bridge_model.py:73-91 gamma / gamma_der, :103-147 interpolant, :149-181 interpolant_dev):
    x0 / x1 / z [B, ...] (z already scaled by beta_max), t [B] -> xt, target_v, target_s, target_b (in `dtype`), t_clipped (fp32).
    The clip and the piecewise interpolants' indicator `t <= 0.5` are taken on the fp32 value, everything after that in `dtype`."""
    tc32 = clip_t(t, t_min)
    lo = (tc32 <= 0.5).to(dtype)
    shape = (-1,) + (1,) * (x0.dim() - 1)
    tt, lo = tc32.to(dtype).reshape(shape), lo.reshape(shape)
    a, c, zz = x0.to(dtype), x1.to(dtype), z.to(dtype)
    if gamma_type == "(2t(t-1))^0.5":
        g, gd = 1.4142 * torch.sqrt(tt * (1 - tt)), (1 - 2 * tt) / torch.sqrt(2 * (tt - tt ** 2) + 1e-4)
    elif gamma_type == "2^0.5*t(t-1)":
        g, gd = 1.4142 * tt * (1 - tt), 1.4142 * (1 - 2 * tt)
    elif gamma_type == "(1-t)^2(2t)^0.5":
        g = 1.4142 * (1 - tt) ** 2 * torch.sqrt(tt)
        gd = 1.4142 * (2 * (tt - 1) * torch.sqrt(tt) + (1 - tt) ** 2 / (2.0 * torch.sqrt(tt + 1e-4)))
    else:
        raise NotImplementedError(gamma_type)
    if interpolant_type == "linear":
        w0, w1, dv = 1 - tt, tt, c - a
    elif interpolant_type == "power3":
        w0 = (1 - tt) ** 3
        w1, dv = 1 - w0, 3 * (1 - tt) ** 2 * (c - a)
    elif interpolant_type == "power4":
        w0 = (1 - tt) ** 4
        w1, dv = 1 - w0, 4 * (1 - tt) ** 3 * (c - a)
    elif interpolant_type == "reverse_power3":
        w1 = tt ** 3
        w0, dv = 1 - w1, 3 * tt ** 2 * (c - a)
    elif interpolant_type == "reverse_power4":
        w1 = tt ** 4
        w0, dv = 1 - w1, 4 * tt ** 3 * (c - a)
    elif interpolant_type == "gaussian_encode_decode":
        c2 = torch.cos(tt * math.pi) ** 2
        w0, w1 = c2 * lo, c2 * (1 - lo)
        k = -2 * math.pi * torch.cos(math.pi * tt) * torch.sin(math.pi * tt)
        dv = k * lo * a + k * (1 - lo) * c
    elif interpolant_type == "reverse_linear":
        w0 = (1 - 2 * tt) * lo
        w1, dv = 1 - w0, -2 * lo * a + 2 * lo * c
    else:
        raise NotImplementedError(interpolant_type)
    return w0 * a + w1 * c + g * zz, dv, -zz, dv + gd * zz, tc32


# ---------------------------------------------------------------------------------------------- the conditional 1-D U-Net, any dtype
def mish(x: torch.Tensor) -> torch.Tensor:
    return x * torch.tanh(F.softplus(x))


def posemb(t32: torch.Tensor, dim: int, dtype) -> torch.Tensor:
    """SinusoidalPosEmb (conditional_unet_1D.py:12-19): the frequencies and the product t f are fp32 (t is the fp32 clipped draw and the
    table is built in fp32 there); sin / cos in `dtype`."""
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1)))
    e = (t32.float()[:, None] * f[None, :]).to(dtype)
    return torch.cat((e.sin(), e.cos()), dim=-1)


def _conv_block(sd: SD, p: str, x: torch.Tensor, n_groups: int) -> torch.Tensor:
    w = sd[f"{p}.block.0.weight"]
    y = F.conv1d(x, w, sd[f"{p}.block.0.bias"], padding=w.shape[-1] // 2)
    return mish(F.group_norm(y, n_groups, sd[f"{p}.block.1.weight"], sd[f"{p}.block.1.bias"], eps=1e-5))


def _res_block(sd: SD, p: str, x: torch.Tensor, g: torch.Tensor, n_groups: int) -> torch.Tensor:
    out = _conv_block(sd, f"{p}.blocks.0", x, n_groups)
    cout = out.shape[1]
    emb = F.linear(mish(g), sd[f"{p}.cond_encoder.1.weight"], sd[f"{p}.cond_encoder.1.bias"])
    out = emb[:, :cout, None] * out + emb[:, cout:, None]
    out = _conv_block(sd, f"{p}.blocks.1", out, n_groups)
    res = F.conv1d(x, sd[f"{p}.residual_conv.weight"], sd[f"{p}.residual_conv.bias"]) if f"{p}.residual_conv.weight" in sd else x
    return out + res


def unet_forward(sd: SD, prefix: str, sample: torch.Tensor, t32: torch.Tensor, cond: torch.Tensor, n_down: int = 3, n_groups: int = 8) -> torch.Tensor:
    """DiffusionConditionalUnet1D.forward (conditional_unet_1D.py:194-247) in the dtype of `sd` / `sample`: [B,T,C], t [B] fp32, cond [B,G]."""
    dtype = sample.dtype
    x = sample.movedim(-1, -2)
    e = posemb(t32, sd[f"{prefix}diffusion_step_encoder.1.weight"].shape[1], dtype)
    e = mish(F.linear(e, sd[f"{prefix}diffusion_step_encoder.1.weight"], sd[f"{prefix}diffusion_step_encoder.1.bias"]))
    e = F.linear(e, sd[f"{prefix}diffusion_step_encoder.3.weight"], sd[f"{prefix}diffusion_step_encoder.3.bias"])
    g = torch.cat([e, cond], dim=-1)
    h = []
    for i in range(n_down):
        x = _res_block(sd, f"{prefix}down_modules.{i}.0", x, g, n_groups)
        x = _res_block(sd, f"{prefix}down_modules.{i}.1", x, g, n_groups)
        h.append(x)
        if f"{prefix}down_modules.{i}.2.conv.weight" in sd:
            x = F.conv1d(x, sd[f"{prefix}down_modules.{i}.2.conv.weight"], sd[f"{prefix}down_modules.{i}.2.conv.bias"], stride=2, padding=1)
    for i in range(2):
        x = _res_block(sd, f"{prefix}mid_modules.{i}", x, g, n_groups)
    for i in range(n_down - 1):
        x = torch.cat((x, h.pop()), dim=1)
        x = _res_block(sd, f"{prefix}up_modules.{i}.0", x, g, n_groups)
        x = _res_block(sd, f"{prefix}up_modules.{i}.1", x, g, n_groups)
        if f"{prefix}up_modules.{i}.2.conv.weight" in sd:
            x = F.conv_transpose1d(x, sd[f"{prefix}up_modules.{i}.2.conv.weight"], sd[f"{prefix}up_modules.{i}.2.conv.bias"], stride=2, padding=1)
    x = _conv_block(sd, f"{prefix}final_conv.0", x, n_groups)
    x = F.conv1d(x, sd[f"{prefix}final_conv.1.weight"], sd[f"{prefix}final_conv.1.bias"])
    return x.movedim(-1, -2)


def mlp_gelu(sd: SD, x: torch.Tensor, prefix: str = "") -> torch.Tensor:
    """Linear (-GELU(erf)-Linear)*: nn.Sequential keys '0', '2'[, '4'] (bridge_controller.py:42-48, lstm_step_controller.py:44-60)."""
    idx = sorted(int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix) and k.endswith(".weight"))
    for n, i in enumerate(idx):
        x = F.linear(x, sd[f"{prefix}{i}.weight"], sd[f"{prefix}{i}.bias"])
        if n + 1 < len(idx):
            x = F.gelu(x)
    return x


def si_loss_and_grads(net_sd: SD, enc_sd: Optional[SD], inp: Dict[str, torch.Tensor], *, gamma_type: str = GAMMAS[0], interpolant_type: str = "linear",
                      beta_max: float = 0.03, t_min: float = 0.001, dtype=torch.float64):
    """`StochasticInterpolants.get_loss` (bridge_model.py:183-246) + backward.  inp: obs_in (the observation MLP's input, or obs_cond itself when
    `enc_sd` is None), vla_n, expert_n [B,T,10], t [B], z [B,T,10] ~ N(0,1).
    -> (loss, {'v_loss','s_loss','b_loss'}, {reference parameter name (net keys, 'state_encoder.*'): gradient in fp64}, d loss / d obs_cond)."""
    net = leaf_sd(net_sd, dtype)
    enc = leaf_sd(enc_sd, dtype) if enc_sd is not None else None
    z = inp["z"].float() * beta_max                                    # `self.d * torch.randn_like(x0).float()`: an fp32 product in the reference
    with torch.enable_grad():                                          # other test modules switch autograd off process-wide
        obs = inp["obs_in"].to(dtype)
        cond = mlp_gelu(enc, obs) if enc is not None else obs.clone().requires_grad_(True)
        cond.retain_grad()
        xt, tv, ts, tb, tc = si_targets(inp["vla_n"], inp["expert_n"], z, inp["t"], gamma_type, interpolant_type, t_min, dtype)
        info = {}
        for name, tgt in (("v", tv), ("s", ts), ("b", tb)):
            o = unet_forward(net, f"{name}_net.", xt, tc, cond).flatten(1)
            info[f"{name}_loss"] = torch.mean(0.5 * torch.norm(o, dim=-1) ** 2 - torch.sum(tgt.flatten(1) * o, dim=-1))
        loss = info["v_loss"] + info["s_loss"] + info["b_loss"]
        loss.backward()
    grads = _grads(net)
    if enc is not None:
        grads.update(("state_encoder." + k, v) for k, v in _grads(enc).items())
    return float(loss.detach()), {k: float(v.detach()) for k, v in info.items()}, grads, cond.grad.double()


# ---------------------------------------------------------------------------------------------- the LSTM residual head
def lstm_loss_and_grads(mods: Dict[str, SD], inp: Dict[str, torch.Tensor], *, masks: Optional[Dict[str, torch.Tensor]] = None, dtype=torch.float64):
    """`TactileLSTMController.forward` + `get_loss` (lstm_step_controller.py:176-211, 321-337) + backward for any hidden width / layer count
    (both read off the checkpoint).  inp: obs_in (obs_encoder's input, or obs_cond when mods has no 'obs_encoder'), vla_n / expert_n [B,T,D],
    forces [B,T,F].  masks: None = eval-mode arithmetic, else keep-masks of 0 / 1/(1-p) entries [B,T,H]: 'lstm' between the layers of a
    two-layer LSTM ('lstm{l}' behind layer l otherwise), 'head' behind the head's GELU.
    -> (loss, pred [B,T,D] fp64, {'<module>.<key>': gradient fp64}, d loss / d obs_cond)."""
    leaves = {m: leaf_sd(sd, dtype) for m, sd in mods.items() if sd is not None}
    ls, hd = leaves["lstm"], leaves["output_head"]
    nl = len([k for k in ls if k.startswith("weight_ih_l")])
    H = ls["weight_hh_l0"].shape[1]
    vla, expert, forces = inp["vla_n"].to(dtype), inp["expert_n"].to(dtype), inp["forces"].to(dtype)
    B, T, _ = vla.shape
    with torch.enable_grad():
        obs = inp["obs_in"].to(dtype)
        cond = mlp_gelu(leaves["obs_encoder"], obs) if "obs_encoder" in leaves else obs.clone().requires_grad_(True)
        cond.retain_grad()
        x = torch.cat([mlp_gelu(leaves["force_encoder"], forces), vla], dim=-1)
        for l in range(nl):
            gx = F.linear(x, ls[f"weight_ih_l{l}"], ls[f"bias_ih_l{l}"] + ls[f"bias_hh_l{l}"])
            h, c, hs = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype), []
            for t in range(T):
                i, f, g, o = (gx[:, t] + F.linear(h, ls[f"weight_hh_l{l}"])).chunk(4, dim=-1)      # torch.nn.LSTM gate order
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                hs.append(h)
            x = torch.stack(hs, dim=1)
            if l + 1 < nl and masks is not None:
                m = masks.get("lstm" if nl == 2 else f"lstm{l}")
                if m is not None:
                    x = x * m.to(dtype).reshape(B, T, H)
        a = F.linear(torch.cat([x, cond[:, None].expand(B, T, H)], dim=-1), hd["0.weight"], hd["0.bias"])
        a = F.gelu(F.layer_norm(a, (H,), hd["1.weight"], hd["1.bias"], 1e-5))
        if masks is not None and masks.get("head") is not None:
            a = a * masks["head"].to(dtype).reshape(B, T, H)
        pred = vla + F.linear(a, hd["4.weight"], hd["4.bias"])
        loss = F.mse_loss(pred, expert)
        loss.backward()
    grads = OrderedDict((f"{m}.{k}", v) for m in ("obs_encoder", "force_encoder", "lstm", "output_head") if m in leaves for k, v in _grads(leaves[m]).items())
    return float(loss.detach()), pred.detach().double(), grads, cond.grad.double()


# ---------------------------------------------------------------------------------------------- AdamW + EMA
def adamw_ema_steps(params: SD, grads_per_step: Sequence[Union[SD, Callable[[SD], SD]]], *, lr: Union[float, Sequence[float]] = 1e-4, wd: float = 1e-6,
                    betas=(0.9, 0.999), eps: float = 1e-8, ema_decay: float = 0.75, dtype=torch.float64, ema_keys=None):
    """torch.optim.AdamW over `params` + the torch_ema update (shadow -= (1 - d)(shadow - p), d = min(decay, (1 + n) / (10 + n)) with n counted from 1)
    of the tensors named in `ema_keys` (default: all), in `dtype`.  An entry of `grads_per_step` is a dict of gradients or a function of the current
    parameters returning one (a step whose gradients depend on the previous update); `lr` may be one value per step.
    -> list per step of dict(params {k: fp64}, ema {k: fp64})."""
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in params.items())
    ema = OrderedDict((k, leaves[k].detach().clone()) for k in (leaves if ema_keys is None else ema_keys))
    lr0 = lr if isinstance(lr, (int, float)) else lr[0]
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr0, betas=betas, eps=eps, weight_decay=wd)
    out = []
    for n, g in enumerate(grads_per_step):
        if callable(g):
            g = g(OrderedDict((k, v.detach()) for k, v in leaves.items()))
        if not isinstance(lr, (int, float)):
            for grp in opt.param_groups:
                grp["lr"] = lr[n]
        for k, v in leaves.items():
            v.grad = g[k].detach().to(dtype).clone()
        opt.step()
        d = min(ema_decay, (1 + (n + 1)) / (10 + (n + 1)))
        with torch.no_grad():
            for k, s in ema.items():
                s.sub_((1.0 - d) * (s - leaves[k].detach()))
        out.append(dict(params=OrderedDict((k, v.detach().double().clone()) for k, v in leaves.items()),
                        ema=OrderedDict((k, v.double().clone()) for k, v in ema.items())))
    return out
