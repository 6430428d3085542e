"""Anchors tests/train_ref.py (the fp64 statement the GPU training tests compare the HIP path with) to the goldens recorded from the
reference's own autograd runs, on the CPU: g13_train (SI losses, gradients, d loss / d obs_cond, two AdamW + EMA steps), every entry of
g13_train_interpolants, g14_train_lstm.  The bars are the ones tests/test_gpu_train.py applies to the HIP path against the same files:
losses 1e-5 relative, gradient summaries and d loss / d obs_cond 1e-4 of the tensor's norm, updated parameters / EMA shadows 1e-6."""
import numpy as np
import pytest
import torch

from tests import cases, train_ref as R
from tools.make_golden_train import direction, train_inputs


def summarize(name, a):
    v = a.detach().double().cpu().numpy()
    return np.concatenate([[np.sqrt((v * v).sum()), (v * direction(name, v.shape).astype(np.float64)).sum()], v.reshape(-1)[:4]])


def worst_summary(table, names, tensors):
    worst, wk = 0.0, None
    for i, k in enumerate(names):
        e = float(np.abs(summarize(k, tensors[k]) - table[i]).max()) / max(table[i][0], 1e-12)
        if e > worst:
            worst, wk = e, k
    return worst, wk


def _check_si(tag, want_loss, want_dcond, want_grad, names, got):
    loss, info, grads, dcond = got
    l = np.array([loss, info["v_loss"], info["s_loss"], info["b_loss"]])
    el = float(np.abs(l - want_loss).max() / np.abs(want_loss).max())
    assert set(names) == set(grads), set(names) ^ set(grads)
    eg, kg = worst_summary(want_grad, names, grads)
    ed = R.rel_err(dcond, torch.from_numpy(want_dcond))
    print(f"[train_ref {tag}] loss {loss:.8f} (golden {want_loss[0]:.8f}): losses {el:.2e}, worst gradient summary {eg:.2e} ({kg}), dcond {ed:.2e}")
    assert el < 1e-5 and eg < 1e-4 and ed < 1e-4, (tag, el, eg, kg, ed)


def test_si_statement_matches_reference_step_and_two_adamw_ema_steps():
    g = np.load(f"{cases.GOLDEN}/g13_train.npz")
    names = [str(n) for n in g["names"]]
    net, enc = cases.si_net_sd(""), cases.state_encoder_sd(781)
    params = dict(net)
    params.update({"state_encoder." + k: v for k, v in enc.items()})

    def grads_of(step):
        def f(p):
            got = R.si_loss_and_grads({k: v for k, v in p.items() if not k.startswith("state_encoder.")},
                                      {k[len("state_encoder."):]: v for k, v in p.items() if k.startswith("state_encoder.")}, train_inputs(step))
            if step == 1:
                _check_si("g13 step 1", g["s1_loss"], g["s1_dcond"], g["s1_grad"], names, got)
            return got[2]
        return f
    steps = R.adamw_ema_steps(params, [grads_of(1), grads_of(2)], lr=1e-4, wd=1e-6, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.75, ema_keys=list(net))
    for n, st in enumerate(steps, 1):
        ep, kp = worst_summary(g[f"s{n}_param"], names, st["params"])
        ee, ke = worst_summary(g[f"s{n}_ema"], names[:len(g[f"s{n}_ema"])], st["ema"])
        print(f"[train_ref g13 step {n}] worst summary error: params {ep:.2e} ({kp}), ema {ee:.2e} ({ke})")
        assert ep < 1e-6 and ee < 1e-6, (n, ep, kp, ee, ke)


@pytest.mark.parametrize("kind", [k for k in R.INTERPOLANTS if k != "linear"])
def test_si_statement_matches_reference_for_every_interpolant(kind):
    g = np.load(f"{cases.GOLDEN}/g13_train_interpolants.npz")
    names = [str(n) for n in g["names"]]
    inp = train_inputs(1)
    inp["t"] = cases.T(g["t"])
    gamma = str(g[f"{kind}_gamma"])
    got = R.si_loss_and_grads(cases.si_net_sd(""), cases.state_encoder_sd(781), inp, gamma_type=gamma, interpolant_type=kind)
    _check_si(f"{kind} / {gamma}", g[f"{kind}_loss"], g[f"{kind}_dcond"], g[f"{kind}_grad"], names, got)


def test_lstm_statement_matches_reference_step():
    from tools.make_golden_train_lstm import lstm_train_inputs
    g = np.load(f"{cases.GOLDEN}/g14_train_lstm.npz")
    names = [str(n) for n in g["names"]]
    loss, pred, grads, dcond = R.lstm_loss_and_grads(cases.lstm_mods(), lstm_train_inputs(1), masks=None)
    want = float(g["s1_loss"][0])
    assert set(names) == set(grads), set(names) ^ set(grads)
    eg, kg = worst_summary(g["s1_grad"], names, grads)
    ed, ep = R.rel_err(dcond, torch.from_numpy(g["s1_dcond"])), float((pred - torch.from_numpy(g["s1_pred"]).double()).abs().max())
    print(f"[train_ref g14 step 1] loss {loss:.8f} (golden {want:.8f}), pred {ep:.2e} abs, worst gradient summary {eg:.2e} ({kg}), dcond {ed:.2e}")
    assert abs(loss - want) < 1e-5 * abs(want) and ep < 2e-5 and eg < 1e-4 and ed < 1e-4, (loss, want, ep, eg, kg, ed)


def test_si_targets_clip_and_indicator_are_taken_on_the_fp32_value():
    t = torch.tensor([0.0002, 0.9999, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), 0.3], dtype=torch.float32)
    x0, x1, z = torch.ones(5, 2), 2 * torch.ones(5, 2), torch.zeros(5, 2)
    xt, tv, ts, tb, tc = R.si_targets(x0, x1, z, t, R.GAMMAS[0], "reverse_linear")
    assert tc.dtype == torch.float32 and torch.equal(tc, torch.clip(t, 0.001, 0.999))
    assert tv[:, 0].tolist() == [2.0, 0.0, 2.0, 0.0, 2.0]                    # 2 [t <= .5] (x1 - x0): 0.5 is inside, 0.5 + 1 ulp outside
