"""Host-side checks of the RDT fine-tuning step (no GPU): the schedules the trainer computes on the host (DDPM alpha-bar table, EMA warm-up
decay, learning-rate schedulers) and argument validation of the RDTRunner surface."""
import pytest
import torch

from tests import cases
from tests import rdt_train_ref as R


def test_alpha_bar_table_is_the_schedulers():
    from vlatouch.rdt_train import alphas_cumprod
    from oracle import dpm_solver
    for sched in ("squaredcos_cap_v2", "linear", "scaled_linear"):
        want = torch.cumprod(1.0 - torch.from_numpy(dpm_solver.make_betas(1000, sched)), dim=0)
        got = alphas_cumprod(1000, sched)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    with pytest.raises(NotImplementedError):
        alphas_cumprod(1000, "sigmoid")


def test_ema_model_decay_schedule():
    """EMAModel.get_decay (models/ema_model.py:45-55): 0 for the first two steps, then 1 - (1 + step / inv_gamma)^-power, clamped."""
    from models.ema_model import EMAModel
    e = EMAModel(None)
    assert e.get_decay(0) == 0.0 and e.get_decay(1) == 0.0
    assert e.get_decay(2) == pytest.approx(1 - 2 ** (-2 / 3), abs=1e-15)
    assert e.get_decay(10 ** 9) == 0.9999
    e2 = EMAModel(None, update_after_step=5, inv_gamma=2.0, power=0.75, min_value=0.3, max_value=0.99)
    assert e2.get_decay(6) == 0.0
    assert e2.get_decay(7) == max(0.3, 1 - (1 + 1 / 2.0) ** -0.75)
    assert e2.get_decay(10 ** 7) == 0.99
    for s in range(0, 40, 3):
        assert e.get_decay(s) == R.ema_decay(s) and e2.get_decay(s) == R.ema_decay(s, 5, 2.0, 0.75, 0.3, 0.99)
    for _ in range(3):
        e.step()
    assert e.optimization_step == 3 and e.decay == e.get_decay(2)


def test_lr_schedulers():
    from vlatouch.rdt_train import lr_at
    assert lr_at(5e-6, "constant", 0, 500) == 5e-6 and lr_at(5e-6, "constant", 10 ** 6, 500) == 5e-6
    assert lr_at(1e-3, "constant_with_warmup", 0, 500) == 0.0
    assert lr_at(1e-3, "constant_with_warmup", 250, 500) == pytest.approx(5e-4)
    assert lr_at(1e-3, "constant_with_warmup", 500, 500) == 1e-3 and lr_at(1e-3, "constant_with_warmup", 9000, 500) == 1e-3
    assert lr_at(1e-3, "constant_with_warmup", 3, 0) == 1e-3
    for other in ("cosine", "linear", "polynomial", ""):
        with pytest.raises(ValueError):
            lr_at(1e-3, other, 0, 500)


def _runner(prediction_type="sample"):
    from models.rdt_runner import RDTRunner
    cfg = cases.RDT_TINY
    config = {"rdt": {"hidden_size": cfg["hidden"], "depth": cfg["depth"], "num_heads": cfg["heads"]}, "lang_adaptor": "mlp2x_gelu",
              "img_adaptor": "mlp2x_gelu", "state_adaptor": "mlp3x_gelu",
              "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "prediction_type": prediction_type,
                                  "beta_schedule": "squaredcos_cap_v2"}}
    return RDTRunner(action_dim=cfg["action_dim"], pred_horizon=cfg["horizon"], config=config, lang_token_dim=cfg["lang_token_dim"],
                     img_token_dim=cfg["img_token_dim"], state_token_dim=cfg["state_token_dim"], max_lang_cond_len=cfg["max_lang_cond_len"],
                     img_cond_len=cfg["img_cond_len"], dtype=torch.float32, device="cuda", rms_mode="meansq")


def test_compute_loss_validates_its_arguments_before_touching_the_device():
    b = R.batch(cases.RDT_TINY, 3, 12)
    args = [b[k] for k in ("lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs")]
    r = _runner()
    bad = list(args)
    bad[4] = b["action_gt"][0]                         # action_gt without its batch dimension
    with pytest.raises(ValueError):
        r.compute_loss(*bad, noise=b["noise"], timesteps=b["timesteps"])
    bad = list(args)
    bad[1] = b["lang_attn_mask"][0]
    with pytest.raises(ValueError):
        r.compute_loss(*bad, noise=b["noise"], timesteps=b["timesteps"])
    with pytest.raises(ValueError):
        _runner("v_prediction").compute_loss(*args, noise=b["noise"], timesteps=b["timesteps"])
    with pytest.raises(TypeError):
        r.compute_loss(*args, b["noise"])               # the two draws are keyword-only, as x_init is not part of the reference's positional surface


def test_trainer_rejects_what_it_does_not_build():
    """Constructor validation happens before the device is required."""
    from vlatouch.rdt_train import RdtTrainer
    kw = dict(heads=4, horizon=8, action_dim=128)
    with pytest.raises(ValueError):
        RdtTrainer({}, precision="fp16", **kw)
    with pytest.raises(ValueError):
        RdtTrainer({}, prediction_type="v_prediction", **kw)
    with pytest.raises(ValueError):
        RdtTrainer({}, lr_scheduler="cosine", **kw)
    with pytest.raises(ValueError):
        RdtTrainer({}, rms_mode="l2", **kw)


# ------------------------------------------------------------------------------------------------ reference -> golden -> oracle autograd
def _g16():
    import numpy as np
    return np.load(f"{cases.GOLDEN}/g16_rdt_train.npz")


_summary, _worst = R.summary, R.worst_summary


@pytest.mark.parametrize("prediction_type", ["sample", "epsilon"])
@pytest.mark.parametrize("rms_mode", ["meansq", "var"])
def test_oracle_autograd_matches_the_references_own_run(rms_mode, prediction_type):
    """g16 = the reference's own compute_loss / backward / clip / AdamW / EMAModel in fp32 (tools/make_golden_rdt_train.py; its add_noise is an
    UNPINNED closed-form stand-in).  The fp64 helper the GPU tests measure against reproduces it: loss 1e-5 relative, every tensor's gradient
    within 1e-4 of its norm, the norm before clipping 1e-5, and the updates p_k - p_0 / ema_k - p_0 within 5 x what fp32 torch loses against
    fp64 torch on the same three steps (computed here; Adam's division by sqrt(v) amplifies rounding where a gradient is near zero)."""
    import numpy as np
    SEEDS, B, LANG_LEN, HP, MAX_GRAD_NORM = R.G16_SEEDS, R.G16_B, R.G16_LANG_LEN, R.G16_HP, R.G16_MAX_GRAD_NORM
    g = _g16()
    assert "UNPINNED" in str(g["add_noise"])
    names = [str(n) for n in g["names"]]
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    assert sorted(names) == sorted(sd) and len(names) == 114
    batches = [R.batch(cfg, B, LANG_LEN, seed=s) for s in SEEDS]
    kw = dict(lr=HP["lr"], weight_decay=HP["weight_decay"], betas=HP["betas"], eps=HP["eps"], max_grad_norm=MAX_GRAD_NORM, rms_mode=rms_mode,
              prediction_type=prediction_type)
    r64 = R.train_steps(sd, batches, cfg, dtype=torch.float64, **kw)
    r32 = R.train_steps(sd, batches, cfg, dtype=torch.float32, **kw)
    p0 = {k: v.double() for k, v in sd.items()}
    tag = f"{rms_mode}_{prediction_type}"
    # gradients of the first step: the parameters are still the golden's
    _, g64 = R.loss_and_grads(sd, batches[0], cfg, rms_mode=rms_mode, prediction_type=prediction_type)
    wg, kg = _worst(g[f"{tag}_s1_grad"], names, g64)
    assert wg <= 1e-4, (kg, wg)
    for n in range(3):
        loss, norm, decay = g[f"{tag}_s{n + 1}_scalars"]
        assert abs(r64[n]["loss"] - loss) <= 1e-5 * loss and abs(r64[n]["grad_norm"] - norm) <= 1e-5 * norm
        assert decay == R.ema_decay(n)
        # the same three steps in fp32 torch against fp64 torch, measured the way the golden can be: on the summaries
        t64 = np.stack([_summary(k, r64[n]["params"][k] - p0[k]) for k in names])
        base, _ = _worst(t64, names, {k: r32[n]["params"][k] - p0[k] for k in sd})
        wu, ku = _worst(g[f"{tag}_s{n + 1}_update"], names, {k: r64[n]["params"][k] - p0[k] for k in sd})
        we, ke = _worst(g[f"{tag}_s{n + 1}_ema"], names, {k: r64[n]["ema"][k] - p0[k] for k in sd})
        print(f"[g16 {tag} step {n + 1}] loss {loss:.6f}, norm {norm:.4f}; update {wu:.2e} ({ku}), ema {we:.2e}; fp32-vs-fp64 torch {base:.2e}; grad s1 {wg:.2e}")
        assert wu <= 5 * base and we <= 5 * base, (wu, we, base)
