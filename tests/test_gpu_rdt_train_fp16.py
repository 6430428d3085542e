"""precision="fp16" of the RDT trainer (vlatouch/rdt_train.py) on the device: gradients against fp64 autograd next to the oracle in fp16 and
next to the bf16 trainer, the loss scale as a lever against underflow, overflow -> skip -> back-off -> recovery, accumulation windows,
the 8-bit optimizer, checkpoints, thirty steps, and the sampler.  tests/loss_scale_ref.py states the scaler; tests/rdt_train16_ref.py holds
the references (computed once and shared)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import loss_scale_ref as S
from tests import rdt_train16_ref as R16
from tests import rdt_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs")


def _trainer(cfg, sd, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], device=DEV, **kw)


def _get_loss(tr, b, **kw):
    return tr.get_loss(*[b[k] for k in KEYS], noise=b["noise"], timesteps=b["timesteps"], **kw)


def _step(tr, b):
    return tr.train_step(*[b[k] for k in KEYS], noise=b["noise"], timesteps=b["timesteps"])


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _snap(d):
    return {k: v.detach().clone() for k, v in d.items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _bad(b):
    """The batch with an inf planted in action_gt: the loss and every gradient of that micro-batch are non-finite."""
    out = dict(b)
    out["action_gt"] = b["action_gt"].clone()
    out["action_gt"][0, 0, 0] = float("inf")
    return out


_HIP = {}


def _hip_grads(name, precision, kernel, scale=None):
    """The trainer's gradients, DIVIDED by the static loss scale, for one model size / precision / attention backward; shared."""
    key = (name, precision, kernel, scale)
    if key not in _HIP:
        cfg, sd, b = (R16.problem(name) if precision == "fp16" else R16.problem_bf16(name))[:3]
        kw = dict(loss_scale=scale) if precision == "fp16" else {}
        tr = _trainer(cfg, sd, precision=precision, attention_backward=kernel, **kw)
        loss = float(_get_loss(tr, b))
        grads = tr.grads()
        assert set(grads) == set(sd) and all(v.dtype == torch.float32 for v in grads.values())
        _HIP[key] = (loss, {k: v.double() / (scale or 1.0) for k, v in grads.items()})
    return _HIP[key]


@pytest.mark.parametrize("kernel", ["wave", "mfma"])
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_gradients_fp16(name, kernel):
    """Static loss_scale=1024, against fp64 autograd from the same fp16-rounded weights and batch.  Per tensor e_hip <= max(1.5 e_ref,
    1.25e-3 |g|) with e_ref the oracle in fp16 on the CPU under the same scale (recorded: tests/golden/g21_fp16_oracle_errors.json; 1.25e-3: the bf16 test's 1e-2 floor over the 8 x finer mantissa);
    over all parameters e_hip <= 1.5 e_ref; and the fp16 trainer is closer to its fp64 than the bf16 trainer (same batch rounded to bf16) is to
    its own."""
    cfg, sd, b, l64, g64 = R16.problem(name)
    ref = R16.oracle_errors(name)                                      # the fp16 oracle on the CPU under the same scale, recorded
    lref = ref["loss"]
    loss, grads = _hip_grads(name, "fp16", kernel, 1024.0)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    rel_h, rel_r, bad = [], [], []
    n_h = n_r = 0
    for k in sd:
        gn = float(g64[k].norm())
        eh, er = float((grads[k] - g64[k]).norm()), ref["tensor_error"][k]
        rel_h.append(eh / gn), rel_r.append(er / gn)
        n_h, n_r = n_h + (eh > 1.25e-3 * gn), n_r + (er > 1.25e-3 * gn)
        if not eh <= max(1.5 * er, 1.25e-3 * gn):
            bad.append((k, eh / gn, er / gn))
    (tot_h, gall), tot_r = R16.total_error(grads, g64), ref["total_error"]
    # the recording belongs to this problem: same tensors, and the fp64 gradient norm it was taken against (the oracle's fp32 tables and libm
    # calls move that norm by some 1e-8 between CPUs; another batch or seed moves it in the first digit)
    assert set(ref["tensor_error"]) == set(sd) and abs(gall - ref["grad_norm"]) <= 1e-6 * gall
    _, _, _, _, g64b = R16.problem_bf16(name)
    _, gb = _hip_grads(name, "bf16", kernel)
    tot_b, gallb = R16.total_error(gb, g64b)
    print(f"[rdt_train fp16 {name} {kernel}] loss {loss:.5f} (oracle fp16 {lref:.5f}, fp64 {l64:.5f}); per-tensor error / norm: HIP median {np.median(rel_h):.2e} "
          f"worst {max(rel_h):.2e}, oracle fp16 median {np.median(rel_r):.2e} worst {max(rel_r):.2e}; all parameters: HIP {tot_h / gall:.2e}, oracle "
          f"{tot_r / gall:.2e}, bf16 trainer {tot_b / gallb:.2e}; above 1.25e-3: HIP {n_h}, oracle {n_r} of {len(sd)}")
    assert abs(loss - l64) <= 2e-3 * abs(l64), (loss, l64)             # the loss is reported unscaled
    assert not bad, bad[:8]
    assert tot_h <= 1.5 * tot_r, (tot_h, tot_r)
    assert tot_h / gall < tot_b / gallb, (tot_h / gall, tot_b / gallb)


def test_the_scale_is_a_lever_against_underflow():
    """RDT_WIDE: the all-parameter error at loss_scale=1024 is below that at loss_scale=1 (the CPU oracle: 4.4e-4 against 1.57e-3)."""
    _, _, _, _, g64 = R16.problem("wide")
    e1024, gall = R16.total_error(_hip_grads("wide", "fp16", "wave", 1024.0)[1], g64)
    e1, _ = R16.total_error(_hip_grads("wide", "fp16", "wave", 1.0)[1], g64)
    print(f"[rdt_train fp16 wide] all-parameter error / norm: loss_scale 1024 {e1024 / gall:.2e}, loss_scale 1 {e1 / gall:.2e}")
    assert e1024 < e1, (e1024, e1)


def _moments(tr):
    return {k: torch.cat([t.reshape(-1) for t in tr.moments(k)]) for k in tr.p}


def test_overflow_backoff_recovery():
    """Dynamic scaling from 2^24 with growth_interval 2, one repeated batch.  The CPU oracle's gradients are non-finite at 2^24 and finite at
    2^16, so the trainer must skip at least once and must take a real step within 13 calls (2^24 -> 2^12: a cap, the count is printed).  Every
    skipped call leaves parameters, moments, step_count and lr alone, advances ema_updates, global_step and skipped_steps, halves the scale,
    clears the tracker and moves the shadows exactly as ema_step() moves a twin's.  Two clean steps in a row double the scale."""
    cfg, sd, b, _, _ = R16.problem("tiny")
    _, g24 = R16.oracle("tiny", 2.0 ** 24)
    _, g16 = R16.oracle("tiny", 2.0 ** 16)
    assert not all(bool(torch.isfinite(v).all()) for v in g24.values()) and all(bool(torch.isfinite(v).all()) for v in g16.values())
    settings = dict(init_scale=2.0 ** 24, growth_interval=2)
    tr, twin = _trainer(cfg, sd, precision="fp16", loss_scale=settings, lr=1e-3), _trainer(cfg, sd, precision="fp16", loss_scale=settings, lr=1e-3)
    st = S.Scaler(**settings)
    assert tr.loss_scale_value == 2.0 ** 24 and tr.growth_tracker == 0 and tr.skipped_steps == 0 and tr.last_step_skipped is False
    _get_loss(twin, b)                                                 # the twin only needs gradients for its table; it never steps
    calls = skips = clean_in_a_row = 0
    while clean_in_a_row < 2:
        assert calls < 15
        before = dict(p=_snap(tr.p), mom=_moments(tr), step=tr.step_count, lr=tr.lr, ema=tr.ema_updates, gs=tr.global_step, sk=tr.skipped_steps,
                      scale=tr.loss_scale_value, tracker=tr.growth_tracker)
        loss = float(_step(tr, b))
        calls += 1
        assert np.isfinite(loss) and tr.sync_gradients and tr.micro_step == 0
        st.update(tr.last_step_skipped)
        assert (tr.loss_scale_value, tr.growth_tracker, tr.skipped_steps) == (st.value, st.tracker, st.skipped)
        assert tr.ema_updates == before["ema"] + 1 and tr.global_step == before["gs"] + 1
        if tr.last_step_skipped:
            skips += 1
            clean_in_a_row = 0
            assert _same(tr.p, before["p"]) and _same(_moments(tr), before["mom"])
            assert tr.step_count == before["step"] and tr.lr == before["lr"]
            assert tr.skipped_steps == before["sk"] + 1 and tr.loss_scale_value == before["scale"] / 2 and tr.growth_tracker == 0
            assert tr.skipped_nonfinite_loss == 0                      # the forward is finite: only the scaled backward overflows
            if tr.step_count == 0:                                     # while the parameters are still the twin's
                twin.ema_step()
                assert _same(tr.shadow, twin.shadow)
        else:
            clean_in_a_row += 1
            if tr.step_count == 1:
                first = (calls, before["scale"])
                assert calls <= 13, "no real step within 13 calls"
            assert tr.step_count == before["step"] + 1 and not _same(tr.p, before["p"])
            assert bool(torch.isfinite(tr.grad_norm)) and all(bool(torch.isfinite(v).all()) for v in tr.p.values())
            if clean_in_a_row == 2:
                assert tr.loss_scale_value == 2 * before["scale"] and tr.growth_tracker == 0
    print(f"[rdt_train fp16 overflow] {skips} skipped calls from 2^24, first real step at call {first[0]} with scale 2^{int(np.log2(first[1]))}")
    assert skips >= 1


@pytest.mark.parametrize("loss_scale", [1024.0, dict(init_scale=1024.0, growth_interval=1000)], ids=["static", "dynamic"])
def test_accumulation_window_with_a_bad_micro_batch(loss_scale):
    """k = 4, the second micro-batch non-finite: the whole window is skipped; its three EMA-only calls and the closing call count four EMA
    updates.  Under a static scale the next clean window then gives the parameters and moments of a twin that never saw the bad one, bit for
    bit (the shadows follow the EMA update count, a counter, and are not compared); a dynamic scale has halved."""
    cfg, sd, _, _, _ = R16.problem("tiny")
    good = [R16.round_fp16(R.batch(cfg, 3, 12, seed=s)) for s in (6, 16, 26, 36)]
    tr = _trainer(cfg, sd, precision="fp16", loss_scale=loss_scale, gradient_accumulation_steps=4, lr=1e-3)
    p0 = _snap(tr.p)
    for n, b in enumerate([good[0], _bad(good[1]), good[2], good[3]]):
        loss = float(_step(tr, b))
        assert np.isfinite(loss) == (n != 1) and tr.sync_gradients == (n == 3)
    assert tr.last_step_skipped and (tr.step_count, tr.skipped_steps, tr.global_step, tr.ema_updates, tr.micro_step) == (0, 1, 1, 4, 0)
    assert tr.skipped_nonfinite_loss == 0 and _same(tr.p, p0)          # the window's LAST loss was finite
    assert tr.loss_scale_value == (1024.0 if loss_scale == 1024.0 else 512.0)
    for b in good:
        _step(tr, b)
    assert not tr.last_step_skipped and (tr.step_count, tr.skipped_steps, tr.global_step, tr.ema_updates) == (1, 1, 2, 8)
    if loss_scale == 1024.0:
        twin = _trainer(cfg, sd, precision="fp16", loss_scale=loss_scale, gradient_accumulation_steps=4, lr=1e-3)
        for b in good:
            _step(twin, b)
        assert (twin.step_count, twin.skipped_steps, twin.ema_updates) == (1, 0, 4)
        assert _same(tr.p, twin.p) and _same(_moments(tr), _moments(twin))
        assert torch.equal(_bits(tr.grad_norm.reshape(1)), _bits(twin.grad_norm.reshape(1)))


def test_adamw8bit_clean_and_skipped_step():
    cfg, sd, b, _, _ = R16.problem("tiny")
    tr = _trainer(cfg, sd, precision="fp16", loss_scale="dynamic", optimizer="adamw8bit", lr=1e-3)
    assert np.isfinite(float(_step(tr, b))) and not tr.last_step_skipped and tr.step_count == 1
    before = dict(p=_snap(tr.p), m=_snap(tr._m), v=_snap(tr._v), am=_snap(tr._am), av=_snap(tr._av))
    assert before["am"] and before["m"]
    loss = float(_step(tr, _bad(b)))
    assert not np.isfinite(loss) and tr.last_step_skipped and (tr.step_count, tr.skipped_steps, tr.skipped_nonfinite_loss) == (1, 1, 1)
    assert tr.loss_scale_value == 32768.0
    for name in ("p", "_m", "_v", "_am", "_av"):
        assert _same(getattr(tr, name), before[name.lstrip("_")]), name
    assert np.isfinite(float(_step(tr, b))) and tr.step_count == 2


def _state(tr):
    return dict(p=_snap(tr.p), m=_snap(tr._m), v=_snap(tr._v), shadow=_snap(tr.shadow))


def _counters(tr):
    return (tr.step_count, tr.ema_updates, tr.global_step, tr.loss_scale_value, tr.growth_tracker, tr.skipped_steps, tr.skipped_nonfinite_loss)


def test_resume_is_bit_for_bit(tmp_path):
    """clean, skipped, clean, clean (growth_interval 3: the tracker stands at 2), save, load into a fresh trainer: three more steps, one of
    them skipped, give the same bits; scale, tracker and both skip counters come back.  trainer_state.json records them."""
    cfg, sd, _, _, _ = R16.problem("tiny")
    batches = [R16.round_fp16(R.batch(cfg, 3, 12, seed=s)) for s in (6, 16, 26, 36)]
    kw = dict(precision="fp16", loss_scale=dict(init_scale=4096.0, growth_interval=3), lr=1e-3)
    a = _trainer(cfg, sd, **kw)
    for b in (batches[0], _bad(batches[1]), batches[2], batches[3]):
        _step(a, b)
    assert _counters(a) == (3, 4, 4, 2048.0, 2, 1, 1)
    ck = str(tmp_path / "ck")
    a.save_checkpoint(ck)
    with open(os.path.join(ck, "trainer_state.json")) as f:
        js = json.load(f)
    assert js["precision"] == "fp16" and js["global_step"] == 4
    assert js["loss_scale"] == dict(scale=2048.0, growth_tracker=2, skipped_steps=1, skipped_nonfinite_loss=1,
                                    settings=dict(init_scale=4096.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3, dynamic=True))
    fresh = _trainer(cfg, sd, precision="fp16", loss_scale="dynamic", lr=1e-3)
    fresh.load_checkpoint(ck)
    assert _counters(fresh) == _counters(a) and _same(_state(a)["p"], _state(fresh)["p"])
    for b in (batches[1], _bad(batches[0]), batches[2]):
        la, lf = _step(a, b), _step(fresh, b)
        assert torch.equal(_bits(la.reshape(1)), _bits(lf.reshape(1)))
        sa, sf = _state(a), _state(fresh)
        assert all(_same(sa[part], sf[part]) for part in sa) and _counters(a) == _counters(fresh)
    assert _counters(a) == (5, 7, 7, 2048.0, 1, 2, 2)                  # grew to 4096 on the third clean step, halved by the skip


def test_checkpoints_cross_the_precisions(tmp_path):
    """A bf16 checkpoint (no `loss_scale` key) loads into an fp16 trainer, which starts from its init_scale; an fp16 checkpoint loads into a
    bf16 trainer, which ignores the key.  The master state is fp32 either way."""
    cfg, sd, b, _, _ = R16.problem("tiny")
    bf = _trainer(cfg, sd, precision="bf16", lr=1e-3)
    _step(bf, b), _step(bf, b)
    ck_b = str(tmp_path / "bf16")
    bf.save_checkpoint(ck_b)
    with open(os.path.join(ck_b, "trainer_state.json")) as f:
        assert "loss_scale" not in json.load(f)
    h = _trainer(cfg, sd, precision="fp16", loss_scale=dict(init_scale=2048.0), lr=1e-3)
    _step(h, _bad(b))
    assert h.loss_scale_value == 1024.0 and h.skipped_steps == 1
    h.load_checkpoint(ck_b)
    assert _counters(h) == (2, 2, 2, 2048.0, 0, 0, 0) and all(_same(_state(bf)[part], _state(h)[part]) for part in ("p", "m", "v", "shadow"))
    assert np.isfinite(float(_step(h, b))) and not h.last_step_skipped and h.step_count == 3
    ck_h = str(tmp_path / "fp16")
    h.save_checkpoint(ck_h)
    back = _trainer(cfg, sd, precision="bf16", lr=1e-3)
    back.load_checkpoint(ck_h)
    assert (back.step_count, back.global_step, back.skipped_steps, back.loss_scale_value) == (3, 3, 0, 1.0)
    assert all(_same(_state(h)[part], _state(back)[part]) for part in ("p", "m", "v", "shadow"))
    assert np.isfinite(float(_step(back, b))) and back.global_step == 4


@pytest.mark.parametrize("prediction_type", ["sample", "epsilon"])
def test_thirty_steps_follow_the_bf16_trainer(prediction_type):
    """Thirty steps on one batch under the dynamic defaults, through RDTRunner.trainer: last / first loss at most 1.5 x the bf16 trainer's."""
    from tests.test_gpu_rdt_train import _runner
    cfg = cases.RDT_TINY
    b = R.batch(cfg, 3, 12)
    frac, info = {}, ""
    for precision, kw in (("fp16", dict(loss_scale="dynamic")), ("bf16", {})):
        tr = _runner(cfg, prediction_type).trainer(lr=1e-3, precision=precision, **kw)
        losses = [float(_step(tr, b)) for _ in range(30)]
        frac[precision] = float(_get_loss(tr, b, backward=False)) / losses[0]
        if precision == "fp16":
            info = f"scale {tr.loss_scale_value:g}, {tr.skipped_steps} skipped"
            assert tr.global_step == 30 == tr.step_count + tr.skipped_steps
    print(f"[rdt_train fp16 30 steps {prediction_type}] last / first loss: fp16 {frac['fp16']:.4f} ({info}), bf16 {frac['bf16']:.4f}")
    assert np.isfinite(frac["fp16"]) and frac["bf16"] < 1.0
    assert frac["fp16"] <= 1.5 * frac["bf16"], frac


def test_sampler_equals_sync_to():
    from tests.test_gpu_rdt_train import _runner
    cfg = cases.RDT_TINY
    b = R.batch(cfg, 3, 12)
    d = cases.rdt_inputs(cfg, 3, 12)
    r = _runner(cfg)
    pa = lambda rr: rr.predict_action(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_mask"], b["ctrl_freqs"],
                                      x_init=d["x_init"]).float().cpu()
    before = pa(r)
    tr = r.trainer(lr=1e-3, precision="fp16", loss_scale="dynamic", attention_backward="mfma")
    for _ in range(3):
        _step(tr, b)
    assert tr.step_count >= 1
    a1 = pa(tr.sampler())
    a2 = pa(tr.sync_to(r))
    assert torch.equal(a1, a2) and float((a1 - before).abs().max()) > 1e-4
