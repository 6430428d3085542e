"""fp16 fine-tuning's loss scaling on the host: the statement of tests/loss_scale_ref.py against torch.amp.GradScaler("cpu") and accelerate,
the trainer's own LossScaler against that statement, the constructor's validation, unscale-then-clip against GradScaler.unscale_ +
clip_grad_norm_ bit for bit, and the fp16 statement of the MFMA attention backward against fp64.  No GPU."""
import math

import pytest
import torch

from tests import attn_bwd_mfma16_ref as A16
from tests import loss_scale_ref as S


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sequence_properties(seq, interval):
    """(two overflows in a row, an overflow on the step where growth would fire, growth fired) under the statement."""
    sc, twice, on_growth, grew = S.Scaler(growth_interval=interval), False, False, False
    for n, bad in enumerate(seq):
        twice |= bad and n > 0 and seq[n - 1]
        on_growth |= bad and sc.tracker == interval - 1
        before = sc.value
        sc.update(bad)
        grew |= sc.value > before
    return twice, on_growth, grew


def test_scaler_statement_against_torch_gradscaler():
    """growth_interval 3, the fixed 40-step overflow sequence: scale and growth tracker equal torch's after every step (so do the trainer's
    LossScaler's), and a one-parameter AdamW run under GradScaler moves the parameter and Adam's step count on clean steps only."""
    from vlatouch.rdt_train import LossScaler, loss_scale_settings
    seq = S.OVERFLOW_SEQUENCE
    assert len(seq) == 40 and _sequence_properties(seq, 3) == (True, True, True)
    p = torch.nn.Parameter(torch.tensor([1.0]))
    opt = torch.optim.AdamW([p], lr=0.1)
    gs = torch.amp.GradScaler("cpu", growth_interval=3)
    st = S.Scaler(growth_interval=3)
    mine = LossScaler(loss_scale_settings(dict(growth_interval=3)))
    clean = 0
    for n, bad in enumerate(seq):
        opt.zero_grad()
        with torch.enable_grad():
            gs.scale((p * (0.3 + 0.1 * n)).sum()).backward()
        assert float(p.grad) == float(torch.tensor(0.3 + 0.1 * n, dtype=torch.float32) * st.scale)      # .grad holds the SCALED gradient
        if bad:
            p.grad.fill_(float("inf"))
        before = p.detach().clone()
        gs.step(opt)
        gs.update()
        st.update(bad)
        mine.update(bad)
        clean += not bad
        assert gs.get_scale() == st.value == mine.scale, (n, gs.get_scale(), st.value, mine.scale)
        assert int(gs._growth_tracker) == st.tracker == mine.growth_tracker, n
        assert torch.equal(p.detach(), before) == bad, (n, "the parameter moves on clean steps only")
        assert int(opt.state[p]["step"]) == clean if clean else p not in opt.state or int(opt.state[p]["step"]) == 0
    assert st.skipped == mine.skipped_steps == sum(seq)


def test_static_scaler_counts_but_never_moves():
    from vlatouch.rdt_train import LossScaler, loss_scale_settings
    st, mine = S.Scaler(init_scale=3000.0, growth_interval=2, dynamic=False), LossScaler(loss_scale_settings(3000.0))
    assert mine.settings["dynamic"] is False
    for bad in (False, False, True, False, True, True):
        st.update(bad), mine.update(bad)
        assert st.value == mine.scale == 3000.0
    assert st.skipped == mine.skipped_steps == 3 and mine.growth_tracker == 0


def test_scheduler_does_not_advance_on_a_skipped_step_under_accelerate():
    """Accelerator(mixed_precision="fp16", cpu=True) constructs here, but accelerate builds its GradScaler only off the CPU
    (accelerate/accelerator.py:563-583: `self.device.type != "cpu"`), so the test hands the accelerator a torch.amp.GradScaler("cpu") before
    `prepare`; from there the reference's calls run unchanged: accelerator.backward (scaler.scale(loss).backward(), accelerator.py:2845),
    accelerator.clip_grad_norm_ (unscale_ first), AcceleratedOptimizer.step (scaler.step + scaler.update, sets step_was_skipped:
    accelerate/optimizer.py:163-173), AcceleratedScheduler.step (returns early when an optimizer skipped: accelerate/scheduler.py:66-68)."""
    from accelerate import Accelerator
    from accelerate.state import AcceleratorState
    try:
        acc = Accelerator(mixed_precision="fp16", cpu=True)
        assert acc.scaler is None
        acc.scaler = torch.amp.GradScaler("cpu", growth_interval=3)
        model = torch.nn.Linear(1, 1, bias=False)
        opt = torch.optim.AdamW(model.parameters(), lr=0.1)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda n: 1.0 / (1 + n))
        model, opt, sched = acc.prepare(model, opt, sched)
        st, clean = S.Scaler(growth_interval=3), 0
        w = next(model.parameters())
        for n, bad in enumerate(S.OVERFLOW_SEQUENCE):
            opt.zero_grad()
            with torch.enable_grad():
                loss = (w * (float("inf") if bad else 0.3 + 0.1 * n)).sum()
                acc.backward(loss)
            before = w.detach().clone()
            acc.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            sched.step()
            st.update(bad)
            clean += not bad
            assert opt.step_was_skipped == bad, n
            assert acc.scaler.get_scale() == st.value and int(acc.scaler._growth_tracker) == st.tracker, n
            assert sched.scheduler.last_epoch == clean, (n, "the scheduler advances on clean steps only")
            assert torch.equal(w.detach(), before) == bad, n
    finally:
        AcceleratorState._reset_state(True)


def test_constructor_validation():
    """Every case of the interface, before the device is needed (the state dict is empty and no GPU is asked for)."""
    from vlatouch.rdt_train import COMM_DTYPES, RdtTrainer, loss_scale_settings, LOSS_SCALE_DEFAULTS
    kw = dict(heads=4, horizon=8, action_dim=128)
    assert COMM_DTYPES == ("fp32", "bf16")
    with pytest.raises(ValueError, match="loss_scale"):
        RdtTrainer({}, precision="fp16", **kw)                          # as before this mode existed
    for prec in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="loss_scale"):
            RdtTrainer({}, precision=prec, loss_scale="dynamic", **kw)
    bad = [0.0, -1.0, float("inf"), float("nan"), 1e-50, True, "static", None.__class__, dict(init_scale=0.0), dict(init_scale=float("inf")),
           dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=0.0), dict(backoff_factor=1.0), dict(backoff_factor=1.5),
           dict(growth_interval=0), dict(growth_interval=2.5), dict(growth=2.0), dict(init_scale="big")]
    for value in bad:
        with pytest.raises(ValueError, match="loss_scale"):
            RdtTrainer({}, precision="fp16", loss_scale=value, **kw)
    with pytest.raises(ValueError, match="fp32"):
        RdtTrainer({}, precision="fp32", attention_backward="mfma", **kw)
    assert loss_scale_settings("dynamic") == dict(LOSS_SCALE_DEFAULTS, dynamic=True)
    assert LOSS_SCALE_DEFAULTS == dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000) == S.DEFAULTS
    assert loss_scale_settings(dict(init_scale=2.0 ** 24, growth_interval=2)) == dict(init_scale=2.0 ** 24, growth_factor=2.0, backoff_factor=0.5,
                                                                                      growth_interval=2, dynamic=True)
    assert loss_scale_settings(1024) == dict(LOSS_SCALE_DEFAULTS, init_scale=1024.0, dynamic=False)
    # a valid fp16 request passes every check and then asks for the device: any error from here on is not a ValueError about the arguments
    for ok in (dict(loss_scale="dynamic"), dict(loss_scale=1024.0, attention_backward="mfma", comm_dtype="bf16", optimizer="adamw8bit",
                                                gradient_accumulation_steps=4)):
        try:
            RdtTrainer({}, precision="fp16", device="cpu", **ok, **kw)
        except ValueError as e:                                          # pragma: no cover
            pytest.fail(f"a valid fp16 request was refused: {e}")
        except Exception:
            pass


def _torch_unscale_clip(chunks, scale, max_norm):
    params = [torch.nn.Parameter(torch.zeros_like(c)) for c in chunks]
    for p, c in zip(params, chunks):
        p.grad = c.clone()
    opt = torch.optim.SGD(params, lr=0.0)
    gs = torch.amp.GradScaler("cpu", init_scale=scale)
    gs.scale(torch.zeros(()))                                            # GradScaler creates its scale tensor lazily
    gs.unscale_(opt)
    found = sum(float(v) for v in gs._per_optimizer_states[id(opt)]["found_inf_per_device"].values()) > 0
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return found, norm, [p.grad for p in params]


@pytest.mark.parametrize("scale", [2.0 ** 16, 3000.0])
def test_unscale_then_clip_bit_equal_to_torch(scale):
    """200 000 mixed-magnitude fp32 values as four tensors: the statement (raw-element check, torch's inv_S, two multiplications) gives the
    bits of GradScaler.unscale_ + clip_grad_norm_, with the clip active and with it idle, at a power of two and at S = 3000."""
    v = S.mixed_magnitudes()
    assert v.numel() == 200_000 and 1e10 < float(v.abs().max() / v[v != 0].abs().min())
    sizes = [1, 4097, 100_000, 200_000 - 104_098]
    chunks = [c.clone() for c in torch.split(v, sizes)]
    for max_norm in (1.0, 1e9):
        found_t, norm_t, out_t = _torch_unscale_clip(chunks, scale, max_norm)
        found, norm, coef, out = S.unscale_clip(chunks, scale, max_norm)
        assert found is False and found_t is False
        assert torch.equal(_bits(norm.reshape(1)), _bits(norm_t.reshape(1)))
        assert (float(coef) < 1.0) == (max_norm == 1.0)
        for a, b in zip(out, out_t):
            assert torch.equal(_bits(a), _bits(b))
    if scale == 3000.0:                                                  # one multiplication by inv_S * coef would NOT give these bits
        inv, (_, _, coef, out) = S.inv_scale(scale), S.unscale_clip(chunks, scale, 1.0)
        assert any(not torch.equal(_bits(c * (inv * coef)), _bits(o)) for c, o in zip(chunks, out))


def test_unscale_then_clip_flags_inf_and_nan():
    v = S.mixed_magnitudes()
    chunks = [c.clone() for c in torch.split(v, [1, 4097, 100_000, 200_000 - 104_098])]
    chunks[1][4096] = float("inf")
    chunks[3][77] = float("nan")
    found_t, _, _ = _torch_unscale_clip(chunks, 2.0 ** 16, 1.0)
    found, _, _, out = S.unscale_clip(chunks, 2.0 ** 16, 1.0)
    assert found is True and found_t is True
    for a, b in zip(out, chunks):                                        # untouched
        assert torch.equal(_bits(a), _bits(b))
    for i, val in ((1, float("inf")), (3, float("nan"))):               # either alone is enough
        one = [c.clone() for c in torch.split(v, [1, 4097, 100_000, 200_000 - 104_098])]
        one[i][5] = val
        assert S.unscale_clip(one, 2.0 ** 16, 1.0)[0] is True and _torch_unscale_clip(one, 2.0 ** 16, 1.0)[0] is True


def test_inv_scale_is_torchs():
    from vlatouch.rdt_train import inv_scale
    for s in (1.0, 3000.0, 65536.0, 2.0 ** 24, 1e-3, 7.0):
        assert inv_scale(s) == float(S.inv_scale(s)) == float(torch.tensor(s).double().reciprocal().float())


@pytest.mark.parametrize("case", A16.CASES, ids=lambda c: f"{c[1]}x{c[2]}-H{c[3]}")
def test_fp16_mfma_statement_against_fp64(case):
    """The fp16 statement's max-abs error per gradient is at most 1.5 x that of torch's own fp16 backward on the CPU (the bar the bf16 statement
    is held to); masked keys and fully masked rows are exactly zero."""
    (bufs, views, do, mask), ref, th = A16.refs(case)
    q, k, v = views(*bufs)
    got = A16.statement(q, k, v, do, mask=mask)
    for i, name in enumerate(("dq", "dk", "dv")):
        e, et = float((got[i].double() - ref[i]).abs().max()), float((th[i] - ref[i]).abs().max())
        print(f"[fp16 mfma statement {case[1]}x{case[2]} H{case[3]}] {name}: max err {e:.3e}; torch fp16 on the CPU {et:.3e}")
        assert bool(torch.isfinite(got[i]).all()) and e <= 1.5 * et, (name, e, et)
    if mask is not None:
        assert float(got[1][~mask].abs().max()) == 0.0 and float(got[2][~mask].abs().max()) == 0.0
        assert all(float(got[i][1].abs().max()) == 0.0 for i in range(3))


def test_inverse_of_the_largest_scale_is_finite():
    assert math.isfinite(S.inv_scale(2.0 ** 24))


def test_recorded_fp16_oracle_errors_are_what_the_oracle_reaches():
    """tests/golden/g21_fp16_oracle_errors.json against the oracle run now, on RDT_TINY (RDT_WIDE takes over a minute where the CPU has no
    native half arithmetic): same tensors, the fp64 gradient norm to 1e-6 (fp32 tables and libm calls inside the oracle move it by some 1e-8 between CPUs), and the all-parameter error within 10 % — two CPUs' fp16 matmul
    kernels sum in different orders, which moved this figure by 4 % between the two machines it was taken on."""
    from tests import rdt_train16_ref as R16
    want, got = R16.oracle_errors("tiny"), R16.oracle_errors_fresh("tiny")
    assert set(want["tensor_error"]) == set(got["tensor_error"])
    assert abs(want["grad_norm"] - got["grad_norm"]) <= 1e-6 * got["grad_norm"]
    assert abs(want["total_error"] - got["total_error"]) <= 0.10 * got["total_error"], (want["total_error"], got["total_error"])
    for name in ("tiny", "wide"):
        rec = R16.oracle_errors(name)
        assert 2e-4 < rec["total_error"] / rec["grad_norm"] < 1e-3
