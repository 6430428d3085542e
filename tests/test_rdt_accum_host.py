"""Host-side checks of gradient accumulation and resumable checkpoints for the RDT fine-tuning step (no GPU): the fp64 restatement of the
accumulated loop (tests/rdt_accum_ref.py) against the reference's own run under accelerate (tests/golden/g17_rdt_accum.npz,
tools/make_golden_rdt_accum.py), the lr and EMA-decay sequences exactly, and the host logic of the trainer and of the loop helper."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import rdt_train_ref as R
from tests import rdt_accum_ref as A


def _g17():
    return np.load(f"{cases.GOLDEN}/g17_rdt_accum.npz")


def test_golden_records_the_run_the_restatement_is_configured_for():
    g = _g17()
    assert "UNPINNED" in str(g["add_noise"]) and "UNPINNED" in str(g["lr_lambda"])
    assert tuple(int(s) for s in g["seeds"]) == A.G17_SEEDS and len(A.G17_SEEDS) == 3 * A.G17_K
    assert list(g["hyper"]) == [A.G17_HP["lr"], A.G17_HP["weight_decay"], A.G17_MAX_GRAD_NORM, A.G17_K, A.G17_WARMUP]


@pytest.mark.parametrize("rms_mode,scheduler", A.G17_RUNS)
def test_accumulated_loop_matches_the_references_own_run(rms_mode, scheduler):
    """g17 = the reference's compute_loss / EMAModel / AdamW under accelerate's accumulation in fp32.  The fp64 restatement reproduces it with the
    bars of the g16 host test: loss and norm before clipping 1e-5 relative, every tensor's accumulated gradient (first window: the parameters are
    still the golden's) within 1e-4 of its norm, updates and EMAs within 5 x what the same loop in fp32 torch loses against fp64 torch.  The logged
    lr, the EMA decay of every micro-batch and the sync pattern are equal."""
    g = _g17()
    names = [str(n) for n in g["names"]]
    cfg, k = cases.RDT_TINY, A.G17_K
    sd = cases.rdt_sd(cfg)
    assert sorted(names) == sorted(sd)
    batches = [R.batch(cfg, A.G17_B, A.G17_LANG_LEN, seed=s) for s in A.G17_SEEDS]
    kw = dict(lr=A.G17_HP["lr"], weight_decay=A.G17_HP["weight_decay"], betas=A.G17_HP["betas"], eps=A.G17_HP["eps"], max_grad_norm=A.G17_MAX_GRAD_NORM,
              lr_scheduler=scheduler, lr_warmup_steps=A.G17_WARMUP, rms_mode=rms_mode, prediction_type="sample")
    r64 = A.accum_train_steps(sd, batches, cfg, k, dtype=torch.float64, **kw)
    r32 = A.accum_train_steps(sd, batches, cfg, k, dtype=torch.float32, **kw)
    p0 = {n: v.double() for n, v in sd.items()}
    tag = f"{rms_mode}_{scheduler}"
    sc, norms = g[f"{tag}_scalars"], g[f"{tag}_norms"]
    assert sc.shape == (len(batches), 4) and norms.shape == (len(batches) // k,)
    step = 0
    for n, rec in enumerate(r64):
        loss, decay, lr, sync = sc[n]
        assert abs(rec["loss"] - loss) <= 1e-5 * loss, (n, rec["loss"], loss)
        assert decay == rec["ema_decay"] == R.ema_decay(n), (n, decay)
        assert lr == rec["lr"], (n, lr, rec["lr"])
        assert bool(sync) == rec["sync"] == ((n + 1) % k == 0)
        t64 = np.stack([R.summary(key, rec["ema"][key] - p0[key]) for key in names])
        base_e, _ = R.worst_summary(t64, names, {key: r32[n]["ema"][key] - p0[key] for key in sd})
        we, ke = R.worst_summary(g[f"{tag}_m{n + 1}_ema"], names, {key: rec["ema"][key] - p0[key] for key in sd})
        assert we <= 5 * base_e, ("ema", n, ke, we, base_e)
        if not rec["sync"]:
            continue
        step += 1
        assert abs(rec["grad_norm"] - norms[step - 1]) <= 1e-5 * norms[step - 1]
        if step == 1:
            wg, kg = R.worst_summary(g[f"{tag}_s1_grad"], names, rec["grad"])
            assert wg <= 1e-4, (kg, wg)
        t64 = np.stack([R.summary(key, rec["params"][key] - p0[key]) for key in names])
        base, _ = R.worst_summary(t64, names, {key: r32[n]["params"][key] - p0[key] for key in sd})
        wu, ku = R.worst_summary(g[f"{tag}_s{step}_update"], names, {key: rec["params"][key] - p0[key] for key in sd})
        print(f"[g17 {tag} step {step}] loss {loss:.6f}, norm {norms[step - 1]:.4f}, lr {lr:g}; update {wu:.2e} ({ku}), ema {we:.2e}; "
              f"fp32-vs-fp64 torch {base:.2e} / {base_e:.2e}")
        assert wu <= 5 * base, ("update", step, ku, wu, base)
        assert np.array_equal(g[f"{tag}_s{step}_ema"], g[f"{tag}_m{n + 1}_ema"])
    assert step == 3


def test_lr_sequence_of_the_trainer_is_the_references():
    """`lr_at` with the warm-up multiplied by k, evaluated once per optimizer step, gives the lr the reference's optimizer used and logged."""
    from vlatouch.rdt_train import lr_at
    g, k = _g17(), A.G17_K
    for rms_mode, scheduler in A.G17_RUNS:
        logged = g[f"{rms_mode}_{scheduler}_scalars"][:, 2]
        for n in range(len(logged)):
            steps_done = (n + 1) // k                                   # scheduler steps behind micro-batch n
            assert logged[n] == lr_at(A.G17_HP["lr"], scheduler, steps_done, A.G17_WARMUP * k), (scheduler, n)
            assert logged[n] == A.G17_HP["lr"] * A.lr_multiplier(scheduler, steps_done, A.G17_WARMUP * k)
    assert [lr_at(1e-3, "constant_with_warmup", s, 1 * 4) for s in range(6)] == [0.0, 2.5e-4, 5e-4, 7.5e-4, 1e-3, 1e-3]


def test_ema_decay_advances_per_micro_batch():
    """Decays in g17 are EMAModel.get_decay(0 .. 11): the count runs over micro-batches, k times as fast as the optimizer's."""
    from vlatouch.rdt_train import ema_decay
    g = _g17()
    for rms_mode, scheduler in A.G17_RUNS:
        dec = g[f"{rms_mode}_{scheduler}_scalars"][:, 1]
        assert [float(d) for d in dec] == [ema_decay(n) for n in range(12)] == [R.ema_decay(n) for n in range(12)]
    assert dec[0] == 0.0 and dec[1] == 0.0 and dec[2] == 1 - 2 ** (-2 / 3)


def test_two_fp64_references_agree():
    """(1/k) sum of the micro-batch gradients = the gradient of the concatenated batch (equal-size micro-batches), to the fp32 rounding of the
    oracle's attention products (A.REFS_AGREE); the loss, a mean over all samples, to 1e-10."""
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, A.G17_B, A.G17_LANG_LEN, seed=s) for s in A.G17_SEEDS[:4]]
    losses, acc = A.accumulated_grads(sd, batches, cfg)
    loss_c, g_c = R.loss_and_grads(sd, A.concat_batch(batches), cfg)
    assert abs(sum(losses) / 4 - loss_c) <= 1e-10 * loss_c
    worst = max(R.rel_err(acc[key], g_c[key]) for key in sd)
    print(f"[accumulated vs concatenated, fp64] worst tensor {worst:.2e} of its norm")
    assert worst <= A.REFS_AGREE


def test_table_builder_matches_the_hand_written_prefix_sum():
    """train.mt_table against the layout written out here: rows {p, g, m, v, shadow, n, first_chunk}, first_chunk the running sum of
    ceil(n / 4096), the total that sum over all rows; a tensor without a shadow carries 0."""
    from vlatouch.train import MT_CHUNK, mt_table
    assert MT_CHUNK == 4096
    sizes = [1, 2, 3, 5, 255, 1023, 4095, 4096, 4097, 4099, 3 * 4096, 70001]
    given = [(1000 + 16 * i, 2000 + 16 * i, 3000 + 16 * i, 4000 + 16 * i, 0 if i % 5 == 1 else 5000 + 16 * i, n) for i, n in enumerate(sizes)]
    want, chunk0 = [], 0
    for p, g, m, v, sh, n in given:
        want.append([p, g, m, v, sh, n, chunk0])
        chunk0 += (n + 4095) // 4096
    rows, total = mt_table(iter(given))
    assert rows.dtype == torch.int64 and rows.device.type == "cpu" and rows.shape == (len(sizes), 7) and rows.is_contiguous()
    assert rows.tolist() == want and total == chunk0 == 8 * 1 + 2 * 2 + 3 + 18
    one, total1 = mt_table([(8, 16, 24, 32, 40, 4096)])
    assert one.tolist() == [[8, 16, 24, 32, 40, 4096, 0]] and total1 == 1


def test_trainer_rejects_accumulation_steps_below_one():
    """Before the device is required, like the other constructor checks."""
    from vlatouch.rdt_train import RdtTrainer
    kw = dict(heads=4, horizon=8, action_dim=128)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            RdtTrainer({}, gradient_accumulation_steps=bad, **kw)


def test_save_in_the_middle_of_a_window_raises(tmp_path):
    from vlatouch.rdt_train import RdtTrainer
    tr = object.__new__(RdtTrainer)                    # the check comes before anything touches the device or the weights
    tr.k, tr.micro_step = 4, 2
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.save_checkpoint(str(tmp_path / "checkpoint-1"))
    assert not os.path.exists(tmp_path / "checkpoint-1")


def test_latest_checkpoint_selection(tmp_path):
    from vlatouch.rdt_train import latest_checkpoint, finetune
    assert latest_checkpoint(str(tmp_path / "missing")) is None and latest_checkpoint(str(tmp_path)) is None
    for name in ("checkpoint-2", "checkpoint-10", "checkpoint-9", "checkpoint-x", "checkpoints", "ema", "checkpoint-1000"):
        os.makedirs(tmp_path / name)
    assert latest_checkpoint(str(tmp_path)) == "checkpoint-1000"                 # numeric order: 1000 > 10 > 9 > 2
    os.rmdir(tmp_path / "checkpoint-1000")
    assert latest_checkpoint(str(tmp_path)) == "checkpoint-10"
    with pytest.raises(ValueError):
        finetune(None, [], max_train_steps=1, checkpointing_period=2)
