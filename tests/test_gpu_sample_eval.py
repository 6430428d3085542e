"""Fine-tuning's periodic sampling evaluation on the device: vt_sample_metrics (csrc/vt_sample_eval.hip) as a unit, the device-side hand-over of
the live weights (`RdtTrainer.sampler`), `sample_eval` / `train.sample.log_sample_res` end to end, and `finetune(sample_period=...)`, against
the fp64 restatement of the reference's `log_sample_res` (tests/sample_eval_ref.py, itself held to the reference's own run by
tests/test_sample_eval_host.py).

Bar of every metric, the project's standing rule: max(3 x the error of the fp32 torch statement on the CPU against fp64, 1e-6 relative), per
output; NaN where the restatement has NaN and nowhere else."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import rdt_train_ref as R
from tests import sample_eval_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
SENTINEL = 12345
SHAPES = [(1, 1, 1), (3, 8, 128), (5, 64, 128), (2, 7, 10), (4, 3, 130)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
N_DATASETS = 3
VT_ERR_ARG = -22


def _L():
    from vlatouch import _lib as L
    return L


class _Out:
    """n values of `dtype` filled with `fill`, GUARD sentinel words behind them."""

    def __init__(self, n, dtype, fill):
        self.n = n
        self.buf = torch.cat([torch.full((n,), fill, dtype=dtype), torch.full((GUARD,), SENTINEL, dtype=dtype)]).to(DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def values(self):
        return self.buf[:self.n].cpu()

    def guard_intact(self):
        return bool((self.buf[self.n:].cpu() == SENTINEL).all())


def _launch(inp, dtype, outs):
    L = _L()
    B, H, A = inp["pred"].shape
    dev = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    pred = dev["pred"].to(dtype).contiguous()
    code = L.lib().vt_sample_metrics(L.ptr(pred), L.dt_code(dtype), L.ptr(dev["target"]), L.ptr(dev["mask"]), L.ptr(dev["state_norm"]),
                                     L.ptr(dev["dataset_idx"]), B, H, A, N_DATASETS, outs["per"].ptr, outs["overall"].ptr, outs["acc"].ptr,
                                     outs["count"].ptr, outs["ws"].ptr, L.stream_ptr(torch.device(DEV)))
    L.check(code, "vt_sample_metrics")
    torch.cuda.synchronize()


def _fresh_outs(B):
    nan = float("nan")
    return dict(per=_Out(2 * B, torch.float32, nan), overall=_Out(2, torch.float32, nan), ws=_Out(3 * B, torch.float64, nan),
                acc=_Out(2 * (N_DATASETS + 1), torch.float64, 0.0), count=_Out(N_DATASETS + 1, torch.int32, 0))


def _rounded(inp, dtype):
    """The inputs as the kernel sees them: pred on the grid of `dtype`."""
    return dict(inp, pred=inp["pred"].to(dtype).float())


def _within(got, want64, want32, what):
    """got against the fp64 restatement under the standing bar; -> worst error / bar."""
    got, want64, want32 = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want64, want32))
    assert np.array_equal(np.isnan(got), np.isnan(want64)), (what, "NaN places", got, want64)
    ok = ~np.isnan(want64)
    err = np.abs(got[ok] - want64[ok])
    bar = np.maximum(3 * np.abs(want32[ok] - want64[ok]), 1e-6 * np.abs(want64[ok]))
    assert bool((err <= bar).all()), (what, got[ok], want64[ok], err / bar)
    return float((err[bar > 0] / bar[bar > 0]).max()) if bool((bar > 0).any()) else 0.0


@functools.lru_cache(maxsize=None)
def _case(shape, dname, zero_mask_sample=None):
    B, H, A = shape
    inp = _rounded(S.metric_inputs(B, H, A, seed=sum(shape) + len(dname), zero_mask_sample=zero_mask_sample, n_datasets=N_DATASETS), DTYPES[dname])
    refs = tuple(S.batch_metrics(inp["pred"], inp["target"], inp["mask"], inp["state_norm"], dt) for dt in (torch.float64, torch.float32))
    return inp, refs


# ------------------------------------------------------------------------------------------------ the kernel as a unit
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics_kernel_against_fp64(shape, dname):
    """One call on NaN-filled outputs, twice: bit-equal as integer views, guard words untouched; per_sample and overall within the bar of the
    fp64 restatement from the same (rounded) inputs; acc / count = the one batch folded into zeros."""
    inp, ((per64, ov64), (per32, ov32)) = _case(shape, dname)
    B = shape[0]
    runs = []
    for _ in range(2):
        outs = _fresh_outs(B)
        _launch(inp, DTYPES[dname], outs)
        assert all(o.guard_intact() for o in outs.values()), "guard words"
        runs.append({k: o.values() for k, o in outs.items()})
    a, b = runs
    for k in ("per", "overall"):
        assert a[k].view(torch.int32).equal(b[k].view(torch.int32)), ("two runs differ", k)
    for k in ("acc", "ws"):
        assert a[k].view(torch.int64).equal(b[k].view(torch.int64)), ("two runs differ", k)
    assert a["count"].equal(b["count"])
    assert not bool(torch.isnan(a["ws"]).any()) and not bool(torch.isnan(a["per"]).any())
    w1 = _within(a["per"].view(B, 2), per64, per32, "per_sample")
    w2 = _within(a["overall"], ov64, ov32, "overall")
    (acc64, cnt64), = S.running_sums([inp], N_DATASETS, torch.float64)
    (acc32, _), = S.running_sums([inp], N_DATASETS, torch.float32)
    w3 = _within(a["acc"].view(-1, 2), acc64, acc32, "acc")
    assert a["count"].tolist() == cnt64.tolist()
    print(f"[vt_sample_metrics {shape} {dname}] worst error / bar: per_sample {w1:.3f}, overall {w2:.3f}, acc {w3:.3f}")


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_running_sums_over_successive_calls(dname):
    """Three batches into one acc / count: after the second and after the third call they equal the restatement's running sums under the bar,
    the counts exactly; rows are folded in index order (two samples of one dataset in a batch)."""
    B, H, A = 3, 8, 128
    batches = [_rounded(S.metric_inputs(B, H, A, seed=40 + j, n_datasets=N_DATASETS), DTYPES[dname]) for j in range(3)]
    batches[0]["dataset_idx"] = torch.tensor([1, 1, 0], dtype=torch.int32)
    r64, r32 = S.running_sums(batches, N_DATASETS, torch.float64), S.running_sums(batches, N_DATASETS, torch.float32)
    outs = _fresh_outs(B)
    for j, inp in enumerate(batches):
        _launch(inp, DTYPES[dname], outs)
        if j >= 1:
            w = _within(outs["acc"].values().view(-1, 2), r64[j][0], r32[j][0], f"acc after {j + 1} calls")
            assert outs["count"].values().tolist() == r64[j][1].tolist()
            print(f"[vt_sample_metrics running, {dname}] after {j + 1} calls: worst error / bar {w:.3f}, counts {r64[j][1].tolist()}")
    assert all(o.guard_intact() for o in outs.values())
    assert outs["count"].values()[N_DATASETS] == 3


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_all_zero_mask_sample_gives_nan_where_the_reference_does(dname):
    shape = (3, 8, 128)
    inp, ((per64, ov64), (per32, ov32)) = _case(shape, dname, 1)
    assert bool(torch.isnan(per64[1]).all()) and not bool(torch.isnan(per64[[0, 2]]).any()) and bool(torch.isfinite(ov64).all())
    outs = _fresh_outs(3)
    _launch(inp, DTYPES[dname], outs)
    _within(outs["per"].values().view(3, 2), per64, per32, "per_sample")
    w = _within(outs["overall"].values(), ov64, ov32, "overall")
    assert bool(torch.isfinite(outs["overall"].values()).all())
    (acc64, cnt64), = S.running_sums([inp], N_DATASETS, torch.float64)
    (acc32, _), = S.running_sums([inp], N_DATASETS, torch.float32)
    _within(outs["acc"].values().view(-1, 2), acc64, acc32, "acc")
    d = int(inp["dataset_idx"][1])
    assert bool(torch.isnan(outs["acc"].values().view(-1, 2)[d]).all()) and outs["count"].values().tolist() == cnt64.tolist()
    print(f"[vt_sample_metrics zero mask, {dname}] overall error / bar {w:.3f}")


def test_bad_arguments_return_err_arg():
    L = _L()
    inp, _ = _case((3, 8, 128), "fp32")
    dev = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    outs = _fresh_outs(3)
    sp = L.stream_ptr(torch.device(DEV))

    def call(**over):
        a = dict(pred=L.ptr(dev["pred"]), target=L.ptr(dev["target"]), mask=L.ptr(dev["mask"]), sn=L.ptr(dev["state_norm"]), idx=L.ptr(dev["dataset_idx"]),
                 B=3, H=8, A=128, per=outs["per"].ptr, acc=outs["acc"].ptr, ws=outs["ws"].ptr)
        a.update(over)
        return L.lib().vt_sample_metrics(a["pred"], 0, a["target"], a["mask"], a["sn"], a["idx"], a["B"], a["H"], a["A"], N_DATASETS, a["per"],
                                         outs["overall"].ptr, a["acc"], outs["count"].ptr, a["ws"], sp)

    null = C.c_void_p(0)
    for over in (dict(pred=null), dict(target=null), dict(mask=null), dict(sn=null), dict(idx=null), dict(per=null), dict(acc=null), dict(ws=null),
                 dict(B=0), dict(H=0), dict(A=0)):
        assert call(**over) == VT_ERR_ARG, over
        assert b"vt_sample_metrics" in L.lib().vt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs["per"].values()).all()), "a refused call launches nothing"
    assert call() == 0


# ------------------------------------------------------------------------------------------------ the weight hand-over
def _runner(cfg, dtype=torch.float32, **kw):
    from models.rdt_runner import RDTRunner
    config = {"rdt": {"hidden_size": cfg["hidden"], "depth": cfg["depth"], "num_heads": cfg["heads"]}, "lang_adaptor": "mlp2x_gelu",
              "img_adaptor": "mlp2x_gelu", "state_adaptor": "mlp3x_gelu",
              "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "prediction_type": "sample",
                                  "beta_schedule": "squaredcos_cap_v2"}}
    r = RDTRunner(action_dim=cfg["action_dim"], pred_horizon=cfg["horizon"], config=config, lang_token_dim=cfg["lang_token_dim"],
                  img_token_dim=cfg["img_token_dim"], state_token_dim=cfg["state_token_dim"], max_lang_cond_len=cfg["max_lang_cond_len"],
                  img_cond_len=cfg["img_cond_len"], dtype=dtype, device=DEV, rms_mode="meansq", **kw)
    r.load_state_dict(cases.rdt_sd(cfg))
    return r


def _step(tr, b):
    return tr.train_step(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                         noise=b["noise"], timesteps=b["timesteps"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sampler_hands_over_the_live_weights_on_the_device(dtype):
    """After train steps with fixed noise / timesteps, `trainer.sampler().predict_action(x_init=x)` is bit-equal to a fresh RDTRunner loaded
    through `sync_to` (the route through host memory), for the trained and for the averaged weights; a second call without a step does not
    repack, a call after a step does and the prediction changes; the engine's weights are copies, never the trainer's own tensors.  bf16: a
    runner of the reference's dtype, whose engine holds converted weights (the cast path of the hand-over)."""
    cfg = cases.RDT_TINY
    batches = [R.batch(cfg, 3, 12, seed=s) for s in (6, 16, 26)]
    b, x = batches[0], cases.rdt_inputs(cfg, 3, 12)["x_init"]
    pa = lambda r: r.predict_action(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_mask"], b["ctrl_freqs"],
                                    x_init=x).float().cpu()
    tr = _runner(cfg, dtype).trainer(lr=1e-3)
    before = pa(tr.sampler())                                            # before any step: the initial weights
    assert tr.sampler_repacks == 1 and torch.equal(before, pa(_runner(cfg, dtype)))
    _step(tr, batches[0])
    s = tr.sampler()
    assert tr.sampler_repacks == 2
    a1 = pa(s)
    assert torch.equal(a1, pa(tr.sync_to(_runner(cfg, dtype)))), "sampler() != sync_to after one step"
    assert float((a1 - before).abs().max()) > 0
    assert tr.sampler() is s and tr.sampler_repacks == 2, "no step in between: no repack"
    assert torch.equal(pa(tr.sampler()), a1)
    own = {w.data_ptr() for w in s.engine()._weights}
    assert not own & {v.data_ptr() for v in list(tr.p.values()) + list(tr.shadow.values())}, "the engine must own its weights"
    assert torch.equal(pa(tr.sampler(ema=True)), pa(tr.sync_to(_runner(cfg, dtype), ema=True))) and tr.sampler_repacks == 3
    _step(tr, batches[1])
    a2 = pa(tr.sampler())
    assert tr.sampler_repacks == 4 and float((a2 - a1).abs().max()) > 0, "a step in between: repack, and the prediction changes"
    assert torch.equal(a2, pa(tr.sync_to(_runner(cfg, dtype))))
    _step(tr, batches[2])                                                # third update: the EMA decay is no longer 0, the average differs
    e3, a3 = pa(tr.sampler(ema=True)), pa(tr.sampler())
    assert torch.equal(e3, pa(tr.sync_to(_runner(cfg, dtype), ema=True))) and torch.equal(a3, pa(tr.sync_to(_runner(cfg, dtype))))
    assert float((e3 - a3).abs().max()) > 0 and tr.sampler_repacks == 6
    tr.release_sampler()
    assert tr._sampler is None
    assert torch.equal(pa(tr.sampler()), a3) and tr.sampler_repacks == 7


def test_sampler_keeps_the_runner_s_execution_settings_and_counts_the_shadows_apart():
    """A runner pinned to compute_dtype / solver_state "bf16" gives a trainer whose config carries both, so `sampler()` executes as that runner
    does (bit-equal to it through `sync_to`).  With two micro-batches per optimizer step, the micro-batch that moves only the EMA shadows
    repacks `sampler(ema=True)` and leaves `sampler()` alone: the master weights did not change."""
    cfg = cases.RDT_TINY
    batches = [R.batch(cfg, 3, 12, seed=s) for s in (6, 16, 26)]
    b, x = batches[0], cases.rdt_inputs(cfg, 3, 12)["x_init"]
    pa = lambda r: r.predict_action(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_mask"], b["ctrl_freqs"],
                                    x_init=x).float().cpu()
    pinned = lambda: _runner(cfg, torch.bfloat16, compute_dtype=torch.bfloat16, solver_state="bf16")
    tr = pinned().trainer(lr=1e-3, gradient_accumulation_steps=2)
    assert tr.config["compute_dtype"] == "bf16" and tr.config["solver_state"] == "bf16"
    assert "compute_dtype" not in _runner(cfg, torch.bfloat16).trainer().config, "settings the caller did not give stay out of config.json"
    s = tr.sampler()
    assert s.compute_dtype == torch.bfloat16 and s.solver_state == "bf16" and s._range is None
    _step(tr, batches[0]), _step(tr, batches[1])                         # one optimizer step
    a1 = pa(tr.sampler())
    assert tr.sampler_repacks == 2 and torch.equal(a1, pa(tr.sync_to(pinned())))
    _step(tr, batches[2])                                                # first micro-batch of the next window: EMAModel.step alone
    assert not tr.sync_gradients
    assert tr.sampler() is s and tr.sampler_repacks == 2, "an EMA-only step leaves the master weights: no repack"
    assert torch.equal(pa(tr.sampler(ema=True)), pa(tr.sync_to(pinned(), ema=True))) and tr.sampler_repacks == 3
    tr.sampler(ema=True)
    assert tr.sampler_repacks == 3


# ------------------------------------------------------------------------------------------------ sample_eval end to end
ID2NAME = S.G18_ID2NAME


class _StubVision:
    """[n, 3, 4, 4] images -> [n, img_cond_len / 2, img_token_dim] tokens (two images per sample fill img_cond_len), a fixed function of the pixels."""

    def __init__(self, cfg):
        self.hidden_size, self.tokens = cfg["img_token_dim"], cfg["img_cond_len"] // 2
        g = torch.Generator().manual_seed(5)
        self.table = torch.randn(3 * 4 * 4, self.tokens * self.hidden_size, generator=g)

    def __call__(self, images):
        assert images.dim() == 4
        return (images.reshape(images.shape[0], -1).float().cpu() @ self.table).reshape(-1, self.tokens, self.hidden_size)


def _predictions(runner, batches, venc):
    out = []
    for b in batches:
        img = b["img_tokens"] if "img_tokens" in b else venc(b["images"].reshape(-1, 3, 4, 4)).reshape(len(b["data_indices"]), -1, venc.hidden_size)
        out.append(runner.predict_action(b["lang_embeds"], b["lang_attn_mask"], img, b["states"][:, -1:, :], b["state_elem_mask"].unsqueeze(1),
                                         b["ctrl_freqs"], x_init=b["x_init"]).float().cpu())
    return out


@pytest.mark.parametrize("images", [False, True], ids=["img_tokens", "images"])
def test_sample_eval_end_to_end(images):
    """Two batches of 3 on RDT_TINY (5 inference steps, x_init given): every value equals the fp64 restatement applied to the runner's own
    predict_action outputs: unrounded under the kernel's bar, rounded under the bar plus the 0.5e-4 of round(., 4); the reference's keys in
    the reference's order; the drop-in `train.sample.log_sample_res` returns the same dict."""
    from vlatouch.rdt_train import sample_eval
    from train.sample import log_sample_res
    cfg = cases.RDT_TINY
    runner, venc = _runner(cfg), _StubVision(cfg)
    batches = [S.collator_batch(cfg, 3, 12, 300 + 10 * j, S.G18_INDICES[j], images=images) for j in range(2)]
    preds = _predictions(runner, batches, venc)
    assert all(bool(torch.isfinite(p).all()) for p in preds) and float((preds[0] - preds[1]).abs().max()) > 0
    want64 = S.log_sample_res_restated(batches, preds, ID2NAME, 2, torch.float64)
    want32 = S.log_sample_res_restated(batches, preds, ID2NAME, 2, torch.float32)
    metrics, raw = sample_eval(runner, batches, num_sample_batches=2, dataset_id2name=ID2NAME, vision_encoder=venc, return_raw=True)
    assert list(metrics) == list(raw) == list(want64)
    assert set(metrics) == {f"{n}{s}" for n in ("agilex", "rh20t", "bridge") for s in S.METRIC_KEYS} | {"overall_avg_sample_mse", "overall_avg_sample_l2err"}
    worst = 0.0
    for k, w in want64.items():
        bar = max(3 * abs(want32[k] - w), 1e-6 * abs(w))
        print(f"[sample_eval {'images' if images else 'img_tokens'}] {k}: {raw[k]:.9g} (fp64 {w:.9g}), error / bar {abs(raw[k] - w) / bar:.3f}, rounded {metrics[k]}")
        worst = max(worst, abs(raw[k] - w) / bar)
        assert abs(raw[k] - w) <= bar, (k, raw[k], w)
        assert abs(metrics[k] - w) <= bar + 0.5e-4, (k, metrics[k], w)
        assert metrics[k] == round(raw[k], 4)
    args = types.SimpleNamespace(num_sample_batches=2, precomp_lang_embed=True)
    assert log_sample_res(None, venc, runner, args, None, torch.float32, ID2NAME, batches, None) == metrics
    _, early = sample_eval(runner, batches[:1], num_sample_batches=2, dataset_id2name=ID2NAME, vision_encoder=venc, return_raw=True)
    e64, e32 = (S.log_sample_res_restated(batches[:1], preds[:1], ID2NAME, 2, dt) for dt in (torch.float64, torch.float32))
    assert list(early) == list(e64) and "bridge_sample_mse" not in early           # the iterable ends early: the overall divisor stays 2
    assert all(abs(early[k] - e64[k]) <= max(3 * abs(e32[k] - e64[k]), 1e-6 * abs(e64[k])) for k in e64)


# ------------------------------------------------------------------------------------------------ the loop
def _state_bits(tr):
    return {n: {k: v.view(torch.int32).clone() for k, v in d.items()} for n, d in (("p", tr.state_dict()), ("ema", tr.ema_state_dict()))}


def test_finetune_evaluates_every_sample_period_and_leaves_training_unchanged():
    """4 optimizer steps with explicit noise / timesteps, sample_period=2: `log` is called at steps 2 and 4 with the reference's keys; losses,
    final weights and averaged weights are bit-equal to the run without evaluation; the metrics move with the weights."""
    from vlatouch.rdt_train import finetune
    cfg = cases.RDT_TINY
    train = [R.batch(cfg, 3, 12, seed=s) for s in (6, 16, 26, 36)]
    sample = [S.collator_batch(cfg, 3, 12, 300 + 10 * j, S.G18_INDICES[j]) for j in range(2)]
    visits = []

    class _Once:                                         # an iterable that counts how often it is started: afresh at each visit
        starts = 0

        def __iter__(self):
            _Once.starts += 1
            return iter(sample)

    plain = _runner(cfg).trainer(lr=1e-3)
    losses_plain = finetune(plain, train, max_train_steps=4)
    tr = _runner(cfg).trainer(lr=1e-3)
    losses = finetune(tr, train, max_train_steps=4, sample_period=2, sample_batches=_Once(), num_sample_batches=2, dataset_id2name=ID2NAME,
                      log=lambda m, step: visits.append((step, m)))
    assert [s for s, _ in visits] == [2, 4] and _Once.starts == 2 and tr.sampler_repacks == 2
    keys = {f"{n}{s}" for n in ("agilex", "rh20t", "bridge") for s in S.METRIC_KEYS} | {"overall_avg_sample_mse", "overall_avg_sample_l2err"}
    for _, m in visits:
        assert set(m) == keys and all(np.isfinite(v) for v in m.values())
    assert visits[0][1] != visits[1][1]
    assert len(losses) == len(losses_plain) == 4 and all(torch.equal(a, b) for a, b in zip(losses, losses_plain))
    sa, sb = _state_bits(tr), _state_bits(plain)
    for part in ("p", "ema"):
        assert all(sa[part][k].equal(sb[part][k]) for k in sb[part]), part
    ema_visits = []
    tr2 = _runner(cfg).trainer(lr=1e-3)
    finetune(tr2, train, max_train_steps=4, sample_period=4, sample_batches=sample, dataset_id2name=ID2NAME, sample_ema=True,
             log=lambda m, step: ema_visits.append((step, m)))
    assert [s for s, _ in ema_visits] == [4] and ema_visits[0][1] != visits[1][1], "sample_ema evaluates the averaged weights"


def test_finetune_with_evaluation_in_bf16_precision():
    from vlatouch.rdt_train import finetune
    cfg = cases.RDT_TINY
    train = [R.round_bf16(R.batch(cfg, 3, 12, seed=s)) for s in (6, 16)]
    sample = [S.collator_batch(cfg, 3, 12, 300 + 10 * j, S.G18_INDICES[j]) for j in range(2)]
    visits = []
    tr = _runner(cfg).trainer(lr=1e-3, precision="bf16")
    losses = finetune(tr, train, max_train_steps=2, sample_period=1, sample_batches=sample, dataset_id2name=ID2NAME, log=lambda m, s: visits.append((s, m)))
    assert [s for s, _ in visits] == [1, 2] and all(np.isfinite(v) for _, m in visits for v in m.values())
    assert all(bool(torch.isfinite(x)) for x in losses)
