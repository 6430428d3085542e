"""vt_attention_bwd_mfma (csrc/vt_attn_bwd.hip) and attention_backward="mfma" of the RDT trainer, on the device.

Kernel level: every case of tests/attn_bwd_mfma_ref.py::KERNEL_CASES on strided views of packed buffers, bf16-rounded inputs, NaN-filled
outputs, run twice and compared bit for bit, against fp64 autograd of the same inputs: per gradient, max-abs error at most 1.5 x that of torch's
bf16 CPU backward (the project's bar for a bf16 attention backward; tests/test_attn_bwd_mfma_host.py shows the kernel's statement holds it).
The row statistics are compared with the wave kernel's.  Masks, another scale, guard words around every workspace, refusals.
Trainer level: the rules of test_gradients_bf16, of the 8-bit optimizer's thirty steps, accumulation, checkpoints across the two settings."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import attn_bwd_mfma_ref as M
from tests import cases
from tests import rdt_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _hip(bufs, views, do, mask, kernel="mfma", scale=None, dtype=BF):
    """-> [dq, dk, dv] on the CPU (views of NaN-filled packed buffers) and the row statistics [B * H * Nq, 3]."""
    from vlatouch.rdt_train import attention_bwd
    dbufs = [b.to(DEV, dtype) for b in bufs]
    gbufs = [torch.full_like(b, float("nan")) for b in dbufs]
    q, k, v = views(*dbufs)
    dq, dk, dv = views(*gbufs)
    km = None if mask is None else mask.to(DEV).to(torch.uint8).contiguous()
    ws = attention_bwd(q, k, v, do.to(DEV, dtype), dq, dk, dv, kmask=km, scale=scale, kernel=kernel)
    torch.cuda.synchronize()
    return [t.float().cpu() for t in (dq, dk, dv)], ws.cpu()


def _check_bar(tag, got, ref, tb):
    for i, name in enumerate(("dq", "dk", "dv")):
        e, et = float((got[i].double() - ref[i]).abs().max()), float((tb[i] - ref[i]).abs().max())
        print(f"[attention_bwd mfma {tag}] {name}: max err {e:.3e}; torch bf16 on the CPU {et:.3e}")
    for i, name in enumerate(("dq", "dk", "dv")):
        e, et = float((got[i].double() - ref[i]).abs().max()), float((tb[i] - ref[i]).abs().max())
        assert e <= 1.5 * et, (tag, name, e, et)


def _check_stats(tag, ws, ws_wave):
    m, mw = ws[:, 0].double(), ws_wave[:, 0].double()
    il, ilw = ws[:, 1].double(), ws_wave[:, 1].double()
    d, dw = ws[:, 2].double(), ws_wave[:, 2].double()
    em = float(((m - mw).abs() / mw.abs().clamp(min=1.0)).max())
    el = float(((il - ilw).abs() / ilw.abs().clamp(min=1e-30)).max())
    ed = float(((d - dw).abs() - 1e-5 * dw.abs() - 1e-6 * float(dw.abs().max())).max())
    print(f"[attention_bwd mfma {tag}] statistics against the wave kernel: m {em:.2e} of max(1, |m|), 1 / l {el:.2e} relative, "
          f"delta worst excess over 1e-5 |delta| + 1e-6 max|delta| {ed:.2e} (max|delta| {float(dw.abs().max()):.3e})")
    assert em <= 1e-6, ("m", em)
    assert bool(((il - ilw).abs() <= 1e-5 * ilw.abs()).all()), ("1 / l", el)
    assert ed <= 0.0, ("delta", ed)


@pytest.mark.parametrize("B,Nq,Nk,H,cross", M.KERNEL_CASES)
def test_kernel_cases(B, Nq, Nk, H, cross):
    bufs, views, do, _ = M.make_case(B, Nq, Nk, H, cross, seed=Nk)
    ref, tb = M.refs((B, Nq, Nk, H, cross, "plain"), bufs, views, do, None)
    got, ws = _hip(bufs, views, do, None)
    again, ws2 = _hip(bufs, views, do, None)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(got[i].view(torch.int32), again[i].view(torch.int32)), f"{name}: two calls differ"
        assert bool(torch.isfinite(got[i]).all()), name
    assert torch.equal(ws.view(torch.int32), ws2.view(torch.int32))
    tag = f"{Nq}x{Nk} H{H}"
    if (Nq, Nk) == (1, 1):                   # P = 1 exactly: dS = 0, dV = dO
        assert float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) == 0.0
        assert torch.equal(got[2], do)
    _check_bar(tag, got, ref, tb)
    _, ws_wave = _hip(bufs, views, do, None, kernel="wave")
    _check_stats(tag, ws, ws_wave)


def _mask(kind, B, Nk):
    mask = torch.ones(B, Nk, dtype=torch.bool)
    if kind == "tail":
        mask[0, Nk - 3:] = False
    elif kind == "holes":
        mask[0, 5:9] = False
        mask[0, 17] = False
        mask[0, 31:34] = False
        mask[1, 40:43] = False
        mask[1, 0] = False
    elif kind == "tile":
        mask[0, 64:128] = False              # the whole second key tile (what there is of it) of a row whose other keys live
    elif kind == "dead":
        mask[1, :] = False
    return mask


@pytest.mark.parametrize("kind", ["tail", "holes", "tile", "dead"])
@pytest.mark.parametrize("B,Nq,Nk,H", [(2, 67, 130, 2), (2, 33, 65, 2)])
def test_masks(B, Nq, Nk, H, kind):
    mask = _mask(kind, B, Nk)
    bufs, views, do, _ = M.make_case(B, Nq, Nk, H, True, seed=Nk)
    ref, tb = M.refs((B, Nq, Nk, H, True, kind), bufs, views, do, mask)
    got, ws = _hip(bufs, views, do, mask)
    again, _ = _hip(bufs, views, do, mask)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(got[i].view(torch.int32), again[i].view(torch.int32)), f"{name}: two calls differ"
        assert bool(torch.isfinite(got[i]).all()), name
    assert bool(torch.isfinite(ws).all())
    dead_keys = ~mask
    assert float(got[1][dead_keys].abs().max()) == 0.0 and float(got[2][dead_keys].abs().max()) == 0.0
    if kind == "dead":
        assert all(float(got[i][1].abs().max()) == 0.0 for i in range(3))
        assert float(ws.view(B, H, Nq, 3)[1].abs().max()) == 0.0
    _check_bar(f"{Nq}x{Nk} H{H} mask={kind}", got, ref, tb)
    _, ws_wave = _hip(bufs, views, do, mask, kernel="wave")
    _check_stats(f"{Nq}x{Nk} H{H} mask={kind}", ws, ws_wave)


def test_scale():
    B, Nq, Nk, H = 2, 67, 130, 2
    bufs, views, do, _ = M.make_case(B, Nq, Nk, H, True, seed=Nk)
    ref, tb = M.refs((B, Nq, Nk, H, True, "scale0.2"), bufs, views, do, None, scale=0.2)
    got, ws = _hip(bufs, views, do, None, scale=0.2)
    _check_bar(f"{Nq}x{Nk} H{H} scale=0.2", got, ref, tb)
    _, ws_wave = _hip(bufs, views, do, None, kernel="wave", scale=0.2)
    _check_stats(f"{Nq}x{Nk} H{H} scale=0.2", ws, ws_wave)


# ------------------------------------------------------------------------------------------------ the C entry, called directly
GUARD = 64            # guard elements on either side


def _direct(B, Nq, Nk, H, *, dtype=BF, q_pad=0, ws2_short=0, seed=3):
    """Calls vt_attention_bwd_mfma on q + packed kv views with NaN-filled outputs; ws2 of exactly the queried size, p->ws and a separately
    allocated dQ, each between guard words.  -> (return code, outputs dict, guards-untouched flag)."""
    from vlatouch import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(seed)
    qb = torch.randn(B, Nq, H * 64 + q_pad, generator=g).to(DEV, dtype)
    kvb = torch.randn(B, Nk, 2 * H * 64, generator=g).to(DEV, dtype)
    do = torch.randn(B, Nq, H, 64, generator=g).to(DEV, dtype)
    q = qb[:, :, :H * 64].view(B, Nq, H, 64) if q_pad == 0 else qb[:, :, :H * 64].unflatten(2, (H, 64))
    k, v = kvb.view(B, Nk, 2, H, 64)[:, :, 0], kvb.view(B, Nk, 2, H, 64)[:, :, 1]
    dkvb = torch.full_like(kvb, float("nan"))
    dk, dv = dkvb.view(B, Nk, 2, H, 64)[:, :, 0], dkvb.view(B, Nk, 2, H, 64)[:, :, 1]
    n_dq = B * Nq * H * 64
    dq_all = torch.full((n_dq + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    dq_all[:GUARD] = 7.0
    dq_all[GUARD + n_dq:] = 7.0
    dq = dq_all[GUARD:GUARD + n_dq].view(B, Nq, H, 64)
    n_ws = B * H * Nq * 3
    ws_all = torch.full((n_ws + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ws_all[:GUARD] = 7.0
    ws_all[GUARD + n_ws:] = 7.0
    need = lib.vt_attention_bwd_mfma_ws_bytes(B, H, Nq, Nk)
    nbytes = max(need, 1024)
    ws2_all = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws2 = ws2_all[256:256 + nbytes]
    p = L.AttnBwdParams()
    for name, t in (("q", q), ("k", k), ("v", v), ("do", do), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert t.stride(3) == 1
        setattr(p, {"q": "Q", "k": "K", "v": "V", "do": "dO", "dq": "dQ", "dk": "dK", "dv": "dV"}[name], t.data_ptr())
        setattr(p, f"{name}_bs", t.stride(0)), setattr(p, f"{name}_rs", t.stride(1)), setattr(p, f"{name}_hs", t.stride(2))
    p.ws = ws_all[GUARD:].data_ptr()
    p.B, p.H, p.Nq, p.Nk, p.hd, p.dtype, p.scale = B, H, Nq, Nk, 64, L.dt_code(dtype), 0.125
    rc = lib.vt_attention_bwd_mfma(C.byref(p), L.ptr(ws2), (need if need > 0 else nbytes) - ws2_short, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    guards_ok = (bool((dq_all[:GUARD] == 7.0).all()) and bool((dq_all[GUARD + n_dq:] == 7.0).all()) and bool((ws_all[:GUARD] == 7.0).all())
                 and bool((ws_all[GUARD + n_ws:] == 7.0).all()) and bool((ws2_all[:256] == 0xA5).all()) and bool((ws2_all[256 + nbytes:] == 0xA5).all()))
    if need > 0:
        assert nbytes == need                 # the guard words start right after the queried size
    return rc, dict(dq=dq, dk=dk, dv=dv, ws=ws_all[GUARD:GUARD + n_ws], err=lib.vt_last_error().decode()), guards_ok


@pytest.mark.parametrize("B,Nq,Nk,H", [(2, 67, 130, 2), (1, 128, 257, 2), (2, 5, 3, 2), (1, 67, 581, 2)])
def test_guard_words_around_every_workspace(B, Nq, Nk, H):
    rc, out, guards_ok = _direct(B, Nq, Nk, H)
    assert rc == 0, out["err"]
    assert guards_ok, "a guard word next to ws2, p->ws or dQ was written"
    assert all(bool(torch.isfinite(out[n].float()).all()) for n in ("dq", "dk", "dv", "ws"))


@pytest.mark.parametrize("what", ["Nq=129", "fp32", "stride", "short ws2"])
def test_refusals_write_nothing(what):
    kw = {"Nq=129": dict(Nq=129), "fp32": dict(dtype=torch.float32), "stride": dict(q_pad=4), "short ws2": dict(ws2_short=4)}[what]
    args = dict(B=2, Nq=67, Nk=130, H=2)
    args.update({k: v for k, v in kw.items() if k == "Nq"})
    rc, out, guards_ok = _direct(args["B"], args["Nq"], args["Nk"], args["H"], **{k: v for k, v in kw.items() if k != "Nq"})
    print(f"[attention_bwd mfma refusal {what}] code {rc}: {out['err']}")
    assert rc in (-22, -95) and "vt_attention_bwd_mfma" in out["err"]
    assert guards_ok
    assert all(bool(torch.isnan(out[n].float()).all()) for n in ("dq", "dk", "dv", "ws")), "a refused call wrote an output"


def test_python_refuses_fp32_and_unknown_kernels():
    from vlatouch.rdt_train import attention_bwd
    t = lambda n: torch.zeros(1, n, 1, 64, device=DEV)
    out = [torch.full((1, 4, 1, 64), float("nan"), device=DEV) for _ in range(3)]
    with pytest.raises(ValueError, match="bf16"):
        attention_bwd(t(4), t(4), t(4), t(4), *out, kernel="mfma")
    with pytest.raises(ValueError, match="kernel"):
        attention_bwd(t(4), t(4), t(4), t(4), *out, kernel="tile")
    big = lambda: torch.zeros(1, 129, 1, 64, device=DEV, dtype=BF)
    with pytest.raises(ValueError, match="Nq"):
        attention_bwd(big(), big(), big(), big(), big(), big(), big(), kernel="mfma")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in out)


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(cfg, sd, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], device=DEV, **kw)


def _get_loss(tr, b, **kw):
    return tr.get_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                       noise=b["noise"], timesteps=b["timesteps"], **kw)


def _step(tr, b):
    return tr.train_step(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                         noise=b["noise"], timesteps=b["timesteps"])


def _gradient_rule(tag, grads, g64, gref, sd):
    """test_gradients_bf16's rule -> (summary, bad tensors, total error, the oracle's total error)."""
    tot_h = tot_r = 0.0
    n_h = n_r = 0
    rel_h, rel_r, bad = [], [], []
    for k in sd:
        gn = float(g64[k].norm())
        eh, er = float((grads[k].double() - g64[k]).norm()), float((gref[k] - g64[k]).norm())
        tot_h, tot_r = tot_h + eh * eh, tot_r + er * er
        rel_h.append(eh / gn), rel_r.append(er / gn)
        n_h, n_r = n_h + (eh > 1e-2 * gn), n_r + (er > 1e-2 * gn)
        if not eh <= max(1.5 * er, 1e-2 * gn):
            bad.append((k, eh / gn, er / gn))
    tot_h, tot_r, gall = tot_h ** 0.5, tot_r ** 0.5, sum(float(v.norm()) ** 2 for v in g64.values()) ** 0.5
    line = (f"[rdt_train bf16 {tag}] per-tensor error / norm: HIP median {np.median(rel_h):.2e} worst {max(rel_h):.2e}, oracle bf16 median "
            f"{np.median(rel_r):.2e} worst {max(rel_r):.2e}; all parameters: HIP {tot_h / gall:.2e}, oracle {tot_r / gall:.2e}; above 1e-2: HIP {n_h}, "
            f"oracle {n_r} of {len(sd)}")
    return line, bad, tot_h, tot_r


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_trainer_gradients_bf16(name):
    """The rule of tests/test_gpu_rdt_train.py::test_gradients_bf16 with attention_backward="mfma": per tensor e <= max(1.5 e_ref, 1e-2 |g|), all
    parameters together e <= 1.5 e_ref (e_ref: the oracle in bf16 on the CPU, both against fp64 from the same bf16-rounded weights and inputs)."""
    cfg, B, Ll = (cases.RDT_TINY, 3, 12) if name == "tiny" else (cases.RDT_WIDE, 2, 20)
    sd, b = R.round_bf16(cases.rdt_sd(cfg)), R.round_bf16(R.batch(cfg, B, Ll))
    l64, g64 = R.loss_and_grads(sd, b, cfg)
    lref, gref = R.loss_and_grads(sd, b, cfg, dtype=torch.bfloat16)
    res = {}
    for kind in ("mfma", "wave"):
        tr = _trainer(cfg, sd, precision="bf16", attention_backward=kind)
        loss = float(_get_loss(tr, b))
        grads = tr.grads()
        assert set(grads) == set(sd) and all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in grads.values())
        res[kind] = _gradient_rule(f"{name} {kind}", grads, g64, gref, sd)
        print(f"loss {loss:.4f} (oracle bf16 {lref:.4f}, fp64 {l64:.4f}) " + res[kind][0])
    _, bad, tot_h, tot_r = res["mfma"]
    assert not bad, bad[:8]
    assert tot_h <= 1.5 * tot_r, (tot_h, tot_r)


def test_trainer_thirty_steps_follow_the_wave_kernel():
    """Thirty steps on one batch: last / first loss under "mfma" at most 1.5 x that of the "wave" bf16 trainer (the 8-bit optimizer test's margin)."""
    cfg = cases.RDT_TINY
    sd, b = cases.rdt_sd(cfg), R.batch(cfg, 3, 12)
    frac = {}
    for kind in ("mfma", "wave"):
        tr = _trainer(cfg, sd, lr=1e-3, precision="bf16", attention_backward=kind)
        losses = [_step(tr, b) for _ in range(30)]
        frac[kind] = float(losses[-1]) / float(losses[0])
    print(f"[rdt_train mfma 30 steps] last / first loss: mfma {frac['mfma']:.4f}, wave {frac['wave']:.4f}")
    assert np.isfinite(frac["mfma"]) and frac["wave"] < 1.0
    assert frac["mfma"] <= 1.5 * frac["wave"], frac


def test_trainer_accumulation_k4():
    """gradient_accumulation_steps=4 under "mfma": four micro-batches, one optimizer step; the accumulated gradient holds the per-tensor rule of
    tests/test_gpu_rdt_accum.py::test_accumulated_gradients_bf16."""
    from tests import rdt_accum_ref as A
    cfg = cases.RDT_TINY
    sd = R.round_bf16(cases.rdt_sd(cfg))
    batches = [R.round_bf16(R.batch(cfg, 3, 12, seed=s)) for s in A.G17_SEEDS[:4]]
    _, g64 = A.accumulated_grads(sd, batches, cfg)
    _, gref = A.accumulated_grads(sd, batches, cfg, dtype=torch.bfloat16)
    tr = _trainer(cfg, sd, precision="bf16", gradient_accumulation_steps=4, attention_backward="mfma")
    for b in batches:
        _get_loss(tr, b)
        tr.accumulate()
    line, bad, _, _ = _gradient_rule("tiny mfma k=4", tr.grads(), g64, gref, sd)
    print(line)
    assert not bad, bad[:8]
    tr2 = _trainer(cfg, sd, lr=1e-3, precision="bf16", gradient_accumulation_steps=4, attention_backward="mfma")
    for n, b in enumerate(batches):
        loss = _step(tr2, b)
        assert np.isfinite(float(loss)) and tr2.sync_gradients == (n == 3)
    assert tr2.global_step == 1 and np.isfinite(float(tr2.grad_norm))


def _state(tr):
    c = lambda d: {key: v.detach().cpu().clone() for key, v in d.items()}
    return dict(p=c(tr.p), m=c(tr._m), v=c(tr._v), shadow=c(tr.shadow))


def _assert_same_state(a, b):
    for part in ("p", "m", "v", "shadow"):
        assert set(a[part]) == set(b[part]) and a[part], part
        for key in a[part]:
            assert a[part][key].view(torch.int32).equal(b[part][key].view(torch.int32)), (part, key)


def test_checkpoints_cross_the_two_settings(tmp_path):
    """A checkpoint saved under "wave" resumes under "mfma" and back; trainer_state.json does not record the setting."""
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in (6, 16, 26, 36)]
    kw = dict(lr=1e-3, precision="bf16")
    wave = _trainer(cfg, sd, attention_backward="wave", **kw)
    for b in batches[:2]:
        _step(wave, b)
    ck_w = str(tmp_path / "wave-2")
    wave.save_checkpoint(ck_w)
    mfma = _trainer(cfg, sd, attention_backward="mfma", **kw)
    mfma.load_checkpoint(ck_w)
    assert (mfma.step_count, mfma.ema_updates, mfma.micro_step) == (2, 2, 0) and mfma.attention_backward == "mfma"
    _assert_same_state(_state(wave), _state(mfma))
    ck_m0 = str(tmp_path / "mfma-2")
    mfma.save_checkpoint(ck_m0)
    with open(os.path.join(ck_w, "trainer_state.json"), "rb") as f, open(os.path.join(ck_m0, "trainer_state.json"), "rb") as g:
        jw, jm = f.read(), g.read()
    assert jw == jm and "attention_backward" not in json.loads(jw) and b"mfma" not in jm
    assert sorted(os.listdir(os.path.join(ck_w, "checkpoint"))) == sorted(os.listdir(os.path.join(ck_m0, "checkpoint")))
    assert np.isfinite(float(_step(mfma, batches[2]))) and mfma.global_step == 3
    ck_m = str(tmp_path / "mfma-3")
    mfma.save_checkpoint(ck_m)
    back = _trainer(cfg, sd, attention_backward="wave", **kw)
    back.load_checkpoint(ck_m)
    _assert_same_state(_state(mfma), _state(back))
    assert np.isfinite(float(_step(back, batches[3]))) and back.global_step == 4


def test_constructor_refusals_and_the_runner():
    from tests.test_gpu_rdt_train import _runner
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    with pytest.raises(ValueError, match="bf16"):
        _trainer(cfg, sd, precision="fp32", attention_backward="mfma")
    with pytest.raises(ValueError, match="attention_backward"):
        _trainer(cfg, sd, precision="bf16", attention_backward="tile")
    long_cfg = dict(cfg, horizon=126)        # 129 query rows
    with pytest.raises(ValueError, match="128"):
        _trainer(long_cfg, cases.rdt_sd(long_cfg), precision="bf16", attention_backward="mfma")
    assert _trainer(cfg, sd, precision="bf16").attention_backward == "wave"
    r = _runner(cfg)
    tr = r.trainer(precision="bf16", attention_backward="mfma")
    assert tr.attention_backward == "mfma" and r.trainer().attention_backward == "wave"
    b = R.batch(cfg, 3, 12)
    assert np.isfinite(float(_get_loss(tr, b)))
