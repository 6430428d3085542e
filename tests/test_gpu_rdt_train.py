"""RDT fine-tuning step on the device (vlatouch/rdt_train.py, csrc/vt_train_rdt.hip) against torch fp64 autograd on the CPU.

Kernel level: every new backward kernel against fp64 autograd of the same function (bars: 1e-5 of the gradient's max-abs for the attention and
norm kernels in fp32, 2e-6 absolute for the activations, 1.5 x the error of torch's own bf16 CPU backward for bf16 operands), each called
twice and compared bit for bit.  Trainer level: loss 1e-5 relative and every tensor's gradient within 1e-4 of its norm against autograd
through the oracle (tests/rdt_train_ref.py), three clipped AdamW + EMA steps against the same loop in fp64 torch with the bar taken from what
fp32 torch loses against it, and the RDTRunner surface."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases
from tests import rdt_train_ref as R
from oracle import rdt as orr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sdpa_ref(q, k, v, mask):
    """q [B,Nq,H,64], k / v [B,Nk,H,64], mask [B,Nk] bool or None -> o [B,Nq,H,64]; a batch element whose keys are all masked gives zeros."""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * 0.125
    if mask is not None:
        dead = ~mask.any(dim=1)
        m = mask.clone()
        m[dead] = True                                   # keep the softmax finite there; its output is zeroed below, so its gradients are 0
        s = s.masked_fill(~m[:, None, None, :], float("-inf"))
    o = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), v)
    if mask is not None:
        o = o * (~dead)[:, None, None, None].to(o.dtype)
    return o


def _attn_case(B, Nq, Nk, H, masked, cross, seed):
    g = torch.Generator().manual_seed(seed)
    if cross:
        qb, kvb = torch.randn(B, Nq, H * 64, generator=g), torch.randn(B, Nk, 2 * H * 64, generator=g)
        views = lambda qb, kvb: (qb.view(B, Nq, H, 64), kvb.view(B, Nk, 2, H, 64)[:, :, 0], kvb.view(B, Nk, 2, H, 64)[:, :, 1])
        bufs = (qb, kvb)
    else:
        qkv = torch.randn(B, Nq, 3 * H * 64, generator=g)
        views = lambda qkv: tuple(qkv.view(B, Nq, 3, H, 64)[:, :, i] for i in range(3))
        bufs = (qkv,)
    do = torch.randn(B, Nq, H, 64, generator=g)
    mask = None
    if masked:
        mask = torch.ones(B, Nk, dtype=torch.bool)
        mask[0, Nk - 3:] = False
        mask[1, :] = False
    return bufs, views, do, mask


def _attn_ref(bufs, views, do, mask, dtype):
    with torch.enable_grad():                      # other test modules switch autograd off process-wide
        return _attn_ref_(bufs, views, do, mask, dtype)


def _attn_ref_(bufs, views, do, mask, dtype):
    leaves = [b.to(dtype).clone().requires_grad_(True) for b in bufs]
    q, k, v = views(*leaves)
    if dtype == torch.bfloat16:       # torch's own bf16 backward on the CPU: matmuls and softmax in bf16, as the reference's execution dtype does
        s = (q.permute(0, 2, 1, 3) @ k.permute(0, 2, 3, 1)) * 0.125
        if mask is not None:
            dead = ~mask.any(dim=1)
            m = mask.clone()
            m[dead] = True
            s = s.masked_fill(~m[:, None, None, :], float("-inf"))
        o = (torch.softmax(s, dim=-1) @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
        if mask is not None:
            o = o * (~dead)[:, None, None, None].to(o.dtype)
    else:
        o = _sdpa_ref(q, k, v, mask)
    (o * do.to(dtype)).sum().backward()
    return [views(*[l.grad for l in leaves])[i].double() for i in range(3)]


def _attn_hip(bufs, views, do, mask, dtype):
    from vlatouch.rdt_train import attention_bwd
    dbufs = [b.to(DEV, dtype) for b in bufs]
    gbufs = [torch.full_like(b, float("nan")) for b in dbufs]
    q, k, v = views(*dbufs)
    dq, dk, dv = views(*gbufs)
    km = None if mask is None else mask.to(DEV).to(torch.uint8).contiguous()
    attention_bwd(q, k, v, do.to(DEV, dtype), dq, dk, dv, kmask=km)
    torch.cuda.synchronize()
    return [t.cpu() for t in (dq, dk, dv)]


ATTN_CASES = [(2, 11, 11, 4, False, False), (2, 67, 67, 32, False, False), (2, 67, 20, 32, True, True), (2, 67, 4374, 4, False, True)]


@pytest.mark.parametrize("B,Nq,Nk,H,masked,cross", ATTN_CASES)
def test_attention_bwd_fp32(B, Nq, Nk, H, masked, cross):
    """Bar 1e-5 of each gradient's max-abs, the 4374-key case included (measured: <= 4.5e-7 at up to 67 keys, 2.9e-6 at 4374, where fp32 torch
    on the CPU, printed beside it, has 5e-7)."""
    bufs, views, do, mask = _attn_case(B, Nq, Nk, H, masked, cross, seed=Nk)
    ref = _attn_ref(bufs, views, do, mask, torch.float64)
    got = _attn_hip(bufs, views, do, mask, torch.float32)
    again = _attn_hip(bufs, views, do, mask, torch.float32)
    t32 = _attn_ref(bufs, views, do, mask, torch.float32) if Nk > 4000 else None
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(got[i], again[i]), f"{name}: two calls differ"
        scale = float(ref[i].abs().max())
        e = float((got[i].double() - ref[i]).abs().max())
        bar = 1e-5 * scale
        msg = f"[attention_bwd fp32 {Nq}x{Nk} H{H}] {name}: max err {e:.3e} = {e / scale:.2e} of max-abs {scale:.3e}"
        if t32 is not None:
            msg += f"; fp32 torch on the CPU: {float((t32[i] - ref[i]).abs().max()):.3e}"
        print(msg)
        assert e <= bar, msg
    if masked:
        assert float(got[0][1].abs().max()) == 0.0 and float(got[1][1].abs().max()) == 0.0 and float(got[2][1].abs().max()) == 0.0
        assert float(got[1][0, Nk - 3:].abs().max()) == 0.0 and float(got[2][0, Nk - 3:].abs().max()) == 0.0


@pytest.mark.parametrize("B,Nq,Nk,H,masked,cross", ATTN_CASES)
def test_attention_bwd_bf16(B, Nq, Nk, H, masked, cross):
    """bf16 operands (fp32 accumulation, bf16 results) against fp64 autograd from the same bf16-rounded operands: at most 1.5 x the error of
    torch's bf16 CPU backward."""
    bufs, views, do, mask = _attn_case(B, Nq, Nk, H, masked, cross, seed=Nk)
    bufs, do = tuple(b.bfloat16().float() for b in bufs), do.bfloat16().float()
    ref = _attn_ref(bufs, views, do, mask, torch.float64)
    tb = _attn_ref(bufs, views, do, mask, torch.bfloat16)
    got = _attn_hip(bufs, views, do, mask, torch.bfloat16)
    again = _attn_hip(bufs, views, do, mask, torch.bfloat16)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(got[i], again[i]), f"{name}: two calls differ"
        e, et = float((got[i].double() - ref[i]).abs().max()), float((tb[i] - ref[i]).abs().max())
        print(f"[attention_bwd bf16 {Nq}x{Nk} H{H}] {name}: max err {e:.3e}; torch bf16 on the CPU {et:.3e}")
        assert e <= 1.5 * et, (name, e, et)


@pytest.mark.parametrize("mode", ["meansq", "var"])
@pytest.mark.parametrize("D", [256, 2048])
def test_rmsnorm_bwd(mode, D):
    from vlatouch import _lib as L
    from vlatouch.rdt_train import rmsnorm_bwd
    g = torch.Generator().manual_seed(D)
    x, w, dy = torch.randn(37, D, generator=g) * 1.7 + 0.3, 1 + 0.2 * torch.randn(D, generator=g), torch.randn(37, D, generator=g)
    xl, wl = x.double().requires_grad_(True), w.double().requires_grad_(True)
    with torch.enable_grad():
        (orr.rms_norm(xl, wl, 1e-6, mode) * dy.double()).sum().backward()
    code = L.NORM_RMS_MEANSQ if mode == "meansq" else L.NORM_RMS_VAR
    outs = [rmsnorm_bwd(x.to(DEV), w.to(DEV), dy.to(DEV), 1e-6, code) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for name, got, ref in (("dx", outs[0][0], xl.grad), ("dw", outs[0][1], wl.grad)):
        e, scale = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
        print(f"[rmsnorm_bwd {mode} D{D}] {name}: {e / scale:.2e} of max-abs")
        assert e <= 1e-5 * scale, (name, e, scale)


@pytest.mark.parametrize("mode", ["meansq", "var"])
def test_headnorm_bwd(mode):
    from vlatouch import _lib as L
    from vlatouch.rdt_train import headnorm_bwd_
    H, D, M = 4, 256, 33
    g = torch.Generator().manual_seed(5)
    buf, w, dbuf = torch.randn(M, 3 * D, generator=g) * 1.3 + 0.2, 1 + 0.2 * torch.randn(64, generator=g), torch.randn(M, 3 * D, generator=g)
    xl, wl = buf[:, D:2 * D].double().clone().requires_grad_(True), w.double().requires_grad_(True)           # the k slice of a packed qkv buffer
    with torch.enable_grad():
        (orr.rms_norm(xl.view(M, H, 64), wl, 1e-6, mode).reshape(M, D) * dbuf[:, D:2 * D].double()).sum().backward()
    code = L.NORM_RMS_MEANSQ if mode == "meansq" else L.NORM_RMS_VAR
    res = []
    for _ in range(2):
        xb, db = buf.to(DEV), dbuf.to(DEV)
        dw = headnorm_bwd_(xb[:, D:2 * D], db[:, D:2 * D], H, w.to(DEV), 1e-6, code)
        res.append((db.cpu(), dw.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0][:, :D], dbuf[:, :D]) and torch.equal(res[0][0][:, 2 * D:], dbuf[:, 2 * D:])       # the q and v slices are untouched
    for name, got, ref in (("dx", res[0][0][:, D:2 * D], xl.grad), ("dw", res[0][1], wl.grad)):
        e, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
        print(f"[headnorm_bwd {mode}] {name}: {e / scale:.2e} of max-abs")
        assert e <= 1e-5 * scale, (name, e, scale)


@pytest.mark.parametrize("kind", ["gelu_tanh", "silu"])
def test_activation_and_derivative(kind):
    from vlatouch import _lib as L
    from vlatouch.rdt_train import act
    x = torch.linspace(-9, 9, 20001)
    xl = x.double().requires_grad_(True)
    with torch.enable_grad():
        y = F.gelu(xl, approximate="tanh") if kind == "gelu_tanh" else F.silu(xl)
        y.sum().backward()
    code = L.ACT_GELU_TANH if kind == "gelu_tanh" else L.ACT_SILU
    xd = x.to(DEV)
    f1, d1 = act(xd, code), act(xd, code, torch.ones_like(xd))
    assert torch.equal(f1, act(xd, code)) and torch.equal(d1, act(xd, code, torch.ones_like(xd)))
    ef, ed = float((f1.cpu().double() - y.detach()).abs().max()), float((d1.cpu().double() - xl.grad).abs().max())
    print(f"[{kind}] forward {ef:.2e}, derivative {ed:.2e} (absolute)")
    assert ef <= 2e-6 and ed <= 2e-6, (ef, ed)


def test_ddpm_qsample_layout():
    from vlatouch.rdt_train import ddpm_qsample, alphas_cumprod
    B, H, A = 3, 8, 128
    b = R.batch(cases.RDT_TINY, B, 12)
    ab = alphas_cumprod(1000, "squaredcos_cap_v2")
    assert torch.equal(ab, R.alphas_cumprod())
    out = ddpm_qsample(b["state_tokens"].to(DEV), b["action_gt"].to(DEV), b["noise"].to(DEV), b["action_mask"].to(DEV), b["timesteps"].to(DEV),
                       ab.to(DEV)).cpu()
    again = ddpm_qsample(b["state_tokens"].to(DEV), b["action_gt"].to(DEV), b["noise"].to(DEV), b["action_mask"].to(DEV), b["timesteps"].to(DEV),
                         ab.to(DEV)).cpu()
    assert out.shape == (B, H + 1, 2 * A) and torch.equal(out, again)
    assert torch.equal(out[:, :1, :A], b["state_tokens"]) and torch.equal(out[:, :, A:], b["action_mask"].expand(-1, H + 1, -1))
    a = ab[b["timesteps"]].double()[:, None, None]
    want = a.sqrt() * b["action_gt"].double() + (1 - a).sqrt() * b["noise"].double()
    assert float((out[:, 1:, :A].double() - want).abs().max()) <= 1e-6


def test_small_kernels_twice_and_against_torch():
    """vt_timestep_embed, vt_transpose_pad, vt_mse_loss and the typed column sum / add / column copy as units: each twice, bit-equal, and against torch."""
    from vlatouch.rdt_train import timestep_embed, timestep_freqs, transpose_pad, mse_loss, colsum, add_, copy_cols
    g = torch.Generator().manual_seed(3)
    t = torch.tensor([3.0, 437.0, 998.0])
    fr = timestep_freqs(256)
    e1, e2 = timestep_embed(t.to(DEV), fr.to(DEV)).cpu(), timestep_embed(t.to(DEV), fr.to(DEV)).cpu()
    assert torch.equal(e1, e2) and float((e1.double() - orr.timestep_embedding(t, 256, torch.float32).double()).abs().max()) <= 2e-6
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(33, 40, generator=g).to(dt)
        a, b = transpose_pad(x.to(DEV)).cpu(), transpose_pad(x.to(DEV)).cpu()
        pad = 36 if dt == torch.float32 else 40
        assert torch.equal(a, b) and a.shape == (40, pad) and torch.equal(a[:, :33], x.t()) and float(a[:, 33:].abs().sum()) == 0.0
        c1, c2 = colsum(x.to(DEV)).cpu(), colsum(x.to(DEV)).cpu()
        assert torch.equal(c1, c2) and float((c1.double() - x.double().sum(0)).abs().max()) <= 1e-5
        y = torch.randn(33, 40, generator=g).to(dt)
        s1, s2 = add_(x.to(DEV).clone(), y.to(DEV)).cpu(), add_(x.to(DEV).clone(), y.to(DEV)).cpu()
        assert torch.equal(s1, s2) and torch.equal(s1, (x.float() + y.float()).to(dt))
        d = torch.zeros(33, 64, dtype=dt, device=DEV)
        copy_cols(x.to(DEV), 8, d, 16, 24)
        assert torch.equal(d.cpu()[:, 16:40], x[:, 8:32]) and float(d.cpu()[:, :16].abs().sum()) == 0.0 and float(d.cpu()[:, 40:].abs().sum()) == 0.0
        tgt = torch.randn(33, 40, generator=g)
        (l1, d1), (l2, d2) = mse_loss(x.to(DEV), tgt.to(DEV)), mse_loss(x.to(DEV), tgt.to(DEV))
        assert torch.equal(l1, l2) and torch.equal(d1, d2)
        want = ((x.double() - tgt.double()) ** 2).mean()
        assert abs(float(l1) - float(want)) <= 1e-6 * float(want)
        assert float((d1.cpu().double() - 2 * (x.double() - tgt.double()) / x.numel()).abs().max()) <= (1e-9 if dt == torch.float32 else 2e-5)


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(cfg, sd, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], device=DEV, **kw)


def _get_loss(tr, b, **kw):
    return tr.get_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                       noise=b["noise"], timesteps=b["timesteps"], **kw)


@pytest.mark.parametrize("prediction_type", ["sample", "epsilon"])
@pytest.mark.parametrize("rms_mode", ["meansq", "var"])
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_loss_and_gradients_fp32(name, rms_mode, prediction_type):
    cfg, B, Ll = (cases.RDT_TINY, 3, 12) if name == "tiny" else (cases.RDT_WIDE, 2, 20)
    sd, b = cases.rdt_sd(cfg), R.batch(cfg, B, Ll)
    ref_loss, ref_g = R.loss_and_grads(sd, b, cfg, rms_mode=rms_mode, prediction_type=prediction_type)
    tr = _trainer(cfg, sd, rms_mode=rms_mode, prediction_type=prediction_type)
    loss = float(_get_loss(tr, b))
    grads = tr.grads()
    assert set(grads) == set(ref_g) == set(sd)
    worst, wk = 0.0, None
    for k in sd:
        e = R.rel_err(grads[k], ref_g[k])
        if e > worst:
            worst, wk = e, k
    print(f"[rdt_train {name} {rms_mode} {prediction_type}] loss {loss:.7f} vs {ref_loss:.7f}; worst gradient {worst:.2e} of its norm ({wk}), {len(sd)} tensors")
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert worst <= 1e-4, (wk, worst)


def _sdpa_zero_for_empty_rows(q, k, v, mask=None):
    """oracle.rdt._sdpa with the softmax of a row whose keys are all masked set to 0 (torch has NaN there): what vt_attention writes."""
    dt = q.dtype
    s = (q.float() @ k.float().transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    return (torch.softmax(s, dim=-1).nan_to_num(0.0) @ v.float()).to(dt)


def test_loss_and_gradients_fp32_with_an_empty_instruction(monkeypatch):
    """One sample's lang_attn_mask all False: its language cross-attention rows are zeros in the forward (vt_attention) and carry zero gradients
    in the backward (vt_attention_bwd), so the loss and every gradient stay finite and meet the bars of test_loss_and_gradients_fp32."""
    cfg, B, Ll = cases.RDT_TINY, 3, 12
    sd, b = cases.rdt_sd(cfg), R.batch(cfg, B, Ll)
    b["lang_attn_mask"] = b["lang_attn_mask"].clone()
    b["lang_attn_mask"][1] = False
    assert bool(b["lang_attn_mask"][0].any()) and bool(b["lang_attn_mask"][2].any())
    monkeypatch.setattr(orr, "_sdpa", _sdpa_zero_for_empty_rows)
    ref_loss, ref_g = R.loss_and_grads(sd, b, cfg)
    assert np.isfinite(ref_loss) and all(bool(torch.isfinite(g).all()) for g in ref_g.values())
    tr = _trainer(cfg, sd)
    loss = float(_get_loss(tr, b))
    grads = tr.grads()
    assert set(grads) == set(ref_g) == set(sd)
    assert np.isfinite(loss), loss
    bad = [k for k in sd if not bool(torch.isfinite(grads[k]).all())]
    assert not bad, bad[:8]
    worst, wk = 0.0, None
    for k in sd:
        e = R.rel_err(grads[k], ref_g[k])
        if e > worst:
            worst, wk = e, k
    print(f"[rdt_train tiny, sample 1 without instruction] loss {loss:.7f} vs {ref_loss:.7f}; worst gradient {worst:.2e} of its norm ({wk}), {len(sd)} tensors")
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert worst <= 1e-4, (wk, worst)


@pytest.mark.parametrize("prediction_type", ["sample", "epsilon"])
@pytest.mark.parametrize("rms_mode", ["meansq", "var"])
def test_loss_and_gradients_against_the_references_own_run(rms_mode, prediction_type):
    """RDT_TINY against g16 directly (the reference's own compute_loss + backward in fp32, tools/make_golden_rdt_train.py): loss 1e-5 relative,
    every tensor's gradient summary within 1e-4 of the tensor's norm, the norm before clipping 1e-5."""
    SEEDS, B, LANG_LEN, HP, MAX_GRAD_NORM = R.G16_SEEDS, R.G16_B, R.G16_LANG_LEN, R.G16_HP, R.G16_MAX_GRAD_NORM
    g = np.load(f"{cases.GOLDEN}/g16_rdt_train.npz")
    names = [str(n) for n in g["names"]]
    cfg, tag = cases.RDT_TINY, f"{rms_mode}_{prediction_type}"
    b = R.batch(cfg, B, LANG_LEN, seed=SEEDS[0])
    tr = _trainer(cfg, cases.rdt_sd(cfg), rms_mode=rms_mode, prediction_type=prediction_type, lr=HP["lr"], weight_decay=HP["weight_decay"],
                  max_grad_norm=MAX_GRAD_NORM)
    loss = float(_get_loss(tr, b))
    grads = tr.grads()
    assert set(grads) == set(names)
    worst, wk = R.worst_summary(g[f"{tag}_s1_grad"], names, grads)
    tr.optimizer_step()
    want_loss, want_norm, _ = g[f"{tag}_s1_scalars"]
    print(f"[rdt_train vs g16 {tag}] loss {loss:.7f} vs {want_loss:.7f}, norm {float(tr.grad_norm):.5f} vs {want_norm:.5f}, worst gradient summary {worst:.2e} ({wk})")
    assert abs(loss - want_loss) <= 1e-5 * want_loss and abs(float(tr.grad_norm) - want_norm) <= 1e-5 * want_norm
    assert worst <= 1e-4, (wk, worst)


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_gradients_bf16(name):
    """precision="bf16": per-tensor gradient error against fp64 autograd (from the same bf16-rounded weights and inputs), next to the error of the
    oracle run in bf16 on the CPU (the reference's execution dtype): e_hip <= max(1.5 e_ref, 1e-2 |g|) for every tensor, and over all parameters
    together e_hip <= 1.5 e_ref.  Prints how many tensors sit above 1e-2 of their norm for the oracle and for the HIP run."""
    cfg, B, Ll = (cases.RDT_TINY, 3, 12) if name == "tiny" else (cases.RDT_WIDE, 2, 20)
    sd, b = R.round_bf16(cases.rdt_sd(cfg)), R.round_bf16(R.batch(cfg, B, Ll))
    l64, g64 = R.loss_and_grads(sd, b, cfg)
    lref, gref = R.loss_and_grads(sd, b, cfg, dtype=torch.bfloat16)
    tr = _trainer(cfg, sd, precision="bf16")
    loss = float(_get_loss(tr, b))
    grads = tr.grads()
    assert set(grads) == set(sd) and all(v.dtype == torch.float32 for v in grads.values())
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
    print(f"[rdt_train bf16 {name}] loss {loss:.4f} (oracle bf16 {lref:.4f}, fp64 {l64:.4f}); per-tensor error / norm: HIP median {np.median(rel_h):.2e} worst "
          f"{max(rel_h):.2e}, oracle bf16 median {np.median(rel_r):.2e} worst {max(rel_r):.2e}; all parameters: HIP {tot_h / gall:.2e}, oracle {tot_r / gall:.2e}; "
          f"above 1e-2: HIP {n_h}, oracle {n_r} of {len(sd)}")
    assert not bad, bad[:8]
    assert tot_h <= 1.5 * tot_r, (tot_h, tot_r)


def _step_batches(cfg, B, Ll):
    return [R.batch(cfg, B, Ll, seed=s) for s in (6, 16, 26)]


def test_three_clipped_adamw_ema_steps():
    """The update p_k - p_0 and the EMA's ema_k - p_0 per tensor, relative to the fp64 torch run's update norm.  Bar: the worst tensor of the HIP
    run at most 5 x the worst tensor of the same three steps in fp32 torch on the CPU against fp64 torch (Adam's division by sqrt(v) amplifies
    gradient rounding where the gradient is near zero; another summation order has the same kind of rounding)."""
    cfg, B, Ll = cases.RDT_TINY, 3, 12
    sd, batches = cases.rdt_sd(cfg), _step_batches(cfg, B, Ll)
    hp = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    r64 = R.train_steps(sd, batches, cfg, dtype=torch.float64, **hp)
    r32 = R.train_steps(sd, batches, cfg, dtype=torch.float32, **hp)
    p0 = {k: v.double() for k, v in sd.items()}

    def worst(params, ref):
        w, wk = 0.0, None
        for k in sd:
            e = R.rel_err(params[k].double() - p0[k], ref[k] - p0[k])
            if e > w:
                w, wk = e, k
        return w, wk

    trs = [_trainer(cfg, sd, **hp) for _ in range(2)]
    for n, b in enumerate(batches):
        losses = [float(tr.train_step(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"],
                                      b["ctrl_freqs"], noise=b["noise"], timesteps=b["timesteps"])) for tr in trs]
        tr = trs[0]
        norm = float(tr.grad_norm)
        (wp, kp), (we, ke) = worst(tr.state_dict(), r64[n]["params"]), worst(tr.ema_state_dict(), r64[n]["ema"])
        (bp, _), (be, _) = worst(r32[n]["params"], r64[n]["params"]), worst(r32[n]["ema"], r64[n]["ema"])
        print(f"[rdt_train step {n + 1}] loss {losses[0]:.6f} (fp64 {r64[n]['loss']:.6f}), grad norm {norm:.5f} (fp64 {r64[n]['grad_norm']:.5f}); worst update "
              f"error HIP {wp:.2e} ({kp}) / fp32 torch {bp:.2e}; EMA HIP {we:.2e} ({ke}) / fp32 torch {be:.2e}")
        assert abs(losses[0] - r64[n]["loss"]) <= 1e-5 * r64[n]["loss"], "loss"
        assert abs(norm - r64[n]["grad_norm"]) <= 1e-5 * r64[n]["grad_norm"], "clipped norm"
        assert n > 0 or r64[n]["grad_norm"] > 1.0, "the clip must be active in this test"
        assert wp <= 5 * bp and we <= 5 * be, (wp, bp, we, be)
    a, b2 = trs[0].state_dict(), trs[1].state_dict()
    ea, eb = trs[0].ema_state_dict(), trs[1].ema_state_dict()
    assert all(torch.equal(a[k], b2[k]) and torch.equal(ea[k], eb[k]) for k in a), "two trainers from the same weights must agree bit for bit"


# ------------------------------------------------------------------------------------------------ the RDTRunner surface
def _runner(cfg, prediction_type="sample", rms_mode="meansq"):
    from models.rdt_runner import RDTRunner
    config = {"rdt": {"hidden_size": cfg["hidden"], "depth": cfg["depth"], "num_heads": cfg["heads"]}, "lang_adaptor": "mlp2x_gelu",
              "img_adaptor": "mlp2x_gelu", "state_adaptor": "mlp3x_gelu",
              "noise_scheduler": {"num_train_timesteps": 1000, "num_inference_timesteps": 5, "prediction_type": prediction_type,
                                  "beta_schedule": "squaredcos_cap_v2"}}
    r = RDTRunner(action_dim=cfg["action_dim"], pred_horizon=cfg["horizon"], config=config, lang_token_dim=cfg["lang_token_dim"],
                  img_token_dim=cfg["img_token_dim"], state_token_dim=cfg["state_token_dim"], max_lang_cond_len=cfg["max_lang_cond_len"],
                  img_cond_len=cfg["img_cond_len"], dtype=torch.float32, device=DEV, rms_mode=rms_mode)
    r.load_state_dict(cases.rdt_sd(cfg))
    return r


def _args(b):
    return [b[k] for k in ("lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs")]


def test_compute_loss_surface():
    cfg = cases.RDT_TINY
    b = R.batch(cfg, 3, 12)
    r = _runner(cfg)
    loss = r.compute_loss(*_args(b), noise=b["noise"], timesteps=b["timesteps"])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    tr = r.trainer()
    assert torch.equal(loss, _get_loss(tr, b, backward=False))
    ref, _ = R.loss_and_grads(cases.rdt_sd(cfg), b, cfg)
    assert abs(float(loss) - ref) <= 1e-5 * ref
    assert torch.equal(r.forward(*_args(b), noise=b["noise"], timesteps=b["timesteps"]), loss)
    torch.manual_seed(11)
    l1 = r.compute_loss(*_args(b))
    torch.manual_seed(11)
    l2 = r.compute_loss(*_args(b))
    assert torch.equal(l1, l2) and np.isfinite(float(l1))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("prediction_type", ["sample", "epsilon"])
def test_thirty_steps_halve_the_loss(prediction_type, precision):
    cfg = cases.RDT_TINY
    b = R.batch(cfg, 3, 12)
    tr = _runner(cfg, prediction_type).trainer(lr=1e-3, precision=precision)
    first = last = None
    for n in range(30):
        last = tr.train_step(*_args(b), noise=b["noise"], timesteps=b["timesteps"])
        if n == 0:
            first = float(last)
    last = float(_get_loss(tr, b, backward=False))
    print(f"[rdt_train 30 steps {prediction_type} {precision}] loss {first:.4f} -> {last:.4f} ({last / first:.3f} of the first)")
    assert last < 0.5 * first, (first, last)


def test_save_pretrained_round_trip(tmp_path):
    from models.rdt_runner import RDTRunner
    cfg = cases.RDT_TINY
    b = R.batch(cfg, 3, 12)
    r = _runner(cfg)
    d = cases.rdt_inputs(cfg, 3, 12)
    pa = lambda rr: rr.predict_action(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_mask"], b["ctrl_freqs"],
                                      x_init=d["x_init"]).float().cpu()
    before = pa(r)
    tr = r.trainer(lr=1e-3)
    for _ in range(3):
        tr.train_step(*_args(b), noise=b["noise"], timesteps=b["timesteps"])
    tr.save_pretrained(str(tmp_path / "ckpt"))
    assert os.path.exists(tmp_path / "ckpt" / "config.json") and os.path.exists(tmp_path / "ckpt" / "model.safetensors")
    loaded = RDTRunner.from_pretrained(str(tmp_path / "ckpt"), device=DEV)
    tr.sync_to(r)
    a1, a2 = pa(loaded), pa(r)
    assert torch.equal(a1, a2)
    assert float((a1 - before).abs().max()) > 1e-4, "training must change the predicted chunk"
