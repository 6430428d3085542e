"""The fp16 instantiations of the RDT training kernels (csrc/vt_train_rdt.hip, csrc/vt_attn_bwd.hip), vt_mse_loss_scaled and
vt_grad_unscale_clip_multi on the device.

Element-wise kernels: fp16-rounded inputs, fp64 from the same inputs as the reference.  An output stored in fp16 may miss the fp64 result by
at most 1.5 x what rounding that result once to fp16 misses it by (max-abs; one rounding is the best an fp16 store can do, the 1.5 covers fp32
arithmetic landing on the other side of a rounding boundary); fp32 sums keep the bars of their fp32 / bf16 tests.  Every call twice, bit-equal.
The bf16 results of the same calls are compared, by digest, with what the commit before the fp16 mode gave (tests/train16_cases.py).
Attention backward, "wave" and "mfma", on the six shapes of tests/attn_bwd_mfma16_ref.py.  vt_grad_unscale_clip_multi on a hand-built table
against tests/loss_scale_ref.py bit for bit."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import attn_bwd_mfma16_ref as A16
from tests import cases
from tests import loss_scale_ref as S
from tests import train16_cases as K
from oracle import rdt as orr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H16 = torch.float16


def h(x):
    """fp32 tensor rounded to the fp16 grid."""
    return x.half().float()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _stored_fp16_bar(tag, got, ref64):
    """got (fp16) against ref64: max-abs error at most 1.5 x that of ref64 rounded once to fp16."""
    assert got.dtype == H16, tag
    e = float((got.cpu().double() - ref64).abs().max())
    e1 = float((ref64.to(H16).double() - ref64).abs().max())
    print(f"[fp16 {tag}] max err {e:.3e}; one rounding of the fp64 result {e1:.3e}")
    assert e <= 1.5 * e1, (tag, e, e1)


@pytest.mark.parametrize("mode", ["meansq", "var"])
@pytest.mark.parametrize("D", [256, 2048])
def test_rmsnorm_bwd_fp16(mode, D):
    from vlatouch import _lib as L
    from vlatouch.rdt_train import rmsnorm_bwd
    g = torch.Generator().manual_seed(D)
    x, w, dy = h(torch.randn(5, D, generator=g) * 1.7 + 0.3), 1 + 0.2 * torch.randn(D, generator=g), h(torch.randn(5, D, generator=g))
    xl, wl = x.double().requires_grad_(True), w.double().requires_grad_(True)
    with torch.enable_grad():
        (orr.rms_norm(xl, wl, 1e-6, mode) * dy.double()).sum().backward()
    code = L.NORM_RMS_MEANSQ if mode == "meansq" else L.NORM_RMS_VAR
    outs = [rmsnorm_bwd(x.to(DEV, H16), w.to(DEV), dy.to(DEV, H16), 1e-6, code) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    _stored_fp16_bar(f"rmsnorm_bwd {mode} D{D} dx", outs[0][0], xl.grad)
    e, scale = float((outs[0][1].cpu().double() - wl.grad).abs().max()), float(wl.grad.abs().max())
    print(f"[fp16 rmsnorm_bwd {mode} D{D}] dw: {e / scale:.2e} of max-abs")
    assert outs[0][1].dtype == torch.float32 and e <= 1e-5 * scale, (e, scale)


@pytest.mark.parametrize("mode", ["meansq", "var"])
def test_headnorm_bwd_fp16(mode):
    """33 tokens x 4 heads = 132 (token, head) pairs: two full groups of 64 and a ragged one of 4; the k slice of a packed qkv buffer."""
    from vlatouch import _lib as L
    from vlatouch.rdt_train import headnorm_bwd_
    Hh, D, M = 4, 256, 33
    g = torch.Generator().manual_seed(5)
    buf, w, dbuf = h(torch.randn(M, 3 * D, generator=g) * 1.3 + 0.2), 1 + 0.2 * torch.randn(64, generator=g), h(torch.randn(M, 3 * D, generator=g))
    xl, wl = buf[:, D:2 * D].double().clone().requires_grad_(True), w.double().requires_grad_(True)
    with torch.enable_grad():
        (orr.rms_norm(xl.view(M, Hh, 64), wl, 1e-6, mode).reshape(M, D) * dbuf[:, D:2 * D].double()).sum().backward()
    code = L.NORM_RMS_MEANSQ if mode == "meansq" else L.NORM_RMS_VAR
    res = []
    for _ in range(2):
        xb, db = buf.to(DEV, H16), dbuf.to(DEV, H16)
        dw = headnorm_bwd_(xb[:, D:2 * D], db[:, D:2 * D], Hh, w.to(DEV), 1e-6, code)
        res.append((db, dw))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    got = res[0][0].cpu()
    assert torch.equal(got[:, :D].float(), dbuf[:, :D]) and torch.equal(got[:, 2 * D:].float(), dbuf[:, 2 * D:])       # q and v slices untouched
    _stored_fp16_bar(f"headnorm_bwd {mode} dx", res[0][0][:, D:2 * D], xl.grad)
    e, scale = float((res[0][1].cpu().double() - wl.grad).abs().max()), float(wl.grad.abs().max())
    print(f"[fp16 headnorm_bwd {mode}] dw: {e / scale:.2e} of max-abs")
    assert e <= 1e-5 * scale, (e, scale)


@pytest.mark.parametrize("kind", ["gelu_tanh", "silu"])
def test_activation_and_derivative_fp16(kind):
    from vlatouch import _lib as L
    from vlatouch.rdt_train import act
    x = h(torch.linspace(-9, 9, 20001))
    dy = h(torch.linspace(-2, 2, 20001).flip(0))
    xl = x.double().requires_grad_(True)
    with torch.enable_grad():
        y = F.gelu(xl, approximate="tanh") if kind == "gelu_tanh" else F.silu(xl)
        (y * dy.double()).sum().backward()
    code = L.ACT_GELU_TANH if kind == "gelu_tanh" else L.ACT_SILU
    xd, dd = x.to(DEV, H16), dy.to(DEV, H16)
    f1, d1 = act(xd, code), act(xd, code, dd)
    assert torch.equal(_bits(f1), _bits(act(xd, code))) and torch.equal(_bits(d1), _bits(act(xd, code, dd)))
    _stored_fp16_bar(f"{kind} forward", f1, y.detach())
    _stored_fp16_bar(f"{kind} derivative", d1, xl.grad)


def test_small_kernels_fp16():
    """vt_ddpm_qsample, vt_timestep_embed, vt_add_rowvec_, vt_transpose_pad (M = 33: not a multiple of 8), the typed column sum / add / column
    copy (odd offsets) and vt_mse_loss with fp16 activations: each twice, bit-equal, and against torch."""
    from tests import rdt_train_ref as R
    from vlatouch.rdt_train import (add_, add_rowvec_, alphas_cumprod, colsum, copy_cols, ddpm_qsample, mse_loss, timestep_embed, timestep_freqs,
                                    transpose_pad)
    g = torch.Generator().manual_seed(3)
    B, Hz, A = 3, 8, 128
    b = R.batch(cases.RDT_TINY, B, 12)
    ab = alphas_cumprod(1000, "squaredcos_cap_v2")
    qs = [ddpm_qsample(b["state_tokens"].to(DEV), b["action_gt"].to(DEV), b["noise"].to(DEV), b["action_mask"].to(DEV), b["timesteps"].to(DEV),
                       ab.to(DEV), H16) for _ in range(2)]
    assert qs[0].shape == (B, Hz + 1, 2 * A) and torch.equal(_bits(qs[0]), _bits(qs[1]))
    a = ab[b["timesteps"]].double()[:, None, None]
    want = torch.cat([torch.cat([b["state_tokens"].double(), a.sqrt() * b["action_gt"].double() + (1 - a).sqrt() * b["noise"].double()], dim=1),
                      b["action_mask"].double().expand(-1, Hz + 1, -1)], dim=2)
    _stored_fp16_bar("ddpm_qsample", qs[0], want)
    t = torch.tensor([3.0, 437.0, 998.0])
    fr = timestep_freqs(256)
    e1, e2 = timestep_embed(t.to(DEV), fr.to(DEV), H16), timestep_embed(t.to(DEV), fr.to(DEV), H16)
    arg = t.double()[:, None] * fr.double()[None]                     # fp64 from the fp32 frequency table the kernel reads
    assert torch.equal(_bits(e1), _bits(e2))
    _stored_fp16_bar("timestep_embed", e1, torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1))
    x = h(torch.randn(33, 40, generator=g))
    xd = x.to(DEV, H16)
    pos = torch.randn(40, generator=g)
    r1, r2 = xd.clone(), xd.clone()
    add_rowvec_(r1, pos.to(DEV)), add_rowvec_(r2, pos.to(DEV))
    assert torch.equal(_bits(r1), _bits(r2)) and torch.equal(r1.cpu(), (x + pos[None]).to(H16))       # one fp32 sum, one rounding: exactly torch's
    ta, tb = transpose_pad(xd).cpu(), transpose_pad(xd).cpu()
    assert torch.equal(_bits(ta), _bits(tb)) and ta.shape == (40, 40) and torch.equal(ta[:, :33].float(), x.t()) and float(ta[:, 33:].float().abs().sum()) == 0.0
    c1, c2 = colsum(xd).cpu(), colsum(xd).cpu()
    assert c1.dtype == torch.float32 and torch.equal(c1, c2) and float((c1.double() - x.double().sum(0)).abs().max()) <= 1e-5
    y = h(torch.randn(33, 40, generator=g))
    s1, s2 = add_(xd.clone(), y.to(DEV, H16)).cpu(), add_(xd.clone(), y.to(DEV, H16)).cpu()
    assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(s1, (x + y).to(H16))
    d = torch.zeros(33, 64, dtype=H16, device=DEV)
    copy_cols(xd, 7, d, 13, 23)
    dc = d.cpu().float()
    assert torch.equal(dc[:, 13:36], x[:, 7:30]) and float(dc[:, :13].abs().sum()) == 0.0 and float(dc[:, 36:].abs().sum()) == 0.0
    tgt = torch.randn(33, 40, generator=g)
    (l1, d1), (l2, d2) = mse_loss(xd, tgt.to(DEV)), mse_loss(xd, tgt.to(DEV))
    assert torch.equal(l1, l2) and torch.equal(_bits(d1), _bits(d2))
    want = ((x.double() - tgt.double()) ** 2).mean()
    assert abs(float(l1) - float(want)) <= 1e-6 * float(want)
    _stored_fp16_bar("mse_loss dpred", d1, 2 * (x.double() - tgt.double()) / x.numel())


@pytest.mark.parametrize("dtype", [H16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("scale", [1.0, 1024.0, 3000.0, 2.0 ** 16])
def test_mse_loss_scaled(dtype, scale):
    """vt_mse_loss_scaled against fp64: the loss is NOT scaled (1e-6 relative, vt_mse_loss's bar), d pred = S * 2 (pred - target) / n with one
    rounding at a 16-bit store (the 1.5 x one-rounding bar; fp32: two fp32 roundings, 2^-22 relative per element); S = 1 gives vt_mse_loss's bits."""
    from vlatouch.rdt_train import mse_loss
    g = torch.Generator().manual_seed(7)
    x, tgt = torch.randn(33, 40, generator=g).to(dtype), torch.randn(33, 40, generator=g)
    xd, td = x.to(DEV), tgt.to(DEV)
    (l1, d1), (l2, d2) = mse_loss(xd, td, scale), mse_loss(xd, td, scale)
    assert torch.equal(l1, l2) and torch.equal(_bits(d1), _bits(d2)) and d1.dtype == dtype
    want = ((x.double() - tgt.double()) ** 2).mean()
    ref = scale * 2 * (x.double() - tgt.double()) / x.numel()
    assert abs(float(l1) - float(want)) <= 1e-6 * float(want)
    e = float((d1.cpu().double() - ref).abs().max())
    if dtype == torch.float32:
        assert bool(((d1.cpu().double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all()), e
    else:
        e1 = float((ref.to(dtype).double() - ref).abs().max())
        print(f"[mse_loss_scaled {dtype} S={scale}] d pred max err {e:.3e}; one rounding {e1:.3e}")
        assert e <= 1.5 * e1, (e, e1)
    if scale == 1.0:
        l0, d0 = mse_loss(xd, td)
        assert torch.equal(l0, l1) and torch.equal(_bits(d0), _bits(d1))


def test_bf16_results_are_the_parents():
    """The bf16 instantiations after the kernels became templates on the 16-bit type: digest for digest what the commit before gave."""
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        want = json.load(f)["sha256"]
    got = K.bf16_saved_cases(DEV)
    assert list(got) == list(want)
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ attention backward
def _hip(bufs, views, do, mask, kernel):
    from vlatouch.rdt_train import attention_bwd
    dbufs = [b.to(DEV, H16) for b in bufs]
    gbufs = [torch.full_like(b, float("nan")) for b in dbufs]
    q, k, v = views(*dbufs)
    dq, dk, dv = views(*gbufs)
    km = None if mask is None else mask.to(DEV).to(torch.uint8).contiguous()
    ws = attention_bwd(q, k, v, do.to(DEV, H16), dq, dk, dv, kmask=km, kernel=kernel)
    torch.cuda.synchronize()
    return [t.float().cpu() for t in (dq, dk, dv)], ws.cpu()


_IDS = [f"{c[1]}x{c[2]}-H{c[3]}" for c in A16.CASES]


@pytest.mark.parametrize("case", A16.CASES, ids=_IDS)
def test_attention_bwd_wave_fp16(case):
    """vt_attention_bwd on fp16 operands (fp32 probabilities, one rounding at the store): at most 1.5 x the error of torch's fp16 CPU backward."""
    (bufs, views, do, mask), ref, th = A16.refs(case)
    got, ws = _hip(bufs, views, do, mask, "wave")
    again, ws2 = _hip(bufs, views, do, mask, "wave")
    assert torch.equal(_bits(ws), _bits(ws2))
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(_bits(got[i]), _bits(again[i])), f"{name}: two calls differ"
        e, et = float((got[i].double() - ref[i]).abs().max()), float((th[i] - ref[i]).abs().max())
        print(f"[attention_bwd wave fp16 {case[1]}x{case[2]} H{case[3]}] {name}: max err {e:.3e}; torch fp16 on the CPU {et:.3e}")
        assert bool(torch.isfinite(got[i]).all()) and e <= 1.5 * et, (name, e, et)
    _masked_are_zero(got, mask)


def _masked_are_zero(got, mask):
    if mask is None:
        return
    assert float(got[1][~mask].abs().max()) == 0.0 and float(got[2][~mask].abs().max()) == 0.0, "masked keys"
    assert all(float(got[i][1].abs().max()) == 0.0 for i in range(3)), "the fully masked batch row"


@pytest.mark.parametrize("case", A16.CASES, ids=_IDS)
def test_attention_bwd_mfma_fp16(case):
    """vt_attention_bwd_mfma on fp16 operands: per gradient at most 1.25 x the error of the CPU statement on the same inputs (the kernel is
    that arithmetic in another summation order); two calls bit-equal; masked rows and keys exactly zero.  The statistics agree with the wave
    kernel's to 1e-5 of each statistic's largest magnitude over the case (delta = sum P dP cancels, so no summation order holds an
    element-wise relative bound near a zero of it; m and 1 / l are far from zero and hold it element-wise as well)."""
    (bufs, views, do, mask), ref, _ = A16.refs(case)
    q, k, v = views(*bufs)
    st = A16.statement(q, k, v, do, mask=mask)
    got, ws = _hip(bufs, views, do, mask, "mfma")
    again, ws2 = _hip(bufs, views, do, mask, "mfma")
    assert torch.equal(_bits(ws), _bits(ws2))
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(_bits(got[i]), _bits(again[i])), f"{name}: two calls differ"
        e, es = float((got[i].double() - ref[i]).abs().max()), float((st[i].double() - ref[i]).abs().max())
        print(f"[attention_bwd mfma fp16 {case[1]}x{case[2]} H{case[3]}] {name}: max err {e:.3e}; the statement {es:.3e}")
        assert bool(torch.isfinite(got[i]).all()) and e <= 1.25 * es, (name, e, es)
    _masked_are_zero(got, mask)
    _, ws_wave = _hip(bufs, views, do, mask, "wave")
    for col, name in enumerate(("m", "1 / l", "delta")):
        a, b = ws[:, col].double(), ws_wave[:, col].double()
        worst, top = float((a - b).abs().max()), float(b.abs().max())
        print(f"[attention_bwd mfma fp16 {case[1]}x{case[2]} H{case[3]}] {name} against the wave kernel: {worst:.2e} (largest {top:.3e})")
        assert worst <= 1e-5 * top, (name, worst, top)
        if col < 2:
            assert bool(((a - b).abs() <= 1e-5 * b.abs()).all()), name


@pytest.mark.parametrize("kernel", ["wave", "mfma"])
def test_attention_bwd_overflowing_upstream_gradient(kernel):
    """dO scaled by 2^24 leaves fp16's range: the outputs are non-finite (which the loss scaler's flag then catches) and the launch is ordinary
    arithmetic — it completes, and the next call on the same stream gives the usual bits."""
    case = A16.CASES[0]
    (bufs, views, do, mask), _, _ = A16.refs(case)
    clean, _ = _hip(bufs, views, do, mask, kernel)
    got, _ = _hip(bufs, views, do * 2.0 ** 24, mask, kernel)
    assert all(not bool(torch.isfinite(t).all()) for t in got)
    after, _ = _hip(bufs, views, do, mask, kernel)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean, after))


def test_python_still_refuses_fp32_for_mfma():
    from vlatouch.rdt_train import attention_bwd
    t = lambda: torch.zeros(1, 4, 1, 64, device=DEV)
    with pytest.raises(ValueError, match="fp16"):
        attention_bwd(t(), t(), t(), t(), t(), t(), t(), kernel="mfma")


# ------------------------------------------------------------------------------------------------ unscale + check + clip
SIZES = (1, 4095, 4096, 4097, 3 * 4096 + 5)


def _table(grads):
    """A multi-tensor table whose g column is `grads` (p / m / v / shadow are not touched by the kernel: p stands in)."""
    from vlatouch import train as T
    rows, chunks = T.mt_table((g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), 0, g.numel()) for g in grads)
    return rows.to(DEV), chunks


def _unscale_clip(host_grads, scale, max_norm):
    """-> (flag, norm, coef, gradients after the call) with tensor 3 (4097 elements) placed 4 bytes off a 16-byte boundary."""
    from vlatouch import _lib as L
    from vlatouch.rdt_train import inv_scale
    dev_grads = []
    for i, g in enumerate(host_grads):
        if i == 3:
            base = torch.zeros(g.numel() + 4, device=DEV)
            t = base[1:1 + g.numel()]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.zeros(g.numel(), device=DEV)
            assert t.data_ptr() % 16 == 0
        t.copy_(g)
        dev_grads.append(t)
    tab, chunks = _table(dev_grads)
    assert chunks == sum((n + 4095) // 4096 for n in SIZES)
    part = torch.full((chunks,), float("nan"), device=DEV)
    out = torch.full((4,), float("nan"), device=DEV)
    out.view(torch.int32)[2] = 12345                                   # a stale flag: the call clears it
    L.check(L.lib().vt_grad_unscale_clip_multi(L.ptr(tab), len(dev_grads), chunks, max_norm, inv_scale(scale), L.ptr(part), L.ptr(out),
                                               C.c_void_p(out.data_ptr() + 8), L.stream_ptr(torch.device(DEV))), "vt_grad_unscale_clip_multi")
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool(torch.isnan(host[3]))                                   # the word behind the flag is not the kernel's
    return int(host.view(torch.int32)[2]), host[0].clone(), host[1].clone(), [t.cpu() for t in dev_grads]


def _grads(seed=0):
    v = S.mixed_magnitudes(sum(SIZES), seed=seed)
    return [c.clone() for c in torch.split(v, list(SIZES))]


@pytest.mark.parametrize("scale", [2.0 ** 16, 3000.0])
@pytest.mark.parametrize("max_norm", [1.0, 1e9], ids=["clipping", "idle"])
def test_unscale_clip_multi_finite(scale, max_norm):
    """Finite gradients: flag 0; the norm within 1e-6 of the fp64 norm of g / S (fp32 partial sums of 4096 squares); the coefficient and every
    gradient bit-equal to the host statement evaluated at the kernel's norm; two calls bit-equal."""
    grads = _grads()
    flag, norm, coef, out = _unscale_clip(grads, scale, max_norm)
    flag2, norm2, coef2, out2 = _unscale_clip(grads, scale, max_norm)
    assert flag == 0 and flag2 == 0
    assert torch.equal(_bits(norm.reshape(1)), _bits(norm2.reshape(1))) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, out2))
    n64 = float(torch.cat(grads).double().div(scale).norm())
    assert abs(float(norm) - n64) <= 1e-6 * n64, (float(norm), n64)
    found, _, coef_s, want = S.unscale_clip(grads, scale, max_norm, norm=norm)
    assert found is False and torch.equal(_bits(coef.reshape(1)), _bits(coef_s.reshape(1))) and (float(coef) < 1.0) == (max_norm == 1.0)
    for i, (a, b) in enumerate(zip(out, want)):
        assert torch.equal(_bits(a), _bits(b)), f"tensor {i} ({SIZES[i]} elements)"


@pytest.mark.parametrize("where", [(0, 0), (1, 4094), (3, 4096), (4, 3 * 4096 + 4)], ids=lambda w: f"tensor{w[0]}")
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
def test_unscale_clip_multi_planted_nonfinite(where, value):
    """One non-finite element, in a one-element tensor, at the end of a chunk, in the unaligned tensor's second chunk, at the very end: the
    flag is 1, as the statement's, and no gradient is written."""
    grads = _grads(seed=1)
    grads[where[0]][where[1]] = value
    flag, norm, coef, out = _unscale_clip(grads, 2.0 ** 16, 1.0)
    assert flag == 1 and S.unscale_clip(grads, 2.0 ** 16, 1.0)[0] is True
    assert not bool(torch.isfinite(norm))
    for i, (a, b) in enumerate(zip(out, grads)):
        assert torch.equal(_bits(a), _bits(b)), f"tensor {i} was written"


def test_unscale_clip_multi_refuses_bad_arguments():
    from vlatouch import _lib as L
    g = [torch.ones(8, device=DEV)]
    tab, chunks = _table(g)
    part, out = torch.zeros(chunks, device=DEV), torch.zeros(4, device=DEV)
    sp = L.stream_ptr(torch.device(DEV))
    for max_norm, inv in ((0.0, 1.0), (1.0, 0.0), (1.0, float("inf")), (1.0, float("nan"))):
        rc = L.lib().vt_grad_unscale_clip_multi(L.ptr(tab), 1, chunks, max_norm, inv, L.ptr(part), L.ptr(out), C.c_void_p(out.data_ptr() + 8), sp)
        assert rc == -22 and "vt_grad_unscale_clip_multi" in L.lib().vt_last_error().decode()
    assert L.lib().vt_grad_unscale_clip_multi(L.ptr(tab), 1, chunks, 1.0, 1.0, L.ptr(part), L.ptr(out), None, sp) == -22
    torch.cuda.synchronize()
    assert torch.equal(g[0].cpu(), torch.ones(8))
