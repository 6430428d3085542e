"""GPU parity of the T5 encoder's own kernels (csrc/vt_t5.hip), each called alone through the entry vt_t5_forward itself launches it through, and
of the row norm's XXL-width route, against float64 on the CPU.

vt_t5_attention (t5_attn_kernel<float> on mfma_f32_16x16x4f32, t5_attn_kernel<bf16_t>): reference, inputs and grid are tests/t5_attn_ref.py:
softmax(q k^T + rel_bias[bucket(j - i)][h], masked keys at -inf) v per (batch, head), no scale; ones, tile, first / last key, key % 8 and ramp
columns in V under uniform, ascending, descending, random-bias and needle-bias scores; three bucket configurations; lengths 1 .. 1024; masks
that are no suffix, leading masked tiles and per-sample lengths.  qkv sits between NaN rows, out between 4 KiB of a sentinel pattern that must
survive, the mask bytes are followed by bytes that say "attend"; every call runs twice and is compared bit for bit.  A sample without a valid
key (vt_t5_forward rejects one) comes out as exact zeros.
Bars, per (batch, head) slice (t5_attn_ref.BAR_REL / BAR_ABS; tests/test_t5_attn_ref_host.py derives them on the CPU and shows that five
kernel bugs leave them): random columns max|out - ref| / max|ref| <= 3.7e-6 (fp32), 1.35e-2 (bf16); structured columns max|out - ref| <=
6.8e-6 (fp32), 9.3e-3 (bf16): 3 x the format's own cost, all below test_gpu_attention.py's bars for the same arithmetic.
Measured, worst over the grid (random / structured): fp32 2.1e-6 / 3.3e-6; bf16 4.4e-3 / 3.1e-3.

vt_t5_geglu (t5_geglu_kernel): h = gelu_tanh(g[:, :F]) * g[:, F:] against fp64 F.gelu(approximate="tanh") from the stored values, every element,
with row pitches wider than the rows, planted +-60 and +-1e4 gates (T5-XXL's wi_0 range) and a sentinel in the pitch gap and around h.
|out - ref| <= 2e-6 |b| + 2^-22 |ref| (fp32: test_activation_and_derivative's absolute bar for the activation, one rounding of the product),
+ 2^-8 |ref| (bf16: one bf16 rounding, with a factor of two).  Measured, worst |out - ref| / bar: fp32 0.24, bf16 0.996 (a bf16 rounding reaches 2^-8 |ref| just above a power of two).

ops.rownorm at 2048 < D <= 4096 (rownorm_block_kernel<TO, 4>, T5-XXL's width): LayerNorm and both RMS forms, fp32 and bf16 out, against fp64
per row: max|out - ref| / max|ref row| <= 2e-5 / 1e-2, test_rownorm_modes's bars.  Measured: fp32 out 1.8e-7, bf16 out 3.7e-3."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import attn_ref as A
from tests import t5_attn_ref as T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT = {2: (torch.int16, 0x7E5A), 4: (torch.int32, 0x5AA5A55A)}
GUARD = 4096                                            # sentinel bytes before and after an output
PAD_ROWS = 3                                            # NaN rows before and after qkv
VT_ERR_ARG, VT_ERR_UNSUPPORTED = -22, -95               # csrc/vt_common.h


@pytest.fixture(scope="module")
def dev():
    from vlatouch import _lib as L
    L.lib()
    return torch.device("cuda:0")


class T5AttnCall:
    """Device buffers of one case; call() runs vt_t5_attention once, checks the sentinels and returns out [B, L, H, 64] on the CPU."""

    def __init__(self, dev, q, k, v, rel_bias, num_buckets, max_distance, keep):
        from vlatouch import _lib as L
        self.L, self.lib, self.dev = L, L.lib(), dev
        B, Ln, H, hd = q.shape
        self.shape, self.dt, es = (B, Ln, H, hd), q.dtype, q.element_size()
        rows, inner = B * Ln, H * hd
        buf = torch.full((rows + 2 * PAD_ROWS, 3 * inner), float("nan"), dtype=q.dtype)
        buf[PAD_ROWS:PAD_ROWS + rows] = torch.cat([t.reshape(rows, inner) for t in (q, k, v)], 1)
        self.qkv = buf.to(dev)
        self.qkv_ptr = self.qkv.data_ptr() + PAD_ROWS * 3 * inner * es
        self.tab = torch.from_numpy(T.bucket_table(num_buckets, max_distance)).to(dev)
        self.rel_bias = rel_bias.float().contiguous().to(dev)
        self.num_buckets = num_buckets
        self.km = None
        if keep is not None:
            km = torch.ones(rows + 64, dtype=torch.uint8)       # the bytes behind the mask say "attend": what a leak would read
            km[:rows] = keep.reshape(-1).to(torch.uint8)
            self.km = km.to(dev)
        self.idt, self.sent = SENT[es]
        self.g, self.n = GUARD // es, rows * inner
        self.obuf = torch.empty(self.n + 2 * self.g, dtype=self.idt, device=dev)

    def call(self):
        B, Ln, H, hd = self.shape
        L = self.L
        self.obuf.fill_(self.sent)
        L.check(self.lib.vt_t5_attention(C.c_void_p(self.qkv_ptr), C.c_void_p(self.obuf.data_ptr() + GUARD), L.ptr(self.tab), L.ptr(self.rel_bias),
                                         L.ptr(self.km), B, H, Ln, self.num_buckets, L.dt_code(self.dt), L.stream_ptr(self.dev)), "vt_t5_attention")
        torch.cuda.synchronize(self.dev)
        hit = int((self.obuf[:self.g] != self.sent).sum()) + int((self.obuf[self.g + self.n:] != self.sent).sum())
        assert hit == 0, f"{hit} elements written into the 4 KiB before or after out"
        return self.obuf[self.g:self.g + self.n].clone().view(self.dt).reshape(B, Ln, H, hd).cpu()


def _id(c):
    return f"{c['dname']}-B{c['B']}-H{c['H']}-L{c['L']}-{c['mask']}-{c['regime']}-nb{c['num_buckets']}"


@pytest.mark.parametrize("case", [pytest.param(c, id=_id(c)) for c in T.gpu_grid()])
def test_t5_attention_vs_float64(dev, case):
    q, k, v, rel_bias, buckets, keep = T.case_tensors(case)
    ref = T.reference(q, k, v, rel_bias, buckets, keep)
    call = T5AttnCall(dev, q, k, v, rel_bias, case["num_buckets"], case["max_distance"], keep)
    out, again = call.call(), call.call()
    assert torch.equal(out.view(call.idt), again.view(call.idt)), "two calls differ"
    assert bool(torch.isfinite(out.float()).all()), f"NaN or inf in {int((~torch.isfinite(out.float())).sum())} elements of out"
    e_rel, e_abs = T.slice_errors(out, ref)
    print(f"[t5 attn {_id(case)}] rel {e_rel:.3e} abs {e_abs:.3e}")
    d = case["dname"]
    assert e_rel <= T.BAR_REL[d], f"random columns {e_rel} > {T.BAR_REL[d]}"
    assert e_abs <= T.BAR_ABS[d], f"structured columns {e_abs} > {T.BAR_ABS[d]}"


@pytest.mark.parametrize("dname", list(T.DT))
def test_t5_attention_sample_without_keys_is_zero(dev, dname):
    """Not part of vt_t5_forward's contract (it rejects such a mask), but the kernel states `inv = l > 0 ? 1 / l : 0`: the middle sample of three
    has no valid key and must come out as exact zeros, never NaN; its neighbours are held to the bars."""
    B, H, Ln = 3, 3, 65
    q, k, v, rel_bias = T.make_inputs(dname, B, H, Ln, "bias_random", 32, 128, seed=7)
    keep = A.make_mask("sample", B, Ln)
    buckets = T.rel_buckets(Ln, 32, 128)
    ref = T.reference(q, k, v, rel_bias, buckets, keep)
    call = T5AttnCall(dev, q, k, v, rel_bias, 32, 128, keep)
    out, again = call.call(), call.call()
    assert torch.equal(out.view(call.idt), again.view(call.idt))
    assert bool(torch.isfinite(out.float()).all()) and float(out[1].float().abs().max()) == 0.0 and float(ref[1].abs().max()) == 0.0
    e_rel, e_abs = T.slice_errors(out[[0, 2]], ref[[0, 2]])
    assert e_rel <= T.BAR_REL[dname] and e_abs <= T.BAR_ABS[dname], (e_rel, e_abs)


def test_t5_attention_refusals_return_before_any_launch(dev):
    """A null required pointer, B, H or L < 1, L > 1024, num_buckets outside 1 .. 127 and a dtype the kernel is not built for: the error code and
    a message, out untouched.  (The buffers hold L = 1025 and 128 buckets, the largest values asked for.)"""
    from vlatouch import _lib as L
    lib = L.lib()
    B, H, Ln, nb = 1, 2, 16, 32
    qkv = torch.zeros(1025, 3 * H * 64, device=dev)
    out = torch.empty(1025 * H * 64, dtype=torch.int32, device=dev)
    tab = torch.from_numpy(T.bucket_table(32, 128)).to(dev)
    rel_bias = torch.zeros(128, H, device=dev)
    km = torch.ones(1025, dtype=torch.uint8, device=dev)
    good = dict(qkv=qkv.data_ptr(), out=out.data_ptr(), tab=tab.data_ptr(), rel_bias=rel_bias.data_ptr(), km=km.data_ptr(), B=B, H=H, L=Ln, nb=nb, dt=0)

    def run(**over):
        a = dict(good, **over)
        out.fill_(SENT[4][1])
        r = lib.vt_t5_attention(C.c_void_p(a["qkv"]), C.c_void_p(a["out"]), C.c_void_p(a["tab"]), C.c_void_p(a["rel_bias"]), C.c_void_p(a["km"]),
                                a["B"], a["H"], a["L"], a["nb"], a["dt"], L.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        return r, bool((out == SENT[4][1]).all()), lib.vt_last_error().decode()

    r, untouched, _ = run()
    assert r == 0 and not untouched                                       # the template itself is valid, and writes
    assert run(km=0)[0] == 0 and run(dt=1)[0] == 0 and run(L=1024)[0] == 0 and run(nb=1)[0] == 0 and run(nb=127)[0] == 0
    for over in (dict(qkv=0), dict(out=0), dict(tab=0), dict(rel_bias=0), dict(B=0), dict(B=-1), dict(H=0), dict(L=0), dict(L=-3), dict(L=1025),
                 dict(nb=0), dict(nb=128), dict(nb=-1)):
        r, untouched, msg = run(**over)
        assert r == VT_ERR_ARG and untouched and "vt_t5_attention" in msg, (over, r, untouched, msg)
    for code in (2, 3, -1, 7):
        r, untouched, msg = run(dt=code)
        assert r == VT_ERR_UNSUPPORTED and untouched and "vt_t5_attention" in msg, (code, r, untouched, msg)


# ------------------------------------------------------------------ GEGLU gate
GEGLU_ROWS = (1, 37, 257)
PLANTED = (60.0, -60.0, 1e4, -1e4)


def _geglu_inputs(dname, rows, Fh, seed):
    """a: a linspace over [-9, 9] interleaved with N(0, 3), with +-60 and +-1e4 planted (first, last and two inner columns of a row); b ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(rows * Fh, generator=g) * 3.0
    a[0::2] = torch.linspace(-9, 9, (rows * Fh + 1) // 2)
    a = a.reshape(rows, Fh)
    for i, val in enumerate(PLANTED):
        r = (i * 7) % rows
        a[r, (0, Fh - 1, Fh // 2, Fh // 3)[i]] = val
        a[rows - 1 - r, (Fh - 1, 0, Fh // 3 + 1, Fh // 2 - 1)[i]] = -val
    b = torch.randn(rows, Fh, generator=g)
    return a.to(T.DT[dname]), b.to(T.DT[dname])


def _geglu_bar(dname, ref, b):
    return 2e-6 * b.double().abs() + 2.0 ** -22 * ref.abs() + (2.0 ** -8 * ref.abs() if dname == "bf16" else 0.0)


@pytest.mark.parametrize("dname,Fh", [("f32", 64), ("f32", 192), ("f32", 1024), ("bf16", 64), ("bf16", 192), ("bf16", 1024), ("bf16", 2816)])
def test_t5_geglu_vs_float64(dev, dname, Fh):
    from vlatouch import _lib as L
    lib = L.lib()
    dt = T.DT[dname]
    es = 4 if dname == "f32" else 2
    idt, sent = SENT[es]
    gd = GUARD // es
    worst = 0.0
    for rows in GEGLU_ROWS:
        a, b = _geglu_inputs(dname, rows, Fh, seed=rows + Fh)
        ref = F.gelu(a.double(), approximate="tanh") * b.double()
        bar = _geglu_bar(dname, ref, b)
        swapped = F.gelu(b.double(), approximate="tanh") * a.double()          # the gate on the wrong half
        assert bool(((swapped - ref).abs() > bar).any()) and float(((swapped - ref).abs() > bar).double().mean()) > 0.9
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1e3
        for ldg, ldh in ((2 * Fh, Fh), (2 * Fh + 16, Fh + 8), (2 * Fh + 16, Fh), (2 * Fh, Fh + 8)):
            gbuf = torch.full((rows, ldg), float("nan"), dtype=dt)             # the pitch gap of g holds NaN: reading it shows
            gbuf[:, :Fh], gbuf[:, Fh:2 * Fh] = a, b
            gdev = gbuf.to(dev)
            hbuf = torch.full((rows * ldh + 2 * gd,), sent, dtype=idt, device=dev)
            for _ in range(2):
                L.check(lib.vt_t5_geglu(L.ptr(gdev), ldg, C.c_void_p(hbuf.data_ptr() + GUARD), ldh, rows, Fh, L.dt_code(dt), L.stream_ptr(dev)),
                        "vt_t5_geglu")
            torch.cuda.synchronize(dev)
            body = hbuf[gd:gd + rows * ldh].view(rows, ldh)
            hit = int((hbuf[:gd] != sent).sum()) + int((hbuf[gd + rows * ldh:] != sent).sum()) + int((body[:, Fh:] != sent).sum())
            assert hit == 0, f"{hit} elements written outside h's rows (pitch gap or the 4 KiB on either side), rows {rows} ldg {ldg} ldh {ldh}"
            out = body[:, :Fh].contiguous().view(dt).cpu().double()
            assert bool(torch.isfinite(out).all()), (rows, ldg, ldh)
            ratio = (out - ref).abs() / bar.clamp_min(1e-300)
            ratio = torch.where((out - ref).abs() == 0, torch.zeros_like(ratio), ratio)
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 1.0, (rows, ldg, ldh, float(ratio.max()), int((ratio > 1).sum()))
            for val in PLANTED:                                                # the planted gates came through: gelu_tanh(+-60, +-1e4) = x or 0
                at = a.double() == torch.tensor(val, dtype=dt).double()
                assert bool(at.any()) and bool(torch.isfinite(out[at]).all())
    print(f"[t5 geglu {dname} F{Fh}] worst |out - ref| / bar {worst:.3f}")


def test_t5_geglu_refusals_return_before_any_launch(dev):
    """rows < 1, and F, ldg or ldh that is no multiple of the 16-byte vector (4 fp32 / 8 bf16 elements): the error code, h untouched."""
    from vlatouch import _lib as L
    lib = L.lib()
    rows, Fh = 4, 64
    g = torch.zeros(rows * (2 * Fh + 16), device=dev)
    h = torch.empty(rows * (Fh + 16), dtype=torch.int32, device=dev)

    def run(dt=0, ldg=2 * Fh, ldh=Fh, rows=rows, Fh=Fh, g_ptr=None, h_ptr=None):
        h.fill_(SENT[4][1])
        r = lib.vt_t5_geglu(C.c_void_p(g.data_ptr() if g_ptr is None else g_ptr), ldg, C.c_void_p(h.data_ptr() if h_ptr is None else h_ptr), ldh, rows, Fh,
                            dt, L.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        return r, bool((h == SENT[4][1]).all()), lib.vt_last_error().decode()

    assert run()[0] == 0 and not run()[1] and run(dt=1)[0] == 0 and run(ldg=2 * Fh + 16, ldh=Fh + 8)[0] == 0
    refused = [dict(rows=0), dict(rows=-2), dict(Fh=0), dict(g_ptr=0), dict(h_ptr=0),
               dict(Fh=62, ldg=128, ldh=64), dict(ldg=2 * Fh + 2), dict(ldh=Fh + 2),                       # fp32: multiples of 4
               dict(dt=1, Fh=60, ldg=128, ldh=64), dict(dt=1, ldg=2 * Fh + 4), dict(dt=1, ldh=Fh + 4),       # bf16: multiples of 8
               dict(ldg=2 * Fh - 4), dict(ldh=Fh - 4)]                                                       # rows that overlap
    for over in refused:
        r, untouched, msg = run(**over)
        assert r == VT_ERR_ARG and untouched and "vt_t5_geglu" in msg, (over, r, untouched, msg)
    for code in (2, 3, -1):
        r, untouched, msg = run(dt=code)
        assert r == VT_ERR_UNSUPPORTED and untouched and "vt_t5_geglu" in msg, (code, r, untouched, msg)


# ------------------------------------------------------------------ row norm at T5-XXL's width
def _rownorm_ref(x, w, b, mode, L):
    x, w = x.double(), w.double()
    if mode == L.NORM_LAYER:
        return F.layer_norm(x, (x.shape[1],), w, b.double(), 1e-6)
    if mode == L.NORM_RMS_MEANSQ:
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    return x * torch.rsqrt(x.var(-1, keepdim=True) + 1e-6) * w               # NORM_RMS_VAR: timm's unbiased-variance form, x not centred


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("D", [2052, 3072, 4096])
def test_rownorm_xxl_width_vs_float64(dev, D, rows):
    """rownorm_block_kernel<TO, 4>: 513, 768 and 1024 float4 per row (the last thread column partly, never and fully used), every mode, both
    output types, and rows whose mean is 400 standard deviations from zero on the two modes that centre.
    Before the kernel added what its fp32 mean missed (the sum of the centred values over D), LayerNorm of the shifted rows missed the fp32 bar:
    per-row errors up to 2.3e-5 at D = 3072 (rows 37), 1.99e-5 at 2052 and 1.87e-5 at 4096, all from a mean good to an ulp of 400 only."""
    from vlatouch import ops, _lib as L
    g = torch.Generator().manual_seed(D + rows)
    x0 = torch.randn(rows, D, generator=g) * (0.5 + torch.rand(rows, 1, generator=g) * 4.0)
    w, b = torch.randn(D, generator=g) + 1.0, torch.randn(D, generator=g)
    shifted = torch.randn(rows, D, generator=g) + 400.0
    worst = {}
    for mode in (L.NORM_LAYER, L.NORM_RMS_MEANSQ, L.NORM_RMS_VAR):
        for x in (x0, shifted) if mode != L.NORM_RMS_MEANSQ else (x0,):
            ref = _rownorm_ref(x, w, b, mode, L)
            for odt, bar in ((torch.float32, 2e-5), (torch.bfloat16, 1e-2)):
                y = ops.rownorm(x.to(dev), w.to(dev), b.to(dev) if mode == L.NORM_LAYER else None, 1e-6, mode, out_dtype=odt)
                again = ops.rownorm(x.to(dev), w.to(dev), b.to(dev) if mode == L.NORM_LAYER else None, 1e-6, mode, out_dtype=odt)
                assert y.dtype == odt and torch.equal(y, again)
                y = y.cpu().double()
                assert bool(torch.isfinite(y).all())
                e = (y - ref).abs().amax(-1) / ref.abs().amax(-1)                  # per row
                what = (("layer", "meansq", "var")[mode] + ("+400" if x is shifted else ""), "f32" if odt == torch.float32 else "bf16")
                worst[what] = float(e.max())
                assert float(e.max()) <= bar, (mode, odt, x is shifted, e.tolist())
    print(f"[rownorm D{D} rows{rows}] worst per-row error " + ", ".join(f"{m} {o} {e:.2e}" for (m, o), e in worst.items()))


def test_rownorm_wider_than_4096_is_refused(dev):
    from vlatouch import ops
    from vlatouch._lib import VtError
    x, w = torch.zeros(2, 4100, device=dev), torch.ones(4100, device=dev)
    with pytest.raises(VtError):
        ops.rownorm(x, w, None, 1e-6, 1)
