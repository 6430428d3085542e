"""GPU parity of vt_attention (csrc/vt_attn.hip: attn_kernel, attn16u_kernel, attn16g_kernel with 3 and 6 query groups) through the C ABI, row by
row.  Reference: tests/attn_ref.py, softmax(scale q k^T, masked keys at -inf) v in float64 on the CPU per (batch, head) from the same stored
values; a row without a valid key is zero.  The inputs (attn_ref.make_inputs) make a dropped, doubled or leaked key visible: a ones column,
indicators of the key's tile, of the sample's first / last key and of the last tile's first / last key, under needle, uniform, ascending and
descending scores.

VtAttnParams is filled here (ops.attention cannot express the strides): q, k, v as views of one fused [B, N, 3, H, hd] buffer, k and v as halves
of [B, Nk, 2 H hd], or apart; K and V always hold 3 rows more than Nk per sample, NaN in both; a padded mask row (km_bs = Nk + 5) carries 1 in its
padding; O is compact (with Nq = 1: the CLS layout o_bs = o_rs), strided by H hd + 8, or by H hd + 2 (16-bit: back to attn_kernel), inside a
buffer of a sentinel pattern whose row gaps and 4 KiB on either side must survive every call.  Every call runs twice and is compared bit for
bit; 16-bit unmasked cases of 128 or more query rows run under vt_tune(9, v) for v in 0, 1, 3, 6.  Which kernel and how many waves a case
reaches is attn_ref.route, the launcher's routing restated (the library exports no query for it); tests/test_attn_ref_host.py holds the grid
against it.

Bars, per (batch, head) slice: random columns max|out - ref| / max|ref| <= 3e-5 (fp32), 1.5e-2 (bf16), 2e-3 (fp16), the bars test_attention has
for a whole tensor; structured columns (values in [0, 1]) max|out - ref| <= 3e-5, 1e-2, 2e-3.  No bar needed widening.  What rounding P to the
storage type alone costs (test_attn_ref_host.py, 577 and 257 keys): bf16 5.0e-3 / 2.4e-3, fp16 5.9e-4 / 3.0e-4.
Measured, worst over the grid (random columns / structured columns):
  fp32  attn_kernel 2.3e-6 / 2.0e-6
  bf16  attn_kernel 5.0e-3 / 2.8e-3; attn16u_kernel 5.5e-3 / 2.7e-3; attn16g_kernel, 3 and 6 groups, 5.5e-3 / 2.4e-3
  fp16  attn_kernel 6.6e-4 / 3.4e-4; attn16u_kernel 8.0e-4 / 3.4e-4; attn16g_kernel, 3 and 6 groups, 6.3e-4 / 3.4e-4
Before attn_kernel took `inv = l > 0 ? 1 / l : 0` every row of a sample without valid keys was NaN (0 * inf)."""
import ctypes as C

import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BAR_REL = {"f32": 3e-5, "bf16": 1.5e-2, "f16": 2e-3}
BAR_ABS = {"f32": 3e-5, "bf16": 1e-2, "f16": 2e-3}
SENT = {2: (torch.int16, 0x7E5A), 4: (torch.int32, 0x5AA5A55A)}
GUARD = 4096                                            # sentinel bytes before and after O
PAD_ROWS = 3                                            # NaN rows past Nk in K and V (and past Nq in a fused buffer)
VT_ERR_ARG, VT_ERR_UNSUPPORTED = -22, -95               # csrc/vt_common.h


@pytest.fixture(scope="module")
def dev():
    from vlatouch import _lib as L
    L.lib()
    return torch.device("cuda:0")


class AttnCall:
    """Device buffers of one case in its layout; call() runs vt_attention once, checks the sentinels and returns the rows written."""

    def __init__(self, dev, case, q, k, v, keep):
        from vlatouch import _lib as L
        self.L, self.lib, self.dev = L, L.lib(), dev
        B, H, Nq, Nk, hd = case["B"], case["H"], case["Nq"], case["Nk"], case["hd"]
        dt, D = q.dtype, H * hd
        es = q.element_size()
        nan = float("nan")
        p = L.AttnParams()
        if case["qkv"] == "fused3":
            N = max(Nq, Nk) + PAD_ROWS
            buf = torch.full((B, N, 3, H, hd), nan, dtype=dt)
            buf[:, :Nq, 0], buf[:, :Nk, 1], buf[:, :Nk, 2] = q, k, v
            self.keep_alive = [buf.to(dev)]
            base = self.keep_alive[0].data_ptr()
            p.Q, p.K, p.V = base, base + D * es, base + 2 * D * es
            p.q_bs = p.k_bs = p.v_bs = N * 3 * D
            p.q_rs = p.k_rs = p.v_rs = 3 * D
        else:
            qd = q.contiguous().to(dev)
            R = Nk + PAD_ROWS
            if case["qkv"] == "kvhalf":
                kv = torch.full((B, R, 2, H, hd), nan, dtype=dt)
                kv[:, :Nk, 0], kv[:, :Nk, 1] = k, v
                kvd = kv.to(dev)
                self.keep_alive = [qd, kvd]
                p.K, p.V = kvd.data_ptr(), kvd.data_ptr() + D * es
                p.k_bs = p.v_bs = R * 2 * D
                p.k_rs = p.v_rs = 2 * D
            else:
                kd, vd = (torch.cat([t, torch.full((B, PAD_ROWS, H, hd), nan, dtype=dt)], 1).to(dev) for t in (k, v))
                self.keep_alive = [qd, kd, vd]
                p.K, p.V = kd.data_ptr(), vd.data_ptr()
                p.k_bs = p.v_bs = R * D
                p.k_rs = p.v_rs = D
            p.Q, p.q_bs, p.q_rs = qd.data_ptr(), Nq * D, D
        p.q_hs = p.k_hs = p.v_hs = hd
        if keep is not None:
            km_bs = Nk + 5 if case["km_pad"] else Nk
            km = torch.ones(B, km_bs, dtype=torch.uint8)        # the padding bytes say "attend": the bytes a leak would read
            km[:, :Nk] = keep.to(torch.uint8)
            self.km = km.to(dev)
            p.kmask, p.km_bs = self.km.data_ptr(), km_bs
        # O: [B][rows][o_rs] elements behind GUARD bytes of sentinel, the same after it
        self.o_rs = A.o_row_stride(case["o"], H, hd)
        self.rows = Nq if case["o"] == "compact" else Nq + 1
        self.idt, self.sent = SENT[es]
        self.g = GUARD // es
        self.n = B * self.rows * self.o_rs
        self.obuf = torch.empty(self.n + 2 * self.g, dtype=self.idt, device=dev)
        region = torch.zeros(B, self.rows, self.o_rs, dtype=torch.bool, device=dev)
        region[:, :Nq, :D] = True
        self.outside = torch.ones(self.n + 2 * self.g, dtype=torch.bool, device=dev)
        self.outside[self.g:self.g + self.n] = ~region.reshape(-1)
        p.O = self.obuf.data_ptr() + GUARD
        p.o_bs, p.o_rs = self.rows * self.o_rs, self.o_rs
        p.B, p.H, p.Nq, p.Nk = B, H, Nq, Nk
        p.scale, p.dtype, p.hd = A.scale_of(hd), L.dt_code(dt), hd
        self.p, self.dt, self.shape = p, dt, (B, Nq, H, hd)

    def call(self):
        B, Nq, H, hd = self.shape
        self.obuf.fill_(self.sent)
        self.L.check(self.lib.vt_attention(C.byref(self.p), self.L.stream_ptr(self.dev)), "vt_attention")
        torch.cuda.synchronize(self.dev)
        hit = int((self.obuf[self.outside] != self.sent).sum())
        assert hit == 0, f"{hit} elements written outside the rows of O (row gaps, rows >= Nq, or the 4 KiB on either side)"
        o = self.obuf[self.g:self.g + self.n].view(B, self.rows, self.o_rs)[:, :Nq, :H * hd]
        return o.contiguous().view(self.dt).reshape(B, Nq, H, hd).cpu()


def check_against_reference(out, ref, keep, dname, hd, what):
    """-> (worst relative error of the random columns over the (batch, head) slices, worst absolute error of the structured columns)."""
    assert bool(torch.isfinite(out.float()).all()), f"{what}: NaN or inf in {int((~torch.isfinite(out.float())).sum())} elements of the rows written"
    o = out.double()
    B = o.shape[0]
    real = A.REAL[hd]
    empty = torch.zeros(B, dtype=torch.bool) if keep is None else ~keep.any(-1)
    if bool(empty.any()):
        assert float(o[empty].abs().max()) == 0.0, f"{what}: a sample without valid keys must come out as exact zeros"
    if real < hd:
        assert float(o[..., real:].abs().max()) == 0.0, f"{what}: columns >= {real} of a padded head must be exactly zero"
    if bool(empty.all()):
        return 0.0, 0.0
    o, r = o[~empty], ref[~empty]
    d = (o - r).abs()
    e_rel = d[..., A.C_RAND:real].amax((1, 3)) / r[..., A.C_RAND:real].abs().amax((1, 3))        # [samples, H]
    e_abs = d[..., :A.C_RAND].amax((1, 3))
    print(f"    {what}: rel {float(e_rel.max()):.3e} abs {float(e_abs.max()):.3e}")
    assert float(e_rel.max()) <= BAR_REL[dname], f"{what}: random columns {e_rel.tolist()} > {BAR_REL[dname]} (per sample with keys, head)"
    assert float(e_abs.max()) <= BAR_ABS[dname], f"{what}: structured columns {e_abs.tolist()} > {BAR_ABS[dname]} (per sample with keys, head)"
    return float(e_rel.max()), float(e_abs.max())


def _id(c):
    return (f"{c['dname']}-hd{c['hd']}-B{c['B']}-H{c['H']}-Nq{c['Nq']}-Nk{c['Nk']}-{c['mask']}{'-kmpad' if c['km_pad'] else ''}-{c['regime']}"
            f"-{c['qkv']}-{c['o']}")


@pytest.mark.parametrize("case", [pytest.param(c, id=_id(c)) for c in A.gpu_grid()])
def test_attention_vs_float64(dev, case):
    from vlatouch import _lib as L
    lib = L.lib()
    dname, hd, B, H, Nq, Nk = case["dname"], case["hd"], case["B"], case["H"], case["Nq"], case["Nk"]
    q, k, v = A.make_inputs(dname, B, H, Nq, Nk, hd, case["regime"], case["seed"])
    keep = A.make_mask(case["mask"], B, Nk)
    ref = A.reference(q, k, v, keep, A.scale_of(hd))
    call = AttnCall(dev, case, q, k, v, keep)
    report = []
    try:
        for knob in A.knobs_of(dname, hd, case["mask"], Nq, case["o"]):
            L.check(lib.vt_tune(9, knob), "vt_tune")
            kern, G, nw = A.route(dname, hd, keep is not None, Nq, Nk, call.o_rs, knob)
            what = f"{kern}{f' G{G}' if G > 1 else ''} {nw}w knob {knob}"
            out = call.call()
            again = call.call()
            assert torch.equal(out.view(call.idt), again.view(call.idt)), f"{what}: two calls differ"
            e_rel, e_abs = check_against_reference(out, ref, keep, dname, hd, what)
            report.append(f"{what} rel {e_rel:.2e} abs {e_abs:.2e}")
    finally:
        L.check(lib.vt_tune(9, 1), "vt_tune")
    print(f"[attn {_id(case)}] " + "; ".join(report))


def test_argument_errors_return_before_any_launch(dev):
    """Misaligned strides, head dimensions and dtypes the launcher does not have, and an empty key sequence: the error code, no launch."""
    from vlatouch import _lib as L
    lib = L.lib()
    B, H, N = 1, 2, 16

    def run(dt, width, masked=False, **over):
        hd, D = width, H * width
        bufs = [torch.zeros(B, N, D, dtype=dt, device=dev) for _ in range(4)]
        km = torch.ones(B, N, dtype=torch.uint8, device=dev)
        p = L.AttnParams()
        p.Q, p.K, p.V, p.O = (t.data_ptr() for t in bufs)
        p.q_bs = p.k_bs = p.v_bs = p.o_bs = N * D
        p.q_rs = p.k_rs = p.v_rs = p.o_rs = D
        p.q_hs = p.k_hs = p.v_hs = hd
        if masked:
            p.kmask, p.km_bs = km.data_ptr(), N
        p.B, p.H, p.Nq, p.Nk = B, H, N, N
        p.scale, p.dtype, p.hd = 0.125, L.dt_code(dt), hd
        for name, val in over.items():
            setattr(p, name, val)
        r = lib.vt_attention(C.byref(p), L.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        return r

    f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
    assert run(f32, 64) == 0 and run(bf16, 64) == 0 and run(f16, 96, masked=True) == 0 and run(bf16, 80) == 0      # the template itself is valid
    for field in ("q_rs", "k_rs", "v_rs", "q_hs", "k_hs", "v_hs"):
        assert run(f32, 64, **{field: 128 + 2}) == VT_ERR_ARG, field         # fp32: multiples of 4 elements
        for dt in (bf16, f16):
            assert run(dt, 64, **{field: 128 + 4}) == VT_ERR_ARG, field      # 16-bit: multiples of 8
    assert run(bf16, 80, masked=True) == VT_ERR_UNSUPPORTED
    assert run(f16, 80, masked=True) == VT_ERR_UNSUPPORTED
    assert run(f32, 80) == VT_ERR_UNSUPPORTED
    assert run(bf16, 64, hd=72) == VT_ERR_UNSUPPORTED and run(f32, 64, hd=72) == VT_ERR_UNSUPPORTED
    for code in (2, 4, -1, 7):
        assert run(bf16, 64, dtype=code) == VT_ERR_UNSUPPORTED, code
    assert run(bf16, 64, Nk=0) == VT_ERR_ARG and run(f32, 64, Nk=0) == VT_ERR_ARG
