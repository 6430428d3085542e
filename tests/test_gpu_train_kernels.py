"""Every kernel of the controller training step (csrc/vt_train.hip, csrc/vt_train_lstm.hip) and the composites of vlatouch/train.py built on
them, as units: each is called twice on output buffers pre-filled with NaN (the two results bit-equal) and compared with the same function in
fp64 on the CPU computed from the same fp32 inputs.

Bars.  Data movement, t_clipped, target_s, the AdamW / EMA kernel variants against each other, second call against first: bit-equal.
vt_gn_mish_bwd, vt_ln_bwd, the LSTM cell backward: 1e-5 of each output's max-abs (test_rmsnorm_bwd / test_headnorm_bwd / test_attention_bwd_fp32).
LSTM cell forward values, vt_posemb: 2e-6 absolute (test_activation_and_derivative, test_small_kernels_twice_and_against_torch).
Everything else that sums or calls libm (the backward products through split-K slabs, vt_si_qsample_ex, vt_si_loss, vt_mse_residual, vt_colsum,
vt_slab_sum, vt_sum_mid): with e_t32 = the max-abs error of fp32 torch on the CPU for the same function against fp64,
bar = max(3 e_t32, 1e-6 max|fp64 result|) — another, equally valid summation order (fixed tree, slabs added in order) rounds like torch's does,
not less; the floor is there because torch's error is exactly 0 for some tiny cases.  `_bar()` prints e_hip, e_t32 and the bar per output.

Measured on an MI355X, worst e_hip / bar per kernel: conv_bwd 0.91 (dw of the final 1x1 at B 8, T 48), linear_bwd 0.70, TrainMLP 0.67, convT 0.45,
vt_si_qsample_ex 0.21, vt_slab_sum 0.17, vt_sum_mid 0.13, vt_si_loss 0.11, vt_mse_residual 0.10, vt_colsum 0.08 (1.50 before its sums were carried
in fp64).  Worst error of the 1e-5 rows: vt_gn_mish_bwd 8.4e-7, gn_fwd -> gn_bwd 1.8e-6, vt_ln_bwd 1.5e-7, LSTM cell backward 1.3e-7 of max-abs; of the
2e-6 rows: LSTM cell forward 2.4e-7, vt_posemb 5.2e-8 (5.1e-5 at t = 998 before its frequencies were rounded once from fp64).  AdamW + EMA, three
steps: worst update error 1.08e-4 / 1.11e-4 of the update's norm, the same as fp32 torch's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases, train_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(autouse=True)
def nan_filled_outputs(monkeypatch):
    """What the wrappers of vlatouch/train.py allocate through `_empty` starts as NaN, so an element a kernel leaves unwritten shows.  Not covered:
    torch.empty_like outputs (gn_bwd's dc, mish / gelu) and what ops.gemm / ops.conv1d_cl allocate; the direct kernel tests fill their own outputs."""
    from vlatouch import train as tt
    monkeypatch.setattr(tt, "_empty", lambda shape, dev: torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev))


def lib():
    from vlatouch import _lib as L
    return L


def sp():
    return lib().stream_ptr(torch.device(DEV))


def P(t):
    return lib().ptr(t)


def dev(*ts):
    """Device copies that the caller keeps in named variables until the launch is queued (a temporary's memory is handed to the next allocation)."""
    return [None if t is None else t.to(DEV) for t in ts]


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def rnd(gen, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=gen) * scale + shift


def biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice(fn):
    """fn() -> tensor or tuple of tensors (CPU copies of freshly NaN-filled device outputs); called twice, bit-equal -> the first result."""
    a, b = fn(), fn()
    ta, tb = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert biteq(x, y), f"output {i}: the second call differs from the first"
    return a


def _bar(tag, what, hip, t32, ref):
    """Assert |hip - ref| <= max(3 |t32 - ref|, 1e-6 max|ref|) (max-abs) and print the figures -> e_hip / bar."""
    ref = ref.double()
    e_hip, e_t32 = float((hip.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
    bar = max(3 * e_t32, 1e-6 * float(ref.abs().max()))
    print(f"[{tag}] {what}: e_hip {e_hip:.2e}, e_t32 {e_t32:.2e}, bar {bar:.2e}, ratio {e_hip / bar if bar else 0.0:.2f}")
    assert np.isfinite(e_hip) and e_hip <= bar, (tag, what, e_hip, e_t32, bar)
    return e_hip / bar if bar else 0.0


def _rel(tag, what, hip, ref, bar):
    """Assert max|hip - ref| <= bar * max|ref| and print the figure."""
    e = R.max_err(hip, ref)
    print(f"[{tag}] {what}: {e:.2e} of max-abs (bar {bar:.0e})")
    assert e <= bar, (tag, what, e)
    return e


# ================================================================================================ data movement: exact
def im2col_ref(x, tout, taps, stride, off0):
    B, tin, cin = x.shape
    out = torch.zeros(taps * cin, B, tout)
    for tap in range(taps):
        for t in range(tout):
            ti = t * stride + off0 + tap
            if 0 <= ti < tin:
                out[tap * cin:(tap + 1) * cin, :, t] = x[:, ti, :].t()
    return out.reshape(taps * cin, B * tout)


def zero_stuff_ref(x):
    B, T, Cc = x.shape
    out = torch.zeros(B, 2 * T, Cc)
    out[:, 0::2] = x
    return out


IM2COL = [(2, T, 16, 5, 1, -2, T) for T in (8, 16, 48)] + [(2, T, 32, 3, 2, -1, T // 2) for T in (8, 16, 48)] + \
         [(2, T, 16, 1, 1, 0, T) for T in (8, 16, 48)] + [(2, T, 32, 4, 1, -2, T) for T in (8, 16, 48)] + [(3, 7, 5, 3, 1, -1, 7)]


@pytest.mark.parametrize("B,Tin,Cin,taps,stride,off0,Tout", IM2COL)
def test_im2col_t(B, Tin, Cin, taps, stride, off0, Tout):
    """Every conv of the net (k5 s1 p2, k3 s2 p1, k1, the transposed conv as k4 s1 off0 -2 over a zero-stuffed input) at T 8 / 16 / 48, and one
    shape with partial 32 x 32 tiles on both axes (B Tout = 21, taps Cin = 15)."""
    from vlatouch import train as tt
    x = rnd(torch.Generator().manual_seed(1), B, Tin, Cin)
    if taps == 4:
        x = zero_stuff_ref(x[:, :Tin // 2])
    got = twice(lambda: tt.im2col_t(x.to(DEV), Tout, taps, stride, off0).cpu())
    assert biteq(got, im2col_ref(x, Tout, taps, stride, off0))


@pytest.mark.parametrize("M,N", [(1, 1), (33, 65), (512, 37)])
def test_transpose(M, N):
    from vlatouch import train as tt
    x = rnd(torch.Generator().manual_seed(2), M, N)
    assert biteq(twice(lambda: tt.transpose(x.to(DEV)).cpu()), x.t().contiguous())


@pytest.mark.parametrize("B,T,Cc", [(1, 1, 1), (3, 6, 40), (2, 24, 512)])
def test_zero_stuff(B, T, Cc):
    from vlatouch import train as tt
    x = rnd(torch.Generator().manual_seed(3), B, T, Cc)
    assert biteq(twice(lambda: tt.zero_stuff(x.to(DEV)).cpu()), zero_stuff_ref(x))


@pytest.mark.parametrize("taps", [1, 3, 4, 5])
def test_wflip(taps):
    from vlatouch import train as tt
    cout, cin = 16, 24
    w = rnd(torch.Generator().manual_seed(4), cout, taps * cin)
    got = twice(lambda: tt.wflip(w.to(DEV), cout, taps, cin).cpu())
    assert biteq(got, w.reshape(cout, taps, cin).flip(1).permute(2, 1, 0).reshape(cin, taps * cout).contiguous())


@pytest.mark.parametrize("accumulate", [False, True])
def test_copy_cols_offsets_pitches_accumulate(accumulate):
    from vlatouch import train as tt
    g = torch.Generator().manual_seed(5)
    rows, cols, off, doff = 37, 24, 8, 16
    src, d0 = rnd(g, rows, 50), (rnd(g, rows, 64) if accumulate else torch.full((rows, 64), NAN))
    want = d0.clone()
    want[:, doff:doff + cols] = d0[:, doff:doff + cols] + src[:, off:off + cols] if accumulate else src[:, off:off + cols]

    def run():
        d = d0.to(DEV)
        tt.copy_cols(src.to(DEV), off, d, doff, cols, accumulate)
        return d.cpu()
    assert biteq(twice(run), want)                       # the columns outside [doff, doff + cols) keep what they held (NaN / the old values)


def test_bcast_mid_leaves_the_other_columns():
    g = torch.Generator().manual_seed(6)
    B, T, Cc, ldd, doff = 3, 5, 40, 100, 48
    src = rnd(g, B, Cc)
    want = torch.full((B * T, ldd), NAN)
    want[:, doff:doff + Cc] = src[:, None, :].expand(B, T, Cc).reshape(B * T, Cc)

    def run():
        d, (sd,) = nans(B * T, ldd), dev(src)
        lib().check(lib().lib().vt_bcast_mid(P(sd), P(d), ldd, doff, B, T, Cc, sp()), "vt_bcast_mid")
        return d.cpu()
    assert biteq(twice(run), want)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 ** 20 + 3])
def test_add_and_mul_in_place(n):
    from vlatouch import train as tt
    g = torch.Generator().manual_seed(7)
    a, b = rnd(g, n), rnd(g, n)

    def mul():
        x, bd = dev(a, b)
        lib().check(lib().lib().vt_mul_(P(x), P(bd), n, sp()), "vt_mul_")
        return x.cpu()
    assert biteq(twice(lambda: tt.add_(a.to(DEV), b.to(DEV)).cpu()), a + b)
    assert biteq(twice(mul), a * b)


# ================================================================================================ reductions and element-wise arithmetic
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("N", [1, 31, 32, 40, 512])
def test_colsum(N, accumulate):
    """Worst e_hip / bar over the grid on an MI355X: 0.08 (M 2048, N 512, accumulate).  With the fp32 tree the kernel had before, M 2048 / N 1 gave
    e_hip 1.01e-5 against e_t32 2.26e-6: 1.50; the sums are now carried in fp64 and rounded once."""
    g = torch.Generator().manual_seed(8)
    worst = 0.0
    for M in (1, 31, 32, 33, 63, 64, 65, 97, 2048):
        ld = N + 3
        x, o0 = rnd(g, M, ld), rnd(g, N)

        def run():
            o, (xd,) = (o0.to(DEV) if accumulate else nans(N)), dev(x)
            lib().check(lib().lib().vt_colsum(P(xd), ld, P(o), M, N, accumulate, sp()), "vt_colsum")
            return o.cpu()
        ref = x[:, :N].double().sum(0) + (o0.double() if accumulate else 0)
        t32 = x[:, :N].sum(0) + o0 if accumulate else x[:, :N].sum(0)
        worst = max(worst, _bar(f"colsum M{M} N{N} ld{ld} acc{accumulate}", "sum", twice(run), t32, ref))
    print(f"[colsum N{N} acc{accumulate}] worst ratio {worst:.2f}")


def test_sum_mid():
    g = torch.Generator().manual_seed(9)
    for B, T, Cc, lds, off in ((3, 5, 40, 100, 48), (4, 16, 256, 512, 256), (2, 1, 7, 9, 2)):
        src = rnd(g, B * T, lds)

        def run():
            o, (sd,) = nans(B, Cc), dev(src)
            lib().check(lib().lib().vt_sum_mid(P(sd), lds, off, P(o), B, T, Cc, sp()), "vt_sum_mid")
            return o.cpu()
        blk = src[:, off:off + Cc].reshape(B, T, Cc)
        _bar(f"sum_mid B{B} T{T} C{Cc} off{off}", "sum", twice(run), blk.sum(1), blk.double().sum(1))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("S", [1, 2, 16])
def test_slab_sum(S, with_bias):
    from vlatouch import train as tt
    g = torch.Generator().manual_seed(10)
    for M, N in ((33, 40), (64, 256)):                  # n = 1320 is not a multiple of the 1024 elements a block takes
        slabs, bias = rnd(g, S, M, N), (rnd(g, N) if with_bias else None)
        got = twice(lambda: tt._slab_sum(slabs.to(DEV), None if bias is None else bias.to(DEV), (M, N)).cpu())
        ref = slabs.double().sum(0) + (bias.double() if with_bias else 0)
        t32 = slabs.sum(0) + bias if with_bias else slabs.sum(0)
        _bar(f"slab_sum S{S} {M}x{N} bias{int(with_bias)}", "sum", got, t32, ref)


@pytest.mark.parametrize("dim", [256, 4])
def test_posemb(dim):
    """The fp64 sinusoid of the fp32 product t f, f the fp32 rounding of exp(-j ln(10000) / (half - 1)); t at the clipped ends, inside, and large (at
    t = 437 one ulp of a frequency is 2.6e-5 of the embedding, so this also pins the frequencies to their correctly rounded values)."""
    t = torch.tensor([0.001, 0.999, 0.5, 0.2503, 3.0, 437.0, 998.0])
    half = dim // 2
    f = torch.from_numpy(np.exp(-np.arange(half, dtype=np.float64) * (np.log(10000.0) / (half - 1))).astype(np.float32))
    a = (t[:, None] * f[None, :]).double()
    ref = torch.cat([a.sin(), a.cos()], dim=-1)

    def run():
        o, (td,) = nans(len(t), dim), dev(t)
        lib().check(lib().lib().vt_posemb(P(td), P(o), len(t), dim, sp()), "vt_posemb")
        return o.cpu()
    got = twice(run)
    e = (got.double() - ref).abs().amax(1)
    e_stmt = float((R.posemb(t[:4], dim, torch.float64) - ref[:4]).abs().max())
    print(f"[posemb dim{dim}] max-abs error per t {dict(zip(t.tolist(), [float(f'{v:.2e}') for v in e.tolist()]))} (bar 2e-6); "
          f"the statement's fp32 table against this one at t <= 1: {e_stmt:.2e}")
    assert float(e.max()) <= 2e-6 and e_stmt <= 2e-6, (e, e_stmt)


@pytest.mark.parametrize("gamma", R.GAMMAS)
@pytest.mark.parametrize("kind", R.INTERPOLANTS)
def test_si_qsample_all_interpolants_and_gammas(kind, gamma):
    from vlatouch.train import _GAMMA, _INTERPOLANT
    g = torch.Generator().manual_seed(11)
    B, per = 6, 160
    x0, x1, z = torch.rand(B, per, generator=g) * 2 - 1, torch.rand(B, per, generator=g) * 2 - 1, rnd(g, B, per, scale=0.03)
    t = torch.tensor([0.0002, 0.9999, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), 0.137, 0.81], dtype=torch.float32)

    def run():
        o = [nans(B, per) for _ in range(4)] + [nans(B)]
        i = dev(x0, x1, z, t)
        lib().check(lib().lib().vt_si_qsample_ex(*[P(v) for v in i], *[P(v) for v in o], B, per, _GAMMA[gamma], 0.001,
                                                 _INTERPOLANT[kind], sp()), "vt_si_qsample_ex")
        return tuple(v.cpu() for v in o)
    xt, tv, ts, tb, tc = twice(run)
    r64, r32 = R.si_targets(x0, x1, z, t, gamma, kind, 0.001, torch.float64), R.si_targets(x0, x1, z, t, gamma, kind, 0.001, torch.float32)
    assert biteq(tc, R.clip_t(t)) and biteq(tc, r64[4]), "t_clipped"
    assert biteq(ts, -z), "target_s"
    tag = f"si_qsample {kind} / {gamma}"
    _bar(tag, "xt", xt, r32[0], r64[0]), _bar(tag, "target_v", tv, r32[1], r64[1]), _bar(tag, "target_b", tb, r32[3], r64[3])


@pytest.mark.parametrize("rows,B,per", [(1, 1, 160), (16, 16, 160), (4, 4, 480), (8, 5, 160)])
def test_si_loss(rows, B, per):
    """(8, 5, 160): B smaller than the buffers' row count — the zero-weight padding contract: rows >= B of dout stay as they were."""
    g = torch.Generator().manual_seed(12)
    o, tgt = rnd(g, rows, per), rnd(g, rows, per)

    def run():
        d, l = nans(rows, per), nans(1)
        od, td = dev(o, tgt)
        lib().check(lib().lib().vt_si_loss(P(od), P(td), P(d), P(l), B, per, sp()), "vt_si_loss")
        return d.cpu(), l.cpu()
    d, l = twice(run)
    f = lambda dt: (torch.mean(0.5 * torch.norm(o[:B].to(dt), dim=-1) ** 2 - torch.sum(tgt[:B].to(dt) * o[:B].to(dt), dim=-1)).reshape(1),
                    (o[:B].to(dt) - tgt[:B].to(dt)) / B)
    (l64, d64), (l32, d32) = f(torch.float64), f(torch.float32)
    assert bool(torch.isnan(d[B:]).all()), "rows >= B of dout were written"
    tag = f"si_loss rows{rows} B{B} per{per}"
    _bar(tag, "loss", l, l32, l64), _bar(tag, "dout", d[:B], d32, d64)


@pytest.mark.parametrize("with_base", [True, False])
@pytest.mark.parametrize("n", [210, 2560])
def test_mse_residual(n, with_base):
    g = torch.Generator().manual_seed(13)
    base, delta, tgt = (rnd(g, n) if with_base else None), rnd(g, n), rnd(g, n)

    def run():
        p, d, l = nans(n), nans(n), nans(1)
        bd, dd, td = dev(base, delta, tgt)
        lib().check(lib().lib().vt_mse_residual(P(bd), P(dd), P(td), P(p), P(d), P(l), n, sp()), "vt_mse_residual")
        return p.cpu(), d.cpu(), l.cpu()
    p, d, l = twice(run)

    def f(dt):
        pr = delta.to(dt) + (base.to(dt) if with_base else 0)
        return pr, 2 * (pr - tgt.to(dt)) / n, F.mse_loss(pr, tgt.to(dt)).reshape(1)
    r64, r32 = f(torch.float64), f(torch.float32)
    tag = f"mse_residual n{n} base{int(with_base)}"
    _bar(tag, "pred", p, r32[0], r64[0]), _bar(tag, "ddelta", d, r32[1], r64[1]), _bar(tag, "loss", l, r32[2], r64[2])


# ---- GroupNorm + Mish + FiLM backward
# channels per group 32, 64, 128 and the limit 256; T that is not a power of two; (2, 31, 2048) is the largest group the guard admits (see the guard test)
GN_SHAPES = [(3, 16, 256), (3, 8, 512), (2, 4, 512), (2, 64, 256), (2, 32, 512), (2, 2, 512), (1, 12, 1024), (2, 3, 2048), (2, 31, 2048)]


def _gn_inputs(B, T, Cc, with_film, seed=14):
    g = torch.Generator().manual_seed(seed)
    c, dout = rnd(g, B, T, Cc, scale=1.3, shift=0.2), rnd(g, B, T, Cc)
    gamma, beta = rnd(g, Cc, scale=0.5, shift=1.0), rnd(g, Cc, scale=0.5)
    gamma[1::37], beta[1::37] = 6.0, 14.0                    # pre-activations 14 +- 6 xhat: on both sides of mish_grad's x > 20 branch
    film = torch.cat([rnd(g, B, Cc, scale=0.3, shift=1.0), rnd(g, B, Cc)], dim=1) if with_film else None
    return c, gamma, beta, film, dout


def _gn_ref(c, gamma, beta, film, dout, dtype=torch.float64):
    """fp64 autograd of scale * mish(group_norm(c)) + bias (8 groups, eps 1e-5) -> out, dc, dgamma, dbeta, dfilm."""
    B, T, Cc = c.shape
    lv = [v.to(dtype).clone().requires_grad_(True) if v is not None else None for v in (c, gamma, beta, film)]
    with torch.enable_grad():
        y = R.mish(F.group_norm(lv[0].movedim(1, 2), 8, lv[1], lv[2], eps=1e-5))
        if film is not None:
            y = lv[3][:, :Cc, None] * y + lv[3][:, Cc:, None]
        y = y.movedim(1, 2)
        (y * dout.to(dtype)).sum().backward()
    return (y.detach(),) + tuple(None if v is None else v.grad for v in lv)


@pytest.mark.parametrize("with_film", [True, False])
@pytest.mark.parametrize("B,T,Cc", GN_SHAPES)
def test_gn_mish_bwd(B, T, Cc, with_film):
    """Worst error over the shapes on an MI355X: 8.4e-7 of max-abs (dc at B 2, T 3, C 2048, no FiLM); bar 1e-5."""
    c, gamma, beta, film, dout = _gn_inputs(B, T, Cc, with_film)
    assert float((c.reshape(B, T, 8, -1).movedim(1, 2).flatten(2).std(-1).min())) > 0.5

    def run():
        dc, dgp, dbp = nans(B, T, Cc), nans(B, Cc), nans(B, Cc)
        dfilm = nans(B, 2 * Cc) if with_film else None
        i = dev(c, gamma, beta, film, dout)
        lib().check(lib().lib().vt_gn_mish_bwd(*[P(v) for v in i], P(dc), P(dgp), P(dbp), P(dfilm), B, T, Cc, 8, 1e-5, sp()), "vt_gn_mish_bwd")
        return (dc.cpu(), dgp.cpu(), dbp.cpu()) + ((dfilm.cpu(),) if with_film else ())
    got = twice(run)
    _, dc, dg, db, dfl = _gn_ref(c, gamma, beta, film, dout)
    tag = f"gn_mish_bwd B{B} T{T} C{Cc} film{int(with_film)}"
    _rel(tag, "dc", got[0], dc, 1e-5), _rel(tag, "sum_b dgamma_part", got[1].double().sum(0), dg, 1e-5)
    _rel(tag, "sum_b dbeta_part", got[2].double().sum(0), db, 1e-5)
    if with_film:
        _rel(tag, "dfilm", got[3], dfl, 1e-5)


def test_gn_mish_bwd_guard_counts_the_static_lds():
    """The kernel holds 2 n floats of dynamic LDS (n = channels per group x T) plus 32 bytes of static LDS (`red[8]`), and the entry point sets no
    hipFuncAttributeMaxDynamicSharedMemorySize: a launch is only certain to be accepted while static + dynamic stay within the 64 KiB a block gets by
    default.  n = 8192 (256 channels per group x 32) is 65536 + 32 bytes, so the guard must refuse it with VT_ERR_UNSUPPORTED before any launch; the
    largest admitted group of that width, 256 x 31, is in GN_SHAPES.  Nothing here depends on a failed launch."""
    from vlatouch._lib import VtError
    print(f"[gn_mish_bwd guard] shared_memory_per_block {torch.cuda.get_device_properties(0).shared_memory_per_block}")
    B, T, Cc = 2, 32, 2048
    c, gamma, beta, film, dout = (v.to(DEV) for v in _gn_inputs(B, T, Cc, True))
    dc, dgp, dbp, dfilm = nans(B, T, Cc), nans(B, Cc), nans(B, Cc), nans(B, 2 * Cc)
    with pytest.raises(VtError, match="LDS"):
        lib().check(lib().lib().vt_gn_mish_bwd(P(c), P(gamma), P(beta), P(film), P(dout), P(dc), P(dgp), P(dbp), P(dfilm), B, T, Cc, 8, 1e-5, sp()), "vt_gn_mish_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dc).all()) and bool(torch.isnan(dfilm).all())


@pytest.mark.parametrize("Cc", [64, 128, 256, 384, 100])
def test_ln_bwd(Cc):
    """C = 100 is not a multiple of the 64 lanes; rows that are not a multiple of the 4 rows a block takes."""
    g = torch.Generator().manual_seed(15)
    for rows in (1, 3, 4, 5, 37, 4096):
        x, dy, gamma = rnd(g, rows, Cc, scale=1.3, shift=0.2), rnd(g, rows, Cc), rnd(g, Cc, scale=0.5, shift=1.0)

        def run():
            from vlatouch import train as tt
            dx, dyxh = nans(rows, Cc), nans(rows, Cc)
            xd, gd, dyd = dev(x, gamma, dy)
            lib().check(lib().lib().vt_ln_bwd(P(xd), P(gd), P(dyd), P(dx), P(dyxh), rows, Cc, 1e-5, sp()), "vt_ln_bwd")
            return dx.cpu(), tt.colsum(dyxh).cpu(), tt.colsum(dyd).cpu()
        dx, dg, db = twice(run)
        lv = [v.double().clone().requires_grad_(True) for v in (x, gamma, torch.zeros(Cc))]
        with torch.enable_grad():
            (F.layer_norm(lv[0], (Cc,), lv[1], lv[2], 1e-5) * dy.double()).sum().backward()
        tag = f"ln_bwd rows{rows} C{Cc}"
        _rel(tag, "dx", dx, lv[0].grad, 1e-5), _rel(tag, "colsum dyxh", dg, lv[1].grad, 1e-5), _rel(tag, "colsum dy", db, lv[2].grad, 1e-5)


@pytest.mark.parametrize("B,T,H", [(4, 1, 128), (4, 7, 256), (8, 16, 384), (3, 5, 100)])
def test_lstm_cell_fwd_bwd(B, T, H):
    """The two cell kernels driven over t = 0 .. T-1 and back.  The recurrent products (h W_hh^T forward, dgates W_hh backward) are done in fp64 on
    the host from the kernels' own outputs and rounded, so only the element-wise kernels are under test.  Every buffer, the in/out dc_next included,
    starts as NaN: the last tick must not read dc_next, the first must write hprev[:, 0] = 0."""
    g = torch.Generator().manual_seed(16)
    gx, whh, dhseq = rnd(g, B, T, 4 * H), rnd(g, 4 * H, H, scale=H ** -0.5), rnd(g, B, T, H)
    L_ = lib().lib()

    def run():
        act, cseq, hseq, hprev, hcur = nans(B, T, 4 * H), nans(B, T, H), nans(B, T, H), nans(B, T, H), nans(B, H)
        gxd, dhd, gh = gx.to(DEV), dhseq.to(DEV), None
        for t in range(T):
            if t > 0:
                gh = (hcur.cpu().double() @ whh.double().t()).float().to(DEV)
            lib().check(L_.vt_lstm_cell_fwd(P(gxd), P(gh), P(act), P(cseq), P(hseq), P(hprev), P(hcur), B, T, H, t, sp()), "vt_lstm_cell_fwd")
        dgates, dgcur, dc = nans(B, T, 4 * H), nans(B, 4 * H), nans(B, H)
        dh_rec = None
        for t in range(T - 1, -1, -1):
            lib().check(L_.vt_lstm_cell_bwd(P(dhd), P(dh_rec), P(act), P(cseq), P(dc), P(dgates), P(dgcur), B, T, H, t, sp()), "vt_lstm_cell_bwd")
            if t > 0:
                dh_rec = (dgcur.cpu().double() @ whh.double()).float().to(DEV)
        return tuple(v.cpu() for v in (act, cseq, hseq, hprev, hcur, dgates, dgcur, dc))
    act, cseq, hseq, hprev, hcur, dgates, dgcur, dc = twice(run)
    a64, c0 = gx.double().clone().requires_grad_(True), torch.zeros(B, H, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        h, c, hs, cs, acts = torch.zeros(B, H, dtype=torch.float64), c0, [], [], []
        for t in range(T):
            i, f, gg, o = (a64[:, t] + h @ whh.double().t()).chunk(4, dim=-1)
            i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
            c = f * c + i * gg
            h = o * torch.tanh(c)
            hs.append(h), cs.append(c), acts.append(torch.cat([i, f, gg, o], dim=-1))
        hs, cs, acts = torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(acts, 1)
        (hs * dhseq.double()).sum().backward()
    tag = f"lstm_cell B{B} T{T} H{H}"
    hp = torch.cat([torch.zeros(B, 1, H, dtype=torch.float64), hs.detach()[:, :-1]], dim=1)
    for what, got, ref in (("act", act, acts.detach()), ("cseq", cseq, cs.detach()), ("hseq", hseq, hs.detach()), ("hprev", hprev, hp), ("hcur", hcur, hs.detach()[:, -1])):
        e = float((got.double() - ref).abs().max())
        print(f"[{tag}] {what}: {e:.2e} abs (bar 2e-6)")
        assert e <= 2e-6, (tag, what, e)
    assert float(hprev[:, 0].abs().max()) == 0.0 and biteq(hcur, hseq[:, -1]) and biteq(hprev[:, 1:], hseq[:, :-1])
    _rel(tag, "dgates", dgates, a64.grad, 1e-5), _rel(tag, "dgcur", dgcur, a64.grad[:, 0], 1e-5), _rel(tag, "dc_next", dc, c0.grad, 1e-5)
    assert biteq(dgcur, dgates[:, 0])


# ================================================================================================ optimizer kernels
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, ema=0.75)
GUARD = 8
SENTINEL = 12345.0


def _opt_state(sizes, seed=17):
    g = torch.Generator().manual_seed(seed)
    p0 = [rnd(g, n) for n in sizes]
    grads = [[rnd(g, n, scale=0.1) * (torch.rand(n, generator=g) > 0.1) for n in sizes] for _ in range(3)]       # some exactly-zero gradients
    return p0, grads


def _padded(t):
    """[values | GUARD sentinel words] on the device."""
    return torch.cat([t, torch.full((GUARD,), SENTINEL)]).to(DEV)


def _run_optimizer(variant, sizes, shadowed, p0, grads):
    """Three AdamW + EMA steps through one of the three kernel families -> (params, shadows, moments) per tensor on the CPU, guard words included."""
    L_, hp = lib().lib(), HP
    p, m, v = [_padded(x) for x in p0], [_padded(torch.zeros(n)) for n in sizes], [_padded(torch.zeros(n)) for n in sizes]
    sh = [_padded(x) if s else None for x, s in zip(p0, shadowed)]
    hyper_host = torch.zeros(4)
    for step in (1, 2, 3):
        gs = [x.to(DEV) for x in grads[step - 1]]
        dec = min(hp["ema"], (1 + step) / (10 + step))
        lib().check(L_.vt_train_hyper(hp["lr"], hp["b1"], hp["b2"], step, dec, P(hyper_host)), "vt_train_hyper")
        hyper = hyper_host.to(DEV)
        if variant == "scalar":
            for i, n in enumerate(sizes):
                lib().check(L_.vt_adamw(P(p[i]), P(gs[i]), P(m[i]), P(v[i]), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, sp()), "vt_adamw")
                if sh[i] is not None:
                    lib().check(L_.vt_ema_update(P(sh[i]), P(p[i]), n, dec, sp()), "vt_ema_update")
        elif variant == "dev":
            for i, n in enumerate(sizes):
                lib().check(L_.vt_adamw_dev(P(p[i]), P(gs[i]), P(m[i]), P(v[i]), n, P(hyper), hp["b1"], hp["b2"], hp["eps"], hp["wd"], sp()), "vt_adamw_dev")
                if sh[i] is not None:
                    lib().check(L_.vt_ema_update_dev(P(sh[i]), P(p[i]), n, P(hyper), sp()), "vt_ema_update_dev")
        else:
            rows, chunk0 = [], 0
            for i, n in enumerate(sizes):
                rows.append([p[i].data_ptr(), gs[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), 0 if sh[i] is None else sh[i].data_ptr(), n, chunk0])
                chunk0 += (n + 4095) // 4096
            tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
            lib().check(L_.vt_adamw_ema_multi(P(tab), len(rows), chunk0, P(hyper), hp["b1"], hp["b2"], hp["eps"], hp["wd"], sp()), "vt_adamw_ema_multi")
        torch.cuda.synchronize()
    c = lambda xs: [None if x is None else x.cpu() for x in xs]
    return c(p), c(sh), c(m), c(v)


def test_adamw_ema_kernel_families_are_bit_equal_and_match_fp64():
    """vt_adamw / vt_adamw_dev (+ vt_train_hyper) / vt_adamw_ema_multi and vt_ema_update / vt_ema_update_dev / the table kernel's EMA on the same data
    over three steps: bit-equal (csrc/vt_train.hip switches contraction off for this).  The table holds tensors on both sides of the 4096-element chunk,
    some without a shadow; the guard words behind every buffer stay untouched (the chunk search and the `i >= e.n` cut).  Against AdamW + EMA in fp64:
    the update p_3 - p_0 per tensor relative to the fp64 update's norm, worst tensor at most 5 x the worst tensor of fp32 torch on the CPU."""
    sizes = [1, 255, 4095, 4096, 4097, 3 * 4096, 70001]
    shadowed = [True, False, True, True, False, True, True]
    p0, grads = _opt_state(sizes)
    runs = {k: _run_optimizer(k.split()[0], sizes, shadowed, p0, grads) for k in ("scalar", "dev", "table", "scalar again", "table again")}
    a = runs["scalar"]
    for k in ("dev", "table", "scalar again", "table again"):
        for what, xa, xb in zip(("param", "shadow", "m", "v"), a, runs[k]):
            for i, (x, y) in enumerate(zip(xa, xb)):
                assert (x is None and y is None) or biteq(x, y), (k, what, sizes[i])
    for what, xs in zip(("param", "shadow", "m", "v"), runs["table"]):
        for i, x in enumerate(xs):
            assert x is None or bool((x[sizes[i]:] == SENTINEL).all()), ("guard words", what, sizes[i])
    names = [f"t{n}" for n in sizes]
    kw = dict(lr=HP["lr"], wd=HP["wd"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], ema_decay=HP["ema"], ema_keys=[k for k, s in zip(names, shadowed) if s])
    gl = [dict(zip(names, gs)) for gs in grads]
    r64 = R.adamw_ema_steps(dict(zip(names, p0)), gl, dtype=torch.float64, **kw)[-1]
    r32 = R.adamw_ema_steps(dict(zip(names, p0)), gl, dtype=torch.float32, **kw)[-1]
    P0 = {k: v.double() for k, v in zip(names, p0)}
    hip_p = {k: x[:n] for k, x, n in zip(names, a[0], sizes)}
    hip_e = {k: x[:n] for k, x, n in zip(names, a[1], sizes) if x is not None}
    worst = lambda got, ref: max(R.rel_err(got[k].double() - P0[k], ref[k] - P0[k]) for k in ref)
    wp, bp, we, be = worst(hip_p, r64["params"]), worst(r32["params"], r64["params"]), worst(hip_e, r64["ema"]), worst(r32["ema"], r64["ema"])
    print(f"[adamw_ema 3 steps] worst update error: params HIP {wp:.2e} / fp32 torch {bp:.2e}; EMA HIP {we:.2e} / fp32 torch {be:.2e} (bar 5 x fp32 torch)")
    assert wp <= 5 * bp and we <= 5 * be, (wp, bp, we, be)


# ================================================================================================ composites of vlatouch/train.py
# (Cin, Cout, k, stride) of every convolution of the net: the k5 blocks, the 1x1 residual convs, the k3 s2 downsamples, the final 1x1
NET_CONVS = [(16, 256, 5, 1), (256, 256, 5, 1), (256, 512, 5, 1), (512, 512, 5, 1), (1024, 512, 5, 1), (1024, 256, 5, 1),
             (16, 256, 1, 1), (256, 512, 1, 1), (1024, 512, 1, 1), (1024, 256, 1, 1), (256, 256, 3, 2), (512, 512, 3, 2), (256, 16, 1, 1)]
CONV_BT = [(4, 4), (4, 16), (16, 16), (8, 48), (128, 4)]
# `_splits` only returns 16 for a reduction of >= 4096 rows over < 64 output tiles: the weight gradients of the narrow convs (first block, 1x1 input
# residual, final 1x1) once B T reaches 4096; the net has no data-gradient product that long (k Cout <= 2560 gives at most 8)
CONV_CASES = [c + bt for c in NET_CONVS for bt in CONV_BT] + [c + (256, 16) for c in ((16, 256, 5, 1), (16, 256, 1, 1), (256, 16, 1, 1))]


def _conv_splits(cin, cout, k, stride, B, T):
    """Split-K factors `_splits` picks for the weight-gradient and the data-gradient product of conv_bwd."""
    from vlatouch.train import _splits
    tout = T // stride
    return _splits(cout, k * cin, B * tout), _splits(B * T, cin, k * cout)


def test_conv_bwd_grid_reaches_every_split_factor():
    seen = set()
    for case in CONV_CASES:
        seen.update(_conv_splits(*case))
    assert seen == {1, 2, 4, 8, 16}, seen
    assert _conv_splits(1024, 512, 5, 1, 4, 4) == (1, 8) and _conv_splits(256, 16, 1, 1, 256, 16)[0] == 16


def _pack(w):                                   # [Cout][Cin][k] -> tap-major [Cout][k * Cin]
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def _conv_ref(x, w, b, dy, stride, pad, dtype):
    lv = [v.to(dtype).clone().requires_grad_(True) for v in (x, w, b)]
    with torch.enable_grad():
        y = F.conv1d(lv[0].movedim(1, 2), lv[1], lv[2], stride=stride, padding=pad).movedim(1, 2)
        (y * dy.to(dtype)).sum().backward()
    return y.detach(), lv[0].grad, lv[1].grad, lv[2].grad


@pytest.mark.parametrize("cin,cout,k,stride,B,T", CONV_CASES)
def test_conv_bwd(cin, cout, k, stride, B, T):
    """dx, dw, db of conv_bwd against fp64 autograd of F.conv1d.  Worst e_hip / bar on an MI355X: 0.91 (dw of (256, 16, 1, 1) at B 8, T 48: e_hip
    7.2e-5, e_t32 1.25e-5); the 1x1 weight gradients at B T = 384 sit at 0.66 .. 0.91, everything else below 0.8."""
    from vlatouch import train as tt
    g = torch.Generator().manual_seed(18)
    pad, tout = k // 2, T // stride
    x, w, b, dy = rnd(g, B, T, cin), rnd(g, cout, cin, k, scale=(cin * k) ** -0.5), rnd(g, cout), rnd(g, B, tout, cout)
    sw, sx = _conv_splits(cin, cout, k, stride, B, T)
    tag = f"conv_bwd ci{cin} co{cout} k{k} s{stride} B{B} T{T}"
    print(f"[{tag}] split-K: weight gradient {sw}, data gradient {sx}")
    got = twice(lambda: tuple(v.cpu() for v in tt.conv_bwd(x.to(DEV), _pack(w).to(DEV), dy.to(DEV), k, stride, pad)))
    r64, r32 = _conv_ref(x, w, b, dy, stride, pad, torch.float64), _conv_ref(x, w, b, dy, stride, pad, torch.float32)
    _bar(tag, "dx", got[0], r32[1], r64[1]), _bar(tag, "dw", got[1], _pack(r32[2]), _pack(r64[2])), _bar(tag, "db", got[2], r32[3], r64[3])


@pytest.mark.parametrize("T", [2, 4, 12, 32])
@pytest.mark.parametrize("ch", [512, 256])
def test_convT_fwd_bwd(ch, T):
    from vlatouch import train as tt
    g = torch.Generator().manual_seed(19)
    B = 4
    x, w, b, dy = rnd(g, B, T, ch), rnd(g, ch, ch, 4, scale=(ch * 4) ** -0.5), rnd(g, ch), rnd(g, B, 2 * T, ch)
    wc = tt._pack_convT(w)

    def run():
        y, xz = tt.convT_fwd(x.to(DEV), wc.to(DEV), b.to(DEV))
        dx, dwc, db = tt.convT_bwd(xz, wc.to(DEV), dy.to(DEV), ch)
        return y.cpu(), dx.cpu(), tt._unpack_convT(dwc.cpu(), ch), db.cpu()
    got = twice(run)

    def ref(dtype):
        lv = [v.to(dtype).clone().requires_grad_(True) for v in (x, w, b)]
        with torch.enable_grad():
            y = F.conv_transpose1d(lv[0].movedim(1, 2), lv[1], lv[2], stride=2, padding=1).movedim(1, 2)
            (y * dy.to(dtype)).sum().backward()
        return y.detach(), lv[0].grad, lv[1].grad, lv[2].grad
    r64, r32 = ref(torch.float64), ref(torch.float32)
    tag = f"convT ch{ch} B{B} T{T}"
    for i, what in enumerate(("y", "dx", "dw", "db")):
        _bar(tag, what, got[i], r32[i], r64[i])


@pytest.mark.parametrize("B", [4, 16, 128])
def test_linear_bwd(B):
    from vlatouch import train as tt
    g = torch.Generator().manual_seed(20)
    for K, N in ((256, 256), (512, 10752), (784, 256)):
        x, w, dy = rnd(g, B, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, B, N)
        got = twice(lambda: tuple(v.cpu() for v in tt.linear_bwd(x.to(DEV), w.to(DEV), dy.to(DEV))))
        f = lambda dt: (dy.to(dt) @ w.to(dt), dy.to(dt).t() @ x.to(dt), dy.to(dt).sum(0))
        r64, r32 = f(torch.float64), f(torch.float32)
        tag = f"linear_bwd B{B} K{K} N{N}"
        for i, what in enumerate(("dx", "dw", "db")):
            _bar(tag, what, got[i], r32[i], r64[i])


@pytest.mark.parametrize("B", [4, 16, 128])
@pytest.mark.parametrize("which", ["state_encoder", "force_encoder"])
def test_train_mlp_fwd_bwd(which, B):
    """781 -> 256 -> 256 -> 256 (K padded to 784) and the LSTM head's force encoder 3 -> 128 -> 128 (K padded to 16): forward, input gradient and
    every parameter gradient; the padded first-layer columns of the packed weight gradient are exactly zero."""
    from vlatouch.train import TrainMLP
    sd = cases.state_encoder_sd(781) if which == "state_encoder" else cases.lstm_mods()["force_encoder"]
    g = torch.Generator().manual_seed(21)
    kin, nout = sd["0.weight"].shape[1], sd[f"{max(int(k.split('.')[0]) for k in sd)}.weight"].shape[0]
    x, dy = rnd(g, B, kin), rnd(g, B, nout)

    def run():
        m = TrainMLP(sd, DEV)
        y = m.forward(x.to(DEV))
        dx = m.backward(dy.to(DEV))
        assert float(m.g["0.weight"][:, kin:].abs().max()) == 0.0 if m.kpad > kin else True, "padded weight-gradient columns"
        return (y.cpu(), dx.cpu()[:, :kin].contiguous()) + tuple(m.grads()[k] for k in sd)
    got = twice(run)

    def ref(dtype):
        lv, xi = R.leaf_sd(sd, dtype), x.to(dtype).clone().requires_grad_(True)
        with torch.enable_grad():
            y = R.mlp_gelu(lv, xi)
            (y * dy.to(dtype)).sum().backward()
        return (y.detach(), xi.grad) + tuple(lv[k].grad for k in sd)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    tag = f"TrainMLP {which} B{B}"
    for i, what in enumerate(["y", "dx"] + list(sd)):
        _bar(tag, what, got[i], r32[i], r64[i])


@pytest.mark.parametrize("with_film", [True, False])
@pytest.mark.parametrize("B,T,Cc", [(4, 16, 256), (4, 12, 512), (3, 4, 512)])
def test_gn_fwd_bwd_round_trip(B, T, Cc, with_film):
    """gn_fwd -> gn_bwd at the trainer's 8 groups: the forward at the bar tests/test_gpu_primitives.py holds vt_groupnorm to (2e-5 of the norm), the
    backward outputs (the B partials already column-summed on the device) at 1e-5 of max-abs."""
    from vlatouch import train as tt
    c, gamma, beta, film, dout = _gn_inputs(B, T, Cc, with_film, seed=22)

    def run():
        d = lambda v: None if v is None else v.to(DEV)
        y = tt.gn_fwd(d(c), d(gamma), d(beta), film=d(film))
        dc, dg, db, dfl = tt.gn_bwd(d(c), d(gamma), d(beta), d(film), d(dout))
        return (y.cpu(), dc.cpu(), dg.cpu(), db.cpu()) + ((dfl.cpu(),) if with_film else ())
    got = twice(run)
    ref = _gn_ref(c, gamma, beta, film, dout)
    tag = f"gn round trip B{B} T{T} C{Cc} film{int(with_film)}"
    e = R.rel_err(got[0], ref[0])
    print(f"[{tag}] forward: {e:.2e} of the norm (bar 2e-5)")
    assert e < 2e-5
    for i, what in enumerate(("dc", "dgamma", "dbeta", "dfilm")[:len(got) - 1], 1):
        _rel(tag, what, got[i], ref[i], 1e-5)
