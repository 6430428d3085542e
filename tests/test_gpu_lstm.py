"""Every instantiation of the LSTM residual head's persistent kernel (csrc/vt_lstm.hip: 3 arithmetic modes x 11 (hidden, layers) pairs) and
the edges of its I/O widths (state_dim 1..16, force_dim 1..32) and of its 16-row blocks, against the float64 statement of tests/lstm_ref.py.

The measure is max|got - ref| over out, h and c.  The bars are those of tests/test_gpu_api.py::test_lstm_persistent_kernel_ragged_batches_vs_oracle
(fp32 2e-5, x3 1e-4, bf16 3e-2), here against float64; the bf16 mode is compared on the bf16-rounded weight matrices, so its bar measures the
rounding of the activations alone.  tests/test_lstm_ref_host.py shows that each planted mistake of lstm_ref.MISTAKES moves the result by at
least 0.1 on every case: 3.3 x the bf16 bar, 1000 x the x3 bar.

Measured on the MI355X (largest over the 22 cases; every case passed):

  mode   largest    bar     case
  fp32   1.90e-6    2e-5    h384l3-s10f3-b19t5, out       (10.5 x under its bar: every case is more than 10 x under)
  x3     3.93e-5    1e-4    h128l1-s1f1-b19t5, c          (out at most 1.92e-5, h128l1-s10f3)
  bf16   1.09e-2    3e-2    h256l3-s10f3-b19t5, c         (out at most 6.77e-3, h384l2-s10f3)
  saturated gates (LSTM matrices x 3.5, two ticks): fp32 2.29e-6, x3 7.11e-5, both on c; x 40: finite, max|h| 0.9958956 = tanh(max|c| 3.114)

Checked by hand: with two gate tiles swapped in LstmEngine's packer, or with vla_n staged one LDS column off in the kernel, every parity and
saturated-gate test fails.

Beside parity: a T-tick launch is bit-equal to two launches of ceil(T/2) and floor(T/2) ticks with the carried state (the cases with T > 1; a
zero-tick launch is refused, so T = 1 has no split); a row of a 19-row batch is bit-equal to the same row run alone; nothing is stored
behind layers x B x H of h and c or B x T x S of out; saturated gates; and every refusal of vt_lstm_create and LstmEngine."""
import ctypes as C

import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
SENTINEL, GUARD = -7777.25, 4096
CASE_MODES = [pytest.param(c, m, id=f"{m}-{c.id}") for c in R.CASES for m in R.MODES]
_engines = {}


def engine(case, mode, mods=None, key=None):
    """One LstmEngine per (weights, mode): packing on the host is most of a test's time, and cases that differ in (B, T) alone share weights."""
    from vlatouch.engine import LstmEngine
    k = (case.hidden, case.layers, case.S, case.F, mode, key)
    if k not in _engines:
        _engines[k] = LstmEngine(mods or R.case_mods(case), state_dim=case.S, hidden=case.hidden, layers=case.layers, force_dim=case.F,
                                 precision=mode, device=DEV)
    return _engines[k]


def run(eng, i, rows=slice(None), ticks=slice(None), state=None):
    """eng.sequence on batch rows `rows` and ticks `ticks` of the inputs `i`, from `state` (default: the case's h0, c0): (out, h, c) on the device."""
    h, c = state if state is not None else (i["h0"][:, rows].to(DEV).contiguous(), i["c0"][:, rows].to(DEV).contiguous())
    out = eng.sequence(i["obs_cond"][rows], i["vla_n"][rows, ticks], i["force"][rows, ticks], h, c)
    torch.cuda.synchronize()
    return out, h, c


_results = {}


def result(case, mode):
    """The whole case in one launch, computed once per (case, mode) and left unchanged."""
    if (case, mode) not in _results:
        _results[case, mode] = run(engine(case, mode), R.inputs(case))
    return _results[case, mode]


@pytest.mark.parametrize("case,mode", CASE_MODES)
def test_parity_vs_fp64(case, mode):
    out, h, c = result(case, mode)
    ref = R.case_reference(case, "bf16" if mode == "bf16" else "fp32")
    assert out.shape == (case.B, case.T, case.S) and h.shape == c.shape == (case.layers, case.B, case.hidden)
    errs = [R.max_err(g, r) for g, r in zip((out, h, c), ref)]
    print(f"lstm-parity {mode} {case.id}: out {errs[0]:.2e} h {errs[1]:.2e} c {errs[2]:.2e} (bar {R.BARS[mode]:g})")
    assert max(errs) < R.BARS[mode], errs


@pytest.mark.parametrize("case,mode", [p for p in CASE_MODES if p.values[0].T > 1])
def test_one_launch_equals_two(case, mode):
    eng, i = engine(case, mode), R.inputs(case)
    out, h, c = result(case, mode)
    k = (case.T + 1) // 2
    o1, h2, c2 = run(eng, i, ticks=slice(0, k))
    o2, h2, c2 = run(eng, i, ticks=slice(k, case.T), state=(h2, c2))
    assert torch.equal(torch.cat((o1, o2), dim=1), out) and torch.equal(h2, h) and torch.equal(c2, c)


@pytest.mark.parametrize("case", R.PAIR_CASES, ids=lambda c: c.id)
def test_rows_are_independent(case):
    """A batch row is one MFMA column and shares nothing with its neighbours: rows 0 and 15 (the ends of the full block), 16 and 18 (the ends of
    the ragged one) equal the same row run alone, where all 16 columns of the block stand for it."""
    eng, i = engine(case, "x3"), R.inputs(case)
    out, h, c = result(case, "x3")
    for r in (0, 15, 16, 18):
        o1, h1, c1 = run(eng, i, rows=slice(r, r + 1))
        assert torch.equal(o1[0], out[r]) and torch.equal(h1[:, 0], h[:, r]) and torch.equal(c1[:, 0], c[:, r]), r


@pytest.mark.parametrize("case,mode", [p for p in CASE_MODES if p.values[0].B == 19])
def test_nothing_written_past_the_batch(case, mode):
    """vt_lstm_sequence on buffers with a guard of sentinels behind them: the 13 clamped rows of the ragged block are computed and never stored,
    and columns S..15 of the output tile are not stored either.  The live part is poisoned first and equals the engine's own call afterwards."""
    from vlatouch import _lib as L
    eng, i = engine(case, mode), R.inputs(case)
    H, Ly, S, F, B, T = case
    dev = lambda t: t.to(DEV).contiguous()
    obs, vla, force = dev(i["obs_cond"]), dev(i["vla_n"]), dev(i["force"])

    def guarded(live):
        buf = torch.full((live.numel() + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        buf[:live.numel()] = live.flatten()
        return buf
    nst, nout = Ly * B * H, B * T * S
    hb, cb = guarded(dev(i["h0"])), guarded(dev(i["c0"]))
    ob = guarded(torch.full((nout,), float("nan")))
    L.check(L.lib().vt_lstm_sequence(eng._h, L.ptr(obs), L.ptr(vla), L.ptr(force), L.ptr(hb), L.ptr(cb), L.ptr(ob), B, T, L.stream_ptr(torch.device(DEV))),
            "vt_lstm_sequence")
    torch.cuda.synchronize()
    for name, buf, n in (("h", hb, nst), ("c", cb, nst), ("out", ob, nout)):
        assert bool((buf[n:] == SENTINEL).all()), f"{name}: written behind its {n} elements"
    out, h, c = result(case, mode)
    assert torch.equal(ob[:nout], out.flatten()) and torch.equal(hb[:nst], h.flatten()) and torch.equal(cb[:nst], c.flatten())


@pytest.mark.parametrize("mode", ["fp32", "x3"])
def test_saturated_gates(mode):
    """The fast_exp / rcp forms of sigmoid and tanh at both tails: inside the bars at the scale the fp32 oracle itself resolves (lstm_ref.SATURATED),
    and finite with |h| <= 1 at 40 x, where pre-activations reach +-80."""
    case, i = R.SATURATED, R.inputs(R.SATURATED)
    m = R.scaled(R.case_mods(case), R.SATURATED_SCALE)
    got = run(engine(case, mode, m, key="saturated"), i)
    ref = R.reference(m, i["obs_cond"], i["vla_n"], i["force"], i["h0"], i["c0"], case.layers)
    errs = [R.max_err(g, r) for g, r in zip(got, ref)]
    print(f"lstm-saturated {mode} x{R.SATURATED_SCALE:g}: out {errs[0]:.2e} h {errs[1]:.2e} c {errs[2]:.2e} (bar {R.BARS[mode]:g})")
    assert max(errs) < R.BARS[mode], errs
    out, h, c = run(engine(case, mode, R.scaled(R.case_mods(case), R.SATURATED_TAIL_SCALE), key="tail"), i)
    assert all(bool(torch.isfinite(t).all()) for t in (out, h, c))
    print(f"lstm-saturated {mode} x{R.SATURATED_TAIL_SCALE:g}: max|h| {float(h.abs().max()):.7f} max|c| {float(c.abs().max()):.3f}")
    assert float(h.abs().max()) <= 1.0 + 1e-6


def _create(hidden=256, layers=2, state_dim=10, force_dim=3, cdt=0):
    """vt_lstm_create on a descriptor alone (create stores the weight pointers and reads none of them): (code, handle)."""
    from vlatouch import _lib as L
    from vlatouch.engine import _pad_to
    lib = L.lib()
    desc = L.LstmDesc()
    desc.state_dim, desc.hidden, desc.layers, desc.force_dim, desc.force_pad, desc.in_pad, desc.cdt = \
        state_dim, hidden, layers, force_dim, _pad_to(max(force_dim, 1)), _pad_to(hidden // 2 + max(state_dim, 1)), cdt
    n = lib.vt_lstm_num_weights(C.byref(desc))
    dummy = torch.zeros(64, device=DEV)
    handle = C.c_void_p()
    code = lib.vt_lstm_create(C.byref(desc), L.ptr_array([dummy] * max(n, 1)), n, C.byref(handle))
    return code, handle


@pytest.mark.parametrize("bad", [dict(hidden=64), dict(hidden=200), dict(hidden=512), dict(layers=0), dict(layers=5), dict(hidden=384, layers=4),
                                 dict(state_dim=0), dict(state_dim=17), dict(force_dim=0), dict(force_dim=33), dict(cdt=3), dict(cdt=7)],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_create_refuses(bad):
    from vlatouch import _lib as L
    code, handle = _create(**bad)
    assert code != 0 and not handle.value, (bad, code)
    assert b"vt_lstm_create" in L.lib().vt_last_error()


def test_create_accepts_every_instantiation():
    """The control of test_create_refuses: the same call succeeds on all 33 (mode, hidden, layers) and on the width extremes."""
    from vlatouch import _lib as L
    ok = [dict(hidden=c.hidden, layers=c.layers, cdt=cdt) for c in R.PAIR_CASES for cdt in (L.F32, L.F32X3, L.BF16)]
    ok += [dict(state_dim=1, force_dim=1), dict(state_dim=16, force_dim=32)]
    assert len(ok) == 35
    for d in ok:
        code, handle = _create(**d)
        assert code == 0 and handle.value, d
        L.lib().vt_lstm_destroy(handle)


@pytest.mark.parametrize("bad,names", [(dict(force_dim=33), "force_dim must be 1..32"), (dict(force_dim=0), "force_dim must be 1..32"),
                                       (dict(layers=0), "layers must be 1..4"), (dict(layers=5), "layers must be 1..4"),
                                       (dict(hidden=384, layers=4), "384 with 4 layers"), (dict(state_dim=17), "state_dim must be 1..16"),
                                       (dict(state_dim=0), "state_dim must be 1..16"), (dict(hidden=200), "hidden_dim must be 128, 256 or 384")],
                         ids=["force_dim33", "force_dim0", "layers0", "layers5", "hidden384-layers4", "state_dim17", "state_dim0", "hidden200"])
def test_engine_names_the_limit(bad, names):
    """LstmEngine refuses before it packs: a VtError that names the limit, not a shape error out of the packer."""
    from vlatouch import _lib as L
    from vlatouch.engine import LstmEngine
    kw = dict(hidden=256, layers=2, state_dim=10, force_dim=3)
    kw.update(bad)
    mods = R.mods(kw["hidden"] if kw["hidden"] in (128, 256, 384) else 256, min(max(kw["layers"], 1), 4), min(max(kw["state_dim"], 1), 16),
                  kw["force_dim"] if kw["force_dim"] > 0 else 1)
    with pytest.raises(L.VtError, match=names):
        LstmEngine(mods, precision="fp32", device=DEV, **kw)
