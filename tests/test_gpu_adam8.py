"""Block-wise 8-bit AdamW on the device (csrc/vt_adam8.hip, `RdtTrainer(optimizer="adamw8bit")`) against the numpy statement of DESIGN.md §8
(tests/adam8_ref.py) and against the 32-bit step (vt_adamw_ema_multi).

Kernel level, one table of tensors of 1 .. 70 001 elements placed twice (every tensor once on 16-byte-aligned and once on unaligned bases, guard
words around every p / shadow / code / scale buffer; the reference does not depend on the placement and is computed once): step 1 from the zero
state and the sub-4096 tensors over three steps bit-equal to vt_adamw_ema_multi; steps 2 and 3 from the reference's uploaded state: scales
bit-equal, codes equal up to ratios within 2^-20 of a boundary, p / shadow within max(3 x the fp32 reference's own error against fp64, 1e-6 of
max-abs); three chained steps: moments within one code step; two runs bit-equal, guards intact.  Every buffer of the step kernel is read before
it is written, so there is no output to pre-fill with NaN there; vt_adam8_quantize / vt_adam8_dequantize write theirs over NaN / 0xFF fills.
Trainer level on RDT_TINY (fp32 / bf16, k = 1 / 4): first step bit-equal to the "adamw" trainer, exact resume, refusal of the other optimizer's
checkpoint, state size, sampler hand-over, and the loss of thirty steps on one batch beside the "adamw" trainer's."""
import json
import os

import numpy as np
import pytest
import torch

from tests import adam8_ref as A
from tests import cases
from tests import rdt_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
SENTINEL8 = 0xA5
GUARD = 8
SIZES = [1, 255, 4095, 4096, 4097, 4351, 8192, 70001]
NO_SHADOW = {1, 5}                       # tensors without an EMA shadow: one with fp32 moments, one quantised
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 1e-2, 1e-3
DECAYS = [0.0, 0.37, 0.9]
F = np.float32


def _L():
    from vlatouch import _lib as L
    return L


def _sp():
    return _L().stream_ptr(torch.device(DEV))


class _Guarded:
    """[pre sentinels | n values | GUARD sentinels] on the device, fp32 or uint8; pre = 4 keeps fp32 values 16-byte (uint8: 4-byte) aligned, 5 does not."""

    def __init__(self, values: np.ndarray, pre: int):
        self.n, self.pre, self.dt = values.size, pre, values.dtype
        s = SENTINEL8 if values.dtype == np.uint8 else SENTINEL
        host = np.concatenate([np.full(pre, s, values.dtype), values.reshape(-1), np.full(GUARD, s, values.dtype)])
        self.buf = torch.from_numpy(host).to(DEV)
        self.ptr = self.buf.data_ptr() + values.dtype.itemsize * pre
        self.s = s

    def values(self) -> np.ndarray:
        return self.buf[self.pre:self.pre + self.n].cpu().numpy()

    def guards_intact(self) -> bool:
        b = self.buf.cpu().numpy()
        return bool((b[:self.pre] == self.s).all()) and bool((b[self.pre + self.n:] == self.s).all())


def _hyper(step):
    L = _L()
    host = torch.zeros(4)
    L.check(L.lib().vt_train_hyper(LR, B1, B2, step, DECAYS[step - 1], L.ptr(host)), "vt_train_hyper")
    return host.numpy().copy()


def _tables():
    from vlatouch import adam8
    return adam8.device_tables(DEV)


@pytest.fixture(scope="module")
def ref():
    """Inputs and the statement's three chained steps, fp32 and (from each step's starting codes) fp64."""
    rng = np.random.default_rng(8)
    p0 = [rng.standard_normal(n).astype(F) for n in SIZES]
    sh0 = [None if i in NO_SHADOW else (p0[i] + 0.01 * rng.standard_normal(n)).astype(F) for i, n in enumerate(SIZES)]
    g = [[(rng.standard_normal(n) * np.exp(rng.standard_normal(n)) * 1e-3).astype(F) for n in SIZES] for _ in range(3)]
    g[1][6][512:768] = 0                                      # a block whose gradient vanishes
    hy = [_hyper(s) for s in (1, 2, 3)]
    steps = [dict(p=p0, sh=sh0, st=[A.zero_state(n) for n in SIZES])]
    f64 = []
    for s in range(3):
        cur, nxt, hi = steps[-1], dict(p=[], sh=[], st=[], info=[]), dict(p=[], sh=[])
        for i in range(len(SIZES)):
            pn, sn, st, info = A.step8(cur["p"][i], g[s][i], cur["st"][i], cur["sh"][i], hy[s], B1, B2, EPS, WD)
            nxt["p"].append(pn), nxt["sh"].append(sn), nxt["st"].append(st), nxt["info"].append(info)
            ph, shh, _, _ = A.step8(cur["p"][i], g[s][i], cur["st"][i], cur["sh"][i], hy[s], B1, B2, EPS, WD, dtype=np.float64)
            hi["p"].append(ph), hi["sh"].append(shh)
        steps.append(nxt), f64.append(hi)
    return dict(g=g, hy=hy, steps=steps, f64=f64)


class _Placed:
    """One placement of a state on the device: flip = 0 puts even tensors on aligned bases and odd ones on unaligned, flip = 1 the reverse."""

    def __init__(self, flip, p, sh, st, g, eight=True):
        self.eight = eight
        pre = [4 if (i + flip) % 2 == 0 else 5 for i in range(len(SIZES))]
        self.p = [_Guarded(x, pre[i]) for i, x in enumerate(p)]
        self.sh = [None if x is None else _Guarded(x, pre[i]) for i, x in enumerate(sh)]
        self.g = [_Guarded(x, pre[i]) for i, x in enumerate(g)]
        self.m, self.v, self.am, self.av = [], [], [], []
        for i, s in enumerate(st):
            q = eight and "m8" in s
            self.m.append(_Guarded(s["m8"] if q else s["m"], pre[i]))
            self.v.append(_Guarded(s["v8"] if q else s["v"], pre[i]))
            self.am.append(_Guarded(s["am"], 4) if q else None)
            self.av.append(_Guarded(s["av"], 4) if q else None)
        rows, aux, chunk0 = [], [], 0
        for i, n in enumerate(SIZES):
            rows.append([self.p[i].ptr, self.g[i].ptr, self.m[i].ptr, self.v[i].ptr, 0 if self.sh[i] is None else self.sh[i].ptr, n, chunk0])
            aux.append([0, 0] if self.am[i] is None else [self.am[i].ptr, self.av[i].ptr])
            chunk0 += (n + 4095) // 4096
        self.tab, self.aux, self.chunks = torch.tensor(rows, dtype=torch.int64).to(DEV), torch.tensor(aux, dtype=torch.int64).to(DEV), chunk0
        self.tables = _tables()

    def set_grads(self, g):
        for x, new in zip(self.g, g):
            x.buf[x.pre:x.pre + x.n].copy_(torch.from_numpy(new))

    def step(self, hy):
        L = _L()
        hyd = torch.from_numpy(hy).to(DEV)
        if self.eight:
            L.check(L.lib().vt_adamw8_ema_multi(L.ptr(self.tab), L.ptr(self.aux), L.ptr(self.tables), len(SIZES), self.chunks, L.ptr(hyd), B1, B2, EPS, WD,
                                                _sp()), "vt_adamw8_ema_multi")
        else:
            L.check(L.lib().vt_adamw_ema_multi(L.ptr(self.tab), len(SIZES), self.chunks, L.ptr(hyd), B1, B2, EPS, WD, _sp()), "vt_adamw_ema_multi")
        torch.cuda.synchronize()

    def check_guards(self, g_want):
        for what, xs in (("p", self.p), ("shadow", self.sh), ("g", self.g), ("m", self.m), ("v", self.v), ("am", self.am), ("av", self.av)):
            for x in xs:
                assert x is None or x.guards_intact(), ("guard words", what, x.n)
        for x, want in zip(self.g, g_want):
            assert np.array_equal(x.values(), want), ("gradient changed", x.n)

    def out(self):
        val = lambda xs: [None if x is None else x.values() for x in xs]
        return dict(p=val(self.p), sh=val(self.sh), m=val(self.m), v=val(self.v), am=val(self.am), av=val(self.av))


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _fp32_state(st):
    return [{"m": np.zeros(s["m8"].size, F), "v": np.zeros(s["m8"].size, F)} if "m8" in s else s for s in st]


@pytest.mark.parametrize("flip", [0, 1])
def test_step_one_from_the_zero_state_is_the_32bit_step(ref, flip):
    """The dequantised zero state is exactly 0, so p and shadow of every tensor equal vt_adamw_ema_multi's bit for bit."""
    s0 = ref["steps"][0]
    a = _Placed(flip, s0["p"], s0["sh"], s0["st"], ref["g"][0])
    b = _Placed(flip, s0["p"], s0["sh"], _fp32_state(s0["st"]), ref["g"][0], eight=False)
    a.step(ref["hy"][0]), b.step(ref["hy"][0])
    a.check_guards(ref["g"][0])
    oa, ob = a.out(), b.out()
    for i, n in enumerate(SIZES):
        assert np.array_equal(_bits(oa["p"][i]), _bits(ob["p"][i])), ("p", n)
        assert float(np.abs(oa["p"][i] - s0["p"][i]).max()) > 0, ("p did not move", n)
        if i not in NO_SHADOW:
            assert np.array_equal(_bits(oa["sh"][i]), _bits(ob["sh"][i])), ("shadow", n)
        if n >= A.MIN_8BIT_SIZE:
            assert oa["m"][i].dtype == np.uint8 and bool((oa["am"][i] > 0).all()) and bool((oa["av"][i] > 0).all())


@pytest.mark.parametrize("flip", [0, 1])
def test_small_tensors_keep_the_bits_of_the_32bit_step(ref, flip):
    """Three chained steps of both kernels: the tensors under 4096 elements (fp32 moments, null aux pair) agree in p, shadow, m and v."""
    s0 = ref["steps"][0]
    a = _Placed(flip, s0["p"], s0["sh"], s0["st"], ref["g"][0])
    b = _Placed(flip, s0["p"], s0["sh"], _fp32_state(s0["st"]), ref["g"][0], eight=False)
    for s in range(3):
        for x in (a, b):
            x.set_grads(ref["g"][s])
            x.step(ref["hy"][s])
        oa, ob = a.out(), b.out()
        for i, n in enumerate(SIZES):
            if n >= A.MIN_8BIT_SIZE:
                continue
            for part in ("p", "m", "v") + (() if i in NO_SHADOW else ("sh",)):
                assert np.array_equal(_bits(oa[part][i]), _bits(ob[part][i])), (s + 1, part, n)
            assert np.array_equal(_bits(oa["p"][i]), _bits(ref["steps"][s + 1]["p"][i])), ("the statement's fp32 step", s + 1, n)
    a.check_guards(ref["g"][2])


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("step", [2, 3])
def test_steps_from_the_references_uploaded_state(ref, step, flip):
    """Scales bit-equal; codes equal except where the reference's ratio lies within 2^-20 relative of a boundary, where the neighbouring code
    passes, for at most 1e-3 of the elements (the reference alone has 1.7e-5 of its ratios that close on this input); p / shadow within
    max(3 x the fp32 reference's own error against fp64, 1e-6 of max-abs) per tensor.  Two runs are bit-equal."""
    cur, want, hi = ref["steps"][step - 1], ref["steps"][step], ref["f64"][step - 1]
    outs = []
    for _ in range(2):
        a = _Placed(flip, cur["p"], cur["sh"], cur["st"], ref["g"][step - 1])
        a.step(ref["hy"][step - 1])
        a.check_guards(ref["g"][step - 1])
        outs.append(a.out())
    o = outs[0]
    for part in o:
        for x, y in zip(o[part], outs[1][part]):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), ("two runs differ", part)
    excused = total = near_total = 0
    for i, n in enumerate(SIZES):
        for part, key in (("p", "p"), ("sh", "sh")):
            if want[key][i] is None:
                continue
            h = hi[key][i]
            own = float(np.abs(want[key][i].astype(np.float64) - h).max())
            err = float(np.abs(o[part][i].astype(np.float64) - h).max())
            bar = max(3 * own, 1e-6 * float(np.abs(h).max()))
            print(f"[adam8 step {step} n={n} {part}] error vs fp64 {err:.3e}, the fp32 statement's own {own:.3e}, bar {bar:.3e}")
            assert err <= bar, (part, n, err, bar)
        if n < A.MIN_8BIT_SIZE:
            continue
        st, info = want["st"][i], want["info"][i]
        assert np.array_equal(_bits(o["am"][i]), _bits(st["am"])), ("am", n)
        assert np.array_equal(_bits(o["av"][i]), _bits(st["av"])), ("av", n)
        for part, key, r, b in (("m", "m8", info["rm"], A.BS), ("v", "v8", info["rv"], A.BU)):
            diff = o[part][i] != st[key]
            near, other = A.near_boundary(r, b)
            near_total += int(near.sum())
            assert bool((~diff | near).all()), (part, n, "a code differs away from a boundary", int((diff & ~near).sum()))
            assert bool((o[part][i][diff].astype(np.int64) == other[diff]).all()), (part, n, "not the neighbouring code")
            excused += int(diff.sum())
            total += n
    print(f"[adam8 step {step}] {excused} of {total} codes excused next to a boundary; {near_total} ratios ({near_total / total:.1e}) lie that close")
    assert excused <= 1e-3 * total


def test_three_chained_steps_keep_the_moments_within_one_code_step(ref):
    """The device's own chain against the statement's: dequantised (vt_adam8_dequantize) moments within one code step x scale of the reference's."""
    from vlatouch import adam8
    s0 = ref["steps"][0]
    a = _Placed(0, s0["p"], s0["sh"], s0["st"], ref["g"][0])
    for s in range(3):
        a.set_grads(ref["g"][s])
        a.step(ref["hy"][s])
    a.check_guards(ref["g"][2])
    o, want = a.out(), ref["steps"][3]["st"]
    for i, n in enumerate(SIZES):
        if n < A.MIN_8BIT_SIZE:
            continue
        for part, sc, signed, key, skey, table in (("m", "am", True, "m8", "am", A.TS), ("v", "av", False, "v8", "av", A.TU)):
            got = adam8.dequantize(torch.from_numpy(o[part][i]).to(DEV), torch.from_numpy(o[sc][i]).to(DEV), a.tables, signed).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(A.dequantize(o[part][i], o[sc][i], signed))), ("vt_adam8_dequantize", part, n)
            refv = A.dequantize(want[i][key], want[i][skey], signed, np.float64)
            bound = A.code_step(want[i][key], table) * np.repeat(want[i][skey].astype(np.float64), 256)[:n]
            err = np.abs(got.astype(np.float64) - refv)
            assert bool((err <= bound).all()), (part, n, float((err - bound).max()))
            assert float(np.abs(refv).max()) > 0


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_quantize_and_dequantize_state_the_block_rule(n, signed):
    """Codes, scales and the round trip equal the statement's bit for bit (the division is IEEE on both sides), written over 0xFF / NaN fills;
    an all-zero block gives code 127 / 0 and scale 0; guard bytes / words intact; twice, bit-equal."""
    L, lib, tables = _L(), _L().lib(), _tables()
    rng = np.random.default_rng(n + int(signed))
    x = (rng.standard_normal(n) * np.exp(2 * rng.standard_normal(n))).astype(F)
    if not signed:
        x = np.abs(x)
    if n > 1024:
        x[512:768] = 0
    wc, wa, _ = A.quantize(x, signed)
    runs = []
    for _ in range(2):
        xs = _Guarded(x, 5)
        codes, absmax = _Guarded(np.full(n, 0xFF, np.uint8), 5), _Guarded(np.full(A.nblocks(n), np.nan, F), 4)
        out = _Guarded(np.full(n, np.nan, F), 5)
        L.check(lib.vt_adam8_quantize(xs.ptr, codes.ptr, absmax.ptr, L.ptr(tables), int(signed), n, _sp()), "vt_adam8_quantize")
        L.check(lib.vt_adam8_dequantize(codes.ptr, absmax.ptr, L.ptr(tables), int(signed), out.ptr, n, _sp()), "vt_adam8_dequantize")
        torch.cuda.synchronize()
        assert all(b.guards_intact() for b in (xs, codes, absmax, out)) and np.array_equal(xs.values(), x)
        runs.append((codes.values(), absmax.values(), out.values()))
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b)), "two runs differ"
    gc, ga, go = runs[0]
    assert np.array_equal(_bits(ga), _bits(wa)) and np.array_equal(gc, wc), (n, int((gc != wc).sum()))
    assert np.array_equal(_bits(go), _bits(A.dequantize(wc, wa, signed)))
    if n > 1024:
        assert ga[2] == 0 and bool((gc[512:768] == (127 if signed else 0)).all()) and bool((go[512:768] == 0).all())


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(precision, k, optimizer, **kw):
    from tests.test_gpu_sample_eval import _runner
    return _runner(cases.RDT_TINY).trainer(lr=1e-3, precision=precision, gradient_accumulation_steps=k, optimizer=optimizer, **kw)


def _step(tr, b):
    return tr.train_step(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                         noise=b["noise"], timesteps=b["timesteps"])


def _batches(count):
    return [R.batch(cases.RDT_TINY, 3, 12, seed=6 + 10 * j) for j in range(count)]


def _same(a, b, what):
    assert set(a) == set(b) and a, what
    for key in a:
        x, y = a[key].cpu().contiguous(), b[key].cpu().contiguous()
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, key)


CASES = [("fp32", 1), ("fp32", 4), ("bf16", 1), ("bf16", 4)]


@pytest.mark.parametrize("precision,k", CASES)
def test_trainer_first_step_state_size_and_sampler(precision, k):
    """One optimizer step (k micro-batches): master weights and shadows bit-equal to the "adamw" trainer's; optimizer_state_bytes() is the count
    from the shapes before and after the step and a quarter of the 32-bit state plus the scales; moments() has the parameters' shapes and is
    non-zero; sampler() on the stepped weights is bit-equal to the route through sync_to."""
    from tests.test_gpu_sample_eval import _runner
    cfg = cases.RDT_TINY
    batches = _batches(k)
    a, b = _trainer(precision, k, "adamw8bit"), _trainer(precision, k, "adamw")
    numels = [v.numel() for v in a.p.values()]
    want = sum(8 * n if n < 4096 else 2 * n + 8 * ((n + 255) // 256) for n in numels)
    assert any(n < 4096 for n in numels) and any(n >= 4096 for n in numels)
    assert a.optimizer_state_bytes() == want and b.optimizer_state_bytes() == 8 * sum(numels)
    for bt in batches:
        la, lb = _step(a, bt), _step(b, bt)
        assert torch.equal(la, lb)
    assert a.global_step == b.global_step == 1 and torch.equal(a.grad_norm, b.grad_norm)
    _same(a.p, b.p, "master weights after step 1")
    _same(a.shadow, b.shadow, "shadows after step 1")
    assert a.optimizer_state_bytes() == want and b.optimizer_state_bytes() == 8 * sum(numels)
    for name, p in a.p.items():
        (m, v), (m32, v32) = a.moments(name), b.moments(name)
        assert m.shape == v.shape == p.shape and m.dtype == v.dtype == torch.float32
        if p.numel() < 4096:
            assert torch.equal(m, m32) and torch.equal(v, v32), name
            assert a._m[name].dtype == torch.float32 and name not in a._am
        else:
            assert a._m[name].dtype == a._v[name].dtype == torch.uint8 and a._am[name].numel() == (p.numel() + 255) // 256
            # step 1 quantises the 32-bit step's own moments: half the widest gap of either table (the signed one's top decade) or the distance
            # from -1 to the signed table's first entry, plus the fp32 rounding of the product T[code] x scale, times the block's scale, itself
            # at most the tensor's, bounds the distance
            widest = max(0.5 * float(np.diff(A.TS.astype(np.float64)).max()), 1.0 + float(A.TS[0])) + 2.0 ** -22
            for q, full in ((m, m32), (v, v32)):
                scale = full.abs().flatten().max()
                assert float((q.double() - full.double()).abs().max()) <= widest * float(scale), name
    d = cases.rdt_inputs(cfg, 3, 12)
    bt = batches[0]
    pa = lambda rr: rr.predict_action(bt["lang_tokens"], bt["lang_attn_mask"], bt["img_tokens"], bt["state_tokens"], bt["action_mask"], bt["ctrl_freqs"],
                                      x_init=d["x_init"]).float().cpu()
    assert torch.equal(pa(a.sampler()), pa(a.sync_to(_runner(cfg))))
    assert torch.equal(pa(a.sampler(ema=True)), pa(a.sync_to(_runner(cfg), ema=True)))


@pytest.mark.parametrize("precision,k", CASES)
def test_trainer_resume_is_exact_and_the_other_optimizers_checkpoint_is_refused(precision, k, tmp_path):
    """Two optimizer steps, save_checkpoint, a new trainer, load_checkpoint, two more = four straight: weights, shadows, codes, scales and the
    small tensors' fp32 moments bit-equal.  The checkpoint holds adam8.safetensors (no adam_m / adam_v) and trainer_state.json names the
    optimizer and the block; an "adamw" trainer refuses it, and an "adamw8bit" trainer refuses an "adamw" checkpoint, whose
    trainer_state.json has neither key."""
    batches = _batches(4 * k)
    straight = _trainer(precision, k, "adamw8bit")
    losses = [float(_step(straight, b)) for b in batches]
    first = _trainer(precision, k, "adamw8bit")
    for b in batches[:2 * k]:
        _step(first, b)
    ck = str(tmp_path / "checkpoint-2")
    first.save_checkpoint(ck)
    assert os.path.exists(os.path.join(ck, "checkpoint", "adam8.safetensors"))
    assert not os.path.exists(os.path.join(ck, "checkpoint", "adam_m.safetensors")) and not os.path.exists(os.path.join(ck, "checkpoint", "adam_v.safetensors"))
    with open(os.path.join(ck, "trainer_state.json")) as f:
        js = json.load(f)
    assert js["optimizer"] == "adamw8bit" and js["block"] == 256
    from safetensors.torch import load_file
    held = load_file(os.path.join(ck, "checkpoint", "adam8.safetensors"))
    assert np.array_equal(held["table_signed"].numpy().view(np.int32), A.TS.view(np.int32))
    assert np.array_equal(held["table_unsigned"].numpy().view(np.int32), A.TU.view(np.int32))
    assert {k_.split(".", 1)[0] for k_ in held} == {"m8", "v8", "am", "av", "m", "v", "table_signed", "table_unsigned"}
    second = _trainer(precision, k, "adamw8bit")
    second.load_checkpoint(ck)
    assert (second.step_count, second.ema_updates, second.micro_step) == (2, 2 * k, 0)
    resumed = [float(_step(second, b)) for b in batches[2 * k:]]
    assert resumed == losses[2 * k:]
    for part in ("p", "shadow", "_m", "_v", "_am", "_av"):
        _same(getattr(straight, part), getattr(second, part), part)
    other = _trainer(precision, k, "adamw")
    before = {key: v.clone() for key, v in other.p.items()}
    with pytest.raises(ValueError, match="optimizer"):
        other.load_checkpoint(ck)
    _same(before, other.p, "a refused checkpoint leaves the weights alone")
    for b in batches[:k]:
        _step(other, b)
    ck32 = str(tmp_path / "checkpoint-32")
    other.save_checkpoint(ck32)
    with open(os.path.join(ck32, "trainer_state.json")) as f:
        js32 = json.load(f)
    assert "optimizer" not in js32 and "block" not in js32 and os.path.exists(os.path.join(ck32, "checkpoint", "adam_m.safetensors"))
    with pytest.raises(ValueError, match="optimizer"):
        _trainer(precision, k, "adamw8bit").load_checkpoint(ck32)


@pytest.mark.parametrize("precision,k", CASES)
def test_trainer_loss_follows_the_32bit_optimizer(precision, k):
    """Thirty optimizer steps on one batch with either optimizer: the 8-bit run's last loss as a fraction of its first is at most 1.5 x the
    "adamw" run's fraction (the margin of the CPU toy, tests/test_adam8_host.py)."""
    bt = _batches(1)[0]
    frac = {}
    for opt in ("adamw8bit", "adamw"):
        tr = _trainer(precision, k, opt)
        losses = [_step(tr, bt) for _ in range(30 * k)]
        assert tr.global_step == 30
        first, last = float(losses[0]), float(losses[-1])
        frac[opt] = last / first
    print(f"[adam8 trainer {precision} k={k}] loss after 30 steps / first loss: adamw8bit {frac['adamw8bit']:.4f}, adamw {frac['adamw']:.4f}")
    assert np.isfinite(frac["adamw8bit"]) and frac["adamw"] < 1.0
    assert frac["adamw8bit"] <= 1.5 * frac["adamw"], frac
