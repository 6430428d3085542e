"""Gradient accumulation and resumable checkpoints of the RDT fine-tuning step on the device (vlatouch/rdt_train.py, vt_grad_accum_multi and
vt_ema_multi of csrc/vt_train_rdt.hip) against fp64 torch on the CPU (tests/rdt_accum_ref.py) and the reference's own accumulated run
(tests/golden/g17_rdt_accum.npz).

Kernel level: both kernels twice on NaN-filled outputs, bit-equal; vt_grad_accum_multi within k 2^-23 of sum|g_i| / k per element (k roundings
of fp32), vt_ema_multi bit-equal to vt_ema_update_dev per tensor; vt_grad_clip_multi's norm and clipped gradients within 2^-18 of fp64; guard
words in front of and behind every tensor untouched.  Trainer level: the
accumulated gradient within 1e-4 of each tensor's norm against (1/k) sum of fp64 autograd gradients and against the fp64 gradient of the
concatenated batch; losses and norms 1e-5 against g17; three accumulated optimizer steps within 5 x what fp32 torch loses against fp64 torch; the
bf16 rule of test_gradients_bf16; k = 1 bit-equal to the step without the keyword; resume bit-equal; the loop helper's files."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import rdt_train_ref as R
from tests import rdt_accum_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 12345.0
GUARD = 8
SIZES = [1, 2, 3, 5, 255, 1023, 4095, 4096, 4097, 4099, 3 * 4096, 70001]


def _L():
    from vlatouch import _lib as L
    return L


def _sp():
    return _L().stream_ptr(torch.device(DEV))


class _Guarded:
    """[pre sentinel words | n values | GUARD sentinel words] on the device; pre = 4 keeps the values 16-byte aligned, pre = 5 does not."""

    def __init__(self, values: torch.Tensor, pre: int):
        self.n, self.pre = values.numel(), pre
        self.buf = torch.cat([torch.full((pre,), SENTINEL), values.float(), torch.full((GUARD,), SENTINEL)]).to(DEV)
        self.ptr = self.buf.data_ptr() + 4 * pre
        assert (self.ptr % 16 == 0) == (pre % 4 == 0)

    def values(self):
        return self.buf[self.pre:self.pre + self.n].cpu()

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:self.pre] == SENTINEL).all()) and bool((b[self.pre + self.n:] == SENTINEL).all())


def _table(p, g, m, v, sh, sizes):
    rows, chunk0 = [], 0
    for i, n in enumerate(sizes):
        rows.append([p[i].ptr, g[i].ptr, m[i].ptr, v[i].ptr, 0 if sh[i] is None else sh[i].ptr, n, chunk0])
        chunk0 += (n + 4095) // 4096
    return torch.tensor(rows, dtype=torch.int64).to(DEV), chunk0


# ------------------------------------------------------------------------------------------------ kernels as units
@pytest.mark.parametrize("pre", [4, 5], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_grad_accum_multi_against_fp64(k, pre):
    """k micro-batches folded into NaN-filled accumulators: the first call stores (the NaNs must be gone: the accumulator is not read), the
    others add.  Per element |acc - (1/k) sum g_i| <= k 2^-23 sum|g_i| / k: the rounding of 1/k, of the first product and of k - 1 fused
    multiply-adds, each at most 2^-24 of a partial sum that sum|g_i| / k bounds.  Twice, bit-equal; add mode alone on a given accumulator too;
    p, m, v, the fresh gradients and every guard word unchanged."""
    L, lib = _L(), _L().lib()
    gen = torch.Generator().manual_seed(100 * k + pre)
    fresh_host = [[torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) > 0.1) * 10 ** float(torch.randint(-3, 3, (1,), generator=gen))
                   for n in SIZES] for _ in range(k)]
    others_host = [torch.randn(n, generator=gen) for n in SIZES]
    scale = 1.0 / k

    def run():
        acc = [_Guarded(torch.full((n,), NAN), pre) for n in SIZES]
        p, m, v = ([_Guarded(x, pre) for x in others_host] for _ in range(3))
        tab, chunks = _table(p, acc, m, v, [None] * len(SIZES), SIZES)
        fresh = [[_Guarded(x, pre) for x in gs] for gs in fresh_host]
        for j in range(k):
            ptrs = torch.tensor([x.ptr for x in fresh[j]], dtype=torch.int64).to(DEV)
            L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(ptrs), len(SIZES), chunks, scale, int(j > 0), _sp()), "vt_grad_accum_multi")
        torch.cuda.synchronize()
        for what, xs in (("acc", acc), ("p", p), ("m", m), ("v", v)) + tuple((f"fresh{j}", fresh[j]) for j in range(k)):
            for x in xs:
                assert x.guards_intact(), ("guard words", what, x.n)
        for j in range(k):
            for x, want in zip(fresh[j], fresh_host[j]):
                assert torch.equal(x.values(), want), ("fresh gradient changed", x.n)
        for xs in (p, m, v):
            for x, want in zip(xs, others_host):
                assert torch.equal(x.values(), want), ("p / m / v changed", x.n)
        return [a.values() for a in acc]

    got, again = run(), run()
    worst = 0.0
    for i, n in enumerate(SIZES):
        assert torch.equal(got[i], again[i]), ("two runs differ", n)
        assert bool(torch.isfinite(got[i]).all()), ("store mode left NaN", n)
        ref = sum(x[i].double() for x in fresh_host) / k
        mag = sum(x[i].double().abs() for x in fresh_host) / k
        err = (got[i].double() - ref).abs()
        bound = k * 2.0 ** -23 * mag
        assert bool((err <= bound).all()), (n, float((err - bound).max()))
        nz = mag > 0
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / mag[nz]).max()))
        assert bool((got[i][~nz] == 0).all())
    print(f"[vt_grad_accum_multi k={k} pre={pre}] worst error {worst / 2.0 ** -23:.3f} x 2^-23 of sum|g|/k (bar {k})")
    if k == 1:
        for i in range(len(SIZES)):
            assert torch.equal(got[i], fresh_host[0][i]), "k = 1 in store mode is a copy"
    # add mode alone: acc given, one micro-batch added
    acc0 = [torch.randn(n, generator=gen) for n in SIZES]
    res = []
    for _ in range(2):
        acc = [_Guarded(x, pre) for x in acc0]
        zeros = [_Guarded(torch.zeros(n), pre) for n in SIZES]
        tab, chunks = _table(zeros, acc, zeros, zeros, [None] * len(SIZES), SIZES)
        fresh = [_Guarded(x, pre) for x in fresh_host[0]]
        ptrs = torch.tensor([x.ptr for x in fresh], dtype=torch.int64).to(DEV)
        L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(ptrs), len(SIZES), chunks, scale, 1, _sp()), "vt_grad_accum_multi")
        torch.cuda.synchronize()
        assert all(a.guards_intact() for a in acc)
        res.append([a.values() for a in acc])
    for i, n in enumerate(SIZES):
        assert torch.equal(res[0][i], res[1][i])
        ref = acc0[i].double() + fresh_host[0][i].double() / k
        mag = acc0[i].double().abs() + fresh_host[0][i].double().abs() / k
        assert bool(((res[0][i].double() - ref).abs() <= 2 * 2.0 ** -23 * mag).all()), ("add mode", n)


@pytest.mark.parametrize("pre", [4, 5], ids=["aligned", "unaligned"])
def test_ema_multi_is_bit_equal_to_the_per_tensor_kernel(pre):
    """Three EMA-only updates with different decays over a table with and without shadows, against vt_ema_update_dev tensor by tensor."""
    L, lib = _L(), _L().lib()
    gen = torch.Generator().manual_seed(7 + pre)
    shadowed = [i % 5 != 1 for i in range(len(SIZES))]
    p_host = [torch.randn(n, generator=gen) for n in SIZES]
    sh_host = [torch.randn(n, generator=gen) for n in SIZES]
    decays = [0.0, 1 - 2 ** (-2 / 3), 0.9999]

    def run(multi):
        p = [_Guarded(x, pre) for x in p_host]
        sh = [_Guarded(x, pre) if s else None for x, s in zip(sh_host, shadowed)]
        other = [_Guarded(torch.full((n,), NAN), pre) for n in SIZES]                 # g, m, v: the kernel must not touch them
        tab, chunks = _table(p, other, other, other, sh, SIZES)
        host = torch.zeros(4)
        for d in decays:
            L.check(lib.vt_train_hyper(1e-3, 0.9, 0.999, 1, d, L.ptr(host)), "vt_train_hyper")
            hyper = host.to(DEV)
            if multi:
                L.check(lib.vt_ema_multi(L.ptr(tab), len(SIZES), chunks, L.ptr(hyper), _sp()), "vt_ema_multi")
            else:
                for i, n in enumerate(SIZES):
                    if sh[i] is not None:
                        L.check(lib.vt_ema_update_dev(sh[i].ptr, p[i].ptr, n, L.ptr(hyper), _sp()), "vt_ema_update_dev")
            torch.cuda.synchronize()
        for xs in (p, sh, other):
            assert all(x is None or x.guards_intact() for x in xs), "guard words"
        assert all(torch.equal(x.values(), want) for x, want in zip(p, p_host)), "parameters changed"
        assert all(bool(torch.isnan(x.values()).all()) for x in other), "g / m / v touched"
        return [None if x is None else x.values() for x in sh]

    a, b, c = run(True), run(True), run(False)
    for i, n in enumerate(SIZES):
        if not shadowed[i]:
            assert a[i] is None
            continue
        assert torch.equal(a[i], b[i]), ("two runs differ", n)
        assert a[i].view(torch.int32).equal(c[i].view(torch.int32)), ("vt_ema_multi != vt_ema_update_dev", n)
        want = sh_host[i].double()
        for d in decays:
            want = want - (1 - d) * (want - p_host[i].double())
        assert float((a[i].double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("pre", [4, 5], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("clipped", [True, False], ids=["clipped", "unclipped"])
def test_grad_clip_multi_against_fp64(clipped, pre):
    """vt_grad_clip_multi over the table, with the fp64 norm of the gradients above max_norm and, the same gradients scaled down, below it.
    norm_coef[0] within 2^-18 of the fp64 norm; clipped, every element within 2^-18 |g| of g min(1, max_norm / (norm64 + 1e-6)); unclipped,
    the gradients bit-unchanged.  The bar: any chain of additions of the non-negative squares is under 64 roundings (16 per thread, 8 levels in
    the block, at most 1 + 8 in the coefficient kernel), so the sum of squares is within 64 x 2^-24 = 2^-18 and its root within 2^-19; the
    coefficient and the product add four roundings, under 2^-22.  Twice, bit-equal; p, m, v, shadow and every guard word unchanged."""
    L, lib = _L(), _L().lib()
    gen = torch.Generator().manual_seed(40 + pre)
    max_norm = 1.0
    g_host = [torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) > 0.1) * 10 ** float(torch.randint(-3, 3, (1,), generator=gen)) for n in SIZES]
    norm_of = lambda gs: float(torch.sqrt(sum((x.double() ** 2).sum() for x in gs)))
    s = (1.7 if clipped else 0.5) * max_norm / norm_of(g_host)     # a coefficient near 0.6: the bar is relative to |g|, so a small one would hide an error
    g_host = [(x.double() * s).float() for x in g_host]
    norm64 = norm_of(g_host)
    assert (norm64 > max_norm) == clipped
    coef64 = min(1.0, max_norm / (norm64 + 1e-6))
    others_host = [torch.randn(n, generator=gen) for n in SIZES]

    def run():
        g = [_Guarded(x, pre) for x in g_host]
        p, m, v, sh = ([_Guarded(x, pre) for x in others_host] for _ in range(4))
        tab, chunks = _table(p, g, m, v, sh, SIZES)
        part, out2 = _Guarded(torch.full((chunks,), NAN), 4), _Guarded(torch.full((2,), NAN), 4)
        L.check(lib.vt_grad_clip_multi(L.ptr(tab), len(SIZES), chunks, max_norm, part.ptr, out2.ptr, _sp()), "vt_grad_clip_multi")
        torch.cuda.synchronize()
        for what, xs in (("g", g), ("p", p), ("m", m), ("v", v), ("shadow", sh), ("chunk_part", [part]), ("norm_coef", [out2])):
            for x in xs:
                assert x.guards_intact(), ("guard words", what, x.n)
        for xs in (p, m, v, sh):
            for x, want in zip(xs, others_host):
                assert torch.equal(x.values(), want), ("p / m / v / shadow changed", x.n)
        return out2.values(), [x.values() for x in g]

    (nc, got), (nc2, again) = run(), run()
    assert nc.view(torch.int32).equal(nc2.view(torch.int32)), "two runs differ in norm_coef"
    err_norm = abs(float(nc[0]) - norm64) / norm64
    worst = 0.0
    for i, n in enumerate(SIZES):
        assert got[i].view(torch.int32).equal(again[i].view(torch.int32)), ("two runs differ", n)
        if not clipped:
            assert got[i].view(torch.int32).equal(g_host[i].view(torch.int32)), ("unclipped gradients changed", n)
            continue
        mag = g_host[i].double().abs()
        err = (got[i].double() - g_host[i].double() * coef64).abs()
        nz = mag > 0
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / mag[nz]).max()))
        assert bool((err <= 2.0 ** -18 * mag).all()), (n, float((err - 2.0 ** -18 * mag).max()))
    print(f"[vt_grad_clip_multi clipped={clipped} pre={pre}] norm error {err_norm / 2.0 ** -18:.4f} x 2^-18, worst element {worst / 2.0 ** -18:.4f} x 2^-18 of |g|")
    assert err_norm <= 2.0 ** -18, (float(nc[0]), norm64)


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(cfg, sd, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], device=DEV, **kw)


def _step(tr, b):
    return tr.train_step(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                         noise=b["noise"], timesteps=b["timesteps"])


def _case(name):
    return (cases.RDT_TINY, 3, 12) if name == "tiny" else (cases.RDT_WIDE, 2, 20)


def _worst(got, ref, keys):
    w, wk = 0.0, None
    for key in keys:
        e = R.rel_err(got[key], ref[key])
        if e > w:
            w, wk = e, key
    return w, wk


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_accumulated_gradient_fp32(name):
    """Four micro-batches at fixed weights through get_loss + accumulate (what train_step does before its optimizer step, so the accumulators are
    read before the clip scales them).  grads() against (1/4) sum of the fp64 autograd gradients and against the fp64 gradient of the
    concatenated batch: every tensor within 1e-4 of its norm; the two fp64 references within A.REFS_AGREE of each other (the oracle's attention
    products are fp32 in any run: tests/rdt_accum_ref.py)."""
    cfg, B, Ll = _case(name)
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, B, Ll, seed=s) for s in A.G17_SEEDS[:4]]
    ref_losses, ref_acc = A.accumulated_grads(sd, batches, cfg)
    _, ref_cat = R.loss_and_grads(sd, A.concat_batch(batches), cfg)
    w_refs, _ = _worst(ref_acc, ref_cat, sd)
    print(f"[rdt_accum {name}] the two fp64 references are {w_refs:.2e} apart (bar {A.REFS_AGREE:g})")
    assert w_refs <= A.REFS_AGREE, w_refs
    runs = []
    for _ in range(2):
        tr = _trainer(cfg, sd, gradient_accumulation_steps=4)
        losses = []
        for j, b in enumerate(batches):
            tr.get_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                        noise=b["noise"], timesteps=b["timesteps"])
            losses.append(float(tr.last_loss))
            tr.accumulate()
            assert tr.micro_step == j + 1
        runs.append((losses, tr.grads()))
    (losses, grads), (_, grads2) = runs
    assert set(grads) == set(sd) and all(torch.equal(grads[key], grads2[key]) for key in sd), "two trainers must accumulate bit for bit"
    wa, ka = _worst(grads, ref_acc, sd)
    wc, kc = _worst(grads, ref_cat, sd)
    print(f"[rdt_accum {name}] worst accumulated gradient: {wa:.2e} of its norm vs (1/4) sum fp64 ({ka}), {wc:.2e} vs the concatenated batch ({kc}); "
          f"fp64 references apart {w_refs:.1e}")
    for got, want in zip(losses, ref_losses):
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert wa <= 1e-4 and wc <= 1e-4, (ka, wa, kc, wc)


@pytest.mark.parametrize("rms_mode,scheduler", A.G17_RUNS)
def test_against_the_references_own_accumulated_run(rms_mode, scheduler):
    """RDT_TINY against g17 directly: every micro-batch loss and every norm before clipping 1e-5 relative, the accumulated gradient of the first
    window (the parameters are still the golden's) within 1e-4 of each tensor's norm on the summaries; the logged lr, the EMA decay and
    sync_gradients of every micro-batch equal."""
    from vlatouch.rdt_train import lr_at
    g = np.load(f"{cases.GOLDEN}/g17_rdt_accum.npz")
    names = [str(n) for n in g["names"]]
    cfg, k, tag = cases.RDT_TINY, A.G17_K, f"{rms_mode}_{scheduler}"
    tr = _trainer(cfg, cases.rdt_sd(cfg), rms_mode=rms_mode, lr=A.G17_HP["lr"], weight_decay=A.G17_HP["weight_decay"], max_grad_norm=A.G17_MAX_GRAD_NORM,
                  lr_scheduler=scheduler, lr_warmup_steps=A.G17_WARMUP, gradient_accumulation_steps=k)
    sc, norms = g[f"{tag}_scalars"], g[f"{tag}_norms"]
    fails = []
    for n, seed in enumerate(A.G17_SEEDS):
        b = R.batch(cfg, A.G17_B, A.G17_LANG_LEN, seed=seed)
        if n == k - 1:                                           # the first window's accumulated gradient, read before the clip scales it
            tr.get_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                        noise=b["noise"], timesteps=b["timesteps"])
            loss = float(tr.last_loss)
            tr.accumulate()
            wg, kg = R.worst_summary(g[f"{tag}_s1_grad"], names, tr.grads())
            tr.optimizer_step()
        else:
            loss = float(_step(tr, b))
        want_loss, want_decay, want_lr, want_sync = sc[n]
        lr_logged = lr_at(tr.base_lr, tr.lr_scheduler, tr.step_count, tr.lr_warmup_steps * tr.k)
        line = f"[rdt_accum vs g17 {tag} micro-batch {n + 1}] loss {loss:.7f} vs {want_loss:.7f}"
        assert tr.sync_gradients == bool(want_sync) and tr.ema_updates == n + 1 and tr.global_step == (n + 1) // k
        assert tr._ema_decay(tr.ema_updates) == want_decay and lr_logged == want_lr, (n, lr_logged, want_lr)
        if tr.sync_gradients:
            norm, want_norm = float(tr.grad_norm), norms[tr.global_step - 1]
            line += f", norm {norm:.5f} vs {want_norm:.5f}, lr used {tr.lr:g}"
            if not abs(norm - want_norm) <= 1e-5 * want_norm:
                fails.append(("norm", n, norm, want_norm))
        print(line)
        if not abs(loss - want_loss) <= 1e-5 * want_loss:
            fails.append(("loss", n, loss, want_loss))
    print(f"[rdt_accum vs g17 {tag}] worst accumulated-gradient summary {wg:.2e} ({kg})")
    assert not fails, fails
    assert wg <= 1e-4, (kg, wg)


def test_three_accumulated_optimizer_steps():
    """12 micro-batches, k = 4, fp32: p - p_0 after every optimizer step and ema - p_0 after every micro-batch, per tensor relative to the fp64
    run's.  Bar: the worst tensor at most 5 x the worst tensor of the same loop in fp32 torch on the CPU against fp64 torch, measured here (the
    rule of test_three_clipped_adamw_ema_steps).  EMA decays per micro-batch equal the restatement's."""
    cfg, k = cases.RDT_TINY, 4
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in A.G17_SEEDS]
    hp = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    r64 = A.accum_train_steps(sd, batches, cfg, k, dtype=torch.float64, **hp)
    r32 = A.accum_train_steps(sd, batches, cfg, k, dtype=torch.float32, **hp)
    p0 = {key: v.double() for key, v in sd.items()}

    def worst(params, ref):
        w, wk = 0.0, None
        for key in sd:
            e = R.rel_err(params[key].double() - p0[key], ref[key] - p0[key])
            if e > w:
                w, wk = e, key
        return w, wk

    trs = [_trainer(cfg, sd, gradient_accumulation_steps=k, **hp) for _ in range(2)]
    fails = []
    for n, b in enumerate(batches):
        losses = [float(_step(tr, b)) for tr in trs]
        tr, rec = trs[0], r64[n]
        assert tr._ema_decay(tr.ema_updates) == rec["ema_decay"], (n, "EMA decay")
        assert tr.sync_gradients == rec["sync"] and tr.step_count == (n + 1) // k and tr.ema_updates == n + 1
        (we, ke), (be, _) = worst(tr.ema_state_dict(), rec["ema"]), worst(r32[n]["ema"], rec["ema"])
        line = f"[rdt_accum micro-batch {n + 1}] loss {losses[0]:.6f} (fp64 {rec['loss']:.6f}); EMA HIP {we:.2e} ({ke}) / fp32 torch {be:.2e}"
        if not abs(losses[0] - rec["loss"]) <= 1e-5 * rec["loss"]:
            fails.append(("loss", n, losses[0], rec["loss"]))
        if not we <= 5 * be:
            fails.append(("ema", n, we, be))
        if rec["sync"]:
            norm = float(tr.grad_norm)
            (wp, kp), (bp, _) = worst(tr.state_dict(), rec["params"]), worst(r32[n]["params"], rec["params"])
            line += f"; grad norm {norm:.5f} (fp64 {rec['grad_norm']:.5f}); update HIP {wp:.2e} ({kp}) / fp32 torch {bp:.2e}"
            if not abs(norm - rec["grad_norm"]) <= 1e-5 * rec["grad_norm"]:
                fails.append(("norm", n, norm, rec["grad_norm"]))
            if not wp <= 5 * bp:
                fails.append(("update", n, wp, bp))
        print(line)
    assert r64[k - 1]["grad_norm"] > 1.0, "the clip must be active in this test"
    assert not fails, fails
    a, b2 = trs[0].state_dict(), trs[1].state_dict()
    ea, eb = trs[0].ema_state_dict(), trs[1].ema_state_dict()
    assert all(torch.equal(a[key], b2[key]) and torch.equal(ea[key], eb[key]) for key in a), "two trainers from the same weights must agree bit for bit"


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_accumulated_gradients_bf16(name):
    """precision="bf16", k = 4: per-tensor error of the accumulated gradient against fp64 (from the same bf16-rounded weights and inputs) beside the
    oracle's bf16 CPU run accumulated the same way: e_hip <= max(1.5 e_ref, 1e-2 |g|) for every tensor (the rule of test_gradients_bf16)."""
    cfg, B, Ll = _case(name)
    sd = R.round_bf16(cases.rdt_sd(cfg))
    batches = [R.round_bf16(R.batch(cfg, B, Ll, seed=s)) for s in A.G17_SEEDS[:4]]
    _, g64 = A.accumulated_grads(sd, batches, cfg)
    _, gref = A.accumulated_grads(sd, batches, cfg, dtype=torch.bfloat16)
    tr = _trainer(cfg, sd, precision="bf16", gradient_accumulation_steps=4)
    for b in batches:
        tr.get_loss(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"],
                    noise=b["noise"], timesteps=b["timesteps"])
        tr.accumulate()
    grads = tr.grads()
    assert set(grads) == set(sd) and all(v.dtype == torch.float32 for v in grads.values())
    bad, rel_h, rel_r = [], [], []
    for key in sd:
        gn = float(g64[key].norm())
        eh, er = float((grads[key].double() - g64[key]).norm()), float((gref[key] - g64[key]).norm())
        rel_h.append(eh / gn), rel_r.append(er / gn)
        if not eh <= max(1.5 * er, 1e-2 * gn):
            bad.append((key, eh / gn, er / gn))
    print(f"[rdt_accum bf16 {name}] per-tensor error / norm: HIP median {np.median(rel_h):.2e} worst {max(rel_h):.2e}; oracle bf16 median "
          f"{np.median(rel_r):.2e} worst {max(rel_r):.2e}")
    assert not bad, bad[:8]


def _state(tr):
    c = lambda d: {key: v.detach().cpu().clone() for key, v in d.items()}
    return dict(p=c(tr.p), m=c(tr._m), v=c(tr._v), shadow=c(tr.shadow))


def _assert_same_state(a, b):
    for part in ("p", "m", "v", "shadow"):
        assert set(a[part]) == set(b[part]) and a[part], part
        for key in a[part]:
            assert a[part][key].view(torch.int32).equal(b[part][key].view(torch.int32)), (part, key)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_k1_is_todays_step(precision):
    """gradient_accumulation_steps=1 and no keyword: bit-equal weights, moments and shadows after three steps; no accumulator exists."""
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in (6, 16, 26)]
    a, b = _trainer(cfg, sd, lr=1e-3, precision=precision), _trainer(cfg, sd, lr=1e-3, precision=precision, gradient_accumulation_steps=1)
    for bt in batches:
        la, lb = _step(a, bt), _step(b, bt)
        assert torch.equal(la, lb) and torch.equal(a.grad_norm, b.grad_norm)
        assert b.sync_gradients and b.micro_step == 0
    _assert_same_state(_state(a), _state(b))
    assert not b._acc and b.global_step == b.step_count == b.ema_updates == 3
    with pytest.raises(RuntimeError):
        b.accumulate()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resume_is_exact(precision, tmp_path):
    """Two windows, save_checkpoint, a fresh trainer from the initial weights, load_checkpoint, two more windows = four windows straight: weights,
    moments, shadows bit-equal, counters equal.  The warm-up scheduler is on, so a wrong step count after the resume would show in the lr."""
    cfg, k = cases.RDT_TINY, 2
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in A.G17_SEEDS[:4 * k]]
    kw = dict(lr=1e-3, precision=precision, gradient_accumulation_steps=k, lr_scheduler="constant_with_warmup", lr_warmup_steps=3)
    straight = _trainer(cfg, sd, **kw)
    losses_straight = [float(_step(straight, b)) for b in batches]
    first = _trainer(cfg, sd, **kw)
    for b in batches[:2 * k - 1]:
        _step(first, b)
    with pytest.raises(RuntimeError):
        first.save_checkpoint(str(tmp_path / "mid"))                # one micro-batch short of the window's end
    _step(first, batches[2 * k - 1])
    ck = str(tmp_path / "checkpoint-2")
    first.save_checkpoint(ck)
    for f in ("checkpoint/model.safetensors", "checkpoint/adam_m.safetensors", "checkpoint/adam_v.safetensors", "ema/model.safetensors", "trainer_state.json"):
        assert os.path.exists(os.path.join(ck, f)), f
    second = _trainer(cfg, sd, **kw)
    second.load_checkpoint(ck)
    assert (second.step_count, second.ema_updates, second.global_step, second.micro_step) == (2, 2 * k, 2, 0)
    losses_resumed = [float(_step(second, b)) for b in batches[2 * k:]]
    assert losses_resumed == losses_straight[2 * k:]
    assert (second.step_count, second.ema_updates, second.global_step, second.lr) == (straight.step_count, straight.ema_updates, straight.global_step, straight.lr)
    assert straight.global_step == 4 and straight.ema_updates == 4 * k
    _assert_same_state(_state(straight), _state(second))
    with pytest.raises(ValueError):
        _trainer(cfg, sd, lr=1e-3, gradient_accumulation_steps=k + 1).load_checkpoint(ck)


def test_finetune_loop_checkpoints_and_resumes(tmp_path):
    """finetune with checkpointing_period=2, stopped after 2 optimizer steps and resumed from "latest" to 4: checkpoint-2 and checkpoint-4 where the
    reference puts them, the final weights in output_dir and output_dir/ema, both loadable by RDTRunner.from_pretrained; the resumed run's weights
    are those of an uninterrupted one."""
    from models.rdt_runner import RDTRunner
    from vlatouch.rdt_train import finetune
    from tests.test_gpu_rdt_train import _runner
    cfg, k = cases.RDT_TINY, 2
    batches = [R.batch(cfg, 3, 12, seed=s) for s in A.G17_SEEDS[:4 * k + 2]]             # two more than max_train_steps needs: the loop must stop
    out = str(tmp_path / "run")
    kw = dict(lr=1e-3, gradient_accumulation_steps=k)
    straight = _runner(cfg).trainer(**kw)
    finetune(straight, batches, max_train_steps=4)
    assert straight.global_step == 4 and straight.ema_updates == 4 * k
    tr = _runner(cfg).trainer(**kw)
    losses = finetune(tr, batches, max_train_steps=2, checkpointing_period=2, output_dir=out)
    assert len(losses) == 2 * k and tr.global_step == 2
    assert sorted(d for d in os.listdir(out) if d.startswith("checkpoint")) == ["checkpoint-2"]
    tr2 = _runner(cfg).trainer(**kw)
    losses2 = finetune(tr2, batches[2 * k:], max_train_steps=4, checkpointing_period=2, output_dir=out, resume_from_checkpoint="latest")
    assert len(losses2) == 2 * k and tr2.global_step == 4
    for f in ("checkpoint-2/trainer_state.json", "checkpoint-4/checkpoint/model.safetensors", "checkpoint-4/checkpoint/adam_m.safetensors",
              "checkpoint-4/checkpoint/adam_v.safetensors", "checkpoint-4/ema/model.safetensors", "checkpoint-4/ema/config.json", "config.json",
              "model.safetensors", "ema/config.json", "ema/model.safetensors"):
        assert os.path.exists(os.path.join(out, f)), f
    _assert_same_state(_state(straight), _state(tr2))
    b = batches[0]
    d = cases.rdt_inputs(cfg, 3, 12)
    pa = lambda rr: rr.predict_action(b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_mask"], b["ctrl_freqs"],
                                      x_init=d["x_init"]).float().cpu()
    final, ema, ck_ema = (RDTRunner.from_pretrained(p, device=DEV) for p in (out, os.path.join(out, "ema"), os.path.join(out, "checkpoint-4", "ema")))
    a_final, a_ema, a_ck = pa(final), pa(ema), pa(ck_ema)
    assert bool(torch.isfinite(a_final).all()) and bool(torch.isfinite(a_ema).all())
    assert torch.equal(a_ema, a_ck), "output_dir/ema and checkpoint-4/ema hold the same averaged weights"
    assert torch.equal(a_final, pa(tr2.sync_to(_runner(cfg))))
    assert float((a_final - a_ema).abs().max()) > 0, "the averaged weights differ from the trained ones"
