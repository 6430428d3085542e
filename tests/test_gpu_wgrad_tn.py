"""vt_gemm_tn (csrc/vt_gemm_tn.hip) and weight_gradient="tn" of the RDT trainer, on the device.

Kernel level.  Exact cases: integer inputs in {-2 .. 2}, for which every partial sum is an integer below 2^24 and any correct summation order
gives the fp64 product bit for bit, on every shape of tests/wgrad_tn_ref.py::KERNEL_CASES (the issue's six plus (96, 136, 264): the kernel's
m-step is 32 and none of the six has M a multiple of it) and on the smallest M whose plan has three row splits for a 128 x 128 weight (a ragged
last split); outputs and workspace NaN-filled between guard words, the workspace of exactly the planned size, two calls bit-equal.  Pitched
operands read in place.  Random cases against fp64 next to the parent's transpose + GEMM + column-sum path.  Refusals write nothing.
Trainer level, every trainer with attention_backward="mfma" and weight_gradient="tn": the rules of test_gradients_bf16 and test_gradients_fp16,
bit-equality of everything that is not a Linear's weight or bias with the "gemm" trainer, thirty steps, accumulation, checkpoints across the
two settings, constructor refusals."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import rdt_train_ref as R
from tests import wgrad_tn_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
GUARD = 64            # guard elements on either side
VT_ERR_ARG = -22


def _guarded(n):
    """-> (whole buffer, the n NaN-filled fp32 elements between two runs of GUARD sevens)."""
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=F32, device=DEV)
    whole[:GUARD] = 7.0
    whole[GUARD + n:] = 7.0
    return whole, whole[GUARD:GUARD + n]


def _guards_ok(whole, n):
    return bool((whole[:GUARD] == 7.0).all()) and bool((whole[GUARD + n:] == 7.0).all())


def _direct(dy, x, *, N=None, K=None, ld_dy=None, ld_x=None, dt=None, ws_short=0):
    """Calls vt_gemm_tn on device tensors with NaN-filled dW, db and workspace, each between guard words; the workspace has exactly the planned
    size (the call is told `ws_short` elements fewer).  -> (return code, dW [N, K], db [N], guards untouched, last error)."""
    from vlatouch import _lib as L
    lib = L.lib()
    M = dy.shape[0]
    N, K = N or dy.shape[1], K or x.shape[1]
    rc, S, _, _, need = W.plan(M, N, K)
    need = need if rc == 0 else 0
    assert need % 4 == 0
    dw_all, dw = _guarded(N * K)
    db_all, db = _guarded(N)
    ws_all, ws = _guarded(need // 4)
    rc = lib.vt_gemm_tn(L.ptr(dy), ld_dy or dy.stride(0), L.ptr(x), ld_x or x.stride(0), L.dt_code(dy.dtype) if dt is None else dt, M, N, K,
                        L.ptr(dw), L.ptr(db), L.ptr(ws) if need else None, need - 4 * ws_short, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    ok = _guards_ok(dw_all, N * K) and _guards_ok(db_all, N) and _guards_ok(ws_all, need // 4)
    return rc, dw.view(N, K), db, ok, lib.vt_last_error().decode()


def _all_cases():
    return W.KERNEL_CASES + [W.split_case()]


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("dtype", [BF, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", range(len(W.KERNEL_CASES) + 1))
def test_exact_cases(case, dtype):
    M, N, K = _all_cases()[case]
    rc, S, rps, _, need = W.plan(M, N, K)
    assert rc == 0
    if case == len(W.KERNEL_CASES):
        assert (N, K) == (128, 128) and S >= 3 and M % rps != 0, (M, S, rps)          # three splits, the last one ragged
    dy, x = W.exact_inputs(M, N, K, dtype)
    dw64, db64 = W.ref(dy, x)
    assert float(dw64.abs().max()) < 2 ** 24
    d, xx = dy.to(DEV), x.to(DEV)
    rc, dw, db, ok, err = _direct(d, xx)
    assert rc == 0, err
    assert ok, "a guard word next to dW, db or the workspace was written"
    print(f"[gemm_tn exact {M}x{N}x{K} {dtype}] splits {S}, rows per split {rps}, workspace {need} B; max |dW| {float(dw64.abs().max()):.0f}")
    assert torch.equal(dw.double().cpu(), dw64), f"dW differs from the exact product in {int((dw.double().cpu() != dw64).sum())} of {N * K} elements"
    assert torch.equal(db.double().cpu(), db64), "db differs from the exact column sums"
    rc2, dw2, db2, ok2, _ = _direct(d, xx)
    assert rc2 == 0 and ok2
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32)), "two calls differ"


def test_the_cases_cover_every_edge_of_the_tiling():
    """Ragged and exact on every axis, and more than one tile / m-step on every axis (tests/wgrad_tn_ref.py says which case does what)."""
    cs = _all_cases()
    for axis, unit in ((0, W.M_STEP), (1, W.TILE), (2, W.TILE)):
        assert any(c[axis] % unit == 0 for c in cs) and any(c[axis] % unit != 0 for c in cs), axis
        assert any(c[axis] > unit and c[axis] % unit != 0 for c in cs) and any(c[axis] < unit for c in cs), axis
    assert any(W.plan(*c)[1] == 1 for c in cs) and any(W.plan(*c)[1] == 2 for c in cs) and W.plan(*cs[-1])[1] >= 3


def test_without_bias_db_is_not_touched():
    from vlatouch.rdt_train import weight_grad_tn
    for M, N, K in (W.KERNEL_CASES[3], W.split_case()):
        dy, x = W.exact_inputs(M, N, K, BF)
        dw, db = weight_grad_tn(dy.to(DEV), x.to(DEV), bias=False)
        assert db is None and torch.equal(dw.double().cpu(), W.ref(dy, x)[0])


# ------------------------------------------------------------------------------------------------ pitched operands
def test_pitched_operands_are_read_in_place():
    from vlatouch.rdt_train import weight_grad_tn
    M = 201
    dyb, xb = W.exact_inputs(M, 256, 96, BF, pitch_dy=512, pitch_x=136)
    dyb, xb = dyb.to(DEV), xb.to(DEV)
    dy, x = dyb[:, 128:384], xb[:, :96]
    assert dy.stride(0) == 512 and x.stride(0) == 136 and not dy.is_contiguous()
    dw, db = weight_grad_tn(dy, x)
    dwc, dbc = weight_grad_tn(dy.contiguous(), x.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(dw.view(torch.int32), dwc.view(torch.int32)) and torch.equal(db.view(torch.int32), dbc.view(torch.int32))
    dw64, db64 = W.ref(dy, x)
    assert torch.equal(dw.double().cpu(), dw64) and torch.equal(db.double().cpu(), db64)
    rc, dw2, db2, ok, err = _direct(dy, x)
    assert rc == 0 and ok, err
    assert torch.equal(dw2.view(torch.int32), dw.view(torch.int32)) and torch.equal(db2.view(torch.int32), db.view(torch.int32))


# ------------------------------------------------------------------------------------------------ random cases
def _parent(dy, x):
    """The parent's weight gradient of a 16-bit Linear: two transposes, the NT GEMM with an fp32 result, the column sum."""
    from vlatouch import ops
    from vlatouch.rdt_train import colsum, transpose_pad
    return ops.gemm(transpose_pad(dy), transpose_pad(x), out_dtype=F32), colsum(dy)


@pytest.mark.parametrize("case", range(len(W.KERNEL_CASES) + 1))
def test_random_cases_against_fp64(case):
    """N(0, 1) inputs rounded to bf16.  e = max-abs error over max_nk sum_m |dy x| (db: over max_n sum_m |dy|); e_tn <= max(1.5 e_parent,
    M 2^-24): the second term bounds M round-to-nearest fp32 additions; a dropped row costs some 1 / M."""
    from vlatouch.rdt_train import weight_grad_tn
    M, N, K = _all_cases()[case]
    dy, x = W.random_inputs(M, N, K)
    dw64, db64 = W.ref(dy, x)
    uw, ub = W.units(dy, x)
    d, xx = dy.to(DEV), x.to(DEV)
    dw, db = weight_grad_tn(d, xx)
    dwp, dbp = _parent(d, xx)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    e_w, e_wp = float((dw.double().cpu() - dw64).abs().max()) / uw, float((dwp.double().cpu() - dw64).abs().max()) / uw
    e_b, e_bp = float((db.double().cpu() - db64).abs().max()) / ub, float((dbp.double().cpu() - db64).abs().max()) / ub
    floor = M * 2.0 ** -24
    print(f"[gemm_tn random {M}x{N}x{K}] dW: tn {e_w:.3e}, parent {e_wp:.3e}; db: tn {e_b:.3e}, parent {e_bp:.3e}; floor M 2^-24 = {floor:.3e}; "
          f"splits {W.plan(M, N, K)[1]}")
    assert e_w <= max(1.5 * e_wp, floor), ("dW", e_w, e_wp, floor)
    assert e_b <= max(1.5 * e_bp, floor), ("db", e_b, e_bp, floor)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["fp32", "N=12", "K=20", "pitch 12", "short workspace"])
def test_refusals_write_nothing(what):
    M = 353 if what == "short workspace" else 16
    dy = torch.ones(M, 128, dtype=F32 if what == "fp32" else BF, device=DEV)
    x = torch.ones(M, 128, dtype=dy.dtype, device=DEV)
    kw = {"fp32": dict(), "N=12": dict(N=12), "K=20": dict(K=20), "pitch 12": dict(N=8, ld_dy=12), "short workspace": dict(ws_short=1)}[what]
    if what == "short workspace":
        assert W.plan(M, 128, 128)[1] >= 3
    rc, dw, db, ok, err = _direct(dy, x, **kw)
    print(f"[gemm_tn refusal {what}] code {rc}: {err}")
    assert rc == VT_ERR_ARG and "vt_gemm_tn" in err
    assert ok and bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), "a refused call wrote an output"


def test_python_refuses_fp32_mixed_dtypes_and_bad_widths():
    from vlatouch.rdt_train import linear_bwd, weight_grad_tn
    t = lambda n, dt: torch.ones(16, n, dtype=dt, device=DEV)
    with pytest.raises(ValueError, match="bf16"):
        weight_grad_tn(t(16, F32), t(16, F32))
    with pytest.raises(ValueError, match="bf16"):
        weight_grad_tn(t(16, BF), t(16, FP16))
    with pytest.raises(ValueError, match="N=12"):
        weight_grad_tn(t(12, BF), t(16, BF))
    with pytest.raises(ValueError, match="K=20"):
        weight_grad_tn(t(16, BF), t(20, BF))
    with pytest.raises(ValueError, match="kernel"):
        linear_bwd(t(16, BF), t(16, BF), t(16, BF), kernel="nt")
    with pytest.raises(ValueError, match="16-bit"):
        linear_bwd(t(16, F32), t(16, F32), t(16, F32), kernel="tn")


# ------------------------------------------------------------------------------------------------ the trainer
KW = dict(attention_backward="mfma", weight_gradient="tn")
KEYS = ("lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs")


def _trainer(cfg, sd, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], device=DEV, **kw)


def _get_loss(tr, b, **kw):
    return tr.get_loss(*[b[k] for k in KEYS], noise=b["noise"], timesteps=b["timesteps"], **kw)


def _step(tr, b):
    return tr.train_step(*[b[k] for k in KEYS], noise=b["noise"], timesteps=b["timesteps"])


def _linear_keys(sd):
    names = {k[:-len(".weight")] for k, v in sd.items() if k.endswith(".weight") and v.dim() == 2}
    return {f"{n}.weight" for n in names} | {f"{n}.bias" for n in names}


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_trainer_gradients_bf16(name):
    """The rule and the case sizes of tests/test_gpu_rdt_train.py::test_gradients_bf16 under "tn": per tensor e <= max(1.5 e_ref, 1e-2 |g|), all
    parameters together e <= 1.5 e_ref (e_ref: the oracle in bf16 on the CPU, both against fp64 from the same bf16-rounded weights and inputs).
    Every gradient that is not a Linear's weight or bias is bit-equal to the "gemm" trainer's (dx does not change), and two "tn" trainers agree
    bit for bit."""
    cfg, B, Ll = (cases.RDT_TINY, 3, 12) if name == "tiny" else (cases.RDT_WIDE, 2, 20)
    sd, b = R.round_bf16(cases.rdt_sd(cfg)), R.round_bf16(R.batch(cfg, B, Ll))
    l64, g64 = R.loss_and_grads(sd, b, cfg)
    lref, gref = R.loss_and_grads(sd, b, cfg, dtype=torch.bfloat16)
    runs = {}
    for kind in ("tn", "tn again", "gemm"):
        tr = _trainer(cfg, sd, precision="bf16", attention_backward="mfma", weight_gradient=kind.split()[0])
        assert tr.weight_gradient == kind.split()[0]
        runs[kind] = (float(_get_loss(tr, b)), {k: v.detach().cpu() for k, v in tr.grads().items()})
    loss, grads = runs["tn"]
    assert set(grads) == set(sd) and all(v.dtype == F32 and bool(torch.isfinite(v).all()) for v in grads.values())
    tot_h = tot_r = 0.0
    rel_h, rel_r, bad = [], [], []
    for k in sd:
        gn = float(g64[k].norm())
        eh, er = float((grads[k].double() - g64[k]).norm()), float((gref[k] - g64[k]).norm())
        tot_h, tot_r = tot_h + eh * eh, tot_r + er * er
        rel_h.append(eh / gn), rel_r.append(er / gn)
        if not eh <= max(1.5 * er, 1e-2 * gn):
            bad.append((k, eh / gn, er / gn))
    tot_h, tot_r, gall = tot_h ** 0.5, tot_r ** 0.5, sum(float(v.norm()) ** 2 for v in g64.values()) ** 0.5
    print(f"[rdt_train bf16 {name} tn] loss {loss:.4f} (oracle bf16 {lref:.4f}, fp64 {l64:.4f}); per-tensor error / norm: HIP median {np.median(rel_h):.2e} "
          f"worst {max(rel_h):.2e}, oracle bf16 median {np.median(rel_r):.2e} worst {max(rel_r):.2e}; all parameters: HIP {tot_h / gall:.2e}, oracle "
          f"{tot_r / gall:.2e}")
    assert not bad, bad[:8]
    assert tot_h <= 1.5 * tot_r, (tot_h, tot_r)
    lin = _linear_keys(sd)
    rest = [k for k in sd if k not in lin]
    assert lin and any("pos_embed" in k for k in rest) and any("norm" in k for k in rest)
    assert runs["gemm"][0] == loss
    for k in rest:
        assert torch.equal(grads[k].view(torch.int32), runs["gemm"][1][k].view(torch.int32)), f"{k}: differs from the 'gemm' trainer"
    assert any(not torch.equal(grads[k], runs["gemm"][1][k]) for k in lin), "the 'tn' trainer produced the 'gemm' trainer's bits: was vt_gemm_tn called?"
    for k in sd:
        assert torch.equal(grads[k].view(torch.int32), runs["tn again"][1][k].view(torch.int32)), f"{k}: two 'tn' trainers differ"


def test_trainer_gradients_fp16():
    """tests/test_gpu_rdt_train_fp16.py::test_gradients_fp16's rule on RDT_TINY under "tn": static loss_scale=1024, per tensor
    e <= max(1.5 e_ref, 1.25e-3 |g|), all parameters together e <= 1.5 e_ref, e_ref the recorded error of the oracle in fp16."""
    from tests import rdt_train16_ref as R16
    cfg, sd, b, l64, g64 = R16.problem("tiny")
    ref = R16.oracle_errors("tiny")
    tr = _trainer(cfg, sd, precision="fp16", loss_scale=1024.0, **KW)
    loss = float(_get_loss(tr, b))
    grads = {k: v.double().cpu() / 1024.0 for k, v in tr.grads().items()}
    assert set(grads) == set(sd) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    bad, rel_h = [], []
    for k in sd:
        gn = float(g64[k].norm())
        eh, er = float((grads[k] - g64[k]).norm()), ref["tensor_error"][k]
        rel_h.append(eh / gn)
        if not eh <= max(1.5 * er, 1.25e-3 * gn):
            bad.append((k, eh / gn, er / gn))
    (tot_h, gall), tot_r = R16.total_error(grads, g64), ref["total_error"]
    print(f"[rdt_train fp16 tiny tn] loss {loss:.5f} (fp64 {l64:.5f}); per-tensor error / norm: HIP median {np.median(rel_h):.2e} worst {max(rel_h):.2e}; "
          f"all parameters: HIP {tot_h / gall:.2e}, oracle {tot_r / gall:.2e}")
    assert abs(loss - l64) <= 2e-3 * abs(l64), (loss, l64)
    assert not bad, bad[:8]
    assert tot_h <= 1.5 * tot_r, (tot_h, tot_r)


@pytest.mark.parametrize("prediction_type", ["sample", "epsilon"])
def test_trainer_thirty_steps_halve_the_loss(prediction_type):
    """tests/test_gpu_rdt_train.py::test_thirty_steps_halve_the_loss under "tn", bf16."""
    from tests.test_gpu_rdt_train import _runner
    cfg = cases.RDT_TINY
    b = R.batch(cfg, 3, 12)
    tr = _runner(cfg, prediction_type).trainer(lr=1e-3, precision="bf16", **KW)
    assert tr.weight_gradient == "tn"
    first = float(_step(tr, b))
    for _ in range(29):
        _step(tr, b)
    last = float(_get_loss(tr, b, backward=False))
    print(f"[rdt_train 30 steps {prediction_type} bf16 tn] loss {first:.4f} -> {last:.4f} ({last / first:.3f} of the first)")
    assert last < 0.5 * first, (first, last)


def test_trainer_accumulation_window_is_the_concatenated_batch():
    """gradient_accumulation_steps=2 under "tn": the window's gradient against the fp64 gradient of the concatenated batch, per tensor
    e <= max(1.5 e_ref, 1e-2 |g|) with e_ref the bf16 oracle accumulated the same way (tests/test_gpu_rdt_accum.py's bf16 rule), beside one "tn"
    step on the concatenated batch itself under the same rule; then a window of train_step calls takes one optimizer step."""
    from tests import rdt_accum_ref as A
    cfg = cases.RDT_TINY
    sd = R.round_bf16(cases.rdt_sd(cfg))
    batches = [R.round_bf16(R.batch(cfg, 3, 12, seed=s)) for s in A.G17_SEEDS[:2]]
    cat = A.concat_batch(batches)
    _, g64 = R.loss_and_grads(sd, cat, cfg)
    _, gref = A.accumulated_grads(sd, batches, cfg, dtype=torch.bfloat16)
    win = _trainer(cfg, sd, precision="bf16", gradient_accumulation_steps=2, **KW)
    for b in batches:
        _get_loss(win, b)
        win.accumulate()
    one = _trainer(cfg, sd, precision="bf16", **KW)
    _get_loss(one, cat)
    for tag, grads in (("window k=2", win.grads()), ("one step", one.grads())):
        bad, rel = [], []
        for k in sd:
            gn = float(g64[k].norm())
            eh, er = float((grads[k].double().cpu() - g64[k]).norm()), float((gref[k] - g64[k]).norm())
            rel.append(eh / gn)
            if not eh <= max(1.5 * er, 1e-2 * gn):
                bad.append((k, eh / gn, er / gn))
        print(f"[rdt_accum bf16 tn {tag}] per-tensor error / norm against fp64 of the concatenated batch: median {np.median(rel):.2e} worst {max(rel):.2e}")
        assert not bad, (tag, bad[:8])
    tr2 = _trainer(cfg, sd, lr=1e-3, precision="bf16", gradient_accumulation_steps=2, **KW)
    for n, b in enumerate(batches):
        assert np.isfinite(float(_step(tr2, b))) and tr2.sync_gradients == (n == 1)
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
    """A checkpoint saved under "gemm" resumes under "tn" and back; trainer_state.json does not record the setting."""
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in (6, 16, 26, 36)]
    kw = dict(lr=1e-3, precision="bf16", attention_backward="mfma")
    gemm = _trainer(cfg, sd, weight_gradient="gemm", **kw)
    for b in batches[:2]:
        _step(gemm, b)
    ck_g = str(tmp_path / "gemm-2")
    gemm.save_checkpoint(ck_g)
    tn = _trainer(cfg, sd, weight_gradient="tn", **kw)
    tn.load_checkpoint(ck_g)
    assert (tn.step_count, tn.ema_updates, tn.micro_step) == (2, 2, 0) and tn.weight_gradient == "tn"
    _assert_same_state(_state(gemm), _state(tn))
    ck_t0 = str(tmp_path / "tn-2")
    tn.save_checkpoint(ck_t0)
    with open(os.path.join(ck_g, "trainer_state.json"), "rb") as f, open(os.path.join(ck_t0, "trainer_state.json"), "rb") as g:
        jg, jt = f.read(), g.read()
    assert jg == jt and "weight_gradient" not in json.loads(jg) and b'"tn"' not in jt
    assert np.isfinite(float(_step(tn, batches[2]))) and tn.global_step == 3
    ck_t = str(tmp_path / "tn-3")
    tn.save_checkpoint(ck_t)
    back = _trainer(cfg, sd, weight_gradient="gemm", **kw)
    back.load_checkpoint(ck_t)
    _assert_same_state(_state(tn), _state(back))
    assert np.isfinite(float(_step(back, batches[3]))) and back.global_step == 4


def test_constructor_refusals_and_the_runner():
    from tests.test_gpu_rdt_train import _runner
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    with pytest.raises(ValueError, match="weight_gradient"):
        _trainer(cfg, sd, precision="bf16", weight_gradient="nt")
    with pytest.raises(ValueError, match="bf16"):
        _trainer(cfg, sd, precision="fp32", weight_gradient="tn")
    narrow = dict(sd)
    narrow["lang_adaptor.0.weight"] = sd["lang_adaptor.0.weight"][:, :12].clone()
    with pytest.raises(ValueError, match=r"lang_adaptor\.0\.weight"):
        _trainer(cfg, narrow, precision="bf16", weight_gradient="tn")
    assert _trainer(cfg, sd, precision="bf16").weight_gradient == "gemm"
    r = _runner(cfg)
    tr = r.trainer(precision="bf16", **KW)
    assert tr.weight_gradient == "tn" and r.trainer().weight_gradient == "gemm"
    assert np.isfinite(float(_get_loss(tr, R.batch(cfg, 3, 12))))


def test_composes_with_the_8bit_optimizer_and_fp16_loss_scaling():
    cfg = cases.RDT_TINY
    sd, b = cases.rdt_sd(cfg), R.batch(cfg, 3, 12)
    for kw in (dict(precision="bf16", optimizer="adamw8bit"), dict(precision="fp16", loss_scale=1024.0, gradient_accumulation_steps=2)):
        tr = _trainer(cfg, sd, lr=1e-3, **kw, **KW)
        losses = [float(_step(tr, b)) for _ in range(4)]
        assert all(np.isfinite(l) for l in losses) and tr.global_step == 4 // tr.k and np.isfinite(float(tr.grad_norm)), (kw, losses)
