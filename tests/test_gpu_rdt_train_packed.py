"""`RdtTrainer(small_batch_linear="packed")` on cases.RDT_TINY (hidden 256: its square Linears meet the small-M packed tile's N % 64 and
K % 256; B = 3 with 12 language tokens gives 33 rows): the packed path is really taken, the default is the trainer it was, the gradients meet
the bars of the existing 16-bit trainer tests against fp64, runs are reproducible, launches above 512 rows keep their bits, and every way the
16-bit copies are refreshed (construction, step, skipped step, load_checkpoint) keeps the packed copies current."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import rdt_train16_ref as R16
from tests import rdt_train_ref as R
from tests import rdt_trainer_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = cases.RDT_TINY
ROWS = K.B * (CFG["horizon"] + 3)                   # 33
PACKED = dict(small_batch_linear="packed")
MFMA_TN = dict(attention_backward="mfma", weight_gradient="tn")
SQUARE = ("attn.proj", "cross_attn.q", "cross_attn.proj", "ffn.fc1", "ffn.fc2")


def _trainer(sd, **kw):
    return K._trainer(CFG, sd, DEV, **kw)


def _get_loss(tr, b, **kw):
    a, k = K._args(b)
    return tr.get_loss(*a, **k, **kw)


def _step(tr, b):
    a, k = K._args(b)
    return tr.train_step(*a, **k)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _state(tr):
    c = lambda d: {k: v.detach().clone() for k, v in d.items()}
    return dict(p=c(tr.p), m=c(tr._m), v=c(tr._v), am=c(tr._am), av=c(tr._av), shadow=c(tr.shadow))


def _assert_same_state(a, b, what):
    for part in a:
        assert _same(a[part], b[part]), f"{what}: {part} differs"


def _batches(seeds=(6, 16, 26, 36), B=K.B):
    return [R.batch(CFG, B, K.LANG_LEN, seed=s) for s in seeds]


# ------------------------------------------------------------------------------------------------ the path is taken
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_square_linears_run_on_the_packed_tile_only_under_packed(precision):
    """Forward and data gradient of every square Linear of every block: route `PWS` under "packed", as recorded from the very blocks the
    trainer launched; under "gemm" the same launches (rebuilt as `_linear` builds them) go where they go without a packed copy, not to `PWS`."""
    from vlatouch import ops
    sd, b = cases.rdt_sd(CFG), _batches()[0]
    extra = dict(loss_scale=1024.0) if precision == "fp16" else {}
    tr = _trainer(sd, precision=precision, **extra, **PACKED)
    assert tr.small_batch_linear == "packed" and tr.packed is not None
    tr.packed.log = []
    assert np.isfinite(float(_get_loss(tr, b)))
    seen = {(tag, rows): route for tag, rows, route in tr.packed.log}
    for i in range(CFG["depth"]):
        for lin in SQUARE:
            for leg in ("forward", "dgrad"):
                assert seen.get((f"model.blocks.{i}.{lin}/{leg}", ROWS)) == "PWS", (i, lin, leg, seen.get((f"model.blocks.{i}.{lin}/{leg}", ROWS)))
            key = f"model.blocks.{i}.{lin}.weight"
            assert key in tr.wp and key in tr.wtp
    # the qkv projection (768 x 256) qualifies both ways too; the narrow final projection (K = 256, N = 128 forward: fits; data gradient
    # N = 256, K = 128: does not) shows a weight with one packed form only
    assert seen[("model.blocks.0.attn.qkv/forward", ROWS)] == "PWS" and seen[("model.blocks.0.attn.qkv/dgrad", ROWS)] == "PWS"
    fc2 = "model.final_layer.ffn_final.fc2.weight"
    assert fc2 in tr.wp and fc2 not in tr.wtp and tr._forms[fc2] == ("w16", "w16t", "wp")
    assert all(route == "PWS" for _, _, route in tr.packed.log), "a launch that was offered a packed copy at <= 512 rows went elsewhere"

    plain = _trainer(sd, precision=precision, **extra)
    assert plain.small_batch_linear == "gemm" and plain.packed is None and not plain.wp and not plain.wtp
    x = torch.zeros(ROWS, CFG["hidden"], dtype=plain.adt, device=DEV)
    for lin in SQUARE:
        name = f"model.blocks.0.{lin}"
        fwd = ops.gemm_route(ops.gemm_params(x, plain.w16[f"{name}.weight"], plain.p[f"{name}.bias"])[0])
        dg = ops.gemm_route(ops.gemm_params(x, plain.w16t[f"{name}.weight"])[0])
        assert fwd == dg == "REG", (lin, fwd, dg)            # the register-staged kernel the committed trace shows for these launches


def test_the_default_gives_the_parents_digests(monkeypatch):
    """small_batch_linear="gemm", spelled out, on the 16-bit cases of tests/rdt_trainer_cases.py: sha256 for sha256 the recorded trainer."""
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        golden = json.load(f)["sha256"]
    names = [n for n, c in K.CASES.items() if c[1].get("precision") in ("bf16", "fp16")]
    assert names == ["bf16_wave_gemm", "bf16_mfma_tn_k2", "fp16_mfma_tn_adam8"]
    for n in names:
        over, kw, micro, masked = K.CASES[n]
        monkeypatch.setitem(K.CASES, n, (over, dict(kw, small_batch_linear="gemm"), micro, masked))
    got = {}
    for n in names:
        K._case(got, n, DEV)
    want = {k: v for k, v in golden.items() if k.split("/")[0] in names}
    assert list(got) == list(want)
    diff = K.differing(want, got)
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ parity against fp64
# The per-tensor bars of the default path, as tests/test_gpu_rdt_train.py::test_gradients_bf16 and tests/test_gpu_rdt_train_fp16.py::
# test_gradients_fp16 state them (they are written inside those tests, so they are repeated here, not widened): e <= max(1.5 e_ref, floor |g|)
# per tensor and e <= 1.5 e_ref over all parameters, e_ref the error of the oracle run in the same 16-bit type on the CPU; floor 1e-2 for bf16
# and 1.25e-3 for fp16.  The step losses are held to the fp64 run of the same three steps at 2e-3 (the fp16 test's loss bar) and, for bf16's
# 8 x coarser mantissa, 1.6e-2.
PARITY = {"bf16_mfma_tn": (dict(precision="bf16", **MFMA_TN), 1e-2, 1.6e-2),
          "bf16_defaults": (dict(precision="bf16"), 1e-2, 1.6e-2),
          "fp16_dynamic": (dict(precision="fp16", loss_scale="dynamic"), 1.25e-3, 2e-3)}
_ORACLE = {}


def _problem(kind):
    if kind not in _ORACLE:
        if kind.startswith("bf16"):
            cfg, sd, b, l64, g64 = R16.problem_bf16("tiny")
            _, gref = R.loss_and_grads(sd, b, cfg, dtype=torch.bfloat16)
            err = {k: float((gref[k] - g64[k]).norm()) for k in g64}
            tot = sum(e * e for e in err.values()) ** 0.5
        else:
            cfg, sd, b, l64, g64 = R16.problem("tiny")
            ref = R16.oracle_errors("tiny")
            err, tot = ref["tensor_error"], ref["total_error"]
        _ORACLE[kind] = (sd, b, l64, g64, err, tot)
    return _ORACLE[kind]


@pytest.mark.parametrize("setting", ["packed", "gemm"])
@pytest.mark.parametrize("case", list(PARITY))
def test_gradients_and_three_steps_against_fp64(case, setting):
    kw, floor, loss_bar = PARITY[case]
    sd, b, l64, g64, err, tot_r = _problem(case[:4])
    tr = _trainer(sd, small_batch_linear=setting, **kw)
    loss = float(_get_loss(tr, b))
    scale = tr.loss_scale_value
    grads = {k: v.double().cpu() / scale for k, v in tr.grads().items()}
    assert set(grads) == set(sd) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    bad, rel = [], []
    for k in sd:
        gn = float(g64[k].norm())
        eh = float((grads[k] - g64[k]).norm())
        rel.append(eh / gn)
        if not eh <= max(1.5 * err[k], floor * gn):
            bad.append((k, eh / gn, err[k] / gn))
    tot_h, gall = R16.total_error(grads, g64)
    print(f"[rdt_train {case} {setting}] loss {loss:.5f} (fp64 {l64:.5f}); per-tensor error / norm: median {np.median(rel):.2e} worst {max(rel):.2e}; "
          f"all parameters: HIP {tot_h / gall:.2e}, oracle {tot_r / gall:.2e}")
    assert abs(loss - l64) <= loss_bar * abs(l64), (loss, l64)
    assert not bad, bad[:8]
    assert tot_h <= 1.5 * tot_r, (tot_h, tot_r)
    # three steps: each loss against the fp64 run of the same steps from the same rounded weights
    rnd = R.round_bf16 if case.startswith("bf16") else R16.round_fp16
    batches = [rnd(x) for x in _batches((6, 16, 26))]
    r64 = R.train_steps(sd, batches, CFG, dtype=torch.float64, lr=K.LR, weight_decay=1e-2, max_grad_norm=1.0)
    tr = _trainer(sd, small_batch_linear=setting, **kw)
    for n, bt in enumerate(batches):
        ls = float(_step(tr, bt))
        print(f"[rdt_train {case} {setting}] step {n + 1}: loss {ls:.5f} (fp64 {r64[n]['loss']:.5f})")
        assert abs(ls - r64[n]["loss"]) <= loss_bar * r64[n]["loss"], (n, ls, r64[n]["loss"])
    assert tr.step_count == 3 and tr.skipped_steps == 0 and all(bool(torch.isfinite(v).all()) for v in tr.p.values())


@pytest.mark.parametrize("setting", ["packed", "gemm"])
def test_thirty_steps_halve_the_loss(setting):
    """tests/test_gpu_rdt_train.py::test_thirty_steps_halve_the_loss's bound, bf16 with the MFMA backward and the one-launch weight gradient."""
    sd, b = cases.rdt_sd(CFG), R.batch(CFG, K.B, K.LANG_LEN)
    tr = _trainer(sd, precision="bf16", small_batch_linear=setting, **MFMA_TN)
    first = float(_step(tr, b))
    for _ in range(29):
        _step(tr, b)
    last = float(_get_loss(tr, b, backward=False))
    print(f"[rdt_train 30 steps bf16 {setting}] loss {first:.4f} -> {last:.4f} ({last / first:.3f} of the first)")
    assert last < 0.5 * first, (first, last)


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("k", [1, 2])
def test_two_packed_trainers_agree_bit_for_bit(k):
    sd, batches = cases.rdt_sd(CFG), _batches()
    trs = [_trainer(sd, precision="bf16", gradient_accumulation_steps=k, **MFMA_TN, **PACKED) for _ in range(2)]
    gemm = _trainer(sd, precision="bf16", gradient_accumulation_steps=k, **MFMA_TN)
    for n in range(3 * k):
        bt = batches[n % len(batches)]
        la, lb = _step(trs[0], bt), _step(trs[1], bt)
        _step(gemm, bt)
        assert torch.equal(_bits(la.reshape(1)), _bits(lb.reshape(1))), n
    assert trs[0].step_count == 3
    _assert_same_state(_state(trs[0]), _state(trs[1]), f"k = {k}")
    assert not _same(trs[0].p, gemm.p), "the packed trainer gave the 'gemm' trainer's bits: was the packed tile used?"


def test_above_512_rows_packed_gives_the_bits_of_gemm():
    """B = 48: 528 trajectory rows, 576 language and 1 152 image rows.  No launch of a block, of the final layer or of the language / image
    adaptors is offered a packed copy; what still is are the Linears that run on fewer rows whatever the batch (the two embedders, 48 rows, and
    the state adaptor, 432).  With those weights' packed forms dropped from the trainer no launch is offered one, and loss and gradients are
    the 'gemm' trainer's bit for bit."""
    from tests.rdt_accum_ref import concat_batch
    sd, b = cases.rdt_sd(CFG), concat_batch(_batches(tuple(6 + 10 * i for i in range(16))))      # sixteen batches of three samples
    assert b["timesteps"].numel() == 48 and 48 * (CFG["horizon"] + 3) == 528
    pk, plain = _trainer(sd, precision="bf16", **MFMA_TN, **PACKED), _trainer(sd, precision="bf16", **MFMA_TN)
    pk.packed.log = []
    _get_loss(pk, b)
    lg, gg = _get_loss(plain, b), plain.grads()
    small = {tag.split("/")[0] for tag, rows, _ in pk.packed.log}
    assert all(rows <= 512 for _, rows, _ in pk.packed.log)
    assert small and all(t.startswith(("model.t_embedder", "model.freq_embedder", "state_adaptor")) for t in small), sorted(small)
    for name in small:
        pk.wp.pop(f"{name}.weight", None), pk.wtp.pop(f"{name}.weight", None)
    pk.packed.log = []
    lp = _get_loss(pk, b)
    assert pk.packed.log == []
    assert torch.equal(_bits(lp.reshape(1)), _bits(lg.reshape(1)))
    assert _same(pk.grads(), gg), [k for k, v in pk.grads().items() if not torch.equal(_bits(v), _bits(gg[k]))][:8]


def test_checkpoints_resume_under_either_setting(tmp_path):
    """packed, two steps, save.  A fresh packed trainer that loads it takes the third step of the uninterrupted packed run bit for bit (so
    load_checkpoint refreshed the packed copies); a "gemm" trainer that loads it takes the third step of a packed twin switched to "gemm" in
    place at that step.  trainer_state.json does not record the setting."""
    sd, batches = cases.rdt_sd(CFG), _batches()
    kw = dict(precision="bf16", **MFMA_TN)
    run, twin = _trainer(sd, **kw, **PACKED), _trainer(sd, **kw, **PACKED)
    for bt in batches[:2]:
        _step(run, bt), _step(twin, bt)
    ck = str(tmp_path / "packed-2")
    run.save_checkpoint(ck)
    with open(os.path.join(ck, "trainer_state.json")) as f:
        txt = f.read()
    assert "small_batch_linear" not in txt and "packed" not in txt
    fresh, plain = _trainer(sd, **kw, **PACKED), _trainer(sd, **kw)
    stale = {k: v.clone() for k, v in fresh.wp.items()}
    fresh.load_checkpoint(ck), plain.load_checkpoint(ck)
    assert any(not torch.equal(_bits(fresh.wp[k]), _bits(stale[k])) for k in stale), "load_checkpoint left the packed copies of the initial weights"
    assert _same(fresh.wp, run.wp) and _same(fresh.wtp, run.wtp) and _same(fresh.w16, run.w16) and _same(fresh.w16t, run.w16t)
    assert _same(plain.w16, run.w16) and _same(plain.w16t, run.w16t) and not plain.wp
    l_run, l_fresh = _step(run, batches[2]), _step(fresh, batches[2])
    assert torch.equal(_bits(l_run.reshape(1)), _bits(l_fresh.reshape(1)))
    _assert_same_state(_state(run), _state(fresh), "packed -> packed")
    # the switch, in place: drop the packed forms and the scratch, refresh as "gemm" refreshes
    twin.small_batch_linear, twin.packed = "gemm", None
    twin.wp.clear(), twin.wtp.clear(), twin._forms.clear()
    twin._refresh16()
    l_twin, l_plain = _step(twin, batches[2]), _step(plain, batches[2])
    assert torch.equal(_bits(l_twin.reshape(1)), _bits(l_plain.reshape(1)))
    _assert_same_state(_state(twin), _state(plain), "packed -> gemm")
    assert not _same(run.p, plain.p)


def test_skipped_fp16_steps_leave_the_packed_copies_current():
    """The fp16_mfma_tn_adam8 case (loss scale 2^24, growth_interval 2) under "packed": after every call, skipped or not, each weight's four
    forms equal a fresh vt_refresh16 of its master."""
    from vlatouch import ops
    over, kw, _, _ = K.CASES["fp16_mfma_tn_adam8"]
    assert not over and kw["loss_scale"]["init_scale"] == 2.0 ** 24
    sd, batches = cases.rdt_sd(CFG), K._batches(CFG, False)
    tr = _trainer(sd, **kw, **PACKED)
    stores = {"w16": tr.w16, "w16t": tr.w16t, "wp": tr.wp, "wtp": tr.wtp}
    skipped = clean = 0
    for n in range(K.FP16_MAX_STEPS):
        p_before = {k: v.clone() for k, v in tr.p.items()}
        assert np.isfinite(float(_step(tr, batches[n % len(batches)])))
        if tr.last_step_skipped:
            skipped += 1
            assert _same(tr.p, p_before)
        else:
            clean += 1
        for key, forms in tr._forms.items():
            fresh = ops.refresh16(tr.p[key], torch.float16, forms)
            for f in forms:
                assert torch.equal(_bits(stores[f][key]), _bits(fresh[f])), (n, key, f)
        if clean >= 2:
            break
    assert skipped >= 1 and clean >= 2, (skipped, clean)
