"""The ViT driver (csrc/vt_models.hip: vt_dino_embed, vt_dino_forward) against the float64 statement of tests/vit_ref.py: the front end alone
(statistics, the two decisions, patchify, patch embedding), the blocks with the pruned last block against its unpruned statement, and SigLIP's
scaling.

The measure is vit_ref.row_err: per output row max|out - ref| / max|ref row|.  A bar is 3 x the largest CPU-measured cost of its group
(vit_ref.COSTS, held to the measurement by tests/test_vit_ref_host.py; the 3 covers an accumulation order that differs from the CPU's):

  group    cost fp32   bf16     fp16      bar fp32   bf16     fp16
  front    1.1e-6      4.5e-3   5.9e-4    3.3e-6     1.35e-2  1.77e-3
  dino     8.5e-7      9.8e-3   1.5e-3    2.55e-6    2.94e-2  4.5e-3
  siglip   8.6e-7      6.8e-3   8.7e-4    2.58e-6    2.04e-2  2.61e-3

Measured on the MI355X (largest over a group's cases; every case passed):

  group                 fp32      bf16      fp16
  front  D = 64         1.40e-6   4.50e-3   5.89e-4
  front  D = 128        1.30e-6   4.13e-3   5.39e-4
  dino   every token    1.13e-6   9.61e-3   1.25e-3     (d128_l2 / d128_swiglu the largest)
  dino   pruned CLS     1.25e-6   9.23e-3   1.25e-3     (d512_splitk fp32 the largest)
  siglip every token    1.33e-6   6.50e-3   8.87e-4
  siglip, ImageNet statistics through SiglipEngine.forward and SiglipVisionTower: inside the bars; with SiglipEngine put back on
  VT_IMGNORM_OFF (the parent's call) both give 1.40 in every mode: the whole batch is divided by 255 and the final LayerNorm saturates the error.
  decisions and large walks: flags[0..2] equal in all 17 + 4 cases; the mean's error at most 0.19 of its bound (0.10 / 0.05 on the large walks).

The decisions (flags[0..2]) are compared exactly; flags[3], the mean, against vit_ref.mean_bound, which follows from vt_k_imgstats' launch
geometry alone."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import vit_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def upload(a: np.ndarray, dev, offset: bool) -> torch.Tensor:
    """The frames on the device, from an allocation's base or one element past it (4 bytes fp32, 1 byte uint8) inside a larger buffer."""
    t = torch.from_numpy(a)
    if not offset:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def embed_poisoned(eng, cams, layout, pre_scale=1.0, mode=R.AUTO):
    """eng.embed with the workspace and the output filled with 0xFF bytes (NaN in every format) first: a padding column left unzeroed or a row
    left unwritten shows as a non-finite token."""
    from vlatouch import _lib as L
    n, B = len(cams), cams[0].shape[0]
    res = cams[0].shape[1] if layout == "nhwc" else cams[0].shape[2]
    eng._ws.get(L.lib().vt_dino_workspace_bytes(eng._h, n * B, res)).fill_(255)
    out = torch.empty(n, B, (res // 14) ** 2 + 1, eng.hidden, dtype=torch.float32, device=eng.device)
    out.view(torch.uint8).fill_(255)
    got = eng.embed(cams, nhwc=layout == "nhwc", pre_scale=pre_scale, norm_mode=mode, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu(), eng.last_flags.cpu().double().numpy()


def check_flags(what, fl, ref, frames, pre_scale, aligned):
    """fl: the driver's {scale, normalised, max, mean}; ref: prepare's.  The decisions exactly, the mean within the geometry's bound."""
    scale, norm, mx, mean = ref
    assert fl[1] == norm, (what, "normalise", fl, ref)
    assert abs(fl[0] / scale - 1.0) < 2.0 ** -22, (what, "scale", fl, ref)          # the same divisor (1, 255, 255^2); fl(fl(1/255) / 255) rounds twice
    if pre_scale == 1.0:
        assert fl[2] == mx, (what, "max", fl, ref)
    else:
        assert abs(fl[2] / mx - 1.0) <= 2.0 ** -23, (what, "max", fl, ref)          # fl(max * fl(1/255)): two roundings
    bound = R.mean_bound(frames.size, frames.itemsize, aligned)
    e = abs(fl[3] - mean) / mean                                                    # the frames are non-negative: mean|x| = mean
    assert e <= bound, (what, "mean", e, bound)
    return e / bound


def dino_engine(dev, hidden, heads, layers, prec, swiglu=False, out_all=False):
    from vlatouch.engine import DinoEngine
    sd = R.dino_shapes_sd(hidden, layers, swiglu=swiglu, image_size=42)
    return sd, DinoEngine(sd, heads=heads, precision=prec, device=dev, out_all=out_all)


# ------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("model", R.FRONT_MODELS, ids=lambda m: f"d{m[0]}")
def test_front_end(dev, model, prec):
    sd, eng = dino_engine(dev, model[0], model[1], 1, prec)
    bar, worst, worst_mean, fails = R.BARS[("front", prec)], 0.0, 0.0, []
    for c in R.front_cases():
        frames = R.front_frames(c)
        g = c["res"] // 14
        prep = [R.prepare(f, c["layout"], 1.0, R.AUTO) for f in frames]
        ref = R.tokens(sd, np.concatenate([p[0] for p in prep]), g, eng.pos_patch(g))
        for offset in (False, True):
            what = (c, offset)
            tok, flags = embed_poisoned(eng, [upload(f, dev, offset) for f in frames], c["layout"])
            try:                                                        # every case is measured before the test fails
                assert bool(torch.isfinite(tok).all()), (what, "non-finite token")
                for n, f in enumerate(frames):
                    worst_mean = max(worst_mean, check_flags(what, flags[n], prep[n][1:], f, 1.0, not offset))
                e = R.row_err(tok.reshape(ref.shape), ref)
                worst = max(worst, e)
                assert e <= bar, (what, e, bar)
            except AssertionError as err:
                fails.append(str(err))
    print(f"front d{model[0]} {prec}: worst {worst:.3e} (bar {bar:.3e}); mean error at most {worst_mean:.2f} of its bound; {len(fails)} failures")
    assert not fails, fails[:4]


def test_decisions(dev):
    sd, eng = dino_engine(dev, 64, 1, 1, "fp32")
    sd16, eng16 = dino_engine(dev, 64, 1, 1, "bf16")
    fails = []
    for name, c in R.decision_cases().items():
        ref = R.prepare(c["frames"], c["layout"], c["pre_scale"], c["mode"])
        res = ref[0].shape[-1]
        for e, s, prec in ((eng, sd, "fp32"), (eng16, sd16, "bf16")):
            tok, flags = embed_poisoned(e, [upload(c["frames"], dev, c["offset"])], c["layout"], c["pre_scale"], c["mode"])
            want = R.tokens(s, ref[0], res // 14, e.pos_patch(res // 14))
            err = R.row_err(tok.reshape(want.shape), want)
            print(f"decision {name} {prec}: flags {flags[0].tolist()} (reference {ref[1:]}), tokens {err:.3e}")
            try:
                check_flags((name, prec), flags[0], ref[1:], c["frames"], c["pre_scale"], not c["offset"])
                assert err <= R.BARS[("front", prec)], (name, prec, err)
            except AssertionError as ex:
                fails.append(str(ex))
    assert not fails, fails[:4]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("et", ["f32", "u8"])
def test_large_walks(dev, et, where):
    """201 243 vectors of 16 bytes: lanes below 4 635 take one round of the four-deep unrolled loop (entered above 3 x 65 536 vectors), the
    others the one-vector loop.  The only value above 1 is the frame's first or last element."""
    sd, eng = dino_engine(dev, 64, 1, 1, "fp32")
    f = R.large_case(et, where)
    layout = "nhwc" if et == "u8" else "nchw"
    ref = R.prepare(f, layout, 1.0, R.AUTO)
    assert ref[1] == 1 / 255.0 and ref[2] == 0.0 and "unrolled" in R.stat_walks(f.size, f.itemsize, True)[0]
    tok, flags = embed_poisoned(eng, [upload(f, dev, False)], layout)
    want = R.tokens(sd, ref[0], 37, eng.pos_patch(37))
    err = R.row_err(tok.reshape(want.shape), want)
    print(f"large {et} {where}: flags {flags[0].tolist()} (reference {ref[1:]}), tokens {err:.3e}")
    r = check_flags((et, where), flags[0], ref[1:], f, 1.0, True)
    print(f"large {et} {where}: mean at {r:.2f} of its bound")
    assert err <= R.BARS[("front", "fp32")], err


def test_embed_refusals(dev):
    """Null arguments, res < 14 and ncams > 8 are refused before anything is launched."""
    from vlatouch import _lib as L
    sd, eng = dino_engine(dev, 64, 1, 1, "fp32")
    lib = L.lib()
    x = torch.zeros(1, 3, 14, 14, device=dev)
    out = torch.zeros(1, 2, 64, device=dev)
    ws = torch.zeros(lib.vt_dino_workspace_bytes(eng._h, 1, 14), dtype=torch.uint8, device=dev)
    good = dict(h=eng._h, imgs=L.ptr_array([x]), ncams=1, res=14, pos=L.ptr(eng.pos_patch(1)), out=L.ptr(out), ws=L.ptr(ws))

    def call(**over):
        a = dict(good, **over)
        return lib.vt_dino_embed(a["h"], a["imgs"], a["ncams"], 0, 0, C.c_float(1.0), R.AUTO, 1, a["res"], a["pos"], a["out"], None, a["ws"], L.stream_ptr(dev))

    assert call() == 0
    torch.cuda.synchronize(dev)
    for over in (dict(h=None), dict(imgs=None), dict(pos=None), dict(out=None), dict(ws=None), dict(imgs=L.ptr_array([None])), dict(res=13), dict(ncams=9),
                 dict(ncams=0)):
        assert call(**over) != 0, over
    with pytest.raises(ValueError):
        eng.embed([torch.zeros(1, 3, 13, 13)], nhwc=False)
    with pytest.raises(ValueError):
        eng.embed([x], nhwc=False, out=torch.zeros(1, 1, 3, 64, device=dev))


# ------------------------------------------------------------------------------------------------ blocks
BLOCK_PARAMS = [(name, prec) for name, cfg in R.BLOCK_CONFIGS.items() for prec in cfg["precs"]]


@pytest.mark.parametrize("name,prec", BLOCK_PARAMS)
def test_dino_blocks_pruned_and_full(dev, name, prec):
    """Every token of the `out_all` handle (the last block in full) and the pooled output of the pruned handle (CLS query only: strided A with
    lda = N D, M = Bt rows, attention with Nq = 1) against the same float64 statement.

    d256_packed: Bt N = 65 rows, fc1 on the packed-weight tile for the 1-row remainder and the 13 CLS rows (vt_dino_packed_bytes > 0).
    d512_splitk: 130 rows meet the split-K fc2 and slab-reduction condition of vt_dino_forward:
        w.slab_bytes && rows > 64 && DINO_SPLITK * rows * D * 4 <= w.slab_bytes && Dm >= 2048 && (Dm / 64) % DINO_SPLITK == 0 && D % 4 == 0
        && !vt_gemm_lds_fits(p)
      with slab_bytes != 0 iff Bt N <= 1100, DINO_SPLITK = 4, Dm = 2048; its pruned block (13 rows) does not."""
    from vlatouch import _lib as L
    cfg = R.BLOCK_CONFIGS[name]
    sd, full = dino_engine(dev, cfg["hidden"], cfg["heads"], cfg["layers"], prec, cfg["swiglu"], out_all=True)
    _, pruned = dino_engine(dev, cfg["hidden"], cfg["heads"], cfg["layers"], prec, cfg["swiglu"])
    if name == "d256_packed":
        assert L.lib().vt_dino_packed_bytes(full._h) > 0 and L.lib().vt_dino_packed_bytes(pruned._h) > 0
    bar, worst_all, worst_cls, fails = R.BARS[("dino", prec)], 0.0, 0.0, []
    for n, (res, ncams, B) in enumerate(cfg["runs"]):
        frames = R.block_frames(res, ncams, B, seed=n + 1)
        ref = R.dino_reference(sd, cfg["heads"], frames, full.pos_patch(res // 14))[1]
        cams = [upload(f, dev, False) for f in frames]
        tok = full.forward(cams, nhwc=False).cpu()
        cls = pruned.forward(cams, nhwc=False).cpu()
        assert tok.shape == (ncams, B, (res // 14) ** 2 + 1, cfg["hidden"]) and cls.shape == (ncams, B, cfg["hidden"])
        assert full.last_flags[:, 1].tolist() == [1.0, 0.0][:ncams]            # the two cameras decide differently
        e_all = R.row_err(tok.reshape(ref.shape), ref)
        e_row0 = R.row_err(tok.reshape(ref.shape)[:, 0], ref[:, 0])
        e_cls = R.row_err(cls.reshape(-1, cfg["hidden"]), ref[:, 0])
        worst_all, worst_cls = max(worst_all, e_all), max(worst_cls, e_cls)
        print(f"blocks {name} {prec} res {res} cams {ncams} B {B}: all tokens {e_all:.3e}, out_all row 0 {e_row0:.3e}, pruned CLS {e_cls:.3e} (bar {bar:.3e})")
        if not (e_all <= bar and e_row0 <= bar and e_cls <= bar):
            fails.append((name, prec, res, ncams, B, e_all, e_row0, e_cls, bar))
    print(f"blocks {name} {prec}: worst all tokens {worst_all:.3e}, pruned CLS {worst_cls:.3e} (bar {bar:.3e})")
    assert not fails, fails


@pytest.mark.parametrize("prec", R.PRECS)
def test_siglip_blocks(dev, prec):
    """Hidden 576, 8 heads of 72 (packed to 96 in fp32, 80 in the 16-bit modes), inter 1072 (padded to 1088): every token."""
    from vlatouch.engine import SiglipEngine
    bar, worst, fails = R.BARS[("siglip", prec)], 0.0, []
    for res, B in R.SIGLIP_RUNS:
        sd = R.siglip_shapes_sd(res)
        eng = SiglipEngine(sd, heads=R.SIGLIP_HEADS, precision=prec, device=dev)
        px = R.siglip_pixels(B, res, seed=res + B)
        ref = R.blocks(sd, R.tokens(sd, px.astype(np.float64), res // 14, R.pos_rows(sd, res // 14)), R.SIGLIP_HEADS)
        e = R.row_err(eng.forward(torch.from_numpy(px)).cpu(), ref)
        worst = max(worst, e)
        print(f"siglip {prec} res {res} B {B}: {e:.3e} (bar {bar:.3e})")
        if not e <= bar:
            fails.append((prec, res, B, e, bar))
    print(f"siglip {prec}: worst {worst:.3e} (bar {bar:.3e})")
    assert not fails, fails


@pytest.mark.parametrize("prec", R.PRECS)
def test_siglip_takes_pixel_values_as_they_are(dev, prec):
    """Pixel values made with ImageNet statistics reach 2.64.  The reference's SiglipVisionTower.forward hands them to the tower unchanged; the
    driver's max > 1 rule (the controller's DINOv2Encoder, visual_encoder.py:78) divided the whole batch by 255 until SiglipEngine got
    VT_IMGNORM_RAW: before that this test misses its bar by a factor of the order of 255."""
    from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
    from vlatouch.engine import SiglipEngine
    res, B, bar = 28, 3, R.BARS[("siglip", prec)]
    sd = R.siglip_shapes_sd(res)
    px = R.siglip_pixels(B, res, seed=1, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    assert abs(float(px.max()) - (1 - 0.406) / 0.225) < 1e-6
    ref = R.blocks(sd, R.tokens(sd, px.astype(np.float64), res // 14, R.pos_rows(sd, res // 14)), R.SIGLIP_HEADS)
    eng = SiglipEngine(sd, heads=R.SIGLIP_HEADS, precision=prec, device=dev)
    e_eng = R.row_err(eng.forward(torch.from_numpy(px)).cpu(), ref)
    flags = eng.last_flags[0].tolist()
    cfg = dict(hidden_size=576, intermediate_size=1072, num_hidden_layers=2, num_attention_heads=R.SIGLIP_HEADS, image_size=res, patch_size=14)
    tower = SiglipVisionTower("synthetic", types.SimpleNamespace(mm_vision_select_feature="patch"), device="cuda:0", precision=prec, state_dict=sd, config=cfg)
    e_tower = R.row_err(tower(torch.from_numpy(px).to(dev)).cpu(), ref)
    from vlatouch import _lib as L
    tbar = R.BARS[("siglip", {L.F32: "fp32", L.BF16: "bf16", L.F16: "fp16"}[tower.engine.adt])]       # the tower's "bf16" stores IEEE fp16
    print(f"siglip ImageNet statistics {prec}: engine {e_eng:.3e} (bar {bar:.3e}), tower {e_tower:.3e} (bar {tbar:.3e})")
    assert flags[:2] == [1.0, 0.0] and abs(flags[2] - float(px.max())) < 1e-6, flags                   # scale 1, not normalised, the maximum reported
    assert e_eng <= bar and e_tower <= tbar, (prec, e_eng, e_tower, bar, tbar)
