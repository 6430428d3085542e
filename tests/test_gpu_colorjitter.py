"""The colour augmentation on the device (csrc/vt_colorjitter.hip, vlatouch/imgprep.py `jitter=`, vlatouch/rdt_train.py prepare_batch)
against PIL (tests/imgaug_ref.py): every comparison is for equal bits.  Outputs go into buffers pre-filled with a sentinel; the pad
bytes between frames and after the last frame must keep it."""
import itertools

import numpy as np
import pytest
import torch

from tests import cases
from tests import imgaug_ref as R
from vlatouch import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_, C_, S_, H_, NONE = 0, 1, 2, 3, 4          # operation ids of the record
SENT = 0xA5


def spec(slots=(), b=1.0, c=1.0, s=1.0, shift=0):
    """One frame's record contents: the operation id per slot (padded with NONE), the three factors, the hue byte."""
    slots = tuple(slots) + (NONE,) * (4 - len(slots))
    return (slots, float(b), float(c), float(s), int(shift))


def pil_spec(arr, sp, lift):
    """PIL on one frame: the lift by the existing rule, then the slots in order."""
    from PIL import Image, ImageEnhance
    slots, fb, fc, fs, shift = sp
    img = Image.fromarray(arr)
    if lift:
        px = np.asarray(img, dtype=np.float64)
        if px.sum() / (px.shape[0] * px.shape[1] * 255.0 * 3) <= 0.15:
            img = ImageEnhance.Brightness(img).enhance(1.75)
    for op in slots:
        if op == B_:
            img = ImageEnhance.Brightness(img).enhance(fb)
        elif op == C_:
            img = ImageEnhance.Contrast(img).enhance(fc)
        elif op == S_:
            img = ImageEnhance.Color(img).enhance(fs)
        elif op == H_:
            img = R.hue_pil(img, shift)
    return np.asarray(img)


def run(frames, specs, lift=False):
    """vt_colorjitter on device frames (uint8 [h, w, 3] tensors, pitched views allowed) -> the per-frame outputs as numpy.  Frame i is
    written at a 16-byte aligned offset plus i % 3 (so that tight rows start at every alignment); pads and tails keep the sentinel."""
    from vlatouch import _lib
    L = _lib.lib()
    n = len(frames)
    arr = (_lib.ColorJitterFrame * n)()
    off, spans = 0, []
    for i, (t, (slots, fb, fc, fs, shift)) in enumerate(zip(frames, specs)):
        h, w = int(t.shape[0]), int(t.shape[1])
        assert t.is_cuda and t.dtype == torch.uint8 and t.stride(2) == 1 and t.stride(1) == 3
        f = arr[i]
        f.src, f.pitch, f.h, f.w = t.data_ptr(), (int(t.stride(0)) if h > 1 else 3 * w), h, w
        f.out_off = off + i % 3
        f.order[:] = list(slots)
        f.brightness, f.contrast, f.saturation, f.hue_shift = fb, fc, fs, shift
        spans.append((f.out_off, h, w))
        off = (f.out_off + 3 * h * w + 15) // 16 * 16 + 16
    nws = int(L.vt_colorjitter_workspace_bytes(n))
    assert nws >= n * 3 * 64 * 8
    out = torch.full((off + 64,), SENT, dtype=torch.uint8, device=DEV)
    ws = torch.full((nws + 256,), SENT, dtype=torch.uint8, device=DEV)
    dev = torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(DEV)
    _lib.check(L.vt_colorjitter(arr, _lib.ptr(dev), n, _lib.COLORJITTER_LIFT if lift else 0, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr(DEV)),
               "vt_colorjitter")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    res = []
    for o, h, w in spans:
        res.append(host[o:o + 3 * h * w].reshape(h, w, 3))
        keep[o:o + 3 * h * w] = False
    assert (host[keep] == SENT).all(), "a byte outside the frames was written"
    assert bool((ws[nws:] == SENT).all()), "a byte past the workspace was written"
    return res


def check(frames_host, specs, lift=False, frames_dev=None):
    dev = frames_dev if frames_dev is not None else [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in frames_host]
    got = run(dev, specs, lift)
    bad = []
    for i, (a, sp, g) in enumerate(zip(frames_host, specs, got)):
        want = pil_spec(a, sp, lift)
        if not np.array_equal(g, want):
            bad.append((i, a.shape[:2], sp, int((g != want).any(axis=-1).sum())))
    assert not bad, f"{len(bad)} frames differ from PIL (index, size, spec, pixels): {bad[:4]}"
    return got


_colours = {}


def colours():
    if not _colours:
        a = R.all_colours()
        _colours["host"], _colours["dev"] = a, torch.from_numpy(a).to(DEV)
    return _colours["host"], _colours["dev"]


def rand_frame(g, h, w, scale=1.0):
    return (g.random((h, w, 3)) * 256 * scale).astype(np.uint8)


def threshold_frame(extra):
    """40 x 40 frame whose byte sum is 0.15 * (40 * 40 * 255 * 3) + extra: at the threshold itself the host lifts (<=)."""
    a = np.full((40, 40, 3), 38, dtype=np.uint8).reshape(-1)
    a[: 183600 - 38 * 4800 + extra] += 1
    assert int(a.sum()) == 183600 + extra
    return a.reshape(40, 40, 3)


# ------------------------------------------------------------------------------------------------ 1. exhaustive per operation
@pytest.mark.parametrize("shift", [7, 128, 249])
def test_hue_on_all_colours(shift):
    host, dev = colours()
    check([host], [spec((H_,), shift=shift)], frames_dev=[dev])


@pytest.mark.parametrize("factor", [0.5, 1.5])
def test_saturation_on_all_colours(factor):
    host, dev = colours()
    check([host], [spec((S_,), s=factor)], frames_dev=[dev])


@pytest.mark.parametrize("factor", [0.7, 1.3])
def test_brightness_on_all_bytes(factor):
    a = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=-1)
    check([a], [spec((B_,), b=factor)])


def test_empty_order_with_lift_on_both_sides_of_the_threshold():
    g = np.random.default_rng(2)
    frames = [threshold_frame(0), threshold_frame(1), threshold_frame(-1), rand_frame(g, 48, 64, 0.2), rand_frame(g, 50, 50, 1.0),
              np.zeros((30, 40, 3), dtype=np.uint8)]
    px = [np.asarray(f, dtype=np.float64) for f in frames[:2]]
    assert [p.sum() / (p.shape[0] * p.shape[1] * 255.0 * 3) <= 0.15 for p in px] == [True, False]      # the cases do sit on both sides
    got = check(frames, [spec()] * len(frames), lift=True)
    assert not np.array_equal(got[0], frames[0]) and np.array_equal(got[1], frames[1])               # lifted / copied
    got = check(frames, [spec()] * len(frames), lift=False)
    assert all(np.array_equal(a, b) for a, b in zip(got, frames))


# ------------------------------------------------------------------------------------------------ 2. contrast mean and blend pairs
@pytest.mark.parametrize("factor", [0.6, 1.4])
def test_contrast_means_over_256_frames_in_one_call(factor):
    frames = [R.ramp_frame(m) for m in range(256)] + R.half_mean_frames()
    means = [R.contrast_mean_np(a) for a in frames]
    assert min(means[:256]) <= 2 and max(means[:256]) >= 252 and means[256:] == [11, 101, 100]
    check(frames, [spec((C_,), c=factor)] * len(frames))


# ------------------------------------------------------------------------------------------------ 3. orders, subsets, geometries
def _geometry_case():
    g = np.random.default_rng(3)
    frames, specs = [], []
    base = dict(b=0.83, c=1.31, s=0.61, shift=249)
    for k, order in enumerate(itertools.permutations((B_, C_, S_, H_))):           # every order, on the 37 x 53 frame, bright and dark
        frames.append(rand_frame(g, 37, 53, 0.25 if k % 3 == 0 else 1.0))
        specs.append(spec(order, **(base if k % 2 else dict(b=1.27, c=0.64, s=1.44, shift=7))))
    perms = list(itertools.permutations((B_, C_, S_, H_)))
    for h, w in [(1, 1), (1, 7), (5, 3), (64, 64), (480, 640)]:
        for j in range(4):                                                         # four drawn orders with one or two operations skipped
            order = list(perms[int(g.integers(24))])
            for drop in g.choice(4, size=1 + j % 2, replace=False):
                order[int(drop)] = NONE
            frames.append(rand_frame(g, h, w, 0.2 if j == 1 else 1.0))
            specs.append(spec(order, b=float(np.float32(g.uniform(0.7, 1.3))), c=float(np.float32(g.uniform(0.6, 1.4))),
                              s=float(np.float32(g.uniform(0.5, 1.5))), shift=int(g.integers(256))))
    dev = [torch.from_numpy(a).to(DEV) for a in frames]
    # a pitched view with an odd byte offset (rows 300 bytes apart, odd start: the byte path) and an aligned one (the word path)
    big_host = rand_frame(g, 60, 100)
    big = torch.from_numpy(big_host).to(DEV)
    for view, hv in ((big[5:50, 11:81, :], big_host[5:50, 11:81, :]), (big[2:40, 8:72, :], big_host[2:40, 8:72, :])):
        assert not view.is_contiguous()
        frames.append(np.ascontiguousarray(hv))
        dev.append(view)
        specs.append(spec((S_, H_, C_, B_), **base))
    assert dev[-2].data_ptr() % 2 == 1 and dev[-1].data_ptr() % 4 == 0
    return frames, dev, specs, big, big_host


@pytest.mark.parametrize("lift", [False, True])
def test_orders_subsets_and_geometries(lift):
    frames, dev, specs, big, big_host = _geometry_case()
    got = check(frames, specs, lift=lift, frames_dev=dev)
    again = run(dev, specs, lift)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls must agree bit for bit"
    assert np.array_equal(big.cpu().numpy(), big_host)                             # the frame read in place is untouched


# ------------------------------------------------------------------------------------------------ 4. the pipeline
def _processor(S):
    from scripts.franka_model_eef import SiglipPreprocessor
    return SiglipPreprocessor(S, [0.5, 0.5, 0.5], [0.5, 0.5, 0.5])


def _pipeline_frames():
    """Seven frames: jittered, unjittered and missing, as host arrays, PIL images and device frames (one of them a pitched view), one dark
    and one bright frame among the jittered ones."""
    from PIL import Image
    from vlatouch.imgaug import color_jitter_params
    g = np.random.default_rng(11)
    gen = torch.Generator().manual_seed(11)
    big_host = rand_frame(g, 60, 100)
    big = torch.from_numpy(big_host).to(DEV)
    host = [rand_frame(g, 48, 64), rand_frame(g, 90, 60), None, rand_frame(g, 64, 64), rand_frame(g, 50, 70, 0.2), rand_frame(g, 120, 90, 1.0),
            big_host[5:50, 11:81, :]]
    frames = [host[0], Image.fromarray(host[1]), None, torch.from_numpy(host[3]).to(DEV), host[4], torch.from_numpy(host[5]).to(DEV), big[5:50, 11:81, :]]
    jitter = [color_jitter_params(generator=gen), color_jitter_params(generator=gen), None, None, color_jitter_params(generator=gen),
              color_jitter_params(generator=gen), color_jitter_params(generator=gen)]
    return host, frames, jitter


def _chain(host, jitter, proc, **kw):
    from PIL import Image
    bg = R.background(proc)
    return torch.stack([R.train_image_chain(bg if a is None else Image.fromarray(np.ascontiguousarray(a)), a is not None, p, processor=proc, **kw)
                        for a, p in zip(host, jitter)])


@pytest.mark.parametrize("image_size", [None, 48, (40, 72)], ids=["noresize", "resize48", "resize40x72"])
@pytest.mark.parametrize("pad", [True, False], ids=["pad", "nopad"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pipeline_equals_the_dataset_chain(dtype, pad, image_size):
    from vlatouch.imgprep import DevicePreprocessor
    S = 64
    proc = _processor(S)
    host, frames, jitter = _pipeline_frames()
    px = [np.asarray(a, dtype=np.float64).sum() / (a.shape[0] * a.shape[1] * 255.0 * 3) for a in (host[4], host[5])]
    assert px[0] <= 0.15 < px[1]                                                   # one dark and one bright frame among the jittered
    pp = DevicePreprocessor(S, proc.image_mean, proc.image_std, DEV, dtype, pad=pad, brightness=True, image_size=image_size)
    want = _chain(host, jitter, proc, image_size=image_size, brightness=True, pad=pad).to(DEV, dtype)
    plain = _chain(host, [None] * 7, proc, image_size=image_size, brightness=True, pad=pad).to(DEV, dtype)
    assert not torch.equal(want, plain)
    for force in (False, True):
        pp.force_two_pass = force
        nws, nout = pp.workspace_bytes(frames, jitter), 7 * 3 * S * S
        assert nws > pp.workspace_bytes(frames)
        ws = torch.full((nws + 256,), SENT, dtype=torch.uint8, device=DEV)
        buf = torch.full((nout + 64,), -777.0, dtype=dtype, device=DEV)
        got = pp(frames, out=buf[:nout].view(7, 3, S, S), workspace=ws[:nws], jitter=jitter)
        torch.cuda.synchronize()
        bad = (got != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"frames {bad} differ from the dataset's chain (force_two_pass={force})"
        assert bool((buf[nout:] == -777.0).all()) and bool((ws[nws:] == SENT).all()), force
        assert torch.equal(pp(frames, jitter=jitter), want)                       # the preprocessor's own workspace and output
        # no jitter at all: today's call
        base = pp(frames)
        assert torch.equal(base, plain)
        assert torch.equal(pp(frames, jitter=None), base) and torch.equal(pp(frames, jitter=[None] * 7), base)


def test_pipeline_argument_checks_and_model_wrapper():
    from tests.test_gpu_imgprep import make_model
    from vlatouch import _lib
    from vlatouch.imgaug import ColorJitterParams
    host, frames, jitter = _pipeline_frames()
    m = make_model(64)
    p = ColorJitterParams((0, 1, 2, 3), brightness=1.1)
    with pytest.raises(_lib.VtError, match="missing frame"):
        m.preprocess_images_device(frames, jitter=[None, None, p, None, None, None, None])
    with pytest.raises(_lib.VtError, match="entries"):
        m.preprocess_images_device(frames, jitter=[p])
    with pytest.raises(_lib.VtError, match="ColorJitterParams"):
        m.preprocess_images_device(frames, jitter=[0.5] + [None] * 6)
    got = m.preprocess_images_device(frames, jitter=jitter)
    want = _chain(host, jitter, m.image_processor, image_size=None, brightness=True, pad=True).to(DEV)
    assert torch.equal(got, want)
    assert torch.equal(m.preprocess_images_device(frames), m.preprocess_images_device(frames, jitter=[None] * 7))


# ------------------------------------------------------------------------------------------------ 5. the loop
def test_finetune_from_raw_frames_equals_finetune_from_host_tokens():
    """Four micro-batches as the collator's mappings with raw `frames` and the `jitter` draw_image_aug gave: losses and final weights are
    bit-equal to the same four batches with `img_tokens` computed beforehand by the host chain and the same encoder."""
    import random
    from PIL import Image
    from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
    from tests import rdt_train_ref as T
    from tests.test_gpu_rdt_train import _runner
    from vlatouch.imgaug import draw_image_aug
    from vlatouch.imgprep import DevicePreprocessor
    from vlatouch.rdt_train import finetune
    S, B, N = 64, 2, 2
    c = dict(synth.SIGLIP_CONFIGS["tiny"], image_size=S)
    vcfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                image_size=S, patch_size=14)
    sd = cases.sd_torch(synth.siglip_shapes(**c), prefix="siglip-tiny64.")
    tower = SiglipVisionTower("synthetic", None, device=DEV, precision="fp32", state_dict=sd, config=vcfg)
    cfg = dict(cases.RDT_TINY, img_token_dim=tower.hidden_size, img_cond_len=N * tower.num_patches)
    proc = _processor(S)
    pp = DevicePreprocessor(S, proc.image_mean, proc.image_std, DEV, torch.float32, pad=True, brightness=True, image_size=None)
    g, rng, gen = np.random.default_rng(21), random.Random(21), torch.Generator().manual_seed(21)
    coll, plain, jittered = [], [], 0
    for j in range(4):
        b = T.batch(cfg, B, 12, seed=6 + 10 * j)
        frames = [[rand_frame(g, 48, 64, 0.2 if (j + s + k) % 3 == 0 else 1.0) for k in range(N)] for s in range(B)]
        frames[j % B][j % N] = None                                               # a missing frame per batch
        flat = [f for sample in frames for f in sample]
        jitter = draw_image_aug([f is not None for f in flat], rng=rng, generator=gen)
        jittered += sum(p is not None for p in jitter)
        states = torch.cat([torch.zeros_like(b["state_tokens"]), b["state_tokens"]], dim=1)
        coll.append(dict(states=states, actions=b["action_gt"], state_elem_mask=b["action_mask"].squeeze(1), ctrl_freqs=b["ctrl_freqs"],
                         lang_attn_mask=b["lang_attn_mask"], lang_embeds=b["lang_tokens"], frames=frames, jitter=jitter, noise=b["noise"],
                         timesteps=b["timesteps"]))
        px = _chain(flat, jitter, proc, image_size=None, brightness=True, pad=True).to(DEV)
        tokens = tower(px).detach().reshape(B, -1, tower.hidden_size)
        assert tokens.shape == (B, cfg["img_cond_len"], cfg["img_token_dim"])
        plain.append(dict(b, img_tokens=tokens))
    assert 0 < jittered < 4 * (B * N - 1)                                          # some frames jittered, some not
    kw = dict(lr=1e-3, gradient_accumulation_steps=2)
    a, r = _runner(cfg).trainer(**kw), _runner(cfg).trainer(**kw)
    la = finetune(a, coll, max_train_steps=2, vision_encoder=tower, preprocessor=pp)
    lr = finetune(r, plain, max_train_steps=2)
    assert len(la) == len(lr) == 4 and a.global_step == r.global_step == 2
    assert all(torch.equal(x, y) for x, y in zip(la, lr)), ([float(x) for x in la], [float(y) for y in lr])
    sa, sr = a.state_dict(), r.state_dict()
    assert set(sa) == set(sr) and all(torch.equal(sa[k], sr[k]) for k in sa)
    ea, er = a.ema_state_dict(), r.ema_state_dict()
    assert all(torch.equal(ea[k], er[k]) for k in ea)
