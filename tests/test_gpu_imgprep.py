"""Device image preprocessing (csrc/vt_imgprep.hip, vlatouch/imgprep.py) against the CPU statement it replaces:
`torch.equal(preprocess_images_device(frames), preprocess_images(frames).to(device, dtype))` — exact equality everywhere; the yardstick
is PIL through the wrapper's own `preprocess_images` (pinned to HF's SiglipImageProcessor in tests/test_siglip.py)."""
import copy
import types

import numpy as np
import pytest
import torch

from tests import cases
from vlatouch import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DATASET = {"tokenizer_max_length": 16, "image_aspect_ratio": "pad", "auto_adjust_image_brightness": True}


def make_model(S=64, dtype=torch.float32, mean=None, std=None, image_size=None, **dataset):
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel, SiglipPreprocessor
    vis = types.SimpleNamespace(config=types.SimpleNamespace(image_size=S), num_patches=16, hidden_size=576, eval=lambda: None)
    pol = types.SimpleNamespace(eval=lambda: None)
    args = {"dataset": dict(DATASET, **dataset), "model": {"state_token_dim": 128}}
    m = RoboticDiffusionTransformerModel(args, device=DEV, dtype=dtype, image_size=image_size, vision_model=vis, policy=pol)
    if mean is not None:
        m.image_processor = SiglipPreprocessor(S, mean, std)
    return m


def rand_frame(g, h, w, scale=1.0):
    return (g.random((h, w, 3)) * 256 * scale).astype(np.uint8)


def as_pil(frames):
    from PIL import Image
    return [None if f is None else Image.fromarray(f) for f in frames]


def check(m, frames, pil=None):
    want = m.preprocess_images(as_pil(frames) if pil is None else pil).to(DEV, m.dtype)
    got = m.preprocess_images_device(frames)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device
    if not torch.equal(got, want):
        bad = (got != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
        import PIL
        raise AssertionError(f"frames {bad} differ (max |d| = {float((got.float() - want.float()).abs().max())}, Pillow {PIL.__version__})")


GEOS = [(480, 640), (640, 480), None, (384, 384), (500, 500), (384, 600), (200, 384), (8, 8), (100, 150), (720, 1280), (1080, 1920), (64, 64), (97, 61)]


@pytest.mark.parametrize("S,dtype", [(384, torch.float32), (384, torch.bfloat16), (64, torch.float32), (64, torch.bfloat16)])
def test_mixed_geometries_in_one_call(S, dtype):
    """wide, tall, missing, square at S / not at S, one side at S, 8 x 8, upscales, the camera sizes — one call; at S = 64 the larger frames
    exceed the fused kernel's bound, so the whole call takes the two-launch form."""
    g = np.random.default_rng(S)
    frames = [None if s is None else rand_frame(g, *s) for s in GEOS]
    check(make_model(S, dtype), frames)


def test_each_geometry_alone_takes_the_fused_kernel_when_it_fits():
    from vlatouch import imgprep
    m = make_model(384)
    g = np.random.default_rng(1)
    for s in [(480, 640), (640, 480), (384, 600), (8, 8), (720, 1280), (1080, 1920), (2800, 300)]:
        check(m, [rand_frame(g, *s)])
    pp = next(iter(m._imgprep.values()))
    side_rows = {k: v[2] for k, v in pp._tables.items()}
    assert side_rows[(1920, 384, imgprep.BICUBIC)] <= imgprep.FUSED_ROWS < side_rows[(2800, 384, imgprep.BICUBIC)]      # both forms ran


@pytest.mark.parametrize("n", [1, 2, 7, 48])
def test_batch_sizes_and_missing_frames_anywhere(n):
    g = np.random.default_rng(n)
    frames = [rand_frame(g, int(g.integers(20, 120)), int(g.integers(20, 120))) for _ in range(n)]
    m = make_model(64)
    check(m, frames)
    for pos in {0, n // 2, n - 1}:
        fr = list(frames)
        fr[pos] = None
        check(m, fr)
    check(m, [None] * n)


def threshold_frame(extra):
    """40 x 40 frame whose byte sum is 0.15 * (40 * 40 * 255 * 3) + extra: at the threshold itself the host lifts (<=)."""
    a = np.full((40, 40, 3), 38, dtype=np.uint8).reshape(-1)
    a[: 183600 - 38 * 4800 + extra] += 1
    assert int(a.sum()) == 183600 + extra
    return a.reshape(40, 40, 3)


@pytest.mark.parametrize("flag", [True, False])
def test_brightness_threshold_both_sides(flag):
    from PIL import Image
    g = np.random.default_rng(2)
    frames = [threshold_frame(0), threshold_frame(1), threshold_frame(-1), rand_frame(g, 48, 64, 0.2), rand_frame(g, 64, 48, 0.35), rand_frame(g, 50, 50, 1.0),
              np.zeros((30, 40, 3), dtype=np.uint8), rand_frame(g, 480, 640, 0.29), rand_frame(g, 480, 640, 0.31)]
    m = make_model(64, auto_adjust_image_brightness=flag)
    if flag:      # the threshold cases do sit on both sides for the host
        px = [np.asarray(f, dtype=np.float64) for f in frames[:2]]
        assert [p.sum() / (p.shape[0] * p.shape[1] * 255.0 * 3) <= 0.15 for p in px] == [True, False]
    check(m, frames)
    check(make_model(384, torch.bfloat16, auto_adjust_image_brightness=flag), frames)


@pytest.mark.parametrize("image_size", [48, (40, 72), (64, 64), 200])
def test_image_size_pre_resize(image_size):
    g = np.random.default_rng(4)
    frames = [rand_frame(g, 48, 64), rand_frame(g, 120, 90), None, rand_frame(g, 64, 64), rand_frame(g, 50, 50, 0.2), rand_frame(g, 480, 640)]
    check(make_model(64, image_size=image_size), frames)


def test_other_aspect_ratio_mode_and_dark_mean_colour():
    g = np.random.default_rng(5)
    frames = [rand_frame(g, 48, 64), None, rand_frame(g, 120, 90), rand_frame(g, 64, 64), rand_frame(g, 64, 100), rand_frame(g, 30, 64, 0.2)]
    check(make_model(64, image_aspect_ratio="square"), frames)
    check(make_model(64, image_aspect_ratio="square", image_size=(40, 50)), frames)
    # a mean colour dark enough that the missing frame's background is itself lifted by the host
    check(make_model(64, mean=(0.1, 0.12, 0.05), std=(0.2, 0.3, 0.4)), frames)
    check(make_model(64, mean=(0.1, 0.12, 0.05), std=(0.2, 0.3, 0.4), image_size=(40, 50)), frames)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_non_default_mean_std(dtype):
    g = np.random.default_rng(6)
    frames = [rand_frame(g, 48, 64), None, rand_frame(g, 90, 60), rand_frame(g, 56, 56, 0.2)]
    check(make_model(56, dtype, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)), frames)        # S % 4 == 0 but not a tile multiple
    check(make_model(50, dtype, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)), frames)        # S % 4 != 0: scalar stores


def test_every_input_kind_with_sentinels():
    from PIL import Image
    g = np.random.default_rng(7)
    a = [rand_frame(g, 48, 64) for _ in range(7)]
    big_host = rand_frame(g, 60, 100)
    big = torch.from_numpy(big_host).to(DEV)
    pitched = big[5:50, 11:81, :]                                   # rows 300 bytes apart, 70 pixels wide, odd start address
    assert not pitched.is_contiguous()
    gray = Image.fromarray(a[5][:, :, 0])                              # mode L
    frames = [Image.fromarray(a[0]), a[1], torch.from_numpy(a[2]), torch.from_numpy(a[3]).to(DEV), pitched, None, gray,
              Image.fromarray(a[6]).convert("RGBA").convert("P")]
    pil = [Image.fromarray(a[0]), Image.fromarray(a[1]), Image.fromarray(a[2]), Image.fromarray(a[3]), Image.fromarray(pitched.cpu().numpy()), None,
           gray.convert("RGB"), frames[7].convert("RGB")]
    for S, force in ((64, False), (64, True), (384, False)):
        m = make_model(S)
        want = m.preprocess_images(pil).to(DEV)
        m.preprocess_images_device(frames)                          # builds the preprocessor
        pp = next(iter(m._imgprep.values()))
        pp.force_two_pass = force
        nws, nout = pp.workspace_bytes(frames), len(frames) * 3 * S * S
        assert nws >= 512 * len(frames) and (not force or nws > 512 * len(frames))
        ws = torch.full((nws + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        buf = torch.full((nout + 64,), -777.0, dtype=torch.float32, device=DEV)
        got = pp(frames, out=buf[:nout].view(len(frames), 3, S, S), workspace=ws[:nws])
        torch.cuda.synchronize()
        assert torch.equal(got, want), (S, force)
        assert bool((buf[nout:] == -777.0).all()) and bool((ws[nws:] == 0xA5).all()), (S, force)
        assert np.array_equal(big.cpu().numpy(), big_host)                          # the frame used in place is untouched


def test_two_launch_form_equals_fused_and_runs_beyond_the_bound():
    from vlatouch import imgprep
    g = np.random.default_rng(8)
    m = make_model(64)
    frames = [rand_frame(g, 1080, 1920), rand_frame(g, 1920, 1080, 0.2), None, rand_frame(g, 300, 400)]       # 1920 -> 64: ratio 30
    check(m, frames)
    pp = next(iter(m._imgprep.values()))
    assert pp._tables[(1920, 64, imgprep.BICUBIC)][2] > imgprep.FUSED_ROWS
    small = [rand_frame(g, 48, 64), None, rand_frame(g, 200, 120, 0.2), rand_frame(g, 300, 400)]
    fused = m.preprocess_images_device(small).clone()
    pp.force_two_pass = True
    two = m.preprocess_images_device(small)
    assert torch.equal(fused, two)
    check(m, small)


def _tower_model(device_preprocess, dtype=torch.float32):
    from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    from tests.test_siglip import ARGS
    c = synth.SIGLIP_CONFIGS["tiny"]
    cfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
               image_size=c["image_size"], patch_size=14)
    tower = SiglipVisionTower("synthetic", None, device=DEV, precision="fp32", state_dict=cases.siglip_sd("tiny"), config=cfg)
    return RoboticDiffusionTransformerModel(copy.deepcopy(ARGS), device=DEV, dtype=dtype, control_frequency=10, vision_model=tower,
                                            device_preprocess=device_preprocess)


def test_step_and_encode_frames_equal_with_the_switch_on_and_off():
    from tests.test_siglip import _pil_frames
    from vlatouch.label import encode_frames
    on, off = _tower_model(True), _tower_model(False)
    off.policy = on.policy
    g = torch.Generator().manual_seed(3)
    proprio, text = torch.randn(1, 10, generator=g), torch.randn(1, 12, 96, generator=g)
    torch.manual_seed(11)
    a = on.step(proprio, _pil_frames(), text)
    torch.manual_seed(11)
    b = off.step(proprio, _pil_frames(), text)
    assert on._imgprep and not off._imgprep                              # the device path really ran, and only where it is switched on
    assert torch.equal(a, b)
    rng = np.random.default_rng(9)
    frames = [rand_frame(rng, 56, 56) for _ in range(5)] + [None] + _pil_frames()
    assert torch.equal(encode_frames(on, frames, batch=4), encode_frames(off, frames, batch=4))


def test_graph_capture_of_the_device_input_path():
    """Device-resident frames of a seen geometry: no allocation (out= given), no copy, no synchronise — so one single-stream capture
    replays on new frame contents, the brightness decision included."""
    g = np.random.default_rng(10)
    m = make_model(64)
    shapes = [(48, 64), (64, 48), (40, 40), (120, 160)]
    static = [torch.from_numpy(rand_frame(g, *s)).to(DEV) for s in shapes]
    frames = [static[0], static[1], None, static[2], static[3]]
    out = torch.empty(5, 3, 64, 64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.preprocess_images_device(frames, out=out)                      # warm-up: tables, plan, workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.preprocess_images_device(frames, out=out)
    for rep, scale in enumerate((1.0, 0.2, 0.7)):
        new = [rand_frame(g, *sh, scale) for sh in shapes]
        if rep == 1:
            new[2] = threshold_frame(0)
        for t, a in zip(static, new):
            t.copy_(torch.from_numpy(a))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = m.preprocess_images(as_pil([new[0], new[1], None, new[2], new[3]])).to(DEV)
        assert torch.equal(out, want), rep
