"""CPU-only checks of the device image preprocessing (vlatouch/imgprep.py, csrc/vt_imgprep.hip): the host coefficient builder against
PIL.Image.resize byte for byte, the normalise tables against SiglipPreprocessor.preprocess, and the C entry points' header, ctypes
signatures and argument checks through the loaded library (no launch happens: every check fails before the first GPU call)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)

PRECISION_BITS = 22


def _resize_int(img, out_h, out_w, filt):
    """PIL's two-pass 8-bit resize in plain integer numpy, driven by the tables of vlatouch.imgprep.resample_coeffs."""
    from vlatouch.imgprep import resample_coeffs

    def one_pass(a, axis_len, out):          # resamples axis 1 of a [rows, axis_len, C]
        if axis_len == out:
            return a
        b, k = resample_coeffs(axis_len, out, filt)
        assert b.dtype == np.int32 and k.dtype == np.int32 and b.shape == (out, 2) and k.shape[0] == out
        res = np.empty((a.shape[0], out, a.shape[2]), dtype=np.uint8)
        a32 = a.astype(np.int32)
        for xx in range(out):
            x0, n = int(b[xx, 0]), int(b[xx, 1])
            assert 0 <= x0 and x0 + n <= axis_len and 1 <= n <= k.shape[1]
            acc = (a32[:, x0:x0 + n, :] * k[xx, :n].reshape(1, n, 1)).sum(axis=1, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
            res[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return res

    a = one_pass(np.asarray(img), img.shape[1], out_w)                       # horizontal first, uint8 intermediate
    return one_pass(a.transpose(1, 0, 2), a.shape[0], out_h).transpose(1, 0, 2)


GEOMETRIES = [  # (h, w, out)
    (480, 640, 384), (640, 640, 384), (720, 1280, 384), (1080, 1920, 384), (200, 300, 384), (384, 500, 384), (97, 61, 384), (8, 8, 384),
    (1920, 1920, 64), (30, 40, 64), (64, 100, 64), (50, 1, 64), (1, 50, 384), (8, 8, 64), (384, 384, 384), (1920, 24, 64),
]


@pytest.mark.parametrize("filt_name", ["bicubic", "bilinear"])
@pytest.mark.parametrize("h,w,out", GEOMETRIES)
def test_coefficients_reproduce_pil_resize(h, w, out, filt_name):
    from PIL import Image
    from vlatouch import imgprep
    filt, pil = {"bicubic": (imgprep.BICUBIC, Image.BICUBIC), "bilinear": (imgprep.BILINEAR, Image.BILINEAR)}[filt_name]
    g = np.random.default_rng(h * 7919 + w * 31 + out)
    img = (g.random((h, w, 3)) * 256).astype(np.uint8)
    img[: max(1, h // 4)] = np.where(g.random((max(1, h // 4), w, 3)) < 0.5, 0, 255)       # hard edges: the overshoot of the cubic clips
    want = np.asarray(Image.fromarray(img).resize((out, out), resample=pil))
    got = _resize_int(img, out, out, filt)
    assert np.array_equal(got, want), (int(np.abs(got.astype(int) - want.astype(int)).max()), Image.__version__ if hasattr(Image, "__version__") else "")


def test_coefficients_non_square_target_and_brightness_rule():
    """The `image_size` pre-resize takes non-square bilinear targets; the brightness lift is min(255, (7 v) >> 2)."""
    from PIL import Image, ImageEnhance
    from vlatouch import imgprep
    g = np.random.default_rng(3)
    img = (g.random((48, 64, 3)) * 256).astype(np.uint8)
    for oh, ow in ((30, 40), (96, 128), (48, 100), (17, 64)):
        want = np.asarray(Image.fromarray(img).resize((ow, oh), resample=Image.BILINEAR))
        assert np.array_equal(_resize_int(img, oh, ow, imgprep.BILINEAR), want), (oh, ow)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    want = np.asarray(ImageEnhance.Brightness(Image.fromarray(ramp)).enhance(1.75))
    assert np.array_equal(np.minimum(255, (ramp.astype(np.int32) * 7) >> 2).astype(np.uint8), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mean,std", [((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])
@pytest.mark.parametrize("S", [64, 384])
def test_norm_table_equals_processor_on_a_ramp(S, mean, std, dtype):
    from PIL import Image
    from scripts.franka_model_eef import SiglipPreprocessor
    from vlatouch.imgprep import norm_table
    ramp = (np.arange(S * S) % 256).astype(np.uint8).reshape(S, S, 1).repeat(3, axis=2)      # size S: the processor does not resize
    want = SiglipPreprocessor(S, mean, std).preprocess(Image.fromarray(ramp))["pixel_values"][0].to(dtype)
    lut = norm_table(mean, std, dtype)
    assert lut.shape == (3, 256) and lut.dtype == dtype
    got = torch.stack([lut[c][torch.from_numpy(ramp[:, :, c].astype(np.int64))] for c in range(3)])
    assert torch.equal(got, want)


def _frame(L, **kw):
    f = L.ImgprepFrame()
    vals = dict(src=4096, coef_h=8192, coef_v=8192, pitch=3 * 64, h=48, w=64, out_h=32, out_w=32, ksize_h=9, ksize_v=9, rows_max=40)
    vals.update(kw)
    for k, v in vals.items():
        setattr(f, k, v)
    return f


def test_entry_points_check_their_arguments():
    import os
    from vlatouch import _lib as L
    lib = L.lib()
    assert "scripts/franka_model_eef.py:242-288" in open(os.path.join(cases.ROOT, "include", "vlatouch.h")).read()
    ERR_ARG = -22
    S, flags = 32, L.IMGPREP_PAD
    dev = C.c_void_p(4096)            # never dereferenced: every call below is refused before a launch

    def call(frames, n=1, S=S, lut=dev, out=dev, ws=dev, ws_bytes=1 << 30, flags=flags, fdev=dev):
        arr = (L.ImgprepFrame * max(1, len(frames)))(*frames)
        return lib.vt_imgprep(arr, fdev, n, S, lut, 0x7f7f7f, flags, out, ws, ws_bytes, None)

    # the workspace query: layout, and 0 + a message for a bad table
    arr = (L.ImgprepFrame * 2)(_frame(L), _frame(L, src=None))
    head = 2 * 64 * 8                                                                     # 64 uint64 brightness partials per frame
    assert lib.vt_imgprep_workspace_bytes(arr, 2, S, flags) == head                      # fused: nothing else
    assert lib.vt_imgprep_workspace_bytes(arr, 2, S, flags | L.IMGPREP_TWO_PASS) == head + 64 * 32 * 3     # + padded height x out width x 3
    assert arr[0].ws_off == head
    big = (L.ImgprepFrame * 1)(_frame(L, rows_max=129))
    assert lib.vt_imgprep_workspace_bytes(big, 1, S, flags) == 512 + 64 * 32 * 3          # beyond the fused bound: scratch is planned
    assert lib.vt_imgprep_workspace_bytes(arr, 0, S, flags) == 0 and b"n < 1" in lib.vt_last_error()
    assert lib.vt_imgprep_workspace_bytes(None, 1, S, flags) == 0

    bad = [
        dict(n=0), dict(S=0), dict(lut=None), dict(out=None), dict(ws=None), dict(fdev=None),
        dict(frames=[_frame(L, h=0)]), dict(frames=[_frame(L, w=0)]), dict(frames=[_frame(L, out_h=0, out_w=0)]),
        dict(frames=[_frame(L, pitch=3 * 64 - 1)]), dict(frames=[_frame(L, coef_h=None)]), dict(frames=[_frame(L, coef_v=None)]),
        dict(frames=[_frame(L, ksize_h=0)]), dict(frames=[_frame(L, rows_max=0)]), dict(frames=[_frame(L, out_w=16)]),
        dict(out=C.c_void_p(4100)),                                                      # misaligned output
        dict(frames=[_frame(L, src=None)], flags=L.IMGPREP_OUT_U8),                      # missing frame in the plain-resample mode
        dict(flags=L.IMGPREP_OUT_U8 | L.IMGPREP_BRIGHT),
        dict(flags=flags | L.IMGPREP_TWO_PASS, ws_bytes=100),                            # workspace too small
    ]
    for kw in bad:
        frames = kw.pop("frames", [_frame(L, ws_off=512)])
        assert call(frames, **kw) == ERR_ARG, kw
        assert lib.vt_last_error().startswith(b"vt_imgprep"), kw
    # a table whose ws_off was not planned by the query is refused too
    assert call([_frame(L, ws_off=0)], flags=flags | L.IMGPREP_TWO_PASS) == ERR_ARG


def test_wrapper_exposes_the_switch_and_cpu_devices_are_refused():
    import types
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    from vlatouch import _lib
    from vlatouch.imgprep import DevicePreprocessor
    args = {"dataset": {}, "model": {"state_token_dim": 128}}
    vis = types.SimpleNamespace(config=types.SimpleNamespace(image_size=56), num_patches=16, hidden_size=576, eval=lambda: None)
    pol = types.SimpleNamespace(eval=lambda: None)
    m = RoboticDiffusionTransformerModel(args, device="cpu", dtype=torch.float32, vision_model=vis, policy=pol)
    assert m.device_preprocess is True
    assert RoboticDiffusionTransformerModel(args, device="cpu", dtype=torch.float32, vision_model=vis, policy=pol, device_preprocess=False).device_preprocess is False
    with pytest.raises(_lib.VtError):                # no CPU fallback inside the device path: the PIL path is preprocess_images
        DevicePreprocessor(56, (0.5,) * 3, (0.5,) * 3, "cpu")
    with pytest.raises(_lib.VtError):
        m.preprocess_images_device([None])
