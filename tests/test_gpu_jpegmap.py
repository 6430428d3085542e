"""The JPEG round trip of camera frames on the device (csrc/vt_jpegmap.hip, vlatouch/jpegmap.py) against the Pillow goldens and the numpy
restatement of libjpeg's arithmetic (tests/jpeg_ref.py, itself checked against Pillow in tests/test_jpegmap_host.py), and its way through
DevicePreprocessor, encode_frames and step.  Every comparison is bit-equal: the arithmetic is integer."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_jpegmap.npz")
SMALL = [(kind, h, w) for h, w in J.SHAPES for kind in J.CONTENTS]


@functools.lru_cache(maxsize=None)
def want(kind, h, w, quality, order):
    r = J.jpeg_roundtrip(J.make_frame(kind, h, w), quality, order)
    r.setflags(write=False)
    return r


def same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == np.uint8, (what, got.shape, got.dtype)
    n = int((got != ref).sum())
    assert n == 0, f"{what}: {n} of {ref.size} bytes differ, max |d| = {int(np.abs(got.astype(int) - ref.astype(int)).max())}"


@pytest.mark.parametrize("order", J.ORDERS)
@pytest.mark.parametrize("quality", [95, 75, 1, 100])
def test_small_frames_equal_goldens_and_restatement(quality, order):
    """Every shape x content of tests/jpeg_ref.py in ONE call (45 frames of 9 geometries)."""
    from vlatouch.jpegmap import jpeg_mapping_device
    got = jpeg_mapping_device([J.make_frame(*c) for c in SMALL], quality, order, device=DEV)
    torch.cuda.synchronize()
    g = np.load(GOLDEN) if quality in J.GOLDEN_QUALITIES else None
    for (kind, h, w), t in zip(SMALL, got):
        assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3)
        same(t, want(kind, h, w, quality, order), (kind, h, w, quality, order, "restatement"))
        if g is not None:
            same(t, g[f"out_{kind}_{h}x{w}_q{quality}_{order}"], (kind, h, w, quality, order, "golden"))


def test_narrow_frames_are_replicated_as_libjpeg_does():
    """Frames up to 4 pixels wide: the chroma component is at most 2 samples wide and jdsample.c replicates it."""
    from vlatouch.jpegmap import jpeg_mapping_device
    shapes = [(1, 2), (3, 2), (2, 3), (5, 4), (9, 1), (20, 3), (4, 5)]
    frames = [J.make_frame("noise", h, w) for h, w in shapes]
    got = jpeg_mapping_device(frames, 95, "cv2", device=DEV)
    for (h, w), a, t in zip(shapes, frames, got):
        same(t, J.pillow_roundtrip(a, 95, "cv2"), (h, w))


def test_camera_frame_walks_many_rows_of_mcus():
    from vlatouch.jpegmap import jpeg_mapping_device
    a = J.make_frame("noise", 480, 640)
    (got,) = jpeg_mapping_device([a], 95, "cv2", device=DEV)
    same(got, J.jpeg_roundtrip(a, 95, "cv2"), "480 x 640")


def test_mixed_batch_with_a_missing_frame():
    from vlatouch.jpegmap import jpeg_mapping_device
    cs = [("noise", 33, 16), ("gradient", 48, 64), ("speckle", 1, 1), ("noise", 30, 50)]
    frames = [J.make_frame(*cs[0]), None, J.make_frame(*cs[1]), J.make_frame(*cs[2]), None, J.make_frame(*cs[3])]
    got = jpeg_mapping_device(frames, 75, "rgb", device=DEV)
    assert len(got) == 6 and got[1] is None and got[4] is None
    for c, t in zip(cs, [got[0], got[2], got[3], got[5]]):
        same(t, want(*c, 75, "rgb"), c)
    assert jpeg_mapping_device([None, None], device=DEV) == [None, None]


def test_every_input_kind_gives_the_bits_of_the_contiguous_frame():
    from PIL import Image
    from vlatouch.jpegmap import jpeg_mapping_device
    a = J.make_frame("noise", 19, 21)
    ref = want("noise", 19, 21, 95, "cv2")
    wide = torch.full((19, 40, 3), 77, dtype=torch.uint8, device=DEV)
    wide[:, 5:26] = torch.from_numpy(a).to(DEV)
    view = wide[:, 5:26]                                             # pitched: rows 120 bytes apart, 15 bytes in, odd addresses
    assert not view.is_contiguous()
    got = jpeg_mapping_device([view, Image.fromarray(a), a, torch.from_numpy(a), torch.from_numpy(a).to(DEV)], 95, "cv2")
    for k, t in enumerate(got):
        same(t, ref, f"input kind {k}")
    assert int((wide[:, :5] != 77).sum()) == 0 and int((wide[:, 26:] != 77).sum()) == 0 and torch.equal(wide[:, 5:26].cpu(), torch.from_numpy(a))


def test_repeated_call_on_the_same_buffers_is_identical():
    from vlatouch.jpegmap import jpeg_mapping_device
    frames = [torch.from_numpy(J.make_frame("noise", 30, 50)).to(DEV), torch.from_numpy(J.make_frame("speckle", 17, 33)).to(DEV)]
    out = torch.empty(1 << 14, dtype=torch.uint8, device=DEV)
    ws = torch.full((1 << 14,), 0xA5, dtype=torch.uint8, device=DEV)            # stale bytes in the workspace must not matter
    first = [t.clone() for t in jpeg_mapping_device(frames, 95, "cv2", out=out, workspace=ws)]
    out.fill_(0)
    second = jpeg_mapping_device(frames, 95, "cv2", out=out, workspace=ws)
    for k, (x, y) in enumerate(zip(first, second)):
        assert y.data_ptr() >= out.data_ptr() and torch.equal(x, y), k
    same(second[0], want("noise", 30, 50, 95, "cv2"), "30 x 50")
    same(second[1], want("speckle", 17, 33, 95, "cv2"), "17 x 33")


def test_bad_arguments_return_err_arg_without_a_launch():
    from vlatouch import _lib
    L = _lib.lib()
    src = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device=DEV)
    out = torch.full((1024,), 0x5A, dtype=torch.uint8, device=DEV)
    ws = torch.full((1024,), 0x5A, dtype=torch.uint8, device=DEV)

    def table(h=16, w=16, pitch=48, src_ptr=src.data_ptr(), sized=True):
        arr = (_lib.JpegmapFrame * 1)()
        arr[0].src, arr[0].h, arr[0].w, arr[0].pitch, arr[0].out_off = src_ptr, h, w, pitch, 0
        if sized:
            assert L.vt_jpegmap_workspace_bytes(arr, 1) == 512            # 1.5 bytes per pixel of 16 x 16, carved in units of 256
        return arr

    def call(arr, n=1, quality=95, flags=1, dev=src, o=out, w=ws, ws_bytes=1024):
        return L.vt_jpegmap(arr, _lib.ptr(dev), n, quality, flags, _lib.ptr(o), _lib.ptr(w), ws_bytes, _lib.stream_ptr(DEV))

    good = table()
    bad = [("n < 1", lambda: call(good, n=0)), ("quality 0", lambda: call(good, quality=0)), ("quality 101", lambda: call(good, quality=101)),
           ("flags", lambda: call(good, flags=2)), ("short workspace", lambda: call(good, ws_bytes=511)),
           ("null table", lambda: L.vt_jpegmap(None, _lib.ptr(src), 1, 95, 0, _lib.ptr(out), _lib.ptr(ws), 1024, _lib.stream_ptr(DEV))),
           ("null device table", lambda: call(good, dev=None)), ("null out", lambda: call(good, o=None)), ("null workspace", lambda: call(good, w=None)),
           ("a ws_off the sizing call did not write", lambda: call(_with_ws_off(good, 256)))]
    for h, w, pitch, ptr in ((0, 16, 48, src.data_ptr()), (16, 0, 48, src.data_ptr()), (16, 16, 47, src.data_ptr()), (16, 16, 48, None),
                             (40000, 16, 48, src.data_ptr())):
        t = table(h, w, pitch, ptr, sized=False)
        assert L.vt_jpegmap_workspace_bytes(t, 1) == 0 and L.vt_last_error(), (h, w, pitch, ptr)
        bad.append((f"frame {h} x {w} pitch {pitch} src {ptr}", lambda t=t: call(t)))
    assert L.vt_jpegmap_workspace_bytes(good, 0) == 0 and L.vt_jpegmap_workspace_bytes(None, 1) == 0
    for what, fn in bad:
        assert fn() == -22, what                                          # VT_ERR_ARG
        assert len(L.vt_last_error()) > 10, what
    torch.cuda.synchronize()
    assert int((out != 0x5A).sum()) == 0 and int((ws != 0x5A).sum()) == 0      # nothing was launched
    good_dev = torch.from_numpy(np.frombuffer(bytes(memoryview(good)), dtype=np.uint8).copy()).to(DEV)
    assert call(good, dev=good_dev) == 0                                  # and the good call is one
    torch.cuda.synchronize()
    same(out[:768].view(16, 16, 3), J.jpeg_roundtrip(np.zeros((16, 16, 3), np.uint8), 95, "cv2"), "the good call")


def _with_ws_off(arr, ws_off):
    from vlatouch import _lib
    cp = (_lib.JpegmapFrame * 1).from_buffer_copy(arr)
    cp[0].ws_off = ws_off
    return cp


# ---- through the preprocessor and the model

def _frames48(n=4, seed=5):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(n)]


@pytest.mark.parametrize("image_size", [None, 40, (32, 56)])
def test_preprocess_with_jpeg_equals_preprocess_of_cpu_mapped_frames(image_size):
    from tests.test_gpu_imgprep import make_model
    from vlatouch.jpegmap import jpeg_mapping
    m = make_model(64, image_size=image_size)
    fr = _frames48()
    dark = (fr[1] // 8).astype(np.uint8)                                    # takes the brightness lift, after the mapping
    frames = [fr[0], None, dark, torch.from_numpy(fr[2]).to(DEV), J.make_frame("noise", 30, 50)]
    mapped = [None if f is None else jpeg_mapping(f.cpu().numpy() if isinstance(f, torch.Tensor) else f, 95) for f in frames]
    got = m.preprocess_images_device(frames, jpeg=95).clone()
    ref = m.preprocess_images_device(mapped).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    from PIL import Image
    cpu = m.preprocess_images([None if f is None else Image.fromarray(f) for f in mapped]).to(DEV, m.dtype)
    assert torch.equal(got, cpu)
    plain = m.preprocess_images_device(frames).clone()
    assert not torch.equal(plain, got)                                      # the mapping is no identity
    assert torch.equal(m.preprocess_images_device(frames, jpeg=75), m.preprocess_images_device([None if f is None else jpeg_mapping(
        f.cpu().numpy() if isinstance(f, torch.Tensor) else f, 75) for f in frames]))


def test_preprocess_with_jpeg_and_jitter():
    from tests.test_gpu_imgprep import make_model
    from vlatouch.imgaug import ColorJitterParams
    from vlatouch.jpegmap import jpeg_mapping
    m = make_model(64)
    frames = _frames48(3, seed=6)
    jit = [ColorJitterParams((1, 0, 3, 2), 1.2, 0.8, 1.3, 0.02), None, ColorJitterParams((3, 2, 1, 0), 0.9, 1.3, 0.7, -0.03)]
    got = m.preprocess_images_device(frames, jitter=jit, jpeg=95).clone()
    ref = m.preprocess_images_device([jpeg_mapping(f, 95) for f in frames], jitter=jit)
    assert torch.equal(got, ref)


def test_without_jpeg_the_call_is_todays():
    from tests.test_gpu_imgprep import as_pil, make_model
    m = make_model(64)
    frames = _frames48() + [None]
    ref = m.preprocess_images(as_pil(frames)).to(DEV, m.dtype)
    a = m.preprocess_images_device(frames).clone()
    b = m.preprocess_images_device(frames, jpeg=None).clone()
    m.preprocess_images_device(frames, jpeg=95)                             # a mapped call in between leaves the plain plan alone
    c = m.preprocess_images_device(frames)
    assert torch.equal(a, ref) and torch.equal(b, ref) and torch.equal(c, ref)
    pp = next(iter(m._imgprep.values()))
    assert pp.workspace_bytes(frames) < pp.workspace_bytes(frames, jpeg=95)
    for bad in (0, 101, True, 95.0, "95"):
        with pytest.raises(Exception):
            m.preprocess_images_device(frames, jpeg=bad)


def test_graph_capture_with_jpeg():
    """The mapped call is as capturable as the plain one: its table is cached with the plan, nothing is copied or awaited per call."""
    from tests.test_gpu_imgprep import make_model
    from vlatouch.jpegmap import jpeg_mapping
    g = np.random.default_rng(12)
    m = make_model(64)
    shapes = [(48, 64), (30, 50)]
    static = [torch.from_numpy(g.integers(0, 256, (*s, 3), dtype=np.uint8)).to(DEV) for s in shapes]
    frames = [static[0], None, static[1]]
    out = torch.empty(3, 3, 64, 64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.preprocess_images_device(frames, out=out, jpeg=95)              # warm-up: tables, plan, workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.preprocess_images_device(frames, out=out, jpeg=95)
    for rep in range(2):
        new = [g.integers(0, 256, (*sh, 3), dtype=np.uint8) for sh in shapes]
        for t, a in zip(static, new):
            t.copy_(torch.from_numpy(a))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ref = m.preprocess_images_device([jpeg_mapping(new[0]), None, jpeg_mapping(new[1])])
        assert torch.equal(out, ref), rep


def test_encode_frames_and_step_with_jpeg_mapping():
    from tests.test_gpu_imgprep import _tower_model
    from tests.test_siglip import _pil_frames
    from vlatouch.jpegmap import jpeg_mapping
    from vlatouch.label import encode_frames
    on, off = _tower_model(True), _tower_model(False)
    off.policy = on.policy
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (56, 56, 3), dtype=np.uint8) for _ in range(5)] + [None] + _pil_frames()
    mapped = [None if f is None else jpeg_mapping(f) for f in frames]
    got = encode_frames(on, frames, batch=4, jpeg_mapping=True)
    assert torch.equal(got, encode_frames(on, mapped, batch=4))
    assert torch.equal(got, encode_frames(off, frames, batch=4, jpeg_mapping=True))      # the CPU route of the same flag
    assert not torch.equal(got, encode_frames(on, frames, batch=4))
    assert torch.equal(encode_frames(on, frames, batch=4, jpeg_mapping=75), encode_frames(on, [None if f is None else jpeg_mapping(f, 75) for f in frames], batch=4))
    g = torch.Generator().manual_seed(3)
    proprio, text = torch.randn(1, 10, generator=g), torch.randn(1, 12, 96, generator=g)
    torch.manual_seed(11)
    a = on.step(proprio, _pil_frames(), text, jpeg_mapping=True)
    torch.manual_seed(11)
    b = off.step(proprio, _pil_frames(), text, jpeg_mapping=True)
    # (this configuration's synthetic policy answers with the same chunk whatever the frames: the tokens above show the mapping, not the chunk)
    assert a.shape == on.step(proprio, _pil_frames(), text).shape and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
