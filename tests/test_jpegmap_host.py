"""CPU-only checks of the JPEG round trip of camera frames (vlatouch/jpegmap.py): the numpy restatement of libjpeg's arithmetic
(tests/jpeg_ref.py), which the kernel is tested against, equals the committed Pillow goldens and live Pillow bit for bit; its quantiser
tables are the ones Pillow writes; the CPU statement's channel orders; argument checks."""
import io
import os

import numpy as np
import pytest

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import jpeg_ref as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_jpegmap.npz")
# shapes beyond the golden's: components at most 2 samples wide (frames up to 4 pixels wide) are replicated instead of filtered
NARROW = [(1, 2), (2, 2), (1, 3), (3, 2), (2, 3), (5, 4), (9, 1), (4, 5), (6, 6)]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    n = int((got != want).sum())
    assert n == 0, f"{what}: {n} of {want.size} bytes differ, max |d| = {int(np.abs(got.astype(int) - want.astype(int)).max())}"


def test_restatement_equals_the_goldens():
    g = np.load(GOLDEN)
    seen = 0
    for h, w in J.SHAPES:
        for kind in J.CONTENTS:
            a = g[f"in_{kind}_{h}x{w}"]
            assert np.array_equal(a, J.make_frame(kind, h, w)), "the frame generator changed under the golden"
            for q in J.GOLDEN_QUALITIES:
                for order in J.ORDERS:
                    _same(J.jpeg_roundtrip(a, q, order), g[f"out_{kind}_{h}x{w}_q{q}_{order}"], (kind, h, w, q, order))
                    seen += 1
    assert seen == len(J.SHAPES) * len(J.CONTENTS) * 4 == sum(k.startswith("out_") for k in g.files)


@pytest.mark.parametrize("quality", [95, 75, 1, 10, 50, 100])
def test_restatement_equals_live_pillow(quality):
    for h, w in J.SHAPES + NARROW:
        for kind in J.CONTENTS:
            a = J.make_frame(kind, h, w)
            for order in J.ORDERS:
                _same(J.jpeg_roundtrip(a, quality, order), J.pillow_roundtrip(a, quality, order), (kind, h, w, quality, order))


@pytest.mark.parametrize("quality", [1, 10, 25, 49, 50, 75, 90, 95, 98, 100])
def test_quantiser_tables_equal_the_ones_pillow_writes(quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(J.make_frame("noise", 16, 16)).save(buf, "JPEG", quality=quality)
    buf.seek(0)
    tables = Image.open(buf).quantization          # natural order since Pillow 8.3
    luma, chroma = J.quant_tables(quality)
    assert sorted(tables) == [0, 1]
    assert list(tables[0]) == luma.reshape(-1).tolist() and list(tables[1]) == chroma.reshape(-1).tolist()


def test_cpu_statement_orders():
    from PIL import Image
    from vlatouch.jpegmap import jpeg_mapping
    a = J.make_frame("noise", 30, 50)
    for q in (95, 60):
        _same(jpeg_mapping(a, q, order="rgb"), J.pillow_roundtrip(a, q, "rgb"), ("rgb", q))
        want = J.pillow_roundtrip(a[..., ::-1], q, "rgb")[..., ::-1]
        _same(jpeg_mapping(a, q, order="cv2"), want, ("cv2", q))
        _same(jpeg_mapping(a, q), want, ("default order", q))
    _same(jpeg_mapping(a), J.pillow_roundtrip(a, 95, "cv2"), "default quality")
    _same(jpeg_mapping(Image.fromarray(a), 95), J.pillow_roundtrip(a, 95, "cv2"), "PIL input")
    assert (jpeg_mapping(a, 95, "cv2") != jpeg_mapping(a, 95, "rgb")).any()       # the order matters: the chroma weights are not symmetric
    assert jpeg_mapping(a).flags["C_CONTIGUOUS"]


def test_callers_flag_and_cpu_route():
    from PIL import Image
    from vlatouch.jpegmap import jpeg_mapped_pil, jpeg_mapping, jpeg_quality
    assert jpeg_quality(False) is None and jpeg_quality(None) is None and jpeg_quality(True) == 95 and jpeg_quality(80) == 80
    a = J.make_frame("gradient", 19, 21)
    ims = [Image.fromarray(a), None]
    assert jpeg_mapped_pil(ims, None) == ims
    got = jpeg_mapped_pil(ims, 75)
    assert got[1] is None and np.array_equal(np.asarray(got[0]), jpeg_mapping(a, 75))


@pytest.mark.parametrize("quality", [0, 101, -5, 2.5, True, "95"])
def test_bad_quality_raises(quality):
    from vlatouch.jpegmap import jpeg_mapping, jpeg_quality
    a = J.make_frame("noise", 8, 8)
    with pytest.raises((ValueError, TypeError)):
        jpeg_mapping(a, quality)
    if quality is not True:
        with pytest.raises((ValueError, TypeError)):
            jpeg_quality(quality)


def test_entry_points_check_their_arguments():
    """Through the loaded library, without a device: every call below is refused before a launch, the pointers are never read."""
    import ctypes as C
    from vlatouch import _lib as L
    lib = L.lib()
    dev = C.c_void_p(4096)

    def frame(h=480, w=640, pitch=None, src=4096, out_off=0):
        f = L.JpegmapFrame()
        f.src, f.h, f.w, f.pitch, f.out_off = src, h, w, 3 * w if pitch is None else pitch, out_off
        return f

    # the workspace query: 1.5 bytes per pixel of the frame padded to multiples of 16, every frame on a 256-byte boundary
    arr = (L.JpegmapFrame * 3)(frame(), frame(19, 21), frame(1, 1))
    assert lib.vt_jpegmap_workspace_bytes(arr, 3) == 460800 + 1536 + 512
    assert [f.ws_off for f in arr] == [0, 460800, 460800 + 1536]
    assert lib.vt_jpegmap_workspace_bytes(arr, 0) == 0 and b"n < 1" in lib.vt_last_error()
    assert lib.vt_jpegmap_workspace_bytes(None, 1) == 0
    for f in (frame(h=0), frame(w=0), frame(src=None), frame(pitch=3 * 640 - 1), frame(h=32769), frame(out_off=-1)):
        one = (L.JpegmapFrame * 1)(f)
        assert lib.vt_jpegmap_workspace_bytes(one, 1) == 0 and lib.vt_last_error().startswith(b"vt_jpegmap_workspace_bytes")
        assert lib.vt_jpegmap(one, dev, 1, 95, 1, dev, dev, 1 << 30, None) == -22 and lib.vt_last_error().startswith(b"vt_jpegmap:")

    def call(n=3, quality=95, flags=1, fdev=dev, out=dev, ws=dev, ws_bytes=1 << 30, table=arr):
        return lib.vt_jpegmap(table, fdev, n, quality, flags, out, ws, ws_bytes, None)
    moved = (L.JpegmapFrame * 3).from_buffer_copy(arr)
    moved[1].ws_off = 0
    for kw in (dict(n=0), dict(quality=0), dict(quality=101), dict(flags=2), dict(fdev=None), dict(out=None), dict(ws=None), dict(table=None),
               dict(ws_bytes=460800 + 1536 + 511), dict(ws=C.c_void_p(4100)), dict(table=moved), dict(n=65536)):
        assert call(**kw) == -22, kw                                     # VT_ERR_ARG
        assert lib.vt_last_error().startswith(b"vt_jpegmap:"), kw


def test_restatement_refuses_a_quality_outside_the_range():
    for q in (0, 101):
        with pytest.raises(ValueError):
            J.quant_tables(q)


def test_bad_order_and_frames_raise():
    from vlatouch.jpegmap import jpeg_mapping
    a = J.make_frame("noise", 8, 8)
    for fn in (jpeg_mapping, J.jpeg_roundtrip):
        with pytest.raises(ValueError):
            fn(a, 95, order="bgr")
        for bad in (a.astype(np.float32), a[..., 0], a[..., :2], np.zeros((0, 4, 3), np.uint8)):
            with pytest.raises(ValueError):
                fn(bad, 95)


def test_the_device_mapping_refuses_a_cpu_device_as_the_preprocessor_does():
    """`jpeg_mapping_device` stands on a frame stager of its own, which has no CPU route either."""
    from vlatouch import _lib
    from vlatouch.imgprep import DevicePreprocessor, FrameStager
    from vlatouch.jpegmap import jpeg_mapping_device
    with pytest.raises(_lib.VtError):
        jpeg_mapping_device([J.make_frame("noise", 8, 8)], device="cpu")
    with pytest.raises(_lib.VtError):
        FrameStager("cpu")
    with pytest.raises(_lib.VtError):
        DevicePreprocessor(16, (0.5,) * 3, (0.5,) * 3, "cpu")
