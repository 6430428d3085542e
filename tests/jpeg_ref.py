"""libjpeg's baseline round trip (compress at `quality`, 4:2:0, islow DCT; decompress with fancy up-sampling) restated in numpy, without
the entropy coder, which is lossless.  Integer arithmetic throughout: the result is bit-equal to Pillow's
`Image.save(buf, "JPEG", quality=q)` + `Image.open` (tests/test_jpegmap_host.py), and csrc/vt_jpegmap.hip is checked against it.

`order="rgb"`: channel 0 of the array is red, as Pillow reads it.  `order="cv2"`: channel 0 plays blue's role, as cv2 treats whatever
array it is given, i.e. `roundtrip(img[..., ::-1])[..., ::-1]`."""
from __future__ import annotations

import numpy as np

# Annex K of ITU-T T.81, in natural (row-major) order
LUMA_BASE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    dtype=np.int64).reshape(8, 8)
CHROMA_BASE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99],
    dtype=np.int64).reshape(8, 8)

H = 32768

# the small cases of tests/golden/g25_jpegmap.npz (tools/make_golden_jpegmap.py) and what each shape hits: one block (1 x 1, 7 x 5, 8 x 8),
# one MCU (16 x 16), odd sizes with right and bottom replication (19 x 21, 17 x 33, 33 x 16), the chroma-row rule of an even height that is
# no multiple of 16 (30 x 50), several MCUs a side (48 x 64)
SHAPES = [(1, 1), (7, 5), (8, 8), (16, 16), (19, 21), (17, 33), (33, 16), (30, 50), (48, 64)]
CONTENTS = ["noise", "gradient", "zeros", "full", "speckle"]      # speckle: 0 / 255 per byte, the inverse DCT overshoots into the clamp
GOLDEN_QUALITIES = (95, 75)
ORDERS = ("rgb", "cv2")


def make_frame(kind: str, h: int, w: int) -> np.ndarray:
    """The test frame of a content kind and shape, uint8 [h, w, 3]; a pure function of its arguments."""
    rng = np.random.default_rng(1000 * h + w + 7 * CONTENTS.index(kind))
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(5 * y + x) % 256, (3 * x + 40) % 256, (2 * y + 7 * x) % 256], axis=-1).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((h, w, 3), dtype=np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, dtype=np.uint8)
    if kind == "speckle":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    raise ValueError(kind)


def pillow_roundtrip(img: np.ndarray, quality: int, order: str = "rgb") -> np.ndarray:
    """Image.save(buf, "JPEG", quality=quality) + Image.open of the array, the channel roles swapped for order="cv2"."""
    import io
    from PIL import Image
    a = np.ascontiguousarray(img[..., ::-1] if order == "cv2" else img)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=quality)
    buf.seek(0)
    out = np.asarray(Image.open(buf).convert("RGB"))
    return np.ascontiguousarray(out[..., ::-1] if order == "cv2" else out)


def quant_tables(quality: int):
    """(luma [8, 8], chroma [8, 8]) of jpeg_set_quality(quality, force_baseline), natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must lie in 1..100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * s + 50) // 100, 1, 255) for b in (LUMA_BASE, CHROMA_BASE))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd(t4, t5, t6, t7):
    """The odd part shared by jfdctint and jidctint: -> the four sums (for out7/5/3/1 forward, tmp0..3 inverse)."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _fdct_pass(d, first: bool):
    """One pass of jfdctint over the last axis of d [..., 8]."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    o7, o5, o3, o1 = _odd(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = _descale(o7, n), _descale(o5, n), _descale(o3, n), _descale(o1, n)
    return np.stack(o, axis=-1)


def _idct_pass(c, n: int):
    """One pass of jidctint over the last axis of c [..., 8], descaled by n bits."""
    c = [c[..., k] for k in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = _odd(c[7], c[5], c[3], c[1])
    return np.stack([_descale(t10 + o3, n), _descale(t11 + o2, n), _descale(t12 + o1, n), _descale(t13 + o0, n),
                     _descale(t13 - o0, n), _descale(t12 - o1, n), _descale(t11 - o2, n), _descale(t10 - o3, n)], axis=-1)


def _codec(plane: np.ndarray, t: np.ndarray) -> np.ndarray:
    """plane [8a, 8b] of samples -> the decoded samples: forward DCT, quantise, dequantise, inverse DCT, per 8 x 8 block."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128          # [a, b, row, col]
    x = _fdct_pass(blk, True)                                                             # rows
    x = _fdct_pass(x.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)                  # columns
    d = 8 * t
    c = np.sign(x) * ((np.abs(x) + (d >> 1)) // d) * t
    y = _idct_pass(c.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)                     # columns
    y = _idct_pass(y, 18)                                                                 # rows
    y = np.clip(y + 128, 0, 255)
    return y.transpose(0, 2, 1, 3).reshape(8 * a, 8 * b)


def _upsample(c: np.ndarray) -> np.ndarray:
    """h2v2 up-sampling of c [ch, cw] -> [2 ch, 2 cw]: the "fancy" triangle filter, which libjpeg's jdsample.c selects only for
    cw > 2; narrower components (frames up to 4 pixels wide) are replicated."""
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    j, i = np.arange(ch), np.arange(cw)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for v, nb in ((0, np.maximum(j - 1, 0)), (1, np.minimum(j + 1, ch - 1))):
        s = 3 * c + c[nb]
        out[v::2, 0::2] = (3 * s + s[:, np.maximum(i - 1, 0)] + 8) >> 4
        out[v::2, 1::2] = (3 * s + s[:, np.minimum(i + 1, cw - 1)] + 7) >> 4
    return out


def jpeg_roundtrip(img: np.ndarray, quality: int = 95, order: str = "rgb") -> np.ndarray:
    """img uint8 [h, w, 3] -> the decoded image, uint8 [h, w, 3]."""
    if order not in ("rgb", "cv2"):
        raise ValueError(f"order must be 'rgb' or 'cv2', got {order!r}")
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image must be uint8 [h, w, 3], got {img.dtype} {img.shape}")
    if order == "cv2":
        return jpeg_roundtrip(img[..., ::-1], quality, "rgb")[..., ::-1]
    tl, tc = quant_tables(quality)
    h, w = img.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    H16, W16 = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    p = img.astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + H) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + H - 1) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + H - 1) >> 16
    yy, xx = np.minimum(np.arange(H16), h - 1), np.minimum(np.arange(W16), w - 1)
    Yp = Y[yy][:, xx]
    jj = np.minimum(np.arange(H16 // 2), ch - 1)
    r0, r1 = 2 * jj, np.minimum(2 * jj + 1, h - 1)
    ii = np.arange(W16 // 2)
    c0, c1 = np.minimum(2 * ii, w - 1), np.minimum(2 * ii + 1, w - 1)
    bias = 1 + (ii & 1)

    def down(C):
        return (C[r0][:, c0] + C[r0][:, c1] + C[r1][:, c0] + C[r1][:, c1] + bias) >> 2

    Yd = _codec(Yp, tl)[:h, :w]
    Cbd = _upsample(_codec(down(Cb), tc)[:ch, :cw])[:h, :w]
    Crd = _upsample(_codec(down(Cr), tc)[:ch, :cw])[:h, :w]
    x, y = Crd - 128, Cbd - 128
    out = np.stack([Yd + ((91881 * x + H) >> 16), Yd + ((-22554 * y + H - 46802 * x) >> 16), Yd + ((116130 * y + H) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)
