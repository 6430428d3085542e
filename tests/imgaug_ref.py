"""Statements of the training-time colour augmentation that the device kernel (csrc/vt_colorjitter.hip) is checked against.

(a) `color_jitter_pil`: torchvision's ColorJitter on PIL images, which is a thin layer over PIL.ImageEnhance and Image.convert("HSV")
    (UNPINNED to torchvision, which is not installed; PIL is, and PIL is the reference).
(b) `color_jitter_np`: the same arithmetic spelled out in numpy with explicit fp32 / fp64 casts and no library call; pinned to (a) by
    tests/test_imgaug_host.py.  This is what the kernel restates.
(c) `train_image_chain`: train/dataset.py:373-409 for one image with given parameters (Resize -> lift -> jitter -> pad -> processor); the
    pre-resize and the lift are those of `preprocess_images`' host path.
"""
import numpy as np

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- (a) PIL
def hue_pil(img, shift):
    """The hue step with the byte it adds to H given directly (`shift` = int(hue * 255) mod 256)."""
    from PIL import Image
    h, s, v = img.convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    nh = ((nh.astype(np.int32) + int(shift)) & 255).astype(np.uint8)        # the uint8 wrap-around add
    return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")


def color_jitter_pil(img, params):
    from PIL import ImageEnhance
    from vlatouch.imgaug import hue_shift
    for op in params.order:
        if op == 0 and params.brightness is not None:
            img = ImageEnhance.Brightness(img).enhance(params.brightness)
        elif op == 1 and params.contrast is not None:
            img = ImageEnhance.Contrast(img).enhance(params.contrast)
        elif op == 2 and params.saturation is not None:
            img = ImageEnhance.Color(img).enhance(params.saturation)
        elif op == 3 and params.hue is not None:
            img = hue_pil(img, hue_shift(params.hue))
    return img


# ---------------------------------------------------------------- (b) numpy
def blend_np(a, b, f):
    """Image.blend(a, b, f) per byte: t = (float)a + f32(f) * ((float)b - (float)a), the multiply and the add rounded separately."""
    a, b, f = np.asarray(a).astype(f32), np.asarray(b).astype(f32), f32(f)
    t = (a + (f * (b - a)).astype(f32)).astype(f32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)                    # (uint8)t: a truncation
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def luma_np(arr):
    a = arr.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def contrast_mean_np(arr):
    L = luma_np(arr)
    return int(f64(int(L.astype(np.int64).sum())) / f64(L.size) + 0.5)


def rgb_to_hsv_np(arr):
    r, g, b = (arr[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        mxf, cr = mx.astype(f32), (mx - mn).astype(f32)
        s = (cr / mxf).astype(f32)
        rc, gc, bc = (((mxf - c.astype(f32)).astype(f32) / cr).astype(f32) for c in (r, g, b))
        h_r = (bc - gc).astype(f32)
        h_g = ((f64(2.0) + rc.astype(f64)) - bc.astype(f64)).astype(f32)           # double literals: formed in double, rounded to fp32
        h_b = ((f64(4.0) + gc.astype(f64)) - rc.astype(f64)).astype(f32)
        h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b)).astype(f32)
        x = h.astype(f64) / f64(6.0) + f64(1.0)
        h = np.where(x >= 1.0, x - 1.0, x).astype(f32)                               # fmod(x, 1.0) for 0 <= x < 2, exact
        H = np.clip(np.nan_to_num(h.astype(f64) * f64(255.0)).astype(np.int64), 0, 255)
        S = np.clip(np.nan_to_num(s.astype(f64) * f64(255.0)).astype(np.int64), 0, 255)
    H, S = np.where(grey, 0, H), np.where(grey, 0, S)
    return np.stack([H, S, mx], axis=-1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb_np(hsv):
    H, S, V = (hsv[..., i].astype(np.int32) for i in range(3))
    hh = H.astype(f64) * f64(6.0) / f64(255.0)
    i = np.floor(hh).astype(np.int32)
    f = (hh - i.astype(f32).astype(f64)).astype(f32)
    fs = (S.astype(f64) / f64(255.0)).astype(f32)
    v = V.astype(f64)
    one = f64(1.0)

    def byte(x):
        return np.clip(_round_half_away(x), 0, 255).astype(np.int32)
    p = byte(v * (one - fs.astype(f64)))
    q = byte(v * (one - (fs.astype(f64) * f.astype(f64))))
    t = byte(v * (one - (fs.astype(f64) * (one - f.astype(f64)))))
    k = i % 6
    R = np.choose(k, [V, q, p, p, t, V])
    G = np.choose(k, [t, V, V, q, p, p])
    B = np.choose(k, [p, p, t, V, V, q])
    grey = S == 0
    return np.stack([np.where(grey, V, R), np.where(grey, V, G), np.where(grey, V, B)], axis=-1).astype(np.uint8)


def hue_np(arr, shift):
    hsv = rgb_to_hsv_np(arr)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 255).astype(np.uint8)
    return hsv_to_rgb_np(hsv)


def color_jitter_np(arr, params):
    from vlatouch.imgaug import hue_shift
    arr = np.asarray(arr, dtype=np.uint8)
    for op in params.order:
        if op == 0 and params.brightness is not None:
            arr = blend_np(np.zeros_like(arr), arr, params.brightness)
        elif op == 1 and params.contrast is not None:
            arr = blend_np(np.full_like(arr, contrast_mean_np(arr)), arr, params.contrast)
        elif op == 2 and params.saturation is not None:
            arr = blend_np(np.repeat(luma_np(arr)[..., None], 3, axis=-1), arr, params.saturation)
        elif op == 3 and params.hue is not None:
            arr = hue_np(arr, hue_shift(params.hue))
    return arr


# ---------------------------------------------------------------- (c) the dataset's chain for one image
def train_image_chain(img, valid, params, *, image_size, brightness, pad, processor):
    """dataset.py:373-409 for one image: `img` a PIL image (the background image where `valid` is False), `params` a ColorJitterParams or
    None.  -> pixel_values [3, S, S] fp32."""
    from PIL import Image, ImageEnhance
    if image_size is not None:
        sz = image_size
        if isinstance(sz, int):          # transforms.Resize(int): shorter side -> sz, bilinear
            w, h = img.size
            nw, nh = (sz, max(1, int(sz * h / w))) if w <= h else (max(1, int(sz * w / h)), sz)
            img = img.resize((nw, nh), resample=Image.BILINEAR)
        else:
            img = img.resize((sz[1], sz[0]), resample=Image.BILINEAR)
    if valid and brightness:
        px = np.asarray(img.convert("RGB"), dtype=np.float64)
        if px.sum() / (px.shape[0] * px.shape[1] * 255.0 * 3) <= 0.15:
            img = ImageEnhance.Brightness(img).enhance(1.75)
    if valid and params is not None:
        img = color_jitter_pil(img, params)
    if pad:
        w, h = img.size
        if w != h:
            side = max(w, h)
            sq = Image.new(img.mode, (side, side), tuple(int(x * 255) for x in processor.image_mean))
            sq.paste(img, (0, (w - h) // 2) if w > h else ((h - w) // 2, 0))
            img = sq
    return processor.preprocess(img, return_tensors="pt")["pixel_values"][0]


def background(processor):
    from PIL import Image
    S = processor.size
    mean255 = np.array([int(x * 255) for x in processor.image_mean], dtype=np.uint8).reshape(1, 1, 3)
    return Image.fromarray(np.ones((S["height"], S["width"], 3), dtype=np.uint8) * mean255)


def all_colours():
    """The 4096 x 4096 frame of all 2^24 colours."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def ramp_frame(m):
    """64 x 256 grey: row 0 is the ramp 0 .. 255, rows 1 .. 63 the constant m: over m = 0 .. 255 the rounded mean of L sweeps the byte
    range (it is (32640 + 16128 m) / 16384), and every frame holds every byte value to blend against it."""
    a = np.full((64, 256), m, dtype=np.uint8)
    a[0] = np.arange(256, dtype=np.uint8)
    return np.repeat(a[..., None], 3, axis=-1)


def half_mean_frames():
    """Three tiny grey frames whose sum of L / count is exactly x.5 (1 x 2 and 2 x 2) and, the nearest a 2 x 2 frame gets below it, x.25."""
    g = lambda rows: np.repeat(np.array(rows, dtype=np.uint8)[..., None], 3, axis=-1)
    return [g([[10, 11]]), g([[100, 101], [101, 100]]), g([[100, 101], [100, 100]])]
