"""Parameters of the training-time colour augmentation (train/dataset.py:385-393) for the device pipeline (csrc/vt_colorjitter.hip,
`DevicePreprocessor(..., jitter=)`).

  * `ColorJitterParams`: one frame's operation order and factors, and their conversion to the C record `vt_colorjitter_frame`.
  * `color_jitter_params`: the draws of torchvision's `ColorJitter.get_params`, restated (UNPINNED: torchvision is not installed where this
    project is tested, so the restatement is checked against its own stated draw sequence, not against the package).
  * `draw_image_aug`: which frames of a sample are augmented, consuming the `random` stream exactly as the reference's loop does.

and of the training-time corruption (train/image_corrupt.py, imgaug) for csrc/vt_corrupt.hip and `DevicePreprocessor(..., corrupt=)`:

  * `CorruptParams`: one frame's order, noise and blur; `draw_image_corrupt`: their draws, with the reference's distributions, from a
    numpy generator of the caller's (imgaug's random stream is not reproduced).
  * `noise_table`, `gaussian_taps`, `average_taps`, `motion_taps`: the integer tables the device works from, built in fp64 on the host;
    `pack_corrupt`: records and tables of one call.  UNPINNED against imgaug and cv2 (neither is installed where this project is
    tested): the statement is pinned to scipy.ndimage, the device to the statement.
  * `image_corrupt_device`: the corrupted frames themselves.
"""
from __future__ import annotations

import math
import random as _random
from typing import List, Optional, Sequence

import numpy as np
import torch

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_NONE = 0, 1, 2, 3, 4      # VT_COLORJITTER_* of include/vlatouch.h
AUG_TYPES = ["corrput_only", "color_only", "both"]                               # the reference's spelling


def hue_shift(hue: float) -> int:
    """The byte torchvision's PIL `adjust_hue` adds to H: `np.uint8(hue * 255)`, truncated toward zero, modulo 256 (-0.03 -> 249)."""
    return int(hue * 255) % 256


class ColorJitterParams:
    """`order`: a permutation of (0 brightness, 1 contrast, 2 saturation, 3 hue), the order of application; a factor of None skips its
    operation.  brightness / contrast / saturation are blend factors (rounded to fp32 where they are used, as PIL does), hue is a
    fraction of the hue circle in [-0.5, 0.5]."""
    __slots__ = ("order", "brightness", "contrast", "saturation", "hue")

    def __init__(self, order: Sequence[int], brightness: Optional[float] = None, contrast: Optional[float] = None,
                 saturation: Optional[float] = None, hue: Optional[float] = None):
        order = tuple(int(i) for i in order)
        if sorted(order) != [0, 1, 2, 3]:
            raise ValueError(f"ColorJitterParams: order must be a permutation of 0..3, got {order}")
        if hue is not None and not -0.5 <= hue <= 0.5:
            raise ValueError(f"ColorJitterParams: hue {hue} is not in [-0.5, 0.5]")
        for name, f in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
            if f is not None and not f >= 0:
                raise ValueError(f"ColorJitterParams: {name} factor {f} is negative")
        self.order, self.brightness, self.contrast, self.saturation, self.hue = order, brightness, contrast, saturation, hue

    def factors(self):
        return (self.brightness, self.contrast, self.saturation, self.hue)

    def slots(self) -> List[int]:
        """The record's `order[4]`: the operation id per slot, OP_NONE where the operation's factor is None."""
        f = self.factors()
        return [op if f[op] is not None else OP_NONE for op in self.order]

    def fill_record(self, rec) -> None:
        """Write order, factors and the hue byte into a `_lib.ColorJitterFrame` (the source, sizes and offsets are the caller's)."""
        for k, op in enumerate(self.slots()):
            rec.order[k] = op
        rec.brightness = 1.0 if self.brightness is None else self.brightness
        rec.contrast = 1.0 if self.contrast is None else self.contrast
        rec.saturation = 1.0 if self.saturation is None else self.saturation
        rec.hue_shift = 0 if self.hue is None else hue_shift(self.hue)

    def __eq__(self, other):
        return isinstance(other, ColorJitterParams) and (self.order, self.factors()) == (other.order, other.factors())

    def __repr__(self):
        return (f"ColorJitterParams(order={self.order}, brightness={self.brightness}, contrast={self.contrast}, "
                f"saturation={self.saturation}, hue={self.hue})")


def _range(value, center: float, clip_at_zero: bool):
    if isinstance(value, (tuple, list)):
        lo, hi = float(value[0]), float(value[1])
    else:
        lo, hi = center - float(value), center + float(value)
        if clip_at_zero:
            lo = max(lo, 0.0)
    if lo > hi:
        raise ValueError(f"color_jitter_params: empty range ({lo}, {hi})")
    return lo, hi


def color_jitter_params(brightness=0.3, contrast=0.4, saturation=0.5, hue=0.03, generator: Optional[torch.Generator] = None) -> ColorJitterParams:
    """`transforms.ColorJitter(brightness, contrast, saturation, hue).get_params` restated (UNPINNED to torchvision): ranges
    [max(0, 1 - x), 1 + x] for brightness / contrast / saturation and [-hue, hue] for hue (a (lo, hi) pair is taken as given); the draws are
    `torch.randperm(4)`, then one `torch.empty(1).uniform_(lo, hi)` each for brightness, contrast, saturation and hue, in that order, from
    `generator` or the global one.  A degenerate range (x = 0) still consumes its draw."""
    ranges = [_range(brightness, 1.0, True), _range(contrast, 1.0, True), _range(saturation, 1.0, True), _range(hue, 0.0, False)]
    order = torch.randperm(4, generator=generator).tolist()
    vals = [float(torch.empty(1).uniform_(lo, hi, generator=generator)) for lo, hi in ranges]
    return ColorJitterParams(order, *vals)


def draw_image_aug(valid: Sequence[bool], rng=_random, generator: Optional[torch.Generator] = None, corrupt_rng=None):
    """The augmentation draws of one sample's frames (train/dataset.py:386-393), in frame order: a valid frame calls `rng.random()`; above
    0.5 it calls `rng.choice(["corrput_only", "color_only", "both"])` and, unless that is `corrput_only`, draws ColorJitter parameters.
    -> the per-frame list for `jitter=` (None = the frame stays as it is).

    With `corrupt_rng` (a numpy `Generator` the caller owns) -> (jitter, corrupt): a frame whose type is not `color_only` also gets the
    `CorruptParams` of `draw_image_corrupt(corrupt_rng)`, for `corrupt=`.  The reference's corruption draws from imgaug's own generator,
    not from `rng`; here it draws from `corrupt_rng` alone, so `rng`, `generator` and the jitter list are the same with and without it."""
    out: List[Optional[ColorJitterParams]] = []
    corrupt: List[Optional[CorruptParams]] = []
    for v in valid:
        params = cor = None
        if v and rng.random() > 0.5:
            aug_type = rng.choice(AUG_TYPES)
            if aug_type != "corrput_only":
                params = color_jitter_params(generator=generator)
            if aug_type != "color_only" and corrupt_rng is not None:
                cor = draw_image_corrupt(corrupt_rng)
        out.append(params)
        corrupt.append(cor)
    return out if corrupt_rng is None else (out, corrupt)


# ---------------------------------------------------------------------------------------------------------------- image_corrupt
# train/image_corrupt.py: iaa.Sequential([OneOf(noise), SomeOf((0, 1), [OneOf([Gaussian, Average, Median]), Motion])], random_order=True),
# restated in integers.  UNPINNED against imgaug and cv2, which are not installed where this project is tested: the
# arithmetic below is pinned to scipy.ndimage on the CPU (tests/test_corrupt_host.py), the device to this statement bit for bit.
NOISE_KINDS = {"gaussian": 1, "laplace": 2, "poisson": 3}                        # VT_CORRUPT_NOISE_* of include/vlatouch.h (0 = none)
BLUR_KINDS = {"gaussian": 1, "average": 2, "median": 3, "motion": 4}             # VT_CORRUPT_BLUR_* (0 = none)
THRESHOLDS = 510            # C[n], n = -255 .. 254
TAP_SUM = 1 << 20           # D of the Gaussian and motion taps
MAX_RADIUS = 18             # motion blur at k = 37
NOISE_MAX = 0.05 * 255      # the upper end of s and lam


class CorruptParams:
    """One frame's corruption.  `noise_first`: the order of the two halves.  `noise`: None, "gaussian", "laplace" (both with `scale` = s)
    or "poisson" (`scale` = lam, random sign); `per_channel`: one draw per byte, else one per pixel; `key`: the 64-bit Philox key of the
    frame's draws.  `blur`: None, "gaussian" (`sigma`), "average" (`k` in 2..7), "median" (`k` odd in 3..11) or "motion" (`k` odd in
    3..37, `angle` in degrees, `direction` in [-1, 1])."""
    __slots__ = ("noise_first", "noise", "scale", "per_channel", "key", "blur", "sigma", "k", "angle", "direction", "_tables")

    def __init__(self, noise_first: bool = True, noise: Optional[str] = None, scale: float = 0.0, per_channel: bool = False, key: int = 0,
                 blur: Optional[str] = None, sigma: float = 0.0, k: int = 0, angle: float = 0.0, direction: float = 0.0):
        if noise is not None and noise not in NOISE_KINDS:
            raise ValueError(f"CorruptParams: noise must be None or one of {sorted(NOISE_KINDS)}, got {noise!r}")
        if blur is not None and blur not in BLUR_KINDS:
            raise ValueError(f"CorruptParams: blur must be None or one of {sorted(BLUR_KINDS)}, got {blur!r}")
        if noise is not None and not scale >= 0:
            raise ValueError(f"CorruptParams: noise scale {scale} is negative")
        if not 0 <= int(key) < 1 << 64:
            raise ValueError(f"CorruptParams: key {key} is not a 64-bit unsigned integer")
        k = int(k)
        if blur == "gaussian" and not sigma >= 0:
            raise ValueError(f"CorruptParams: sigma {sigma} is negative")
        if blur == "average" and not 2 <= k <= 7:
            raise ValueError(f"CorruptParams: average blur k = {k} is not in 2..7")
        if blur == "median" and not (3 <= k <= 11 and k % 2):
            raise ValueError(f"CorruptParams: median blur k = {k} is not odd in 3..11")
        if blur == "motion" and not (3 <= k <= 2 * MAX_RADIUS + 1 and k % 2 and -1 <= direction <= 1):
            raise ValueError(f"CorruptParams: motion blur needs k odd in 3..{2 * MAX_RADIUS + 1} and direction in [-1, 1], got {k}, {direction}")
        self.noise_first, self.noise, self.scale, self.per_channel, self.key = bool(noise_first), noise, float(scale), bool(per_channel), int(key)
        self.blur, self.sigma, self.k, self.angle, self.direction = blur, float(sigma), k, float(angle), float(direction)
        self._tables = None

    def _state(self):
        return (self.noise_first, self.noise, self.scale, self.per_channel, self.key, self.blur, self.sigma, self.k, self.angle, self.direction)

    def taps(self):
        """-> (blur id, k, taps int32 [n, 3] of (dy, dx, W) or None): the blur as the device runs it.  A Gaussian below sigma 1e-3 is no blur."""
        if self.blur is None or (self.blur == "gaussian" and self.sigma < 1e-3):
            return 0, 0, None
        if self.blur == "median":
            return BLUR_KINDS["median"], self.k, None
        t = (gaussian_taps(self.sigma) if self.blur == "gaussian" else average_taps(self.k) if self.blur == "average"
             else motion_taps(self.k, self.angle, self.direction))
        k = self.k if self.blur != "gaussian" else gaussian_ksize(self.sigma)
        return BLUR_KINDS[self.blur], k, t

    def tables(self):
        """-> (thresholds uint32 [510] or None, (blur id, k, taps)), computed once per object."""
        if self._tables is None:
            self._tables = (noise_table(self) if self.noise is not None else None, self.taps())
        return self._tables

    def __eq__(self, other):
        return isinstance(other, CorruptParams) and self._state() == other._state()

    def __repr__(self):
        return ("CorruptParams(noise_first={}, noise={!r}, scale={}, per_channel={}, key={}, blur={!r}, sigma={}, k={}, angle={}, "
                "direction={})".format(*self._state()))


def _norm_cdf(z: float) -> float:
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def noise_table(params: CorruptParams) -> np.ndarray:
    """C[n] = min(2^32 - 1, floor(2^32 P(X <= n))) for n = -255 .. 254, uint32 [510], X the frame's noise rounded to an integer: the value
    the device adds to a byte is -255 + #{n : u >= C[n]} for a 32-bit word u, which also limits it to +-255.  fp64 throughout.
    gaussian: Phi((n + 0.5) / s);  laplace: its CDF at n + 0.5;  poisson: sign * K, K ~ Poisson(lam), the sign +-1 equiprobable, so
    P(0) = exp(-lam) and P(+-k) = pmf(k) / 2.  s = 0 or lam = 0 puts all mass at 0."""
    if params.noise is None:
        raise ValueError("noise_table: the parameters carry no noise")
    s = params.scale
    n = np.arange(-255, 255)
    if s == 0:
        p = (n >= 0).astype(np.float64)
    elif params.noise == "gaussian":
        p = np.array([_norm_cdf((i + 0.5) / s) for i in n])
    elif params.noise == "laplace":
        x = (n + 0.5) / s
        p = np.where(x < 0, 0.5 * np.exp(np.minimum(x, 0)), 1.0 - 0.5 * np.exp(-np.maximum(x, 0)))
    else:
        kk = np.arange(0, 256)
        pmf = np.exp(kk * math.log(s) - s - np.array([math.lgamma(i + 1.0) for i in kk]))
        cdf = np.minimum(np.cumsum(pmf), 1.0)                   # P(K <= k), k = 0 .. 255
        p = np.where(n >= 0, 0.5 + 0.5 * cdf[np.maximum(n, 0)], 0.5 * (1.0 - cdf[np.maximum(-n - 1, 0)]))
    c = np.minimum(np.floor(np.clip(p, 0.0, 1.0) * 4294967296.0), 4294967295.0)
    return np.maximum.accumulate(c).astype(np.uint32)           # non-decreasing whatever the last bit of an exp did


def _largest_remainder(w: np.ndarray, total: int) -> np.ndarray:
    """Non-negative real weights -> integers of the same proportions that sum to `total` exactly (ties go to the earlier entry)."""
    x = w / w.sum() * total
    fl = np.floor(x)
    short = int(total - fl.sum())
    if not 0 <= short <= x.size:
        raise ValueError(f"_largest_remainder: {short} units left over {x.size} weights")
    order = np.argsort(-(x - fl), kind="stable")
    fl[order[:short]] += 1
    return fl.astype(np.int64)


def _taps_of(matrix: np.ndarray, total: int) -> np.ndarray:
    """A real k x k correlation kernel (k odd) -> its non-zero taps (dy, dx, W), int32 [n, 3], W summing to `total`, in row-major order."""
    k = matrix.shape[0]
    W = _largest_remainder(matrix.reshape(-1).astype(np.float64), total).reshape(k, k)
    ys, xs = np.nonzero(W)
    return np.stack([ys - k // 2, xs - k // 2, W[ys, xs]], axis=1).astype(np.int32)


def gaussian_ksize(sigma: float) -> int:
    """imgaug's rule for cv2.GaussianBlur: max(int(3.3 sigma), 5), plus 1 if even: 5, 7 or 9 for sigma <= 3."""
    k = max(int(3.3 * sigma), 5)
    return k + 1 - k % 2


def gaussian_kernel(sigma: float) -> np.ndarray:
    """The real k x k weights: exp(-(i - c)^2 / (2 sigma^2)), normalised, as the outer product."""
    k = gaussian_ksize(sigma)
    g = np.exp(-((np.arange(k) - k // 2) ** 2) / (2.0 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g)


def gaussian_taps(sigma: float) -> np.ndarray:
    """The Gaussian blur as integer taps (at most 81), sum 2^20."""
    if not sigma >= 1e-3:
        raise ValueError(f"gaussian_taps: sigma {sigma} < 1e-3 is no blur")
    return _taps_of(gaussian_kernel(sigma), TAP_SUM)


def average_taps(k: int) -> np.ndarray:
    """The k x k box over y - k // 2 .. y - k // 2 + k - 1 (likewise x): k^2 unit taps, D = k^2."""
    if not 2 <= k <= 7:
        raise ValueError(f"average_taps: k = {k} is not in 2..7")
    o = np.arange(k) - k // 2
    dy, dx = np.meshgrid(o, o, indexing="ij")
    return np.stack([dy.reshape(-1), dx.reshape(-1), np.ones(k * k, dtype=np.int64)], axis=1).astype(np.int32)


def motion_kernel(k: int, angle: float, direction: float) -> np.ndarray:
    """imgaug's MotionBlur matrix, real k x k, sum 1: column k // 2 = uint8(255 linspace(d, 1 - d, k)), d = (direction + 1) / 2, rotated by
    `angle` degrees about ((k - 1) / 2, (k - 1) / 2) with bilinear interpolation and zeros outside, rounded to uint8, divided by its sum.
    The choice made here (UNPINNED): output (x, y) reads the source at c + R(-angle)(p - c), R(a) = [[cos a, -sin a], [sin a, cos a]] on
    (x, y) with y down, i.e. the line turns clockwise on the screen for a positive angle; coordinates are rounded to 1e-9 so that a
    multiple of 90 degrees samples exactly."""
    if not (3 <= k <= 2 * MAX_RADIUS + 1 and k % 2):
        raise ValueError(f"motion_kernel: k = {k} is not odd in 3..{2 * MAX_RADIUS + 1}")
    d = (direction + 1.0) / 2.0
    M = np.zeros((k, k), dtype=np.float64)
    M[:, k // 2] = (np.linspace(d, 1.0 - d, k) * 255.0).astype(np.uint8)
    c = (k - 1) / 2.0
    th = math.radians(angle)
    cs, sn = math.cos(th), math.sin(th)
    ys, xs = np.mgrid[0:k, 0:k].astype(np.float64)
    sx = np.round(c + cs * (xs - c) + sn * (ys - c), 9)
    sy = np.round(c - sn * (xs - c) + cs * (ys - c), 9)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    P = np.zeros((k + 2, k + 2), dtype=np.float64)              # zeros outside
    P[1:-1, 1:-1] = M

    def at(yy, xx):
        return P[np.clip(yy + 1, 0, k + 1), np.clip(xx + 1, 0, k + 1)]
    R = ((1 - fy) * ((1 - fx) * at(y0, x0) + fx * at(y0, x0 + 1)) + fy * ((1 - fx) * at(y0 + 1, x0) + fx * at(y0 + 1, x0 + 1)))
    R = np.clip(np.floor(R + 0.5), 0, 255)
    if R.sum() == 0:
        raise ValueError(f"motion_kernel: k = {k}, angle {angle}, direction {direction} leaves an empty kernel")
    return R / R.sum()


def motion_taps(k: int, angle: float, direction: float) -> np.ndarray:
    """The motion blur as integer taps: the non-zero entries of `motion_kernel`, sum 2^20, radius at most k // 2 <= 18."""
    return _taps_of(motion_kernel(k, angle, direction), TAP_SUM)


def draw_image_corrupt(np_rng) -> CorruptParams:
    """One frame's parameters with the distributions of train/image_corrupt.py, from a numpy `Generator` the caller owns (the stream is
    this project's, not imgaug's).  Order: noise first with probability 1/2.  Noise: one of the three kinds uniformly, s or lam ~
    U(0, 12.75), per channel with probability 1/2, a fresh 64-bit key.  Blur: none with probability 1/2 (SomeOf((0, 1))); else one of
    the two children uniformly: OneOf(gaussian sigma ~ U(0, 3); average k ~ U{2..7}; median k ~ U{3..11}, plus 1 if even) or motion
    (k ~ U{3..36}, plus 1 if even, angle ~ U(0, 360), direction ~ U(-1, 1))."""
    g = np_rng
    noise_first = bool(g.random() < 0.5)
    noise = ("gaussian", "laplace", "poisson")[int(g.integers(3))]
    scale = float(g.uniform(0.0, NOISE_MAX))
    per_channel = bool(g.random() < 0.5)
    key = int(g.integers(0, 1 << 64, dtype=np.uint64))
    kw = {}
    if g.random() >= 0.5:
        if int(g.integers(2)) == 0:
            which = int(g.integers(3))
            if which == 0:
                kw = dict(blur="gaussian", sigma=float(g.uniform(0.0, 3.0)))
            elif which == 1:
                kw = dict(blur="average", k=int(g.integers(2, 8)))
            else:
                k = int(g.integers(3, 12))
                kw = dict(blur="median", k=k + 1 - k % 2)
        else:
            k = int(g.integers(3, 37))
            kw = dict(blur="motion", k=k + 1 - k % 2, angle=float(g.uniform(0.0, 360.0)), direction=float(g.uniform(-1.0, 1.0)))
    return CorruptParams(noise_first, noise, scale, per_channel, key, **kw)


def pack_corrupt(records, params: Sequence[Optional["CorruptParams"]]) -> np.ndarray:
    """Write the corruption fields of the `_lib.CorruptFrame` records (source, sizes and offsets are the caller's) from `params`, one entry
    per record, None = the frame is copied -> the tables of all frames as uint32 words, where the records' offsets point."""
    words, off = [], 0
    for rec, p in zip(records, params):
        rec.key = rec.noise = rec.per_channel = rec.blur = rec.k = rec.order = rec.noise_off = rec.taps_off = rec.ntaps = rec.tap_sum = 0
        if p is None:
            continue
        C, (blur, k, taps) = p.tables()
        rec.order = 0 if p.noise_first else 1
        if C is not None:
            rec.noise, rec.per_channel, rec.key, rec.noise_off = NOISE_KINDS[p.noise], int(p.per_channel), p.key, off
            words.append(C)
            off += C.size
        rec.blur, rec.k = blur, k
        if taps is not None:
            rec.taps_off, rec.ntaps, rec.tap_sum = off, taps.shape[0], int(taps[:, 2].sum())
            words.append(taps.reshape(-1).view(np.uint32))
            off += taps.size
    return np.concatenate(words) if words else np.zeros(0, dtype=np.uint32)


# the most table words one frame can need: its thresholds and a dense 37 x 37 tap list
TABLE_WORDS_MAX = THRESHOLDS + 3 * (2 * MAX_RADIUS + 1) ** 2


def corrupt_list(frames: Sequence, corrupt, err=ValueError):
    """`corrupt` checked against the frames -> the per-frame list, or None where no frame is corrupted."""
    if corrupt is None:
        return None
    corrupt = list(corrupt)
    if len(corrupt) != len(frames):
        raise err(f"corrupt has {len(corrupt)} entries for {len(frames)} frames")
    for i, (im, p) in enumerate(zip(frames, corrupt)):
        if p is None:
            continue
        if not isinstance(p, CorruptParams):
            raise err(f"corrupt entry {i} must be None or a CorruptParams, got {type(p).__name__}")
        if im is None:
            raise err(f"corrupt entry {i} belongs to a missing frame (the reference never augments an invalid image)")
    return corrupt if any(p is not None for p in corrupt) else None


@torch.no_grad()
def image_corrupt_device(frames: Sequence, params: Sequence[Optional[CorruptParams]], out: Optional[torch.Tensor] = None,
                         device=None) -> List[Optional[torch.Tensor]]:
    """`image_corrupt` of every frame on the card (csrc/vt_corrupt.hip): per frame a PIL image, uint8 [H, W, 3] array, or uint8 tensor
    (host or device, pitched views included) and its `CorruptParams`; a frame whose entry is None is copied, a `None` frame stays `None`
    (and takes no parameters).  Returns device uint8 [H, W, 3] tensors, views of `out` (a contiguous uint8 device tensor of enough bytes;
    allocated when None).  `device`: where to run when no frame is a device tensor (default: the current one).  Launches go to the
    current stream."""
    from . import _lib
    from .jpegmap import _stager
    frames = list(frames)
    params = corrupt_list(frames, params, _lib.VtError) or [None] * len(frames)
    if device is None:
        device = next((f.device for f in frames if isinstance(f, torch.Tensor) and f.is_cuda), "cuda")
    st = _stager(device)
    idx = [i for i, f in enumerate(frames) if f is not None]
    res: List[Optional[torch.Tensor]] = [None] * len(frames)
    if not idx:
        return res
    with torch.cuda.device(st.device):
        items, _keep = st.gather([frames[i] for i in idx])       # _keep: contiguous copies of exotic views, alive until the launch is queued
        arr = (_lib.CorruptFrame * len(idx))()
        off = 0
        for f, (ptr, h, w, pitch) in zip(arr, items):
            f.src, f.h, f.w, f.pitch, f.out_off = ptr, h, w, pitch, off
            off += (3 * h * w + 15) // 16 * 16
        words = pack_corrupt(arr, [params[i] for i in idx])
        if out is not None and (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != st.device or out.numel() < off):
            raise _lib.VtError(f"out must be a contiguous uint8 tensor of at least {off} bytes on {st.device}")
        if out is None:
            out = torch.empty(off, dtype=torch.uint8, device=st.device)
        dev = st.to_device(arr)
        tdev = torch.from_numpy(words.view(np.uint8).copy()).to(st.device) if words.size else None
        _lib.check(_lib.lib().vt_corrupt(arr, _lib.ptr(dev), len(idx), words.ctypes.data if words.size else None,
                                         _lib.ptr(tdev) if tdev is not None else None, words.size, _lib.ptr(out), _lib.stream_ptr(st.device)),
                   "vt_corrupt")
    flat = out.view(-1)
    for f, i in zip(arr, idx):
        res[i] = flat[f.out_off:f.out_off + 3 * f.h * f.w].view(f.h, f.w, 3)
    return res
