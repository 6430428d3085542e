"""Parameters of the training-time colour augmentation (train/dataset.py:385-393) for the device pipeline (csrc/vt_colorjitter.hip,
`DevicePreprocessor(..., jitter=)`).

  * `ColorJitterParams`: one frame's operation order and factors, and their conversion to the C record `vt_colorjitter_frame`.
  * `color_jitter_params`: the draws of torchvision's `ColorJitter.get_params`, restated (UNPINNED: torchvision is not installed where this
    project is tested, so the restatement is checked against its own stated draw sequence, not against the package).
  * `draw_image_aug`: which frames of a sample are augmented, consuming the `random` stream exactly as the reference's loop does.

Of the reference's two augmentations only ColorJitter is built; `image_corrupt` (imgaug) is skipped, see `draw_image_aug`.
"""
from __future__ import annotations

import random as _random
from typing import List, Optional, Sequence

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


def draw_image_aug(valid: Sequence[bool], rng=_random, generator: Optional[torch.Generator] = None) -> List[Optional[ColorJitterParams]]:
    """The augmentation draws of one sample's frames (train/dataset.py:386-391), in frame order: a valid frame calls `rng.random()`; above
    0.5 it calls `rng.choice(["corrput_only", "color_only", "both"])` and, unless that is `corrput_only`, draws ColorJitter parameters.
    -> the per-frame list for `jitter=` (None = the frame stays as it is).

    Where the reference would also corrupt the frame (`corrput_only`, `both`: `image_corrupt`, imgaug) nothing more happens here: the
    corruption is not built, and it draws from imgaug's own generator, not from `rng`, so the streams stay in step."""
    out: List[Optional[ColorJitterParams]] = []
    for v in valid:
        params = None
        if v and rng.random() > 0.5:
            aug_type = rng.choice(AUG_TYPES)
            if aug_type != "corrput_only":
                params = color_jitter_params(generator=generator)
        out.append(params)
    return out
