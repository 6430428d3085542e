"""CPU-only checks of the numpy statement of the reference's zero pad + INTER_AREA resize (vlatouch.imgprep.pad_and_resize_for_siglip), which
the kernel is tested against bit for bit.  cv2 is not installed, so nothing here is pinned to it: the integer-scale form is checked against
known answers of the cell sums, the fractional form against the exact box integral of the padded canvas in fp64, which it may miss by one
level where fp32 rounding flips a tie, in at most 1 pixel in 1000 (a wrong tap table misses most pixels)."""
import numpy as np
import pytest

from tests import cases  # noqa: F401  (puts the package on sys.path)

from vlatouch.imgprep import area_scale, area_taps, pad_and_resize_for_siglip as statement

REFEREE_SHAPES = [(30, 40), (37, 53), (53, 37), (45, 60), (25, 25), (100, 100)]
T = 24


def frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def padded(img):
    h, w = img.shape[:2]
    m = max(h, w)
    c = np.zeros((m, m, 3), dtype=np.uint8)
    c[(m - h) // 2:(m - h) // 2 + h, (m - w) // 2:(m - w) // 2 + w] = img
    return c


def box_integral(canvas, target):
    """The mean of the canvas over each of the target x target equal cells, exactly up to fp64: W[d, j] = the length of cell d's overlap with
    source position [j, j + 1), as a fraction of the cell."""
    m = canvas.shape[0]
    edges = np.arange(target + 1, dtype=np.float64) * m / target
    j = np.arange(m, dtype=np.float64)
    W = np.clip(np.minimum(edges[1:, None], j[None, :] + 1) - np.maximum(edges[:-1, None], j[None, :]), 0, None) * target / m
    return np.einsum("yi,ijc,xj->yxc", W, canvas.astype(np.float64), W)


def test_known_answer_of_the_fractional_form():
    cols = np.array([10, 20, 30, 40, 50], dtype=np.uint8)
    img = np.repeat(np.broadcast_to(cols[None, :, None], (5, 5, 1)), 3, axis=2)
    out = statement(img, 3)
    assert out.shape == (3, 3, 3) and out.dtype == np.uint8
    assert np.array_equal(out, np.broadcast_to(np.array([14, 30, 46], dtype=np.uint8)[None, :, None], (3, 3, 3)))
    assert np.array_equal(statement(np.ascontiguousarray(img.transpose(1, 0, 2)), 3), out.transpose(1, 0, 2))


@pytest.mark.parametrize("side", [24, 25, 30, 48, 72, 96])
def test_a_constant_frame_stays_constant(side):
    for v in (0, 1, 77, 254, 255):
        assert np.array_equal(statement(np.full((side, side, 3), v, dtype=np.uint8), T), np.full((T, T, 3), v, dtype=np.uint8))


def test_factor_two_rounds_half_up():
    img = frame(48, 48, 1)
    img[0:2, 0:2] = [[[1, 2, 3], [1, 2, 3]], [[0, 2, 4], [0, 2, 4]]]         # sums 2, 8, 14; 2 = 4 * 0 + 2 gives 1 where half-even would give 0
    out = statement(img, T)
    s = img.reshape(T, 2, T, 2, 3).astype(np.int64).sum(axis=(1, 3))
    assert np.array_equal(out, ((s + 2) >> 2).astype(np.uint8))
    assert out[0, 0].tolist() == [1, 2, 4]


@pytest.mark.parametrize("k", [3, 4])
def test_factors_three_and_four_use_the_float_formula(k):
    img = frame(k * T, k * T, k)
    if k == 4:
        img[0:4, 0:4] = 0
        img[0, 0] = [8, 24, 40]                                              # sums 16 k + 8: 0.5, 1.5, 2.5 -> 0, 2, 2 (nearest-even)
    out = statement(img, T)
    s = img.reshape(T, k, T, k, 3).astype(np.int64).sum(axis=(1, 3))
    want = np.clip(np.rint(s.astype(np.float32) * (np.float32(1.0) / np.float32(k * k))), 0, 255).astype(np.uint8)
    assert np.array_equal(out, want)
    if k == 4:
        assert out[0, 0].tolist() == [0, 2, 2]
    assert int(np.abs(out.astype(np.float64) - s / (k * k)).max() <= 0.5)


def test_factor_one_is_a_copy():
    img = frame(T, T, 7)
    assert np.array_equal(statement(img, T), img)


@pytest.mark.parametrize("h,w", REFEREE_SHAPES)
def test_statement_against_the_exact_box_integral(h, w):
    img = frame(h, w, 100 + h)
    out = statement(img, T)
    exact = box_integral(padded(img), T)
    want = np.clip(np.rint(exact), 0, 255).astype(np.int64)
    d = np.abs(out.astype(np.int64) - want)
    n = int((d != 0).sum())
    print(f"{h} x {w}: {n} of {d.size} values differ from the rounded box integral, max {int(d.max())}; "
          f"max distance to the integral {float(np.abs(out - exact).max()):.6f}")
    assert int(d.max()) <= 1 and n * 1000 <= d.size


def test_tap_tables_cover_every_cell_once():
    for m in (25, 40, 53, 60):
        idx, wgt = area_taps(m, T)
        scale = area_scale(m, T)[0]
        assert idx.shape == wgt.shape and idx.dtype == np.int32 and wgt.dtype == np.float32 and idx.shape[1] == T
        assert idx.min() >= 0 and idx.max() <= m - 1
        np.testing.assert_allclose(wgt.sum(axis=0), 1.0, atol=2e-3)          # the 1e-3 threshold may drop a sliver of a cell
        cover = np.zeros(m)
        np.add.at(cover, idx.reshape(-1), wgt.reshape(-1).astype(np.float64) * scale)
        np.testing.assert_allclose(cover, 1.0, atol=2e-3 * scale)
    with pytest.raises(ValueError):
        area_taps(48, T)


def test_pad_geometry():
    img = np.full((4, 7, 3), 255, dtype=np.uint8)                            # m = 7, (7 - 4) // 2 = 1: rows 1..4 of the canvas
    out = statement(img, 7)
    assert np.array_equal(out[1:5], np.full((4, 7, 3), 255, dtype=np.uint8)) and not out[0].any() and not out[5:].any()
    out = statement(np.ascontiguousarray(img.transpose(1, 0, 2)), 7)
    assert np.array_equal(out[:, 1:5], np.full((7, 4, 3), 255, dtype=np.uint8)) and not out[:, 0].any() and not out[:, 5:].any()
    img = np.full((24, 48, 3), 255, dtype=np.uint8)                          # white on a black border, factor 2: border rows exactly black
    out = statement(img, T)
    assert not out[:6].any() and not out[18:].any() and (out[6:18] == 255).all()
    wide = frame(30, 40, 3)
    assert np.array_equal(statement(wide, T), statement(padded(wide), T))


def test_refusals_and_argument_checks():
    with pytest.raises(ValueError, match="up-scale emulation is not built"):
        statement(frame(20, 20, 1), T)
    with pytest.raises(ValueError, match="20"):
        statement(frame(20, 20, 1), T)
    batch = np.stack([frame(30, 40, s) for s in range(3)])
    got = statement(batch, T)
    assert got.shape == (3, T, T, 3)
    for k in range(3):
        assert np.array_equal(got[k], statement(batch[k], T))
    for bad in (frame(30, 40, 1).astype(np.float32), frame(30, 40, 1).astype(np.int32), np.zeros((30, 40, 4), np.uint8), np.zeros((30, 40), np.uint8),
                np.zeros((2, 2, 30, 40, 3), np.uint8)):
        with pytest.raises(ValueError):
            statement(bad, T)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            statement(frame(30, 40, 1), bad)


def test_six_camera_frames_run_well_under_a_second():
    import time
    frames = np.stack([frame(480, 640, s) for s in range(6)])
    statement(frames[:1], 384)                                               # the table of 640 -> 384
    t0 = time.perf_counter()
    out = statement(frames, 384)
    dt = time.perf_counter() - t0
    assert out.shape == (6, 384, 384, 3)
    assert dt < 1.0, dt
