"""CPU-only checks of the frame corruption's host side (vlatouch/imgaug.py) and of its numpy statement (tests/corrupt_ref.py, what
csrc/vt_corrupt.hip reproduces bit for bit): the statement against scipy.ndimage, the threshold tables against their distributions, the
integer taps, the parameter draws, the C entry point's argument checks (no launch happens), and that the corruption leaves every other
draw of a batch where it was.

Bounds.  Tap blurs: weights scaled to D = 2^20 by largest remainder move each real weight by less than 2^-20, so S / D lies within
taps * 255 / 2^20 of the real correlation and the rounded byte within 0.5 + taps * 255 / 2^20.  Moments: 2^18 draws, 5 standard errors,
the standard errors from the rounded distribution's own second and fourth moments (computed here from math.erf / exp, not from the
table).  Frequencies: 20 000 draws, 5 binomial standard errors."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import corrupt_ref as R
from vlatouch import imgaug as A

VT_ERR_ARG = -22                                     # csrc/vt_common.h
KINDS = ("gaussian", "laplace", "poisson")


def rand_frame(g, h, w):
    return g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def smooth_frame(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin(0.3 * x + 0.2 * y)], axis=-1).astype(np.uint8)


def frames():
    g = np.random.default_rng(5)
    return [rand_frame(g, 13, 17), rand_frame(g, 3, 50), rand_frame(g, 1, 1), rand_frame(g, 1, 40), smooth_frame(33, 29), smooth_frame(3, 50)]


# ------------------------------------------------------------------------------------------------ 1. Philox
def test_philox_known_answer_and_word_selection():
    # Random123's known-answer test of philox4x32-10 for a zero counter and key
    assert R.philox4x32_10(np.zeros(1, dtype=np.uint64), 0)[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    key = 0x0123456789ABCDEF
    w = R.philox4x32_10(np.arange(5, dtype=np.uint64) + np.uint64(1 << 33), key)
    idx = (np.arange(20, dtype=np.uint64) + np.uint64(4 << 33))
    assert np.array_equal(R.philox_words(idx, key), w.reshape(-1))
    assert not np.array_equal(w, R.philox4x32_10(np.arange(5, dtype=np.uint64) + np.uint64(1 << 33), key + 1))


# ------------------------------------------------------------------------------------------------ 2. the statement against scipy.ndimage
def test_border_indices():
    i = np.arange(-40, 40)
    for n in (1, 2, 3, 7):
        ref = np.pad(np.arange(n), 40, mode="reflect") if n > 1 else np.zeros(80 + n, dtype=np.int64)
        assert np.array_equal(R.mirror_index(i, n), ref[: i.size]), n
        assert np.array_equal(R.replicate_index(i, n), np.pad(np.arange(n), 40, mode="edge")[: i.size]), n


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
def test_median_equals_scipy(k):
    ndi = pytest.importorskip("scipy.ndimage")
    for a in frames():
        assert np.array_equal(R.median_np(a, k), ndi.median_filter(a, size=(k, k, 1), mode="nearest")), (k, a.shape)


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_average_equals_scipy_rounded_half_to_even(k):
    ndi = pytest.importorskip("scipy.ndimage")
    taps = A.average_taps(k)
    assert taps.shape == (k * k, 3) and (taps[:, 2] == 1).all()
    assert taps[:, :2].min() == -(k // 2) and taps[:, :2].max() == k - 1 - k // 2
    halves = 0
    for a in frames():
        S = ndi.correlate(a.astype(np.int64), np.ones((k, k, 1), dtype=np.int64), mode="mirror")
        assert np.array_equal(R.tap_sums(a, taps)[0], S), (k, a.shape)
        q, r = np.divmod(S, k * k)
        want = q + ((2 * r > k * k) | ((2 * r == k * k) & (q % 2 == 1)))
        assert np.array_equal(want, np.rint(S / (k * k)).astype(np.int64))          # np.rint is half to even; S / k^2 is exact enough at .5
        assert np.array_equal(R.tap_correlate(a, taps), want.astype(np.uint8)), (k, a.shape)
        halves += int((2 * r == k * k).sum())
    assert k % 2 or halves > 0                                                       # even k: exact halves do occur


def _real_blurs():
    out = [("gaussian", s, A.gaussian_kernel(s), A.gaussian_taps(s)) for s in (0.5, 1.0, 2.0, 2.9)]
    for k, angle, direction in [(3, 0.0, 0.0), (17, 37.0, 0.4), (37, 37.0, -1.0), (37, 90.0, 1.0), (9, 200.5, -0.3)]:
        out.append(("motion", (k, angle, direction), A.motion_kernel(k, angle, direction), A.motion_taps(k, angle, direction)))
    return out


def test_gaussian_and_motion_stay_within_the_stated_distance_of_the_real_correlation():
    ndi = pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for kind, p, kernel, taps in _real_blurs():
        ntaps = int((kernel > 0).sum())
        bound = ntaps * 255 / 2 ** 20
        assert bound < 0.83 - 0.5 + 1e-9
        for a in frames():
            real = ndi.correlate(a.astype(np.float64), kernel[:, :, None], mode="mirror")
            S, D = R.tap_sums(a, taps)
            assert D == 1 << 20
            d_exact = float(np.abs(S / D - real).max())
            d_byte = float(np.abs(R.tap_correlate(a, taps).astype(np.float64) - real).max())
            worst = max(worst, d_byte)
            assert d_exact <= bound + 1e-9 and d_byte <= 0.5 + bound, (kind, p, a.shape, d_exact, d_byte, bound)
    print(f"largest |byte - real| = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 3. the threshold tables
def _rounded_pmf(kind, s):
    """P(X_rounded = n), n = -255 .. 255 (the tails collected at the ends), from the distribution's own formulas."""
    n = np.arange(-255, 256)
    if kind == "gaussian":
        cdf = lambda x: 0.5 * (1.0 + math.erf(x / (s * math.sqrt(2.0))))
    elif kind == "laplace":
        cdf = lambda x: 0.5 * math.exp(x / s) if x < 0 else 1.0 - 0.5 * math.exp(-x / s)
    if kind == "poisson":
        pk = np.array([math.exp(k * math.log(s) - s - math.lgamma(k + 1)) for k in range(256)])
        p = np.concatenate([pk[:0:-1] / 2, pk[:1], pk[1:] / 2])
    else:
        edges = np.array([0.0] + [cdf(i + 0.5) for i in n[:-1]] + [1.0])
        p = np.diff(edges)
    assert abs(p.sum() - 1) < 1e-9
    return n, p


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("s", [0.3, 2.5, 12.75])
def test_table_is_monotone_and_its_draws_have_the_distributions_moments(kind, s):
    p = A.CorruptParams(noise=kind, scale=s, key=77)
    Ctab = A.noise_table(p)
    assert Ctab.dtype == np.uint32 and Ctab.shape == (A.THRESHOLDS,) and (np.diff(Ctab.astype(np.int64)) >= 0).all()
    N = 1 << 18
    draws = R.table_lookup(Ctab, R.philox_words(np.arange(N, dtype=np.uint64), p.key)).astype(np.float64)
    n, pmf = _rounded_pmf(kind, s)
    mu = float((n * pmf).sum())
    var = float(((n - mu) ** 2 * pmf).sum())
    m4 = float(((n - mu) ** 4 * pmf).sum())
    se_mean, se_var = math.sqrt(var / N), math.sqrt((m4 - var * var) / N)
    got_mean, got_var = float(draws.mean()), float(draws.var())
    print(f"{kind} s={s}: mean {got_mean:+.4f} (want {mu:+.4f}, se {se_mean:.4f}), var {got_var:.4f} (want {var:.4f}, se {se_var:.4f})")
    assert abs(got_mean - mu) <= 5 * se_mean and abs(got_var - var) <= 5 * se_var
    # the table is the distribution itself, to the last unit of 2^-32
    tab_pmf = np.diff(np.concatenate([[0], Ctab.astype(np.float64), [2.0 ** 32]])) / 2.0 ** 32
    assert np.abs(tab_pmf - pmf).max() <= 2.0 ** -31 + 1e-12
    if kind == "poisson":
        assert abs(tab_pmf[255] - math.exp(-s)) <= 2.0 ** -31                                      # P(0) = exp(-lam)
        assert np.abs(tab_pmf[256:] - tab_pmf[254::-1]).max() <= 2.0 ** -30                        # the sign is symmetric


@pytest.mark.parametrize("kind", KINDS)
def test_zero_scale_is_a_no_op(kind):
    p = A.CorruptParams(noise=kind, scale=0.0, per_channel=True, key=3)
    Ctab = A.noise_table(p)
    u = np.array([0, 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1], dtype=np.uint32)
    assert (R.table_lookup(Ctab, u)[:4] == 0).all()
    a = frames()[0]
    assert np.array_equal(R.image_corrupt_np(a, p), a)


# ------------------------------------------------------------------------------------------------ 4. the taps
def test_gaussian_taps():
    assert [A.gaussian_ksize(s) for s in (0.5, 2.0, 2.9)] == [5, 7, 9]
    for s in (0.001, 0.5, 2.0, 2.9, 3.0):
        t = A.gaussian_taps(s)
        k = A.gaussian_ksize(s)
        assert t.dtype == np.int32 and int(t[:, 2].sum()) == 1 << 20 and (t[:, 2] > 0).all() and len(t) <= 81
        assert np.abs(t[:, :2]).max() <= k // 2
    with pytest.raises(ValueError):
        A.gaussian_taps(0.0)
    assert A.CorruptParams(blur="gaussian", sigma=5e-4).taps() == (0, 0, None)                    # below 1e-3: no blur


def test_motion_taps():
    for k in (3, 17, 37):
        for direction in (-1.0, 0.0, 0.6):
            d = (direction + 1) / 2
            col = np.floor(np.linspace(d, 1 - d, k) * 255).astype(np.int64)
            want = col / col.sum() * 2 ** 20
            t0 = A.motion_taps(k, 0.0, direction)
            nz = np.nonzero(col)[0]
            assert (t0[:, 1] == 0).all() and np.array_equal(t0[:, 0], nz - k // 2)                # angle 0: the column
            assert np.abs(t0[:, 2] - want[nz]).max() < 1 and int(t0[:, 2].sum()) == 1 << 20
            t90 = A.motion_taps(k, 90.0, direction)
            # angle 90: the row; output (x, y) reads the source at (c + dy, c - dx), so the column lies along the row from right to left
            assert (t90[:, 0] == 0).all() and np.array_equal(np.sort(-t90[:, 1]), nz - k // 2)
            assert np.abs(t90[np.argsort(-t90[:, 1]), 2] - t0[:, 2]).max() <= 1                   # equal weights but for where a tied unit went
            if direction == 0.0:
                assert len(t0) == k and np.abs(t0[:, 2] - 2 ** 20 / k).max() < 1                  # direction 0: uniform
    g = np.random.default_rng(1)
    for _ in range(40):
        t = A.motion_taps(37, float(g.uniform(0, 360)), float(g.uniform(-1, 1)))
        assert np.abs(t[:, :2]).max() <= A.MAX_RADIUS and int(t[:, 2].sum()) == 1 << 20 and (t[:, 2] > 0).all()
    # 37 degrees turns the line clockwise on the screen (y down): its lower half (dy > 0) moves to the left (dx < 0)
    t = A.motion_taps(17, 37.0, 0.0)
    low = t[t[:, 0] > 2]
    assert (low[:, 1] < 0).all()


# ------------------------------------------------------------------------------------------------ 5. the draws
def _within(count, n, p, what):
    se = math.sqrt(p * (1 - p) / n)
    assert abs(count / n - p) <= 5 * se, (what, count / n, p, se)


def test_draws_are_deterministic_and_have_the_stated_frequencies():
    a = [A.draw_image_corrupt(np.random.default_rng(9)) for _ in range(2)]
    assert a[0] == a[1]
    g = np.random.default_rng(2024)
    N = 20000
    ps = [A.draw_image_corrupt(g) for _ in range(N)]
    assert len({p.key for p in ps}) == N
    _within(sum(p.noise_first for p in ps), N, 1 / 2, "order")
    _within(sum(p.per_channel for p in ps), N, 1 / 2, "per_channel")
    for kind in KINDS:
        _within(sum(p.noise == kind for p in ps), N, 1 / 3, kind)
    assert all(0 <= p.scale <= A.NOISE_MAX for p in ps)
    _within(sum(p.scale < A.NOISE_MAX / 4 for p in ps), N, 1 / 4, "scale quartile")
    _within(sum(p.blur is None for p in ps), N, 1 / 2, "no blur")
    _within(sum(p.blur == "motion" for p in ps), N, 1 / 4, "motion")
    for kind in ("gaussian", "average", "median"):
        _within(sum(p.blur == kind for p in ps), N, 1 / 12, kind)
    for k in range(2, 8):
        _within(sum(p.blur == "average" and p.k == k for p in ps), N, 1 / 72, f"average k={k}")
    for k, mass in zip((3, 5, 7, 9, 11), (1, 2, 2, 2, 2)):
        _within(sum(p.blur == "median" and p.k == k for p in ps), N, mass / 108, f"median k={k}")
    assert {p.k for p in ps if p.blur == "median"} == {3, 5, 7, 9, 11}
    mk = [p.k for p in ps if p.blur == "motion"]
    assert set(mk) == set(range(3, 38, 2))
    _within(sum(k == 3 for k in mk), N, 1 / 4 / 34, "motion k=3")
    _within(sum(k == 5 for k in mk), N, 2 / 4 / 34, "motion k=5")
    _within(sum(k == 37 for k in mk), N, 1 / 4 / 34, "motion k=37")
    mo = [p for p in ps if p.blur == "motion"]
    assert all(0 <= p.angle < 360 and -1 <= p.direction <= 1 for p in mo)
    _within(sum(p.angle < 90 for p in mo), len(mo), 1 / 4, "angle quadrant")
    _within(sum(p.direction < 0 for p in mo), len(mo), 1 / 2, "direction sign")
    sg = [p.sigma for p in ps if p.blur == "gaussian"]
    assert all(0 <= s <= 3 for s in sg)
    _within(sum(s < 1 for s in sg), len(sg), 1 / 3, "sigma third")


def _old_draw_image_aug(valid, rng, generator):
    """draw_image_aug as it stood before the corruption: the reference's loop with the corruption skipped."""
    out = []
    for v in valid:
        params = None
        if v and rng.random() > 0.5:
            if rng.choice(["corrput_only", "color_only", "both"]) != "corrput_only":
                params = A.color_jitter_params(generator=generator)
        out.append(params)
    return out


def test_draw_image_aug_keeps_its_draws_with_and_without_corruption():
    valid = [True, True, False, True] * 30
    r0, g0 = random.Random(5), torch.Generator().manual_seed(5)
    r1, g1 = random.Random(5), torch.Generator().manual_seed(5)
    r2, g2 = random.Random(5), torch.Generator().manual_seed(5)
    old = _old_draw_image_aug(valid, r0, g0)
    plain = A.draw_image_aug(valid, rng=r1, generator=g1)
    assert isinstance(plain, list) and plain == old
    crng = np.random.default_rng(8)
    jitter, corrupt = A.draw_image_aug(valid, rng=r2, generator=g2, corrupt_rng=crng)
    assert jitter == old and len(corrupt) == len(valid)
    assert r0.getstate() == r1.getstate() == r2.getstate()
    assert torch.equal(g0.get_state(), g1.get_state()) and torch.equal(g0.get_state(), g2.get_state())
    assert all(c is None for c, v in zip(corrupt, valid) if not v)
    kinds = {(j is not None, c is not None) for j, c in zip(jitter, corrupt)}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}                   # untouched, color_only, corrput_only, both
    # the corruption's draws are corrupt_rng's alone, in frame order
    again = np.random.default_rng(8)
    assert [c for c in corrupt if c is not None] == [A.draw_image_corrupt(again) for c in corrupt if c is not None]
    assert crng.bit_generator.state == again.bit_generator.state


def test_episode_store_plans_differ_only_in_corrupt():
    from tests.test_rdt_data_host import _store
    store = _store()
    kw = dict(cond_mask_prob=0.1, state_noise_snr=40.0, image_aug=True)
    streams = lambda: dict(np_rng=np.random.RandomState(3), rng=random.Random(3), generator=torch.Generator().manual_seed(3))
    sa, sb = streams(), streams()
    a = store.draw(24, **sa, **kw)
    b = store.draw(24, **sb, **kw, image_corrupt=True, corrupt_rng=np.random.default_rng(4))
    fields = [s for s in type(a[0]).__slots__ if s not in ("corrupt", "noise")]
    for p, q in zip(a, b):
        assert all(getattr(p, f) == getattr(q, f) for f in fields) and np.array_equal(p.noise, q.noise)
        assert all(c is None for c in p.corrupt) and len(q.corrupt) == len(q.frame_valid)
        assert all(c is None for c, v in zip(q.corrupt, q.frame_valid) if not v)
    assert sa["rng"].getstate() == sb["rng"].getstate() and torch.equal(sa["generator"].get_state(), sb["generator"].get_state())
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(sa["np_rng"].get_state(), sb["np_rng"].get_state()))
    assert sum(c is not None for q in b for c in q.corrupt) > 0
    store.check_plans(b)
    with pytest.raises(ValueError, match="image_aug"):
        store.draw(1, **streams(), image_corrupt=True, corrupt_rng=np.random.default_rng(4))
    with pytest.raises(ValueError, match="corrupt_rng"):
        store.draw(1, **streams(), image_aug=True, image_corrupt=True)
    bad = next(q for q in b if not all(q.frame_valid))
    bad.corrupt[bad.frame_valid.index(False)] = A.CorruptParams(noise="gaussian", scale=1.0)
    with pytest.raises(ValueError, match="missing"):
        store.check_plans(b)


def test_corrupt_list_checks():
    p = A.CorruptParams(noise="gaussian", scale=1.0)
    assert A.corrupt_list([1, 2], None) is None and A.corrupt_list([1, 2], [None, None]) is None
    assert A.corrupt_list([1, None], [p, None]) == [p, None]
    for frames_, c, what in (([1, 2], [p], "entries"), ([1, None], [None, p], "missing frame"), ([1], [0.5], "CorruptParams")):
        with pytest.raises(ValueError, match=what):
            A.corrupt_list(frames_, c)
    for kw in (dict(noise="salt"), dict(blur="box"), dict(noise="gaussian", scale=-1.0), dict(blur="average", k=8), dict(blur="median", k=4),
               dict(blur="median", k=13), dict(blur="motion", k=39), dict(blur="motion", k=6), dict(blur="motion", k=5, direction=1.5),
               dict(key=1 << 64)):
        with pytest.raises(ValueError):
            A.CorruptParams(**kw)


# ------------------------------------------------------------------------------------------------ 6. records and the C entry point
def full_params():
    return A.CorruptParams(False, "laplace", 4.0, True, 0xFEDCBA9876543210, blur="motion", k=9, angle=30.0, direction=0.2)


def test_record_conversion():
    from vlatouch import _lib
    arr = (_lib.CorruptFrame * 3)()
    ps = [full_params(), None, A.CorruptParams(True, None, blur="median", k=5)]
    words = A.pack_corrupt(arr, ps)
    taps = A.motion_taps(9, 30.0, 0.2)
    assert words.dtype == np.uint32 and words.size == A.THRESHOLDS + taps.size
    f = arr[0]
    assert (f.order, f.noise, f.per_channel, f.key, f.blur, f.k) == (1, 2, 1, 0xFEDCBA9876543210, 4, 9)
    assert (f.noise_off, f.taps_off, f.ntaps, f.tap_sum) == (0, A.THRESHOLDS, len(taps), 1 << 20)
    assert np.array_equal(words[:A.THRESHOLDS], A.noise_table(ps[0])) and np.array_equal(words[A.THRESHOLDS:].view(np.int32).reshape(-1, 3), taps)
    assert (arr[1].noise, arr[1].blur) == (0, 0) and (arr[2].noise, arr[2].blur, arr[2].k, arr[2].order) == (0, 3, 5, 0)
    assert words.size <= A.TABLE_WORDS_MAX


def bad_calls():
    """(what, mutate(record, words) -> words or None) for every argument error of vt_corrupt a single record can carry."""
    def setf(**kw):
        def m(f, words):
            for k, v in kw.items():
                setattr(f, k, v)
        return m

    def tap(i, col, val):
        def m(f, words):
            words = words.copy()
            words.view(np.int32)[f.taps_off + 3 * i + col] = val
            return words
        return m

    def thresholds_decrease(f, words):
        words = words.copy()
        words[f.noise_off + 200] = 0xFFFFFFFF
        assert words[f.noise_off + 201] < 0xFFFFFFFF
        return words
    return [("null source", setf(src=None)), ("zero height", setf(h=0)), ("zero width", setf(w=0)), ("short pitch", setf(pitch=3 * 8 - 1)),
            ("negative out_off", setf(out_off=-1)), ("noise kind", setf(noise=4)), ("noise kind < 0", setf(noise=-1)), ("blur kind", setf(blur=5)),
            ("order", setf(order=2)), ("even k", setf(k=8)), ("k too large", setf(k=39)), ("median k", setf(blur=3, k=13)),
            ("even median k", setf(blur=3, k=4)), ("average k", setf(blur=2, k=8)), ("no taps", setf(ntaps=0)), ("D = 0", setf(tap_sum=0)),
            ("D mismatch", setf(tap_sum=(1 << 20) + 1)), ("taps outside the table", setf(taps_off=1 << 20)),
            ("thresholds outside the table", setf(noise_off=1 << 20)), ("negative offset", setf(taps_off=-3)),
            ("tap beyond the radius", tap(0, 0, 5)), ("tap beyond radius 18", tap(0, 1, -19)), ("zero weight", tap(1, 2, 0)),
            ("decreasing thresholds", thresholds_decrease)]


def good_record(src, h=6, w=8):
    from vlatouch import _lib
    arr = (_lib.CorruptFrame * 1)()
    arr[0].src, arr[0].pitch, arr[0].h, arr[0].w, arr[0].out_off = src, 3 * w, h, w, 0
    return arr, A.pack_corrupt(arr, [full_params()])


def test_entry_point_argument_checks():
    from vlatouch import _lib
    L = _lib.lib()
    fake = C.c_void_p(4096)

    def call(arr, words, n=1, frames_dev=fake, tables_dev=fake, out=fake, nwords=None):
        return L.vt_corrupt(arr, frames_dev, n, words.ctypes.data, tables_dev, words.size if nwords is None else nwords, out, None)
    for what, mutate in bad_calls():
        arr, words = good_record(4096)
        new = mutate(arr[0], words)
        assert call(arr, words if new is None else new) == VT_ERR_ARG, what
        assert L.vt_last_error().startswith(b"vt_corrupt"), what
    arr, words = good_record(4096)
    assert call(arr, words, n=0) == VT_ERR_ARG and call(arr, words, frames_dev=None) == VT_ERR_ARG and call(arr, words, out=None) == VT_ERR_ARG
    assert call(arr, words, tables_dev=None) == VT_ERR_ARG and call(arr, words, nwords=words.size - 1) == VT_ERR_ARG
    assert L.vt_corrupt(None, fake, 1, words.ctypes.data, fake, words.size, fake, None) == VT_ERR_ARG
