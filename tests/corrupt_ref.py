"""The CPU statement of the frame corruption (vlatouch/imgaug.py, csrc/vt_corrupt.hip), numpy only: Philox4x32-10, the threshold lookup,
the periodic reflect-101 and the replicate indices, the integer tap correlation, the median, and `image_corrupt_np`.  The integer
tables (thresholds, taps) are the package's own; tests/test_corrupt_host.py pins them and this arithmetic to scipy.ndimage."""
import numpy as np

from vlatouch import imgaug as A

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key: int) -> np.ndarray:
    """counter: uint64 array [n] (the low 64 bits of the 128-bit counter, the rest zero); key: 64-bit -> uint32 [n, 4]."""
    ctr = np.asarray(counter, dtype=np.uint64)
    c = [ctr & M32, ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)]
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_words(idx, key: int) -> np.ndarray:
    """Word idx & 3 of the counter idx >> 2, per entry of the uint64 array idx."""
    idx = np.asarray(idx, dtype=np.uint64)
    flat = idx.reshape(-1)
    w = philox4x32_10(flat >> np.uint64(2), key)
    return w[np.arange(flat.size), (flat & np.uint64(3)).astype(np.int64)].reshape(idx.shape)


def table_lookup(C: np.ndarray, u: np.ndarray) -> np.ndarray:
    """-255 + #{n : u >= C[n]}."""
    return np.searchsorted(C, u, side="right").astype(np.int64) - 255


def noise_values(C: np.ndarray, key: int, h: int, w: int, per_channel: bool) -> np.ndarray:
    """The integer added to every byte of an h x w frame, int64 [h, w, 3]."""
    pix = (np.arange(h, dtype=np.uint64)[:, None] * np.uint64(w) + np.arange(w, dtype=np.uint64)[None, :])[:, :, None]
    idx = pix * np.uint64(3) + np.arange(3, dtype=np.uint64)[None, None, :] if per_channel else np.broadcast_to(pix, (h, w, 3))
    return table_lookup(C, philox_words(idx, key))


def mirror_index(i: np.ndarray, n: int) -> np.ndarray:
    """reflect-101 continued periodically: period 2 (n - 1); n = 1 reads index 0."""
    if n == 1:
        return np.zeros_like(i)
    P = 2 * (n - 1)
    m = np.mod(i, P)
    return np.where(m < n, m, P - m)


def replicate_index(i: np.ndarray, n: int) -> np.ndarray:
    return np.clip(i, 0, n - 1)


def tap_sums(frame: np.ndarray, taps: np.ndarray):
    """-> (S int64 [h, w, 3], D): S = sum of W * p over the taps (dy, dx, W), mirror border."""
    h, w = frame.shape[:2]
    a = frame.astype(np.int64)
    S = np.zeros(a.shape, dtype=np.int64)
    ys, xs = np.arange(h), np.arange(w)
    for dy, dx, W in taps.tolist():
        S += W * a[mirror_index(ys + dy, h)][:, mirror_index(xs + dx, w)]
    return S, int(taps[:, 2].sum())


def tap_correlate(frame: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """q, r = divmod(S, D); out = q + (2 r > D or (2 r == D and q odd))."""
    S, D = tap_sums(frame, taps)
    q, r = np.divmod(S, D)
    return (q + ((2 * r > D) | ((2 * r == D) & (q % 2 == 1)))).astype(np.uint8)


def median_np(frame: np.ndarray, k: int) -> np.ndarray:
    """Per channel the median of the k x k window (k odd), replicate border."""
    h, w = frame.shape[:2]
    r = k // 2
    ys, xs = np.arange(h), np.arange(w)
    win = np.stack([frame[replicate_index(ys + dy, h)][:, replicate_index(xs + dx, w)] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    return np.partition(win, k * k // 2, axis=0)[k * k // 2]


def add_noise(frame: np.ndarray, params) -> np.ndarray:
    C = A.noise_table(params)
    e = noise_values(C, params.key, frame.shape[0], frame.shape[1], params.per_channel)
    return np.clip(frame.astype(np.int64) + e, 0, 255).astype(np.uint8)


def blur(frame: np.ndarray, params) -> np.ndarray:
    kind, k, taps = params.taps()
    if kind == 0:
        return frame
    return median_np(frame, k) if taps is None else tap_correlate(frame, taps)


def image_corrupt_np(frame: np.ndarray, params) -> np.ndarray:
    """uint8 [H, W, 3] -> the corrupted frame; params None = the frame as it is."""
    a = np.ascontiguousarray(frame)
    if params is None:
        return a
    for step in ((0, 1) if params.noise_first else (1, 0)):
        if step == 0 and params.noise is not None:
            a = add_noise(a, params)
        elif step == 1:
            a = blur(a, params)
    return a
