"""The block-wise 8-bit AdamW statement of DESIGN.md §8 in numpy: what csrc/vt_adam8.hip and vlatouch/adam8.py are held against.

Tables in fp64, rounded once to fp32; boundaries the fp32-rounded fp64 midpoints; the code of x = the number of boundaries strictly below x
(nearest value, ties to the lower index).  The step is fp32, one rounding per operation in the order of csrc/vt_optim.h (numpy does
not contract).  `step8(..., dtype=np.float64)` evaluates the same step from the same codes in fp64: the yardstick of the tolerances.
Written on its own: nothing here imports the product."""
import numpy as np

BLOCK, MIN_8BIT_SIZE = 256, 4096
F = np.float32


def tables():
    """(T_s, T_u) float32 [256]: decade i = 0 .. 6, midpoints of n_i equal sub-intervals of [0.1, 1] times 10^(i-6); n_i = 2^i signed (with the
    negatives), 2^(i+1) unsigned; plus 0 and 1."""
    out = []
    for first in (1, 2):
        vals = [0.0, 1.0]
        for i in range(7):
            n = first * 2 ** i
            for k in range(n):
                vals.append((0.1 + 0.9 * (k + 0.5) / n) * 10.0 ** (i - 6))
        if first == 1:
            vals += [-x for x in vals if 0.0 < x < 1.0]
        out.append(np.array(sorted(vals), dtype=np.float64).astype(F))
    return out[0], out[1]


def bounds(t):
    t = t.astype(np.float64)
    return ((t[:-1] + t[1:]) / 2).astype(F)


TS, TU = tables()
BS, BU = bounds(TS), bounds(TU)


def code(x, b):
    """number of boundaries strictly below x"""
    return np.searchsorted(b, x, side="left").astype(np.uint8)


def nblocks(n):
    return (n + BLOCK - 1) // BLOCK


def _blocks(x, fill=0.0):
    """[n] -> [nblocks, 256], the partial last block padded with `fill`."""
    n = x.size
    out = np.full(nblocks(n) * BLOCK, fill, dtype=x.dtype)
    out[:n] = x
    return out.reshape(-1, BLOCK)


def quantize(x, signed):
    """fp32 [n] -> (codes uint8 [n], absmax fp32 [nblocks], ratio fp32 [n] = x / absmax of its block, 0 where absmax is 0)."""
    x = x.astype(F)
    xb = _blocks(x)
    amax = (np.abs(xb) if signed else np.maximum(xb, F(0))).max(axis=1).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (xb / amax[:, None]).astype(F)
    zero = amax == 0
    r[zero] = 0
    c = code(r, BS if signed else BU)
    c[zero] = 127 if signed else 0
    return c.reshape(-1)[:x.size], amax, r.reshape(-1)[:x.size]


def dequantize(codes, absmax, signed, dtype=F):
    t = (TS if signed else TU).astype(dtype)
    return (t[codes] * np.repeat(absmax.astype(dtype), BLOCK)[:codes.size]).astype(dtype)


def hyper(lr, b1, b2, step, ema_decay):
    """[lr, 1 - b1^t, sqrt(1 - b2^t), 1 - decay] in fp32 (vt_train_hyper; a GPU test takes the library's own four floats instead)."""
    return np.array([lr, 1.0 - float(F(b1)) ** step, np.sqrt(1.0 - float(F(b2)) ** step), 1.0 - ema_decay], dtype=F)


def adamw_elem(p, g, m, v, hy, b1, b2, eps, wd, dtype=F):
    """csrc/vt_optim.h's adamw_elem, operation by operation -> (p', m', v')."""
    c = lambda s: dtype(F(s))                                  # the kernel's scalars are fp32 values in either evaluation
    lr, bc1, bc2s = c(hy[0]), c(hy[1]), c(hy[2])
    b1, b2, eps, wd, one = c(b1), c(b2), c(eps), c(wd), dtype(1)
    p, g, m, v = (a.astype(dtype) for a in (p, g, m, v))
    pv = p * (one - lr * wd)
    mv = b1 * m + (one - b1) * g
    vv = b2 * v + (one - b2) * g * g
    denom = np.sqrt(vv) / bc2s + eps
    return pv - (lr / bc1) * (mv / denom), mv, vv


def ema_elem(sh, p, hy, dtype=F):
    return sh.astype(dtype) - dtype(F(hy[3])) * (sh.astype(dtype) - p.astype(dtype))


def zero_state(n):
    if n < MIN_8BIT_SIZE:
        return {"m": np.zeros(n, F), "v": np.zeros(n, F)}
    return {"m8": np.full(n, 127, np.uint8), "v8": np.zeros(n, np.uint8), "am": np.zeros(nblocks(n), F), "av": np.zeros(nblocks(n), F)}


def moments(state, dtype=F):
    if "m" in state:
        return state["m"].astype(dtype), state["v"].astype(dtype)
    return dequantize(state["m8"], state["am"], True, dtype), dequantize(state["v8"], state["av"], False, dtype)


def step8(p, g, state, shadow, hy, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, dtype=F):
    """One step of one tensor -> (p', shadow' | None, state', info).  dtype=np.float64: the same step from the same codes in fp64 (state' and
    info are then not meant to be used).  info: the ratios m' / am', v' / av' the codes were taken from."""
    m_old, v_old = moments(state, dtype)
    pn, mn, vn = adamw_elem(p, g, m_old, v_old, hy, b1, b2, eps, wd, dtype)
    sn = None if shadow is None else ema_elem(shadow, pn, hy, dtype)
    if "m" in state:
        return pn, sn, {"m": mn, "v": vn}, {}
    m8, am, rm = quantize(mn.astype(F), True)
    v8, av, rv = quantize(vn.astype(F), False)
    return pn, sn, {"m8": m8, "v8": v8, "am": am, "av": av}, {"rm": rm, "rv": rv}


def near_boundary(r, b, rel=2.0 ** -20):
    """mask of the ratios within `rel` relative of a decision boundary, and the other code such an element may take."""
    j = np.searchsorted(b, r, side="left")
    lo, hi = b[np.clip(j - 1, 0, b.size - 1)], b[np.clip(j, 0, b.size - 1)]
    near_lo = (j > 0) & (np.abs(r - lo) <= rel * np.abs(lo))
    near_hi = (j < b.size) & (np.abs(hi - r) <= rel * np.abs(hi))
    other = np.where(near_lo, j - 1, np.where(near_hi, j + 1, j))
    return near_lo | near_hi, other.astype(np.int64)


def code_step(codes, table):
    """the larger gap between a code's table value and its neighbours: one code step"""
    t = table.astype(np.float64)
    gap = np.diff(t)
    up = np.concatenate([gap, gap[-1:]])
    dn = np.concatenate([gap[:1], gap])
    return np.maximum(up, dn)[codes]
