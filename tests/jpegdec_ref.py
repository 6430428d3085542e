"""A baseline JPEG decoder in plain Python / numpy: the CPU statement csrc/vt_jpegdec.hip and vlatouch/jpegdec.py are checked against, itself
bit-equal to Pillow's libjpeg-turbo (tests/test_jpegdec_host.py).  Marker parse, byte un-stuffing (a loop per byte: nothing shared with the
vectorised one under test), Huffman decoding, entries; the inverse DCT, the up-sampling and the colour arithmetic are tests/jpeg_ref.py's,
imported, not restated.

An ENTRY is (bit offset in the un-stuffed stream, the three DC predictors) before an MCU: `decode(b, interval=k)` decodes every group of k
MCUs from its entry alone, as one lane of the device decoder does, `decode(b)` sequentially."""
from __future__ import annotations

import functools
import struct

import numpy as np

from tests import jpeg_ref as J

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43,
      36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def parse(b: bytes) -> dict:
    """-> {h, w, comps [(id, hs, vs, tq)], qt {id: int64 [8, 8] natural}, ht {(class, id): (len16, sym16)}, dri, sel {comp id: (td, ta)},
    start: the first entropy byte}."""
    assert b[:2] == b"\xff\xd8"
    i, qt, ht, sof, dri = 2, {}, {}, None, 0
    while True:
        assert b[i] == 0xFF, i
        m, n = b[i + 1], struct.unpack(">H", b[i + 2:i + 4])[0]
        seg = b[i + 4:i + 2 + n]
        if m == 0xDB:
            for k in range(0, len(seg), 65):
                assert seg[k] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZZ] = list(seg[k + 1:k + 65])
                qt[seg[k] & 15] = t.reshape(8, 8)
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                cnt = list(seg[k + 1:k + 17])
                vals = list(seg[k + 17:k + 17 + sum(cnt)])
                ht[seg[k] >> 4, seg[k] & 15] = _lut16(tuple(cnt), tuple(vals))
                k += 17 + sum(cnt)
        elif m == 0xC0:
            h, w = struct.unpack(">HH", seg[1:5])
            sof = (h, w, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
        elif m == 0xDD:
            dri = struct.unpack(">H", seg[:2])[0]
        elif m == 0xDA:
            sel = {seg[1 + 2 * c]: (seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])}
            return {"h": sof[0], "w": sof[1], "comps": sof[2], "qt": qt, "ht": ht, "dri": dri, "sel": sel, "start": i + 2 + n}
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, f"marker FF{m:02X} is outside this statement"
        i += 2 + n


@functools.lru_cache(maxsize=64)
def _lut16(cnt, vals):
    """The canonical code of a DHT table as two lists indexed by the next 16 bits: code length (0: undefined) and symbol."""
    ln, sy = [0] * 65536, [0] * 65536
    code = p = 0
    for l in range(1, 17):
        for _ in range(cnt[l - 1]):
            lo, span = code << (16 - l), 1 << (16 - l)
            ln[lo:lo + span] = [l] * span
            sy[lo:lo + span] = [vals[p]] * span
            p += 1
            code += 1
        code <<= 1
    return ln, sy


def unstuff(b: bytes, start: int):
    """-> (the entropy bytes without stuffing and RSTn markers, the byte at which each restart interval after the first starts)."""
    out, rst, i = bytearray(), [], start
    while True:
        c = b[i]
        if c == 0xFF:
            n = b[i + 1]
            if n == 0:
                out.append(0xFF)
            elif 0xD0 <= n <= 0xD7:
                rst.append(len(out))
            else:
                assert n == 0xD9, f"marker FF{n:02X} in the scan"
                return bytes(out), rst
            i += 2
        else:
            out.append(c)
            i += 1


class Bits:
    """w[pos] = the 16 bits from bit `pos` on; past the end 1-bits, as libjpeg pads."""

    def __init__(self, data: bytes):
        bits = np.unpackbits(np.frombuffer(data + b"\xff" * 8, np.uint8)).astype(np.int64)
        self.w = (np.lib.stride_tricks.sliding_window_view(bits, 16) @ (1 << np.arange(15, -1, -1))).tolist()
        self.nbits = 8 * len(data)


def _extend(v: int, s: int) -> int:
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def _block(w, pos, dc, ac, pred):
    """One block from bit `pos` -> (64 coefficients in natural order, pos, pred)."""
    c = [0] * 64
    e = w[pos]
    l, s = dc[0][e], dc[1][e]
    assert l, "undefined DC code"
    pos += l
    pred += _extend(w[pos] >> (16 - s), s) if s else 0
    pos += s
    c[0] = pred
    k = 1
    while k < 64:
        e = w[pos]
        l, rs = ac[0][e], ac[1][e]
        assert l, "undefined AC code"
        pos += l
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        assert k < 64, "run past coefficient 63"
        c[ZZ[k]] = _extend(w[pos] >> (16 - s), s)
        pos += s
        k += 1
    return c, pos, pred


def geometry(p: dict):
    hmax, vmax = max(c[1] for c in p["comps"]), max(c[2] for c in p["comps"])
    mw, mh = -(-p["w"] // (8 * hmax)), -(-p["h"] // (8 * vmax))
    return hmax, vmax, mw, mh


def _mcus(p, bits, rst, planes, m0, m1, pos, pred, entries=None, interval=None):
    """MCUs [m0, m1) from (pos, pred) into planes; a restart boundary behind m0 re-seeds.  Records entries when asked."""
    _, _, mw, _ = geometry(p)
    pred = list(pred)
    for m in range(m0, m1):
        if p["dri"] and m > m0 and m % p["dri"] == 0:
            pos, pred = 8 * rst[m // p["dri"] - 1], [0, 0, 0]
        if entries is not None and m % interval == 0:
            entries.append((pos, tuple(pred)))
        my, mx = divmod(m, mw)
        for ci, (cid, hs, vs, _) in enumerate(p["comps"]):
            td, ta = p["sel"][cid]
            for by in range(vs):
                for bx in range(hs):
                    c, pos, pred[ci] = _block(bits.w, pos, p["ht"][0, td], p["ht"][1, ta], pred[ci])
                    planes[ci][my * vs + by, mx * hs + bx] = np.asarray(c).reshape(8, 8)
    assert pos <= bits.nbits, "the stream ends before the last MCU"
    return pos, pred


def entries(b: bytes, interval: int):
    """The entry before every MCU that is a multiple of `interval`, from one sequential pass (restart boundaries re-seed)."""
    p = parse(b)
    data, rst = unstuff(b, p["start"])
    _, _, mw, mh = geometry(p)
    out = []
    _mcus(p, Bits(data), rst, _planes(p), 0, mw * mh, 0, (0, 0, 0), out, interval)
    return out


def _planes(p):
    _, _, mw, mh = geometry(p)
    return [np.zeros((mh * vs, mw * hs, 8, 8), np.int64) for _, hs, vs, _ in p["comps"]]


def coefficients(b: bytes, interval=None):
    """Per component the quantised coefficients [block rows, block columns, 8, 8]; interval: every group of that many MCUs from its entry alone."""
    p = parse(b)
    data, rst = unstuff(b, p["start"])
    _, _, mw, mh = geometry(p)
    bits, planes = Bits(data), _planes(p)
    if interval is None:
        _mcus(p, bits, rst, planes, 0, mw * mh, 0, (0, 0, 0))
    else:
        for e, (pos, pred) in enumerate(entries(b, interval)):
            _mcus(p, bits, rst, planes, e * interval, min((e + 1) * interval, mw * mh), pos, pred)
    return p, planes


def decode(b: bytes, interval=None) -> np.ndarray:
    """The file -> uint8 [h, w, 3] RGB, as libjpeg's default decompress (islow, fancy up-sampling)."""
    p, planes = coefficients(b, interval)
    h, w = p["h"], p["w"]
    hmax, vmax, _, _ = geometry(p)
    dec = []
    for (_, _, _, tq), c in zip(p["comps"], planes):
        x = c * p["qt"][tq]
        y = J._idct_pass(x.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)          # columns
        y = np.clip(J._idct_pass(y, 18) + 128, 0, 255)                               # rows
        dec.append(y.transpose(0, 2, 1, 3).reshape(8 * c.shape[0], 8 * c.shape[1]))
    Y = dec[0][:h, :w]
    if (hmax, vmax) == (2, 2):
        ch, cw = (h + 1) // 2, (w + 1) // 2
        Cb, Cr = (J._upsample(d[:ch, :cw])[:h, :w] for d in dec[1:])
    else:
        assert (hmax, vmax) == (1, 1)
        Cb, Cr = dec[1][:h, :w], dec[2][:h, :w]
    x, y = Cr - 128, Cb - 128
    out = np.stack([Y + ((91881 * x + J.H) >> 16), Y + ((-22554 * y + J.H - 46802 * x) >> 16), Y + ((116130 * y + J.H) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


# how the test streams are written: Pillow's save() keywords per mode
MODES = {"default": {}, "optimize": {"optimize": True}, "444": {"subsampling": 0}, "restart": {"restart_marker_blocks": 3},
         "restart_rows": {"restart_marker_rows": 1}}


def encode(img: np.ndarray, quality: int, mode: str = "default") -> bytes:
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **MODES[mode])
    return buf.getvalue()


def pillow_decode(b: bytes) -> np.ndarray:
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


# ---- the device decoder's own tables and bit reader, walked on the CPU: what csrc/vt_jpegdec.hip does with a table set of vlatouch.jpegdec
class DeviceWalk:
    """rec: a vlatouch.jpegdec.JpegRecord.  The 64-bit register buffer refilled by big-endian words below the padded length (1-bits past it),
    the 9-bit look-ahead table with the maxcode / valoff walk for longer codes, the extra bits taken from the same buffer."""

    def __init__(self, rec):
        from vlatouch import jpegdec as D
        self.D, self.rec = D, rec
        self.ts = np.frombuffer(rec.tableset, np.uint8)
        self.len = len(rec.data)
        self.plen = (self.len + 3) // 4 * 4
        self.s = bytes(rec.data) + b"\xff" * (self.plen - self.len)
        self.sel = self.ts[D.TS_SEL:D.TS_SEL + 32].view(np.int32).tolist()
        self.zz = self.ts[D.TS_ZZ:D.TS_ZZ + 64].tolist()
        self.huff = []
        for t in range(4):
            o = D.TS_HUFF + t * D.HUFF_BYTES
            self.huff.append((self.ts[o:o + 1024].view(np.uint16).tolist(), self.ts[o + D.HUFF_MAX:o + D.HUFF_MAX + 68].view(np.int32).tolist(),
                              self.ts[o + D.HUFF_OFF:o + D.HUFF_OFF + 68].view(np.int32).tolist(), self.ts[o + D.HUFF_VAL:o + D.HUFF_VAL + 256].tolist()))

    M64 = (1 << 64) - 1

    def _word(self):
        w = int.from_bytes(self.s[self.wpos:self.wpos + 4], "big") if self.wpos < self.plen else 0xFFFFFFFF
        self.wpos += 4
        return w

    def init(self, bitpos):
        self.wpos = (bitpos >> 5) << 2
        self.buf = self._word() << 32
        k = bitpos & 31
        self.buf, self.cnt = (self.buf << k) & self.M64, 32 - k

    def refill(self):
        if self.cnt <= 32:
            self.buf |= self._word() << (32 - self.cnt)
            self.cnt += 32

    def skip(self, n):
        self.buf, self.cnt = (self.buf << n) & self.M64, self.cnt - n

    def consumed(self):
        return self.wpos * 8 - self.cnt

    def symbol(self, t):
        lut, maxcode, valoff, vals = self.huff[t]
        e = lut[self.buf >> 55]
        if e >> 8:
            return e & 255, e >> 8
        for l in range(10, 17):
            code = self.buf >> (64 - l)
            if code <= maxcode[l]:
                return vals[(code + valoff[l]) & 255], l
        return 0, 0

    def extra(self, l, s):
        v = ((self.buf << l) & self.M64) >> (64 - s)
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v

    def block(self, dc, ac, pred):
        """-> (ok, pred, coefficients in natural order)"""
        c = [0] * 64
        self.refill()
        s, l = self.symbol(dc)
        if l == 0 or s > 15:
            return False, pred, c
        if s:
            pred += self.extra(l, s)
        self.skip(l + s)
        c[0] = pred
        k = 1
        while k < 64:
            self.refill()
            rs, l = self.symbol(ac)
            if l == 0:
                return False, pred, c
            s = rs & 15
            if s == 0:
                self.skip(l)
                if rs >> 4 != 15:
                    break
                k += 16
                continue
            k += rs >> 4
            if k > 63:
                return False, pred, c
            c[self.zz[k]] = self.extra(l, s)
            self.skip(l + s)
            k += 1
        return True, pred, c

    def walk(self, m0, m1, pred, interval, store, out_entries=None):
        """walk_mcus of the kernels -> (bad, coefficient blocks in stream order)"""
        rec, pred, bad, blocks = self.rec, list(pred), False, []
        ri, s420 = rec.restart_interval, rec.sampling == self.D.S420
        for m in range(m0, m1):
            if store and ri and m > m0 and m % ri == 0:
                self.init(int(rec.restart_starts[m // ri]) << 3)
                pred = [0, 0, 0]
            if not store and m % interval == 0:
                out_entries[m // interval] = (self.consumed(), *pred)
            for k in range(6 if s420 else 3):
                c = (0 if k < 4 else k - 3) if s420 else k
                blk = [0] * 64
                if not bad:
                    ok, pred[c], blk = self.block(self.sel[c], 2 + self.sel[3 + c], pred[c])
                    bad = not ok or self.consumed() > 8 * self.len
                    if bad:
                        blk = [0] * 64
                blocks.append(blk)
        return bad, blocks

    def index(self, interval):
        """vt_jpeg_index -> (status, entries)"""
        rec = self.rec
        ent, status, ri = [None] * -(-rec.mcus // interval), 0, rec.restart_interval
        for r in range(-(-rec.mcus // ri) if ri else 1):
            m0 = r * ri if ri else 0
            self.init(int(rec.restart_starts[r]) << 3)
            status |= self.walk(m0, min(m0 + ri, rec.mcus) if ri else rec.mcus, (0, 0, 0), interval, False, ent)[0]
        return int(status), ent

    def coefficients(self, interval):
        """The entropy launch: every entry's lane on its own -> (status, [blocks in stream order][64])"""
        status, ent = self.index(interval)
        blocks = []
        for e, (pos, *pred) in enumerate(ent):
            self.init(pos)
            bad, b = self.walk(e * interval, min((e + 1) * interval, self.rec.mcus), pred, interval, True)
            status |= bad
            blocks += b
        return int(status), blocks


def stream_order_blocks(p: dict, planes) -> list:
    """`coefficients`' planes as the blocks of the scan, in stream order, each 64 values in natural order."""
    _, _, mw, mh = geometry(p)
    out = []
    for m in range(mw * mh):
        my, mx = divmod(m, mw)
        for ci, (_, hs, vs, _) in enumerate(p["comps"]):
            for by in range(vs):
                for bx in range(hs):
                    out.append(planes[ci][my * vs + by, mx * hs + bx].reshape(-1).tolist())
    return out


# ---- a synthetic recording folder (the layout vlatouch.convert reads) for the store tests
def write_recording(ep_dir, n: int, seed: int, cameras=("camera1", "camera2"), hw=(48, 64), quality: int = 95, lang=(3, 8)) -> None:
    """`ep_dir`/{ee_poses.npy, gripper_pos.npy, instruct.pt, <camera>/rgb_<i>.jpg}: n steps that move from step 3 on; every frame a smooth
    image plus a little noise, another one per step."""
    import os
    import torch
    from PIL import Image
    g = np.random.RandomState(seed)
    os.makedirs(ep_dir, exist_ok=True)
    pos, quat = np.cumsum(g.normal(scale=0.02, size=(n, 3)), axis=0), g.normal(size=(n, 4))
    pos[:3], quat[:3] = pos[0], quat[0]
    np.save(os.path.join(ep_dir, "ee_poses.npy"), np.concatenate([pos, quat], axis=1))
    np.save(os.path.join(ep_dir, "gripper_pos.npy"), g.uniform(0, 255, n))
    torch.save(torch.from_numpy(g.normal(size=(1,) + tuple(lang)).astype(np.float32)), os.path.join(ep_dir, "instruct.pt"))
    h, w = hw
    y, x = np.mgrid[0:h, 0:w]
    for c, cam in enumerate(cameras):
        os.makedirs(os.path.join(ep_dir, cam), exist_ok=True)
        for i in range(n):
            smooth = np.stack([128 + 100 * np.sin((x + 3 * i) / 9.0 + c), 128 + 100 * np.cos((y - 2 * i) / 7.0), (2 * x + 3 * y + 5 * i) % 256], axis=-1)
            img = np.clip(smooth + g.normal(scale=2.0, size=(h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(ep_dir, cam, f"rgb_{i}.jpg"), quality=quality)
