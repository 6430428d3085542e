"""Baseline JPEG files decoded on the device, so that camera frames can stay in HBM as the bitstreams they were recorded as.

  * `parse_jpeg(data)`: the host half of one file: the markers, the tables, and the entropy bytes with `FF 00` un-stuffed and the RSTn
    markers removed.  What is not built is refused here, by name.
  * `JpegFrames(list_of_bytes, device)`: parses, uploads one blob (streams, table sets, restart starts, entries) and runs vt_jpeg_index once;
    `.decode(indices)` is one vt_jpeg_decode call (csrc/vt_jpegdec.hip), `.nbytes` what stays resident.
  * `decode_jpeg_device(list_of_bytes)`: the one-shot convenience; `decode_many` decodes frames of several `JpegFrames` in one call
    (what `EpisodeStore(frames="jpeg")` does per micro-batch).

The pixels are those of libjpeg's default decompress (islow inverse DCT, fancy up-sampling), pinned bit for bit to Pillow's libjpeg-turbo
(`np.asarray(Image.open(f).convert("RGB"))`).  Built: SOF0, 8 bit, three components YCbCr, 4:2:0 (2x2,1x1,1x1) or 4:4:4, one interleaved
scan, DRI / RSTn.  Not built: progressive, extended, lossless and arithmetic frames, 4:2:2, grayscale, CMYK.  cv2's decoder is not a referee
here (UNPINNED, as in vlatouch/jpegmap.py): Pillow is.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

MAX_SIDE = 32768
S444, S420 = _lib.JPEG_444, _lib.JPEG_420
SAMPLING_NAMES = {S444: "4:4:4", S420: "4:2:0"}
# zig-zag position -> natural (row-major) order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
                   56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.uint8)
# byte offsets inside a table set (csrc/vt_jpegdec.hip)
TS_SEL, TS_Q, TS_HUFF, HUFF_BYTES, HUFF_MAX, HUFF_OFF, HUFF_VAL, LUT_BITS = 0, 32, 416, 1416, 1024, 1092, 1160, 9
TS_ZZ = TS_HUFF + 4 * HUFF_BYTES
assert TS_ZZ + 64 == _lib.JPEG_TABLESET_BYTES
# columns of a table row (include/vlatouch.h)
C_STREAM, C_LEN, C_H, C_W, C_SAMP, C_TSET, C_ENTRIES, C_INTERVAL, C_RI, C_RST, C_OUT_OFF = range(11)
# MCUs per entry when none is asked for: profiles/jpeg_store_bench.json, the table of DESIGN.md section 6
DEFAULT_INDEX_INTERVAL = 4

_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
              0xC7: "differential lossless", 0xC9: "arithmetic sequential", 0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless",
              0xCD: "arithmetic differential sequential", 0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}


class JpegRecord:
    """One parsed file.  h, w; sampling (S444 / S420); qt uint16 [3, 64]: the quantisation table of each component, natural order; huff
    {(class, id): (counts [16], values)}; dc_sel / ac_sel: the table id of each component; restart_interval in MCUs (0: none); data uint8:
    the un-stuffed entropy bytes (None after a header-only parse); restart_starts int32: the byte of `data` at which each restart interval
    starts ([0] = 0); tableset: the device form of the tables (bytes)."""
    __slots__ = ("h", "w", "sampling", "qt", "huff", "dc_sel", "ac_sel", "restart_interval", "data", "restart_starts", "tableset")

    @property
    def mcu_cols(self) -> int:
        side = 16 if self.sampling == S420 else 8
        return -(-self.w // side)

    @property
    def mcus(self) -> int:
        side = 16 if self.sampling == S420 else 8
        return self.mcu_cols * -(-self.h // side)


def huffman_tables(counts, values):
    """jdhuff.c's derived tables of one DHT table -> (lut uint16 [512] = length << 8 | symbol by the next 9 bits, 0 where the code is longer
    or undefined; maxcode int32 [17], -1 for a length without codes; valoff int32 [17] = valptr - mincode).  None for an over-full table."""
    lut, maxcode, valoff = np.zeros(1 << LUT_BITS, np.uint16), np.full(17, -1, np.int32), np.zeros(17, np.int32)
    code = p = 0
    for l in range(1, 17):
        n = int(counts[l - 1])
        valoff[l] = p - code
        if n:
            if code + n > (1 << l):
                return None
            if l <= LUT_BITS:
                for k in range(n):
                    lo = (code + k) << (LUT_BITS - l)
                    lut[lo:lo + (1 << (LUT_BITS - l))] = (l << 8) | int(values[p + k])
            code += n
            p += n
            maxcode[l] = code - 1
        code <<= 1
    return lut, maxcode, valoff


def _tableset(rec: JpegRecord) -> bytes:
    ts = np.zeros(_lib.JPEG_TABLESET_BYTES, np.uint8)
    ts[TS_SEL:TS_SEL + 32].view(np.int32)[:6] = list(rec.dc_sel) + list(rec.ac_sel)
    ts[TS_Q:TS_Q + 384].view(np.uint16)[:] = rec.qt.reshape(-1)
    for cls in (0, 1):
        for tid in (0, 1):
            o = TS_HUFF + (2 * cls + tid) * HUFF_BYTES
            ts[o + HUFF_MAX:o + HUFF_MAX + 68].view(np.int32)[:] = -1          # an absent table defines no code
            if (cls, tid) in rec.huff:
                counts, values = rec.huff[cls, tid]
                lut, maxcode, valoff = huffman_tables(counts, values)
                ts[o:o + 1024].view(np.uint16)[:] = lut
                ts[o + HUFF_MAX:o + HUFF_MAX + 68].view(np.int32)[:] = maxcode
                ts[o + HUFF_OFF:o + HUFF_OFF + 68].view(np.int32)[:] = valoff
                ts[o + HUFF_VAL:o + HUFF_VAL + len(values)] = values
    ts[TS_ZZ:TS_ZZ + 64] = ZIGZAG
    return ts.tobytes()


def parse_jpeg(data, index: Optional[int] = None, header_only: bool = False) -> JpegRecord:
    """The markers of one file: SOI, APPn / COM (skipped), DQT, SOF0, DHT, DRI, one interleaved SOS, EOI -> a `JpegRecord`.  `index`: the
    file's index, for the messages.  header_only: stop at the scan (sizes and tables, no entropy bytes).  Raises ValueError, by name, on
    everything that is not built."""
    who = "JPEG" if index is None else f"JPEG frame {index}"

    def refuse(msg):
        raise ValueError(f"{who}: {msg}")

    b = bytes(data)
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        refuse("no SOI marker: not a JPEG file")
    qts, huff, sof, ri, i, adobe = {}, {}, None, 0, 2, 1
    while True:
        if i + 4 > n:
            refuse("truncated: the file ends before its scan")
        if b[i] != 0xFF:
            refuse(f"no marker at byte {i}")
        m = b[i + 1]
        if m == 0xFF:                       # fill byte before a marker
            i += 1
            continue
        if m == 0xD9:
            refuse("EOI before any scan")
        seg_len = (b[i + 2] << 8) | b[i + 3]
        if seg_len < 2 or i + 2 + seg_len > n:
            refuse(f"bad segment length: the {seg_len} bytes of marker FF{m:02X} at byte {i} run past the file")
        seg = b[i + 4:i + 2 + seg_len]
        if m == 0xDB:
            k = 0
            while k < len(seg):
                if seg[k] >> 4:
                    refuse("16-bit DQT (12-bit data) is not built")
                if k + 65 > len(seg) or (seg[k] & 15) > 3:
                    refuse("malformed DQT")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg, np.uint8, 64, k + 1)
                if not t.all():
                    refuse("DQT with a zero entry")
                qts[seg[k] & 15] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                cls, tid = seg[k] >> 4, seg[k] & 15
                counts = np.frombuffer(seg, np.uint8, 16, k + 1) if k + 17 <= len(seg) else None
                nv = 0 if counts is None else int(counts.sum())
                if counts is None or cls > 1 or tid > 1 or nv > 256 or k + 17 + nv > len(seg):
                    refuse("malformed DHT (baseline: classes 0..1, ids 0..1)")
                values = np.frombuffer(seg, np.uint8, nv, k + 17)
                if huffman_tables(counts, values) is None:
                    refuse("malformed DHT: more codes than a length holds")
                huff[cls, tid] = (counts.copy(), values.copy())
                k += 17 + nv
        elif m == 0xC0:
            if sof is not None:
                refuse("two SOF markers")
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                refuse("malformed SOF0")
            if seg[0] != 8:
                refuse(f"{seg[0]}-bit precision is not built (12- or 16-bit data)")
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc == 1:
                refuse("grayscale (1 component) is not built")
            if nc == 4:
                refuse("CMYK (4 components) is not built")
            if nc != 3:
                refuse(f"{nc} components")
            if h < 1 or w < 1:
                refuse(f"a zero size ({h} x {w})")
            if h > MAX_SIDE or w > MAX_SIDE:
                refuse(f"{h} x {w} is too large: a side above {MAX_SIDE}")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)]
            fac = [(ch, cv) for _, ch, cv, _ in comps]
            if fac == [(2, 2), (1, 1), (1, 1)]:
                samp = S420
            elif fac == [(1, 1), (1, 1), (1, 1)]:
                samp = S444
            else:
                refuse("sampling " + ",".join(f"{a}x{c}" for a, c in fac) + " is not built (only 2x2,1x1,1x1 and 1x1,1x1,1x1)")
            sof = (h, w, samp, comps)
        elif m in _SOF_NAMES:
            refuse(f"{_SOF_NAMES[m]} frame (SOF{m - 0xC0}) is not built: baseline SOF0 only")
        elif m == 0xDD:
            if len(seg) < 2:
                refuse("malformed DRI")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]                 # judged behind the frame header, which names grayscale and CMYK
        elif m == 0xDA:
            break
        i += 2 + seg_len
    if sof is None:
        refuse("SOS before SOF0")
    h, w, samp, comps = sof
    if adobe != 1:
        refuse(f"Adobe APP14 transform {adobe}: the components are not YCbCr")
    if len(seg) < 1 or seg[0] != 3 or len(seg) != 10:
        refuse("more than one scan: a scan that does not interleave all three components")
    if (seg[7], seg[8], seg[9]) != (0, 63, 0):
        refuse("a scan of part of the spectrum: more than one scan (progressive)")
    rec = JpegRecord()
    rec.h, rec.w, rec.sampling, rec.restart_interval = h, w, samp, ri
    rec.dc_sel, rec.ac_sel, qt = [], [], []
    for c, (cid, _, _, tq) in enumerate(comps):
        if seg[1 + 2 * c] != cid:
            refuse("the scan's components are not in the frame's order")
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if (0, td) not in huff or (1, ta) not in huff:
            refuse(f"component {c} selects a Huffman table that no DHT defines")
        if tq not in qts:
            refuse(f"component {c} selects a quantisation table that no DQT defines")
        rec.dc_sel.append(td)
        rec.ac_sel.append(ta)
        qt.append(qts[tq])
    rec.qt, rec.huff = np.stack(qt), huff
    rec.tableset = _tableset(rec)
    rec.data = rec.restart_starts = None
    if header_only:
        return rec

    # the entropy bytes: every FF is followed by 00 (a stuffed FF), RSTn, or the marker that ends the scan
    a = np.frombuffer(b, np.uint8, offset=i + 2 + seg_len)
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) else np.zeros(0, np.int64)
    nxt = a[ff + 1]
    stuffed, rst = nxt == 0, (nxt & 0xF8) == 0xD0
    ends = np.flatnonzero(~(stuffed | rst))
    if len(ends) == 0:
        refuse("missing EOI: the file ends inside its scan (truncated)")
    e = int(ends[0])
    end, marker = int(ff[e]), int(nxt[e])
    if marker != 0xD9:
        refuse(f"more than one scan: marker FF{marker:02X} follows the first scan" if marker in (0xDA, 0xC4, 0xDB, 0xDD)
               else f"marker FF{marker:02X} inside the scan")
    ff, stuffed, rst, nxt = ff[:e], stuffed[:e], rst[:e], nxt[:e]
    keep = np.ones(end, bool)
    keep[ff[stuffed] + 1] = False
    keep[ff[rst]] = False
    keep[ff[rst] + 1] = False
    rec.data = a[:end][keep]
    starts = np.cumsum(keep)[ff[rst]] if rst.any() else np.zeros(0, np.int64)
    nrst = -(-rec.mcus // ri) - 1 if ri else 0
    if len(starts) != nrst:
        refuse(f"{len(starts)} RSTn markers in the scan, {nrst} expected from DRI {ri}")
    if nrst and not np.array_equal(nxt[rst] - 0xD0, np.arange(nrst) % 8):
        refuse("RSTn markers out of order")
    if len(rec.data) >= 1 << 28:
        refuse("a scan of 256 MiB or more")
    rec.restart_starts = np.concatenate([[0], starts]).astype(np.int32)
    return rec


def _interval(rec: JpegRecord, index_interval) -> int:
    if index_interval == "row":
        v = rec.mcu_cols
    elif index_interval == "frame":
        v = rec.mcus
    elif isinstance(index_interval, bool) or not isinstance(index_interval, (int, np.integer)) or index_interval < 1:
        raise ValueError(f"index_interval must be a positive number of MCUs, 'row' or 'frame', got {index_interval!r}")
    else:
        v = int(index_interval)
    return min(v, rec.mcus)


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class JpegFrames:
    """Frames kept on the device as JPEG bitstreams.  streams: per frame the bytes of a file, or its `JpegRecord`; sizes, samplings and tables
    may differ between frames (equal table sets are stored once).  index_interval: MCUs per entry (an int), "row" (one MCU row) or "frame".
    The constructor uploads one blob, runs vt_jpeg_index and reads the status words back once: a stream the pass flags raises ValueError
    naming the frame.  `.table`: the int64 [N, 16] rows of include/vlatouch.h; `.nbytes`: streams + table sets + restart starts + entries +
    the table, i.e. what stays resident."""

    def __init__(self, streams: Sequence, device="cuda", index_interval: Union[int, str] = DEFAULT_INDEX_INTERVAL):
        self.device = _lib.require_gpu(device)
        recs = [s if isinstance(s, JpegRecord) else parse_jpeg(s, k) for k, s in enumerate(streams)]
        if not recs:
            raise ValueError("JpegFrames: no frames")
        if any(r.data is None for r in recs):
            raise ValueError("JpegFrames: a header-only JpegRecord holds no stream")
        n = len(recs)
        self.shapes = [(r.h, r.w) for r in recs]
        self.samplings = [r.sampling for r in recs]
        sets: dict = {}
        set_id = [sets.setdefault(r.tableset, len(sets)) for r in recs]
        self.table_sets, self.table_set_ids = len(sets), set_id
        table = np.zeros((n, _lib.JPEG_K), np.int64)
        off = _align(len(sets) * _lib.JPEG_TABLESET_BYTES, 16)
        for k, r in enumerate(recs):
            iv = _interval(r, index_interval)
            row = table[k]
            row[C_LEN], row[C_H], row[C_W], row[C_SAMP], row[C_INTERVAL], row[C_RI] = len(r.data), r.h, r.w, r.sampling, iv, r.restart_interval
            row[C_TSET] = set_id[k] * _lib.JPEG_TABLESET_BYTES
            row[C_STREAM], off = off, off + _align(len(r.data), 4)
            row[C_RST], off = off, _align(off + 4 * len(r.restart_starts), 16)
            row[C_ENTRIES], off = off, off + 16 * -(-r.mcus // iv)
        blob = np.full(off, 0xFF, np.uint8)                                    # the bytes behind a stream's end are FF: 1-bits, as libjpeg pads
        for ts, k in sets.items():
            blob[k * _lib.JPEG_TABLESET_BYTES:(k + 1) * _lib.JPEG_TABLESET_BYTES] = np.frombuffer(ts, np.uint8)
        for k, r in enumerate(recs):
            row = table[k]
            blob[row[C_STREAM]:row[C_STREAM] + len(r.data)] = r.data
            blob[row[C_RST]:row[C_RST] + 4 * len(r.restart_starts)] = r.restart_starts.view(np.uint8)
        with torch.cuda.device(self.device):
            self.blob = torch.from_numpy(blob).to(self.device)
            base = self.blob.data_ptr()
            for c in (C_STREAM, C_TSET, C_RST, C_ENTRIES):
                table[:, c] += base
            self.table = table
            tdev = torch.from_numpy(table).to(self.device)
            status = torch.zeros(n, dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().vt_jpeg_index(table.ctypes.data, _lib.ptr(tdev), n, _lib.ptr(status), _lib.stream_ptr(self.device)), "vt_jpeg_index")
            bad = np.flatnonzero(status.cpu().numpy())                         # the one host read, at load
        self.nbytes = int(blob.nbytes + table.nbytes)
        self.index_bytes = int(sum(16 * -(-r.mcus // int(table[k, C_INTERVAL])) for k, r in enumerate(recs)))
        if len(bad):
            raise ValueError(f"JpegFrames: the entropy bytes of JPEG frame {', '.join(str(int(k)) for k in bad)} are broken: an undefined Huffman "
                             "code, a run past coefficient 63, or the stream ends before its last MCU")

    def __len__(self) -> int:
        return len(self.shapes)

    def decode(self, indices: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The chosen frames (default: all; any order, repeats allowed), which must share one size -> uint8 [k, H, W, 3] on the device (`out`,
        contiguous and of that shape, or a new tensor), in one vt_jpeg_decode call on the current stream."""
        idx = list(range(len(self))) if indices is None else [int(i) for i in indices]
        if not idx:
            raise ValueError("JpegFrames.decode: no frames chosen")
        for i in idx:
            if not -len(self) <= i < len(self):
                raise IndexError(f"JpegFrames.decode: frame {i} of {len(self)}")
        h, w = self.shapes[idx[0]]
        if any(self.shapes[i] != (h, w) for i in idx):
            raise ValueError("JpegFrames.decode: the chosen frames differ in size (decode_many takes mixed sizes)")
        shape = (len(idx), h, w, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != self.blob.device:
            raise _lib.VtError(f"JpegFrames.decode: out must be a contiguous uint8 tensor of shape {shape} on {self.blob.device}")
        rows = self.table[idx].copy()
        rows[:, C_OUT_OFF] = np.arange(len(idx), dtype=np.int64) * (3 * h * w)
        _decode_rows(rows, out, self.device)
        return out


def _decode_rows(rows: np.ndarray, out: torch.Tensor, device) -> torch.Tensor:
    """One vt_jpeg_decode call over table rows whose out_off is set; returns the call's status words (device int32, not read)."""
    L = _lib.lib()
    n = len(rows)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    ws_bytes = int(L.vt_jpeg_workspace_bytes(rows.ctypes.data, n))
    if ws_bytes == 0:
        raise _lib.VtError("vt_jpeg_workspace_bytes: " + L.vt_last_error().decode())
    with torch.cuda.device(device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        tdev = torch.from_numpy(rows).to(device)                               # the call's one upload
        status = torch.zeros(n, dtype=torch.int32, device=device)
        _lib.check(L.vt_jpeg_decode(rows.ctypes.data, _lib.ptr(tdev), n, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.ptr(status),
                                    _lib.stream_ptr(device)), "vt_jpeg_decode")
    return status


@torch.no_grad()
def decode_many(picks: Sequence, out: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """picks: (JpegFrames, frame index) pairs, all on one device, of any sizes -> uint8 [H, W, 3] device tensors, views of one buffer (`out`:
    a contiguous uint8 device tensor of enough bytes; allocated when None), frame i at a multiple of 16 bytes.  One vt_jpeg_decode call."""
    picks = list(picks)
    if not picks:
        raise ValueError("decode_many: no frames chosen")
    device = picks[0][0].device
    rows = np.stack([jf.table[int(i)] for jf, i in picks])
    sizes = 3 * rows[:, C_H] * rows[:, C_W]
    offs = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)])
    rows[:, C_OUT_OFF] = offs[:-1]
    need = int(offs[-1])
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.device != picks[0][0].blob.device or out.numel() < need:
        raise _lib.VtError(f"decode_many: out must be a contiguous uint8 tensor of at least {need} bytes on {device}")
    _decode_rows(rows, out, device)
    flat = out.view(-1)
    return [flat[int(o):int(o) + int(s)].view(int(r[C_H]), int(r[C_W]), 3) for o, s, r in zip(offs[:-1], sizes, rows)]


def decode_jpeg_device(streams: Sequence, device="cuda", index_interval: Union[int, str] = DEFAULT_INDEX_INTERVAL) -> List[torch.Tensor]:
    """Every file of `streams` (bytes; sizes, samplings and tables may differ) -> uint8 [H, W, 3] device tensors: `JpegFrames` + one decode
    call."""
    jf = JpegFrames(streams, device, index_interval)
    return decode_many([(jf, i) for i in range(len(jf))])
