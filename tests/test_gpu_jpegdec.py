"""csrc/vt_jpegdec.hip through vlatouch/jpegdec.py on the GPU: stored baseline JPEG files decoded on the device equal Pillow's decode of the
same bytes bit for bit, so no tolerance appears here.  The host half and the CPU statement are tests/test_jpegdec_host.py's."""
import numpy as np
import pytest
import torch

from tests import jpeg_ref as J
from tests import jpegdec_ref as R
from tests.test_jpegdec_host import GRID_MODES, QUALITIES, cut_entropy_in_half, golden_streams, pillow_writes_dri
from vlatouch import _lib as L
from vlatouch import jpegdec as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VT_ERR_ARG = -22


def same(t: torch.Tensor, want: np.ndarray) -> bool:
    return t.dtype == torch.uint8 and tuple(t.shape) == want.shape and np.array_equal(t.cpu().numpy(), want)


@pytest.fixture(scope="module")
def small():
    """A few streams of 48 x 64 and 19 x 21 with their Pillow pixels: default, own Huffman tables, 4:4:4, restart every 3 MCUs and every MCU row
    (the golden streams, quality 90), and one of 30 x 50 at quality 30: other quantisation tables."""
    g = golden_streams()
    out = {k: g[k] for k in ("48x64_default", "48x64_optimize", "48x64_444", "48x64_restart", "48x64_restart_rows", "19x21_restart", "19x21_444")}
    assert D.parse_jpeg(out["48x64_restart"][0]).restart_interval == 3 and D.parse_jpeg(out["48x64_restart_rows"][0]).restart_interval == 4
    b = R.encode(J.make_frame("speckle", 30, 50), 30)
    out["30x50_q30"] = (b, R.pillow_decode(b))
    return out


@pytest.mark.parametrize("mode", GRID_MODES)
def test_device_decode_equals_pillow_on_the_grid(mode):
    """Every shape x content x quality of a mode in ONE call: 1 x 1 to 48 x 64, partial MCUs, replicated narrow chroma, one or several MCU rows."""
    if mode == "restart" and not pillow_writes_dri():
        pairs = [v for k, v in golden_streams().items() if "restart" in k]
    else:
        streams = [R.encode(J.make_frame(kind, h, w), q, mode) for h, w in J.SHAPES for kind in J.CONTENTS for q in QUALITIES]
        pairs = [(b, R.pillow_decode(b)) for b in streams]
    if mode == "restart":
        assert all(b"\xff\xdd" in b for b, _ in pairs)
    got = D.decode_jpeg_device([b for b, _ in pairs], DEV)
    torch.cuda.synchronize()
    bad = [k for k, (g, (_, want)) in enumerate(zip(got, pairs)) if not same(g, want)]
    assert not bad, bad[:10]


def test_a_480_x_640_noise_frame_at_quality_95():
    """1200 MCUs: several workgroups per launch, 123 KB of entropy bytes, the long codes of a busy frame."""
    img = np.random.default_rng(5).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    b = R.encode(img, 95)
    jf = D.JpegFrames([b], DEV)
    assert jf.nbytes < img.nbytes and same(jf.decode()[0], R.pillow_decode(b))


def test_one_call_mixes_sizes_samplings_and_table_sets(small):
    names = list(small)
    jf = D.JpegFrames([small[k][0] for k in names], DEV)
    # three table sets: the standard tables at quality 90 and at quality 30, and one stream's own Huffman tables
    assert jf.table_sets == 3 and len(set(jf.shapes)) == 3 and set(jf.samplings) == {D.S420, D.S444}
    got = D.decode_many([(jf, i) for i in range(len(names))])
    assert all(same(g, small[k][1]) for g, k in zip(got, names))
    assert all(g.data_ptr() % 16 == 0 for g in got)


@pytest.mark.parametrize("interval", [1, 2, 3, 5, 7, "row", "frame"])
def test_every_index_interval_gives_the_same_bits(small, interval):
    """Against restart intervals of 3 MCUs and of one MCU row (4): entries that coincide with the restart boundaries (3, "row"), straddle
    them (2, 5, 7, "frame") and sit inside them (1); 5 and 7 divide no MCU count here (12; 4 and 9 for 19 x 21; 8 for 30 x 50)."""
    names = list(small)
    got = D.decode_jpeg_device([small[k][0] for k in names], DEV, index_interval=interval)
    assert all(same(g, small[k][1]) for g, k in zip(got, names))


def test_decode_of_a_subset_permuted_with_repeats_and_a_second_call(small):
    names = [k for k in small if k.startswith("48x64")]
    jf = D.JpegFrames([small[k][0] for k in names], DEV, index_interval=5)
    pick = [3, 0, 3, 4, 1, -1]
    out = jf.decode(pick)
    assert tuple(out.shape) == (6, 48, 64, 3) and all(same(out[i], small[names[p]][1]) for i, p in enumerate(pick))
    again = torch.full_like(out, 7)
    assert jf.decode(pick, out=again) is again and torch.equal(out, again)
    assert torch.equal(jf.decode(), torch.stack([jf.decode([i])[0] for i in range(len(names))]))
    with pytest.raises(ValueError, match="differ in size"):
        D.JpegFrames([small["48x64_default"][0], small["19x21_444"][0]], DEV).decode()
    with pytest.raises(IndexError):
        jf.decode([5])


def test_a_bad_table_returns_err_arg_without_a_launch(small):
    jf = D.JpegFrames([small["48x64_default"][0], small["19x21_444"][0]], DEV)
    lib = L.lib()
    rows = jf.table.copy()
    rows[:, D.C_OUT_OFF] = (0, 48 * 64 * 3)
    ws_bytes = int(lib.vt_jpeg_workspace_bytes(rows.ctypes.data, 2))
    assert ws_bytes > 0
    out = torch.full((48 * 64 * 3 + 19 * 21 * 3,), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(table=rows, n=2, dev_table=True, outp=out, wsp=ws, wsb=ws_bytes, st=status):
        t = np.ascontiguousarray(table)
        tdev = torch.from_numpy(t).to(DEV)
        return lib.vt_jpeg_decode(t.ctypes.data, L.ptr(tdev) if dev_table else None, n, L.ptr(outp), L.ptr(wsp), wsb, L.ptr(st), L.stream_ptr(DEV))

    def edited(col, value, row=1):
        t = rows.copy()
        t[row, col] = value
        return t

    bad = [dict(n=0), dict(dev_table=False), dict(outp=None), dict(wsp=None), dict(st=None), dict(wsb=ws_bytes - 1), dict(wsp=ws[8:], wsb=ws_bytes),
           dict(table=edited(D.C_H, 0)), dict(table=edited(D.C_W, 32769)), dict(table=edited(D.C_SAMP, 2)), dict(table=edited(D.C_STREAM, 0)),
           dict(table=edited(D.C_STREAM, rows[1, D.C_STREAM] + 1)), dict(table=edited(D.C_TSET, 0)), dict(table=edited(D.C_ENTRIES, rows[1, D.C_ENTRIES] + 4)),
           dict(table=edited(D.C_RST, 0)), dict(table=edited(D.C_LEN, -1)), dict(table=edited(D.C_LEN, 1 << 28)), dict(table=edited(D.C_INTERVAL, 0)),
           dict(table=edited(D.C_INTERVAL, 10)), dict(table=edited(D.C_RI, -1)), dict(table=edited(D.C_OUT_OFF, -16)), dict(table=edited(11, 128)),
           dict(table=edited(12, 0, row=0))]
    for kw in bad:
        assert call(**kw) == VT_ERR_ARG, kw
        assert lib.vt_last_error().decode().startswith("vt_jpeg_decode:"), kw
    assert lib.vt_jpeg_workspace_bytes(edited(D.C_H, 0).ctypes.data, 2) == 0
    assert lib.vt_jpeg_index(rows.ctypes.data, None, 2, L.ptr(status), L.stream_ptr(DEV)) == VT_ERR_ARG
    assert lib.vt_jpeg_index(edited(D.C_INTERVAL, 0).ctypes.data, L.ptr(ws), 2, L.ptr(status), L.stream_ptr(DEV)) == VT_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and not bool(status.any())                     # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert same(out[:48 * 64 * 3].view(48, 64, 3), small["48x64_default"][1]) and same(out[48 * 64 * 3:].view(19, 21, 3), small["19x21_444"][1])
    assert not bool(status.any())


def test_a_stream_cut_in_half_is_reported_through_its_status_word(small):
    """The reporting: the host parse passes (EOI is there), the index pass meets the stream's end before the last MCU and flags that frame."""
    names = ["48x64_default", "48x64_optimize", "48x64_444"]
    streams = [small[k][0] for k in names]
    streams[1] = cut_entropy_in_half(streams[1])
    assert D.parse_jpeg(streams[1], 1).h == 48
    with pytest.raises(ValueError, match=r"JPEG frame 1 are broken"):
        D.JpegFrames(streams, DEV)
    jf = D.JpegFrames([streams[0], streams[2]], DEV)
    out = jf.decode()
    assert same(out[0], small[names[0]][1]) and same(out[1], small[names[2]][1])
