"""The host half of the device JPEG decoder (vlatouch/jpegdec.py) and its CPU statement (tests/jpegdec_ref.py), without a GPU: the statement
equals Pillow bit for bit; the parser's un-stuffed stream, restart starts and tables decode to the statement's coefficients through the
device's own table forms and bit reader (jpegdec_ref.DeviceWalk); every refusal is raised by name; the conversion keeps the files' bytes and
a store of them draws what a store of the decoded file draws."""
import io
import os
import random

import numpy as np
import pytest

from tests import jpeg_ref as J
from tests import jpegdec_ref as R
from tests import rdt_data_ref as RD
from vlatouch import convert, h5lite
from vlatouch import jpegdec as D

QUALITIES = (1, 30, 75, 95, 100)
GRID_MODES = ("default", "optimize", "444", "restart")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_jpeg_streams.npz")


def golden_streams():
    z = np.load(GOLDEN)
    return {k[2:]: (z[k].tobytes(), z["p_" + k[2:]]) for k in z.files if k.startswith("s_")}


def pillow_writes_dri() -> bool:
    return b"\xff\xdd" in R.encode(J.make_frame("gradient", 48, 64), 95, "restart")


@pytest.mark.parametrize("mode", GRID_MODES)
def test_statement_equals_pillow(mode):
    if mode == "restart" and not pillow_writes_dri():          # this Pillow cannot write DRI: the golden streams carry that leg
        cases = [(b, px) for k, (b, px) in golden_streams().items() if "restart" in k]
    else:
        cases = []
        for h, w in J.SHAPES:
            for kind in J.CONTENTS:
                for q in QUALITIES:
                    b = R.encode(J.make_frame(kind, h, w), q, mode)
                    cases.append((b, R.pillow_decode(b)))
    assert cases
    for b, want in cases:
        if mode == "restart":
            assert b"\xff\xdd" in b and D.parse_jpeg(b).restart_interval > 0
        assert np.array_equal(R.decode(b), want)
    if mode == "444":
        assert all(D.parse_jpeg(b).sampling == D.S444 for b, _ in cases[:3])


def test_statement_and_parser_equal_the_golden_streams():
    g = golden_streams()
    assert len(g) == 10 and sum("restart" in k for k in g) == 4
    for name, (b, want) in g.items():
        assert np.array_equal(R.decode(b), want), name
        rec = D.parse_jpeg(b)
        assert (rec.h, rec.w, 3) == want.shape and (rec.restart_interval > 0) == ("restart" in name), name
        assert (rec.sampling == D.S444) == name.endswith("444")


def _grid_for_walks():
    for h, w in ((1, 1), (19, 21), (33, 16), (48, 64)):
        for kind, q in (("noise", 100), ("speckle", 1), ("gradient", 75)):
            for mode in R.MODES:
                yield (h, w, kind, q, mode), R.encode(J.make_frame(kind, h, w), q, mode)


def test_parser_equals_the_statements_unstuffing_and_tables():
    for name, b in _grid_for_walks():
        rec, p = D.parse_jpeg(b, 0), R.parse(b)
        data, rst = R.unstuff(b, p["start"])
        assert bytes(rec.data) == data and rec.restart_starts.tolist() == [0] + rst and rec.restart_interval == p["dri"], name
        assert (rec.h, rec.w) == (p["h"], p["w"]) and len(rec.tableset) == D._lib.JPEG_TABLESET_BYTES
        for c, (_, _, _, tq) in enumerate(p["comps"]):
            assert np.array_equal(rec.qt[c].reshape(8, 8), p["qt"][tq]), name


def test_every_mcu_from_its_entry_alone_equals_sequential_decoding():
    """In the statement, and through the device's table forms and bit reader: intervals 1, one MCU row, the whole frame, and 5."""
    for name, b in _grid_for_walks():
        rec = D.parse_jpeg(b)
        p, planes = R.coefficients(b)
        want = R.stream_order_blocks(p, planes)
        for iv in sorted({1, rec.mcu_cols, rec.mcus, min(5, rec.mcus)}):
            _, again = R.coefficients(b, iv)
            assert all(np.array_equal(x, y) for x, y in zip(planes, again)), (name, iv)
            walk = R.DeviceWalk(rec)
            status, ent = walk.index(iv)
            assert status == 0 and [(e[0], tuple(e[1:])) for e in ent] == R.entries(b, iv), (name, iv)
            status, got = walk.coefficients(iv)
            assert status == 0 and got == want, (name, iv)


def test_tables_are_shared_between_frames_of_one_encoder():
    a, b = (D.parse_jpeg(R.encode(J.make_frame(k, 19, 21), 75)) for k in ("noise", "gradient"))
    c = D.parse_jpeg(R.encode(J.make_frame("noise", 19, 21), 75, "optimize"))
    assert a.tableset == b.tableset and a.tableset != c.tableset


def _pil(img, fmt="JPEG", **kw):
    from PIL import Image
    buf = io.BytesIO()
    (img if isinstance(img, Image.Image) else Image.fromarray(img)).save(buf, fmt, **kw)
    return buf.getvalue()


def cut_entropy_in_half(b: bytes) -> bytes:
    """The file with the second half of its entropy bytes dropped and EOI appended again: the host parse still passes."""
    k = b.index(b"\xff\xda")
    start = k + 2 + ((b[k + 2] << 8) | b[k + 3])
    cut = start + (len(b) - 2 - start) // 2
    while b[cut - 1] == 0xFF:                                 # not between FF and its stuffed 00
        cut -= 1
    return b[:cut] + b"\xff\xd9"


def test_refusals_are_raised_by_name():
    from PIL import Image
    img = J.make_frame("gradient", 19, 21)
    good = _pil(img, quality=75)
    refused = {
        "progressive": _pil(img, quality=75, progressive=True),
        "grayscale": _pil(Image.fromarray(img).convert("L"), quality=75),
        "CMYK": _pil(Image.fromarray(img).convert("CMYK"), quality=75),
        r"sampling 2x1,1x1,1x1 is not built": _pil(img, quality=75, subsampling=1),
        "missing EOI": good[:-2],
        "truncated": good[:good.index(b"\xff\xda")],
        "not a JPEG file": _pil(img, "PNG"),
    }
    k = good.index(b"\xff\xdb")
    refused["bad segment length"] = good[:k + 2] + b"\xff\xf0" + good[k + 4:]
    k = good.index(b"\xff\xc0")
    refused["12- or 16-bit"] = good[:k + 4] + b"\x0c" + good[k + 5:]
    refused["a side above 32768"] = good[:k + 5] + b"\x80\x01" + good[k + 7:]
    refused["extended sequential"] = good[:k + 1] + b"\xc1" + good[k + 2:]
    refused["arithmetic"] = good[:k + 1] + b"\xc9" + good[k + 2:]
    refused["lossless"] = good[:k + 1] + b"\xc3" + good[k + 2:]
    k = good.index(b"\xff\xdb")
    refused["16-bit DQT"] = good[:k + 4] + b"\x10" + good[k + 5:]
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    refused["Adobe APP14 transform 0"] = good[:2] + adobe + b"\x00" + good[2:]
    refused["more than one scan"] = good[:-2] + good[good.index(b"\xff\xda"):]
    for name, data in refused.items():
        with pytest.raises(ValueError, match=f"JPEG frame 7: .*{name}"):
            D.parse_jpeg(data, 7)
    assert D.parse_jpeg(good[:2] + adobe + b"\x01" + good[2:], 7).h == 19          # Adobe's YCbCr transform is what is built
    assert D.parse_jpeg(cut_entropy_in_half(good)).h == 19                          # a cut stream is the device's to flag
    status, _ = R.DeviceWalk(D.parse_jpeg(cut_entropy_in_half(_pil(J.make_frame("noise", 48, 64), quality=95)))).index(4)
    assert status == 1


# ------------------------------------------------------------------------------------------------ conversion and the store
@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_recording")
    for e, n in ((1, 36), (2, 33)):
        R.write_recording(str(root / "raw" / f"episode_{e}"), n, seed=e, cameras=("camera1", "camera2") if e == 1 else ("camera1",), hw=(16, 24))
    convert.convert_dataset_to_hdf5(str(root / "raw"), str(root / "decoded"))
    convert.convert_dataset_to_hdf5(str(root / "raw"), str(root / "jpeg"), images="jpeg")
    return root


def test_convert_keeps_the_files_bytes_and_the_decoded_mode_is_the_parents(recording, tmp_path):
    ep = recording / "raw" / "episode_1"
    with h5lite.File(str(recording / "jpeg" / "episode_1.h5")) as f:
        assert set(f["camera1"].keys()) == {"camera1_jpeg", "camera1_jpeg_offsets"}
        data, off = f["camera1"]["camera1_jpeg"][...], f["camera1"]["camera1_jpeg_offsets"][...]
        assert data.dtype == np.uint8 and off.dtype == np.int64 and off.shape == (37,) and off[0] == 0 and off[-1] == len(data)
        for i in (0, 1, 17, 35):
            assert data[off[i]:off[i + 1]].tobytes() == (ep / "camera1" / f"rgb_{i}.jpg").read_bytes()
        assert f["ee_poses"].shape == (36, 7) and f["instruct_embeddings"].shape == (1, 3, 8)
    # images="decoded", and the call without the argument, write the parent's file: the tree it built, through the same writer
    tree = convert.episode_tree(str(ep))
    assert tree["camera1"]["camera1"].shape == (36, 16, 24, 3)
    assert np.array_equal(tree["camera1"]["camera1"][5], R.pillow_decode((ep / "camera1" / "rgb_5.jpg").read_bytes()))
    h5lite.write_file(str(tmp_path / "parent.h5"), tree, compression="lzf")
    convert.convert_episode_to_hdf5(str(ep), str(tmp_path / "explicit.h5"), images="decoded")
    want = (tmp_path / "parent.h5").read_bytes()
    assert (tmp_path / "explicit.h5").read_bytes() == want == (recording / "decoded" / "episode_1.h5").read_bytes()
    with pytest.raises(ValueError, match="images must be one of"):
        convert.convert_episode_to_hdf5(str(ep), str(tmp_path / "x.h5"), images="raw")


def test_convert_refuses_png_and_unequal_sizes_in_jpeg_mode(tmp_path):
    from PIL import Image
    for name, second in (("png", ("rgb_1.png", (16, 24))), ("unequal", ("rgb_1.jpg", (8, 24)))):
        ep = tmp_path / name / "episode_1"
        (ep / "camera1").mkdir(parents=True)
        Image.fromarray(J.make_frame("gradient", 16, 24)).save(ep / "camera1" / "rgb_0.jpg")
        Image.fromarray(J.make_frame("gradient", *second[1])).save(ep / "camera1" / second[0])
        with pytest.raises(ValueError, match="not a JPEG file" if name == "png" else "unequal size"):
            convert.convert_episode_to_hdf5(str(ep), str(tmp_path / f"{name}.h5"), images="jpeg")
        convert.convert_episode_to_hdf5(str(ep), str(tmp_path / f"{name}_decoded.h5"))          # the decoded route takes both


def test_a_store_of_the_jpeg_file_draws_what_a_store_of_the_decoded_file_draws(recording):
    from vlatouch.rdt_data import EpisodeStore
    kw = dict(dataset_name=RD.DATASET_NAME, dataset_names=RD.DATASET_NAMES, control_freq=RD.CONTROL_FREQ, horizon=16, device="cpu")
    a = EpisodeStore(str(recording / "decoded"), **kw)
    b = EpisodeStore(str(recording / "jpeg"), frames="jpeg", **kw)
    assert len(a.episodes) == len(b.episodes) == 2 and len(a) == len(b) and a.dataset_stat() == b.dataset_stat()
    assert [e.has_cam for e in a.episodes] == [e.has_cam for e in b.episodes] == [[True, True, False], [True, False, False]]
    assert b.episodes[0].frames[0].shape == a.episodes[0].frames[0].shape == (36, 16, 24, 3)
    draw = dict(cond_mask_prob=0.3, state_noise_snr=40, image_aug=True)
    rngs = lambda: dict(np_rng=np.random.RandomState(4), rng=random.Random(4), generator=__import__("torch").Generator().manual_seed(4))
    pa, pb = a.draw(6, **rngs(), **draw), b.draw(6, **rngs(), **draw)
    assert [repr(p) for p in pa] == [repr(p) for p in pb]
    assert all(np.array_equal(x.noise, y.noise) and x.jitter == y.jitter for x, y in zip(pa, pb))
    b.check_plans(pb)
    with pytest.raises(ValueError, match="holds decoded pixels"):
        EpisodeStore(str(recording / "decoded"), frames="jpeg", **kw)
    with pytest.raises(ValueError, match="frames must be"):
        EpisodeStore(str(recording / "jpeg"), frames="jpg", **kw)
