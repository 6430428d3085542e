"""The reference's zero pad + INTER_AREA resize of camera frames on the device (csrc/vt_area.hip, vlatouch.imgprep.pad_and_resize_device)
against the numpy statement `pad_and_resize_for_siglip` (itself checked in tests/test_area_resize_host.py), and its way through
DevicePreprocessor, step, label_episode and EpisodeStore.  Every comparison is bit-equal: the kernel keeps the statement's fp32 order."""
import copy
import functools
import os
import random

import numpy as np
import pytest
import torch

from tests import cases
from vlatouch import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 24
# fractional (landscape, portrait, odd pad), scale just above 1, the integer forms 2, 3, 4, the copy
SHAPES = [(30, 40), (37, 53), (53, 37), (25, 25), (48, 48), (72, 96), (96, 96), (24, 24)]


@functools.lru_cache(maxsize=None)
def raw(h, w, seed=0):
    a = np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(h, w, seed=0, target=T):
    from vlatouch.imgprep import pad_and_resize_for_siglip
    r = pad_and_resize_for_siglip(raw(h, w, seed), target)
    r.setflags(write=False)
    return r


def same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == np.uint8, (what, got.shape, got.dtype)
    n = int((got != ref).sum())
    assert n == 0, f"{what}: {n} of {ref.size} bytes differ, max |d| = {int(np.abs(got.astype(int) - ref.astype(int)).max())}"


@pytest.mark.parametrize("h,w", SHAPES)
def test_each_shape_equals_the_statement(h, w):
    from vlatouch.imgprep import pad_and_resize_device
    got = pad_and_resize_device([raw(h, w)], T, device=DEV)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, T, T, 3)
    same(got[0], want(h, w), (h, w))


def test_mixed_sizes_and_a_missing_frame_in_one_call():
    from vlatouch.imgprep import pad_and_resize_device
    frames = [raw(h, w) for h, w in SHAPES]
    frames.insert(3, None)
    out = torch.full((len(frames), T, T, 3), 0x5A, dtype=torch.uint8, device=DEV)
    got = pad_and_resize_device(frames, T, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert int(got[3].any()) == 0                                            # nothing on the canvas
    for k, (h, w) in enumerate(SHAPES):
        same(got[k + (k >= 3)], want(h, w), (h, w))


def test_a_target_that_is_not_the_block_size_and_a_larger_reduction():
    """25 x 25 outputs (625 pixels: three blocks, the last one partial, frames 1875 bytes apart) and a 7-fold cell sum."""
    from vlatouch.imgprep import pad_and_resize_device
    got = pad_and_resize_device([raw(30, 40), raw(50, 41), raw(175, 160)], 25, device=DEV)
    for k, (h, w) in enumerate([(30, 40), (50, 41), (175, 160)]):
        same(got[k], want(h, w, 0, 25), (h, w))


def test_products_and_sums_are_rounded_separately():
    """40 -> 28 has the weights 0.7 and 0.3, under which many outputs land on a tie that only the fp32 rounding of every product and sum
    decides: with a * b + c contracted into an FMA, 22 of the 14112 bytes of the labeller test's six frames came out one level off, while
    no 24-wide case did.  And one camera frame at the real size, 480 x 640 -> 384 x 384."""
    from vlatouch.imgprep import pad_and_resize_device
    got = pad_and_resize_device([raw(30, 40, s) for s in range(6)], 28, device=DEV)
    for s in range(6):
        same(got[s], want(30, 40, s, 28), ("40 -> 28", s))
    same(pad_and_resize_device([raw(480, 640)], 384, device=DEV)[0], want(480, 640, 0, 384), "480 x 640 -> 384")


def test_every_input_kind_gives_the_bits_of_the_contiguous_frame():
    from PIL import Image
    from vlatouch.imgprep import pad_and_resize_device
    a = np.array(raw(37, 53))
    wide = torch.full((37, 80, 3), 77, dtype=torch.uint8, device=DEV)
    wide[:, 5:58] = torch.from_numpy(a).to(DEV)
    view = wide[:, 5:58]                                                     # pitched: rows 240 bytes apart, 15 bytes in, odd addresses
    assert not view.is_contiguous()
    got = pad_and_resize_device([view, Image.fromarray(a), a, torch.from_numpy(a), torch.from_numpy(a).to(DEV)], T)
    for k in range(5):
        same(got[k], want(37, 53), f"input kind {k}")
    assert int((wide[:, :5] != 77).sum()) == 0 and int((wide[:, 58:] != 77).sum()) == 0


def test_refusals_come_without_a_launch():
    from vlatouch import _lib
    from vlatouch.imgprep import area_table, pad_and_resize_device
    with pytest.raises(_lib.VtError, match="up-scale emulation is not built"):
        pad_and_resize_device([raw(30, 40), raw(20, 20)], T, device=DEV)
    L = _lib.lib()
    src = torch.zeros(30 * 40 * 3, dtype=torch.uint8, device=DEV)
    out = torch.full((2 * 3 * T * T,), 0x5A, dtype=torch.uint8, device=DEV)
    good, _, taps = area_table([(src.data_ptr(), 30, 40, 120)], T)
    tabs = torch.from_numpy(taps).to(DEV)

    def call(arr, n=1, dev=src, o=out, t=tabs, nbytes=None):
        return L.vt_area_resize(arr, _lib.ptr(dev), n, _lib.ptr(o), _lib.ptr(t), taps.size if nbytes is None else nbytes, _lib.stream_ptr(DEV))

    def edit(**kw):
        cp = (_lib.AreaFrame * 1).from_buffer_copy(good)
        for k, v in kw.items():
            setattr(cp[0], k, v)
        return cp

    bad = [("n < 1", lambda: call(good, n=0)), ("null device table", lambda: call(good, dev=None)), ("null out", lambda: call(good, o=None)),
           ("null tables", lambda: call(good, t=None)), ("short tables", lambda: call(good, nbytes=taps.size - 1)),
           ("null table", lambda: L.vt_area_resize(None, _lib.ptr(src), 1, _lib.ptr(out), _lib.ptr(tabs), taps.size, _lib.stream_ptr(DEV))),
           ("h 0", lambda: call(edit(h=0))), ("w 0", lambda: call(edit(w=0))), ("pitch", lambda: call(edit(pitch=119))), ("null src", lambda: call(edit(src=None))),
           ("too large", lambda: call(edit(h=40000))), ("target 0", lambda: call(edit(target=0))), ("up-scale", lambda: call(edit(target=41))),
           ("no taps for a fractional scale", lambda: call(edit(ntaps=0))), ("too many taps", lambda: call(edit(ntaps=9))),
           ("taps for an integer scale", lambda: call(edit(target=20))), ("negative table offset", lambda: call(edit(tab_x=-8))),
           ("misaligned table offset", lambda: call(edit(tab_y=4))), ("table offset beyond the tables", lambda: call(edit(tab_y=8))),
           ("negative out_off", lambda: call(edit(out_off=-1)))]
    for what, fn in bad:
        assert fn() == -22, what                                             # VT_ERR_ARG
        assert len(L.vt_last_error()) > 10, what
    torch.cuda.synchronize()
    assert int((out != 0x5A).sum()) == 0                                     # nothing was launched
    good_dev = torch.from_numpy(np.frombuffer(bytes(memoryview(good)), dtype=np.uint8).copy()).to(DEV)
    assert call(good, dev=good_dev) == 0                                     # and the good call is one
    torch.cuda.synchronize()
    same(out[:3 * T * T].view(T, T, 3), np.zeros((T, T, 3), np.uint8), "the good call")
    assert int((out[3 * T * T:] != 0x5A).sum()) == 0


# ---- through the preprocessor

def _frames():
    return [np.array(raw(30, 40)), None, np.array(raw(53, 37)), torch.from_numpy(np.array(raw(48, 48))).to(DEV), np.array(raw(24, 24)),
            (np.array(raw(72, 96)) // 8).astype(np.uint8)]                   # the last one takes the brightness lift, behind the resize


def _resized(frames, target=T):
    from vlatouch.imgprep import pad_and_resize_for_siglip
    return [None if f is None else pad_and_resize_for_siglip(f.cpu().numpy() if isinstance(f, torch.Tensor) else f, target) for f in frames]


@pytest.mark.parametrize("S", [24, 64])
def test_preprocess_with_area_equals_preprocess_of_the_statement(S):
    from tests.test_gpu_imgprep import as_pil, make_model
    from vlatouch.jpegmap import jpeg_mapping
    m = make_model(S)
    frames = _frames()
    small = _resized(frames)
    got = m.preprocess_images_device(frames, area=T).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, m.preprocess_images(as_pil(small)).to(DEV, m.dtype))
    assert torch.equal(got, m.preprocess_images_device(small))
    mapped = [None if f is None else jpeg_mapping(f, 95) for f in small]    # area first, then the mapping of the 24 x 24 frame
    got_j = m.preprocess_images_device(frames, area=T, jpeg=95).clone()
    assert torch.equal(got_j, m.preprocess_images(as_pil(mapped)).to(DEV, m.dtype))
    assert not torch.equal(got_j, got)
    pp = next(iter(m._imgprep.values()))
    assert pp.workspace_bytes(small) < pp.workspace_bytes(frames, area=T) < pp.workspace_bytes(frames, area=T, jpeg=95)
    for bad in (0, -1, True, 24.0, "24"):
        with pytest.raises(Exception):
            m.preprocess_images_device(frames, area=bad)
    with pytest.raises(Exception, match="up-scale emulation is not built"):
        m.preprocess_images_device(frames, area=25)                          # the 24 x 24 frame is smaller


def test_preprocess_with_area_jitter_and_corruption():
    from tests.test_gpu_imgprep import make_model
    from vlatouch.imgaug import ColorJitterParams
    m = make_model(64)
    frames = _frames()
    jit = [ColorJitterParams((1, 0, 3, 2), 1.2, 0.8, 1.3, 0.02), None, None, ColorJitterParams((3, 2, 1, 0), 0.9, 1.3, 0.7, -0.03), None, None]
    got = m.preprocess_images_device(frames, area=T, jitter=jit).clone()
    assert torch.equal(got, m.preprocess_images_device(_resized(frames), jitter=jit))
    cor = [None, None, _corrupt(1), None, _corrupt(2), None]
    got = m.preprocess_images_device(frames, area=T, jitter=jit, corrupt=cor).clone()
    assert torch.equal(got, m.preprocess_images_device(_resized(frames), jitter=jit, corrupt=cor))
    with pytest.raises(Exception):
        m.preprocess_images_device(frames, area=T, jitter=[None, jit[0], None, None, None, None])      # on the missing frame


def _corrupt(seed):
    from vlatouch.imgaug import draw_image_corrupt
    return draw_image_corrupt(np.random.default_rng(seed))


def test_without_area_the_call_is_todays():
    from tests.test_gpu_imgprep import as_pil, make_model
    m = make_model(64)
    frames = _frames()
    ref = m.preprocess_images(as_pil([f.cpu().numpy() if isinstance(f, torch.Tensor) else f for f in frames])).to(DEV, m.dtype)
    a = m.preprocess_images_device(frames).clone()
    m.preprocess_images_device(frames, area=T)                               # a resized call in between leaves the plain plan alone
    b = m.preprocess_images_device(frames, area=None)
    assert torch.equal(a, ref) and torch.equal(b, ref)


def test_graph_capture_of_an_area_only_call():
    """The resized call is as capturable as the plain one: records and tap tables are cached with the plan."""
    from tests.test_gpu_imgprep import make_model
    g = np.random.default_rng(12)
    m = make_model(64)
    shapes = [(30, 40), (96, 96)]
    static = [torch.from_numpy(g.integers(0, 256, (*s, 3), dtype=np.uint8)).to(DEV) for s in shapes]
    frames = [static[0], None, static[1]]
    out = torch.empty(3, 3, 64, 64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.preprocess_images_device(frames, out=out, area=T)                  # warm-up: tables, plan, workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.preprocess_images_device(frames, out=out, area=T)
    for rep in range(2):
        new = [g.integers(0, 256, (*sh, 3), dtype=np.uint8) for sh in shapes]
        for t, a in zip(static, new):
            t.copy_(torch.from_numpy(a))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ref = m.preprocess_images_device(_resized([new[0], None, new[1]]))
        assert torch.equal(out, ref), rep


# ---- through the model and the labeller

def test_step_with_pad_and_resize_on_the_device_and_through_the_statement():
    from tests.test_gpu_imgprep import _tower_model
    from tests.test_siglip import _pil_frames
    on, off = _tower_model(True), _tower_model(False)
    off.policy = on.policy
    S = on.image_processor.size["height"]                                    # 56: every frame of _pil_frames has a side of at least 56
    raws = [None if f is None else np.asarray(f) for f in _pil_frames()]
    px_on = on.preprocess_images_device(raws, area=S).clone()
    from vlatouch.imgprep import pad_and_resize_pil
    px_off = off.preprocess_images(pad_and_resize_pil(_pil_frames(), S)).to(DEV, off.dtype)
    assert torch.equal(px_on, px_off) and not torch.equal(px_on, on.preprocess_images_device(raws))
    g = torch.Generator().manual_seed(3)
    proprio, text = torch.randn(1, 10, generator=g), torch.randn(1, 12, 96, generator=g)
    torch.manual_seed(11)
    a = on.step(proprio, _pil_frames(), text, pad_and_resize=True)
    torch.manual_seed(11)
    b = off.step(proprio, _pil_frames(), text, pad_and_resize=True)
    torch.manual_seed(11)
    c = on.step(proprio, pad_and_resize_pil(_pil_frames(), S), text)
    torch.manual_seed(11)
    d = on.step(proprio, _pil_frames(), text, pad_and_resize=S, jpeg_mapping=True)
    torch.manual_seed(11)
    e = off.step(proprio, _pil_frames(), text, pad_and_resize=S, jpeg_mapping=True)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c) and torch.equal(d, e)


def _tower28(device_preprocess):
    """A two-layer tower of 28 x 28 pixels (2 x 2 patches), so that `pad_and_resize=True` reduces 30 x 40 frames."""
    from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    from tests.test_siglip import ARGS
    c = dict(synth.SIGLIP_CONFIGS["tiny"], image_size=28)
    cfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"], image_size=28,
               patch_size=14)
    tower = SiglipVisionTower("synthetic", None, device=DEV, precision="fp32", state_dict=cases.sd_torch(synth.siglip_shapes(**c), prefix="siglip-tiny28."),
                              config=cfg)
    return RoboticDiffusionTransformerModel(copy.deepcopy(ARGS), device=DEV, dtype=torch.float32, control_frequency=10, vision_model=tower,
                                            device_preprocess=device_preprocess)


def test_label_episode_from_raw_frames():
    from vlatouch.imgprep import pad_and_resize_for_siglip
    from vlatouch.label import label_episode
    on, off = _tower28(True), _tower28(False)
    off.policy = on.policy
    g = np.random.default_rng(21)
    N = 6
    cam1, cam2 = g.integers(0, 256, (N, 30, 40, 3), dtype=np.uint8), g.integers(0, 256, (N, 30, 40, 3), dtype=np.uint8)
    qpos = g.standard_normal((N, 10)).astype(np.float32)
    qpos[:, 9] = g.uniform(0, 255, N)
    text = torch.from_numpy(g.standard_normal((1, 12, 96)).astype(np.float32))
    noise = torch.from_numpy(g.standard_normal((N, 8, 128)).astype(np.float32))
    kw = dict(batch=4, noise=noise, encode_batch=4)
    act, r1, r2 = label_episode(on, cam1, cam2, qpos, text, pad_and_resize=True, return_resized=True, **kw)
    w1, w2 = pad_and_resize_for_siglip(cam1, 28), pad_and_resize_for_siglip(cam2, 28)
    same(r1, w1, "camera1_resized")
    same(r2, w2, "camera2_resized")
    assert act.shape == (N, 8, 10) and np.isfinite(act).all()
    assert np.array_equal(act, label_episode(on, w1, w2, qpos, text, **kw))                       # labelling the pre-resized frames
    assert np.array_equal(act, label_episode(on, cam1, cam2, qpos, text, pad_and_resize=True, **kw))
    act_off, o1, o2 = label_episode(off, cam1, cam2, qpos, text, pad_and_resize=True, return_resized=True, **kw)
    same(o1, w1, "camera1_resized, CPU route")
    assert np.array_equal(act, act_off) and np.array_equal(o2, w2)
    with pytest.raises(ValueError):
        label_episode(on, cam1, cam2, qpos, text, return_resized=True, **kw)


def test_labelled_episode_file_holds_the_resized_cameras(tmp_path):
    """raw camera1/camera1 frames -> label_episode -> write_labelled_episode: the reference labeller's file, `camera*_resized` included."""
    from tests import rdt_data_ref as R
    from vlatouch import convert
    from vlatouch.imgprep import pad_and_resize_for_siglip
    from vlatouch.label import label_episode
    from vlatouch.rdt_data import episode_qpos
    m = _tower28(True)
    src = os.path.join(R.FIXTURE_DIR, "episode_10.h5")
    tree = convert.read_tree(src)
    N = 6
    g = np.random.default_rng(4)
    tree = {k: (np.asarray(v)[:N] if k in ("ee_poses", "gripper_pos") else v) for k, v in tree.items()}
    tree["camera1"] = {"camera1": g.integers(0, 256, (N, 30, 40, 3), dtype=np.uint8)}
    tree["camera2"] = {"camera2": g.integers(0, 256, (N, 40, 30, 3), dtype=np.uint8)}
    from vlatouch import h5lite
    raw_path, out_path = str(tmp_path / "episode_1.h5"), str(tmp_path / "out" / "episode_1.h5")
    h5lite.write_file(raw_path, tree)
    t = convert.read_tree(raw_path)
    c1, c2 = np.asarray(t["camera1"]["camera1"]), np.asarray(t["camera2"]["camera2"])
    qpos = episode_qpos(t["ee_poses"], t["gripper_pos"]).astype(np.float32)
    text = torch.from_numpy(np.asarray(t["instruct_embeddings"])[:1, :, :96].astype(np.float32))
    act, r1, r2 = label_episode(m, c1, c2, qpos, text, batch=4, pad_and_resize=True, return_resized=True)
    convert.write_labelled_episode(raw_path, out_path, act, r1, r2)
    back = convert.read_tree(out_path)
    same(np.asarray(back["camera1_resized"]), pad_and_resize_for_siglip(c1, 28), "camera1_resized")
    same(np.asarray(back["camera2_resized"]), pad_and_resize_for_siglip(c2, 28), "camera2_resized")
    assert np.array_equal(np.asarray(back["vla_action"]), act) and np.array_equal(np.asarray(back["camera1"]["camera1"]), c1)


# ---- through the store

@pytest.fixture(scope="module")
def episode_dir(tmp_path_factory):
    """The fixture episodes with their 12 x 16 cameras replaced by random 30 x 40 (camera1) and 40 x 30 (camera2) frames: large enough to
    be reduced to 24 x 24.  Everything else, and so every draw, is the fixture's."""
    from tests import rdt_data_ref as R
    from vlatouch import convert, h5lite
    d = tmp_path_factory.mktemp("episodes30x40")
    g = np.random.default_rng(77)
    for name in sorted(os.listdir(R.FIXTURE_DIR)):
        if not name.endswith(".h5"):
            continue
        tree = convert.read_tree(os.path.join(R.FIXTURE_DIR, name))
        n = len(np.asarray(tree["ee_poses"]))
        for cam, (h, w) in (("camera1", (30, 40)), ("camera2", (40, 30))):
            if cam in tree:
                tree[cam] = {cam: g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)}
        h5lite.write_file(str(d / name), tree)
    return str(d)


def _store(path, **kw):
    from tests import rdt_data_ref as R
    from vlatouch.rdt_data import EpisodeStore
    args = dict(dataset_name=R.DATASET_NAME, dataset_names=R.DATASET_NAMES, control_freq=R.CONTROL_FREQ, device=DEV)
    args.update(kw)
    return EpisodeStore(path, **args)


def test_store_keeps_resized_frames(episode_dir):
    from tests import rdt_data_ref as R
    from tests.test_gpu_rdt_data import _tower_and_preprocessor
    from vlatouch.imgprep import pad_and_resize_for_siglip
    from vlatouch.rdt_train import prepare_batch
    rawst, small = _store(episode_dir).upload(), _store(episode_dir, pad_and_resize=T).upload()
    assert rawst.dataset_stat() == small.dataset_stat() == _store(R.FIXTURE_DIR).dataset_stat()
    steps = sum(e.qpos.shape[0] for e in small.episodes)
    assert rawst.resident_bytes - small.resident_bytes == 2 * steps * 3 * (30 * 40 - T * T) and small.host_frame_bytes == 0
    draw = dict(cond_mask_prob=0.3, image_aug=True, image_corrupt=True)
    rngs = lambda: dict(np_rng=np.random.RandomState(3), rng=random.Random(3), generator=torch.Generator().manual_seed(3),
                        corrupt_rng=np.random.default_rng(3))
    plans = rawst.draw(6, **rngs(), **draw)
    again = small.draw(6, **rngs(), **draw)
    assert [(p.episode, p.step_id, p.frame_idx, p.frame_valid) for p in plans] == [(p.episode, p.step_id, p.frame_idx, p.frame_valid) for p in again]
    a, b = rawst.assemble(plans), small.assemble(plans)
    seen = 0
    for fa, fb in zip(a["frames"], b["frames"]):
        for x, y in zip(fa, fb):
            assert (x is None) == (y is None)
            if x is not None:
                assert y.is_cuda and tuple(y.shape) == (T, T, 3)
                same(y, pad_and_resize_for_siglip(x.cpu().numpy(), T), "a resident frame")
                seen += 1
    assert seen >= 8 and any(j is not None for s in b["jitter"] for j in s) and any(c is not None for s in b["corrupt"] for c in s)
    tower, pp = _tower_and_preprocessor()
    ka = prepare_batch(a, vision_encoder=tower, preprocessor=lambda flat, **kw: pp(flat, area=T, **kw))
    kb = prepare_batch(b, vision_encoder=tower, preprocessor=pp)
    assert torch.equal(ka["img_tokens"], kb["img_tokens"]) and torch.equal(ka["action_gt"], kb["action_gt"])
    # a cap that splits the episodes between the device and pinned host memory counts the resized size and changes no batch
    first = 2 * small.episodes[0].qpos.shape[0] * 3 * T * T
    split = _store(episode_dir, pad_and_resize=T, max_device_bytes=first + 100).upload()
    assert split.host_frame_bytes == 2 * steps * 3 * T * T - first and small.resident_bytes - split.resident_bytes == split.host_frame_bytes
    assert {p.episode for p in plans} > {0}
    c = split.assemble(plans)
    for p, fb, fc in zip(plans, b["frames"], c["frames"]):
        for y, z in zip(fb, fc):
            assert (y is None) == (z is None)
            if y is not None:
                assert (isinstance(z, torch.Tensor) and z.is_cuda) == (p.episode == 0)
                same(z if isinstance(z, torch.Tensor) else np.asarray(z), y.cpu().numpy(), "a frame of the split store")
    kc = prepare_batch(c, vision_encoder=tower, preprocessor=pp)
    assert torch.equal(kc["img_tokens"], kb["img_tokens"])


def test_store_on_the_fixture_episodes_and_its_refusal():
    """The committed 12 x 16 episodes: reduced to 10 x 10 (a fractional scale with a pad of 2 rows); a target of 24 is larger than the
    frames and is refused when the store is built, by name."""
    from tests import rdt_data_ref as R
    from vlatouch.imgprep import pad_and_resize_for_siglip
    with pytest.raises(ValueError, match="up-scale emulation is not built"):
        _store(R.FIXTURE_DIR, pad_and_resize=T)
    rawst, small = _store(R.FIXTURE_DIR), _store(R.FIXTURE_DIR, pad_and_resize=10)
    plans = rawst.draw(4, np_rng=np.random.RandomState(1), rng=random.Random(1), cond_mask_prob=0.0)
    a, b = rawst.assemble(plans), small.assemble(plans)
    for fa, fb in zip(a["frames"], b["frames"]):
        for x, y in zip(fa, fb):
            assert (x is None) == (y is None)
            if x is not None:
                same(y, pad_and_resize_for_siglip(x.cpu().numpy(), 10), "a fixture frame")
    assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["states"], b["states"])
