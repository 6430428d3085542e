"""The frame corruption on the device (csrc/vt_corrupt.hip, vlatouch/imgaug.py image_corrupt_device, vlatouch/imgprep.py `corrupt=`,
vlatouch/rdt_train.py prepare_batch) against its numpy statement (tests/corrupt_ref.py): every comparison is for equal bits.  Outputs go
into buffers pre-filled with a sentinel; the pad bytes between frames and after the last frame must keep it.

Sizes: 1 x 1 and 1 x 40 (one row), 3 x 50 (the blur radius exceeds a side: the reflection is periodic), 33 x 65 and 70 x 45 (straddle the
32 x 32 tile in both directions, several workgroups), a pitched view at an odd address."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import corrupt_ref as R
from tests import imgaug_ref as J
from vlatouch import imgaug as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5
VT_ERR_ARG = -22
SIZES = [(1, 1), (1, 40), (3, 50), (33, 65), (70, 45)]


def rand_frame(g, h, w, scale=1.0):
    return (g.random((h, w, 3)) * 256 * scale).astype(np.uint8)


def blurs():
    out = [dict(blur="gaussian", sigma=s) for s in (0.5, 2.0, 2.9)]                     # ksize 5, 7, 9
    out += [dict(blur="average", k=k) for k in range(2, 8)]
    out += [dict(blur="median", k=k) for k in (3, 5, 7, 9, 11)]
    out += [dict(blur="motion", k=k, angle=a, direction=d) for k, d in ((3, 0.0), (17, 0.5), (37, -0.8)) for a in (0.0, 37.0, 90.0)]
    return out


def all_params():
    """Every noise kind per channel and shared; every blur with noise first, with blur first, and alone."""
    noises = [dict(noise=kind, scale=s, per_channel=pc) for kind, s in (("gaussian", 9.0), ("laplace", 6.0), ("poisson", 11.5)) for pc in (True, False)]
    ps = [A.CorruptParams(True, key=1000 + i, **n) for i, n in enumerate(noises)]
    for i, b in enumerate(blurs()):
        n = noises[i % len(noises)]
        ps.append(A.CorruptParams(True, key=(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64), **n, **b))
        ps.append(A.CorruptParams(False, key=(0xC2B2AE3D27D4EB4F * (i + 1)) % (1 << 64), **n, **b))
        ps.append(A.CorruptParams(True, **b))
    return ps


def records(frames, params, odd_offsets=True):
    from vlatouch import _lib
    n = len(frames)
    arr = (_lib.CorruptFrame * n)()
    off, spans = 0, []
    for i, t in enumerate(frames):
        h, w = int(t.shape[0]), int(t.shape[1])
        assert t.is_cuda and t.dtype == torch.uint8 and t.stride(2) == 1 and t.stride(1) == 3
        f = arr[i]
        f.src, f.pitch, f.h, f.w = t.data_ptr(), (int(t.stride(0)) if h > 1 else 3 * w), h, w
        f.out_off = off + (i % 3 if odd_offsets else 0)                               # tight rows start at every alignment
        spans.append((f.out_off, h, w))
        off = (f.out_off + 3 * h * w + 15) // 16 * 16 + 16
    return arr, A.pack_corrupt(arr, params), spans, off


def run(frames, params):
    """vt_corrupt on device frames -> the per-frame outputs as numpy; pads and the tail keep the sentinel."""
    from vlatouch import _lib
    arr, words, spans, total = records(frames, params)
    out = torch.full((total + 64,), SENT, dtype=torch.uint8, device=DEV)
    dev = torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(DEV)
    tdev = torch.from_numpy(np.concatenate([words, np.zeros(1, dtype=np.uint32)]).view(np.uint8).copy()).to(DEV)
    _lib.check(_lib.lib().vt_corrupt(arr, _lib.ptr(dev), len(frames), words.ctypes.data, _lib.ptr(tdev), words.size, _lib.ptr(out), _lib.stream_ptr(DEV)),
               "vt_corrupt")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    res = []
    for o, h, w in spans:
        res.append(host[o:o + 3 * h * w].reshape(h, w, 3))
        keep[o:o + 3 * h * w] = False
    assert (host[keep] == SENT).all(), "a byte outside the frames was written"
    return res


def check(frames_host, params, frames_dev=None):
    dev = frames_dev if frames_dev is not None else [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in frames_host]
    got = run(dev, params)
    bad = []
    for i, (a, p, g) in enumerate(zip(frames_host, params, got)):
        want = R.image_corrupt_np(a, p)
        if not np.array_equal(g, want):
            bad.append((i, a.shape[:2], p, int((g != want).any(axis=-1).sum()), int(np.abs(g.astype(int) - want.astype(int)).max())))
    assert not bad, f"{len(bad)} frames differ from the statement (index, size, params, pixels, largest difference): {bad[:4]}"
    return got


# ------------------------------------------------------------------------------------------------ 1. every operation at every size
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_every_operation(h, w):
    ps = all_params()
    assert len(ps) == 6 + 3 * 23
    g = np.random.default_rng(100 * h + w)
    frames = [rand_frame(g, h, w, 0.3 if i % 5 == 0 else 1.0) for i in range(len(ps))]
    got = check(frames, ps)
    changed = sum(not np.array_equal(a, b) for a, b in zip(frames, got))
    assert changed >= len(ps) // 2                                                     # 1 x 1: a blur alone changes nothing


def test_order_matters_and_copy():
    g = np.random.default_rng(7)
    a = rand_frame(g, 40, 40)
    kw = dict(noise="gaussian", scale=10.0, per_channel=True, key=5, blur="average", k=5)
    got = check([a, a, a], [A.CorruptParams(True, **kw), A.CorruptParams(False, **kw), None])
    assert not np.array_equal(got[0], got[1]) and np.array_equal(got[2], a)


# ------------------------------------------------------------------------------------------------ 2. different frames in one call
def test_mixed_sizes_operations_and_a_pitched_view_in_one_call():
    g = np.random.default_rng(3)
    crng = np.random.default_rng(33)
    frames, params = [], []
    for h, w in SIZES + [(64, 64), (32, 32), (31, 96), (100, 7)]:
        frames.append(rand_frame(g, h, w))
        params.append(A.draw_image_corrupt(crng))
    frames.append(rand_frame(g, 20, 20)); params.append(None)
    dev = [torch.from_numpy(a).to(DEV) for a in frames]
    big_host = rand_frame(g, 60, 100)
    big = torch.from_numpy(big_host).to(DEV)
    for view, hv, p in ((big[5:50, 11:81, :], big_host[5:50, 11:81, :], A.CorruptParams(True, "poisson", 8.0, True, 99, blur="motion", k=37, angle=120.0, direction=0.3)),
                        (big[2:40, 8:72, :], big_host[2:40, 8:72, :], A.CorruptParams(False, "laplace", 5.0, False, 98, blur="median", k=11))):
        assert not view.is_contiguous()
        frames.append(np.ascontiguousarray(hv)); dev.append(view); params.append(p)
    assert dev[-2].data_ptr() % 2 == 1
    assert len({p.blur for p in params if p is not None}) >= 3
    got = check(frames, params, frames_dev=dev)
    again = run(dev, params)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls must agree bit for bit"
    assert np.array_equal(big.cpu().numpy(), big_host)                                # the frame read in place is untouched


def test_image_corrupt_device_takes_every_kind_of_frame():
    from PIL import Image
    g = np.random.default_rng(4)
    host = [rand_frame(g, 48, 64), rand_frame(g, 33, 20), None, rand_frame(g, 50, 50), rand_frame(g, 10, 10)]
    frames = [host[0], Image.fromarray(host[1]), None, torch.from_numpy(host[3]).to(DEV), torch.from_numpy(host[4])]
    crng = np.random.default_rng(44)
    params = [A.draw_image_corrupt(crng), A.draw_image_corrupt(crng), None, A.draw_image_corrupt(crng), None]
    got = A.image_corrupt_device(frames, params, device=DEV)
    torch.cuda.synchronize()
    assert got[2] is None
    for a, p, t in zip(host, params, got):
        if a is not None:
            assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), R.image_corrupt_np(a, p))
    from vlatouch import _lib
    with pytest.raises(_lib.VtError, match="missing frame"):
        A.image_corrupt_device(frames, [None, None, params[0], None, None], device=DEV)


# ------------------------------------------------------------------------------------------------ 3. argument errors
def test_argument_errors_leave_the_output_untouched():
    from tests.test_corrupt_host import bad_calls, full_params
    from vlatouch import _lib
    L = _lib.lib()
    src = torch.zeros(6, 8, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), SENT, dtype=torch.uint8, device=DEV)
    for what, mutate in bad_calls():
        arr, words, _, _ = records([src], [full_params()], odd_offsets=False)
        new = mutate(arr[0], words)
        words = words if new is None else new
        dev = torch.from_numpy(np.frombuffer(bytes(memoryview(arr)), dtype=np.uint8).copy()).to(DEV)
        tdev = torch.from_numpy(words.view(np.uint8).copy()).to(DEV)
        code = L.vt_corrupt(arr, _lib.ptr(dev), 1, words.ctypes.data, _lib.ptr(tdev), words.size, _lib.ptr(out), _lib.stream_ptr(DEV))
        assert code == VT_ERR_ARG, what
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ------------------------------------------------------------------------------------------------ 4. the pipeline
def lift_np(a):
    px = np.asarray(a, dtype=np.float64)
    if px.sum() / (px.shape[0] * px.shape[1] * 255.0 * 3) <= 0.15:
        return np.minimum(255, (a.astype(np.int32) * 7) >> 2).astype(np.uint8)
    return a


def host_chain(a, jitter, corrupt, lift):
    """One frame up to the pad as the dataset orders it: lift, jitter, corruption (None stays None)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if lift:
        a = lift_np(a)
    if jitter is not None:
        a = J.color_jitter_np(a, jitter)
    return R.image_corrupt_np(a, corrupt)


def _pipeline_frames():
    from PIL import Image
    g = np.random.default_rng(12)
    gen = torch.Generator().manual_seed(12)
    crng = np.random.default_rng(12)
    big_host = rand_frame(g, 60, 100)
    big = torch.from_numpy(big_host).to(DEV)
    host = [rand_frame(g, 48, 64), rand_frame(g, 90, 60), None, rand_frame(g, 64, 64), rand_frame(g, 50, 70, 0.2), rand_frame(g, 120, 90),
            big_host[5:50, 11:81, :]]
    frames = [host[0], Image.fromarray(host[1]), None, torch.from_numpy(host[3]).to(DEV), host[4], torch.from_numpy(host[5]).to(DEV), big[5:50, 11:81, :]]
    jitter = [A.color_jitter_params(generator=gen), None, None, None, A.color_jitter_params(generator=gen), A.color_jitter_params(generator=gen), None]
    corrupt = [A.draw_image_corrupt(crng), A.draw_image_corrupt(crng), None, None, A.CorruptParams(False, "gaussian", 7.0, True, 6, blur="median", k=5),
               None, A.CorruptParams(True, "poisson", 9.0, False, 7, blur="motion", k=21, angle=77.0, direction=-0.4)]
    return host, frames, jitter, corrupt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pipeline_equals_the_plain_call_on_corrupted_frames(dtype):
    from vlatouch.imgprep import DevicePreprocessor
    S = 64
    mean = std = [0.5, 0.5, 0.5]
    host, frames, jitter, corrupt = _pipeline_frames()
    n = len(frames)
    plain = DevicePreprocessor(S, mean, std, DEV, dtype, pad=True, brightness=False)
    lifting = DevicePreprocessor(S, mean, std, DEV, dtype, pad=True, brightness=True)
    assert not np.array_equal(lift_np(host[4]), host[4])                              # the dark frame is lifted
    for name, pp, jit, lift in (("corrupt", plain, None, False), ("jitter, corrupt", plain, jitter, False), ("lift, corrupt", lifting, None, True),
                                ("lift, jitter, corrupt", lifting, jitter, True)):
        jl = jit if jit is not None else [None] * n
        want = plain([host_chain(a, j, c, lift) for a, j, c in zip(host, jl, corrupt)])
        base = plain([host_chain(a, j, None, lift) for a, j in zip(host, jl)])
        assert not torch.equal(want, base)
        nws, nout = pp.workspace_bytes(frames, jitter=jit, corrupt=corrupt), n * 3 * S * S
        assert nws > pp.workspace_bytes(frames, jitter=jit)
        ws = torch.full((nws + 256,), SENT, dtype=torch.uint8, device=DEV)
        buf = torch.full((nout + 64,), -777.0, dtype=dtype, device=DEV)
        got = pp(frames, out=buf[:nout].view(n, 3, S, S), workspace=ws[:nws], jitter=jit, corrupt=corrupt)
        torch.cuda.synchronize()
        bad = (got != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"{name}: frames {bad} differ from the plain call on the statement's frames"
        assert bool((buf[nout:] == -777.0).all()) and bool((ws[nws:] == SENT).all()), name
        assert torch.equal(pp(frames, jitter=jit, corrupt=corrupt), want), name          # the preprocessor's own workspace, a second call
        # no corruption at all: the call without the argument
        assert torch.equal(pp(frames, jitter=jit, corrupt=[None] * n), pp(frames, jitter=jit)), name
        assert torch.equal(pp(frames, jitter=jit), base), name


def test_pipeline_with_a_pre_resize_and_the_model_wrapper():
    from PIL import Image
    from tests.test_gpu_imgprep import make_model
    from vlatouch import _lib
    host, frames, jitter, corrupt = _pipeline_frames()
    m = make_model(64, image_size=(40, 72))
    resized = [None if a is None else np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((72, 40), resample=Image.BILINEAR)) for a in host]
    ref = make_model(64, auto_adjust_image_brightness=False)
    want = ref.preprocess_images_device([host_chain(a, j, c, True) for a, j, c in zip(resized, jitter, corrupt)])
    assert torch.equal(m.preprocess_images_device(frames, jitter=jitter, corrupt=corrupt), want)
    p = corrupt[0]
    with pytest.raises(_lib.VtError, match="missing frame"):
        m.preprocess_images_device(frames, corrupt=[None, None, p, None, None, None, None])
    with pytest.raises(_lib.VtError, match="entries"):
        m.preprocess_images_device(frames, corrupt=[p])
    with pytest.raises(_lib.VtError, match="CorruptParams"):
        m.preprocess_images_device(frames, corrupt=[0.5] + [None] * 6)


def test_a_corrupting_call_under_stream_capture_raises():
    from vlatouch import _lib
    from vlatouch.imgprep import DevicePreprocessor
    g = np.random.default_rng(2)
    frames = [torch.from_numpy(rand_frame(g, 48, 64)).to(DEV)]
    corrupt = [A.CorruptParams(True, "gaussian", 3.0, key=1)]
    pp = DevicePreprocessor(64, [0.5] * 3, [0.5] * 3, DEV, torch.float32)
    out = torch.empty(1, 3, 64, 64, device=DEV)
    pp(frames, out=out, corrupt=corrupt)
    pp(frames, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pp(frames, out=out)                                                           # the plain call is capturable, as before
        with pytest.raises(_lib.VtError, match="corrupt= cannot be captured"):
            pp(frames, out=out, corrupt=corrupt)
    want = out.clone()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ 5. the loop
def test_prepare_batch_on_a_store_batch_equals_the_cpu_corrupted_batch():
    import random
    from tests.test_gpu_rdt_data import _store, _tower_and_preprocessor
    from vlatouch.imgprep import DevicePreprocessor
    from vlatouch.rdt_train import prepare_batch
    tower, pp = _tower_and_preprocessor()
    plain = DevicePreprocessor(pp.S, [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], DEV, torch.float32, pad=True, brightness=False, image_size=None)
    store = _store(horizon=cases.RDT_TINY["horizon"])
    it = store.batches(2, np_rng=np.random.RandomState(6), rng=random.Random(6), generator=torch.Generator().manual_seed(6), cond_mask_prob=0.3,
                       image_aug=True, image_corrupt=True, corrupt_rng=np.random.default_rng(6))
    seen = 0
    for _ in range(3):
        b = next(it)
        if "corrupt" not in b:
            continue
        seen += sum(c is not None for s in b["corrupt"] for c in s)
        got = prepare_batch(b, vision_encoder=tower, preprocessor=pp)["img_tokens"]
        jit = b["jitter"] if b["jitter"] is not None else [[None] * len(s) for s in b["frames"]]
        frames = [[host_chain(None if f is None else (f.cpu().numpy() if isinstance(f, torch.Tensor) else f), j, c, True) for f, j, c in zip(fs, js, cs)]
                  for fs, js, cs in zip(b["frames"], jit, b["corrupt"])]
        b2 = {k: v for k, v in b.items() if k not in ("jitter", "corrupt")}
        b2["frames"] = frames
        want = prepare_batch(b2, vision_encoder=tower, preprocessor=plain)["img_tokens"]
        assert torch.equal(got, want)
        without = prepare_batch({k: v for k, v in b.items() if k != "corrupt"}, vision_encoder=tower, preprocessor=pp)["img_tokens"]
        assert not torch.equal(got, without)
    assert seen > 0
