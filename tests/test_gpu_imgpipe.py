"""The camera-frame chain as a list of stages (vlatouch/imgprep.py): every subset of JPEG map, pre-resize, colour jitter and the main pass gives
the bits of the composition of calls that tests/test_gpu_jpegmap.py, test_gpu_colorjitter.py and test_gpu_imgprep.py pin to PIL one by one,
inside exactly the buffers it asked for; a call with three cached stages replays from a graph; the frame stager stands without a
preprocessor; and the workspace every combination asks for is, byte for byte, what the planner of the commit before asked for
(tests/golden/g26_imgpipe_ws_parent.json, written by tools/make_golden_imgpipe_ws_parent.py and never regenerated to make this pass)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import imgpipe_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def cpu_mapped(quality):
    """`jpeg_mapping` on the CPU of every frame of the grid that exists, once per quality (host arrays, read-only)."""
    from vlatouch.jpegmap import jpeg_mapping
    out = []
    for f in K.frames(DEV)[0]:
        a = None if f is None else jpeg_mapping(f.cpu().numpy() if isinstance(f, torch.Tensor) else f, quality)
        if a is not None:
            a.setflags(write=False)
        out.append(a)
    return out


@pytest.mark.parametrize("combo", K.COMBOS, ids=K.combo_id)
def test_every_subset_of_stages_equals_the_composition_inside_its_buffers(combo):
    jpeg, image_size, jit, force = combo
    frames, in_place = K.frames(DEV)
    jitter = K.jitter_list() if jit else None
    pp = K.preprocessor(image_size, DEV, force)
    n, nws = len(frames), pp.workspace_bytes(frames, jitter, jpeg)
    nout = n * 3 * K.S * K.S
    ws = torch.full((nws + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    buf = torch.full((nout + 64,), -777.0, dtype=torch.float32, device=DEV)
    got = pp(frames, out=buf[:nout].view(n, 3, K.S, K.S), workspace=ws[:nws], jitter=jitter, jpeg=jpeg)
    # the composition: the mapping on the CPU, then the same preprocessor without jpeg=, on buffers of its own
    want = pp(frames if jpeg is None else [None if a is None else np.array(a) for a in cpu_mapped(jpeg)], jitter=jitter)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and torch.equal(got, want)
    assert bool((buf[nout:] == -777.0).all()) and bool((ws[nws:] == 0xA5).all())
    for t, a in in_place:
        assert np.array_equal(t.cpu().numpy(), a)                          # the frames used in place are untouched
    if force:                                                               # and the two-launch form gives the fused form's bits
        assert torch.equal(got, K.preprocessor(image_size, DEV)(frames, jitter=jitter, jpeg=jpeg))


def test_graph_capture_with_three_cached_stages():
    """JPEG map, pre-resize and main pass, one frame missing: tables cached with the plan, nothing allocated, copied or awaited per call, so one
    capture replays on new frame contents."""
    from tests.test_gpu_imgprep import make_model
    from vlatouch.jpegmap import jpeg_mapping
    g = np.random.default_rng(13)
    m = make_model(64, image_size=40)
    shapes = [(48, 64), (30, 50)]
    static = [torch.from_numpy(g.integers(0, 256, (*s, 3), dtype=np.uint8)).to(DEV) for s in shapes]
    frames = [static[0], None, static[1]]
    out = torch.empty(3, 3, 64, 64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.preprocess_images_device(frames, out=out, jpeg=95)              # warm-up: tables, plan, workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.preprocess_images_device(frames, out=out, jpeg=95)
    for rep in range(2):
        new = [g.integers(0, 256, (*sh, 3), dtype=np.uint8) for sh in shapes]
        for t, a in zip(static, new):
            t.copy_(torch.from_numpy(a))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ref = m.preprocess_images_device([jpeg_mapping(new[0]), None, jpeg_mapping(new[1])])
        assert torch.equal(out, ref), rep


def test_jpeg_mapping_device_builds_no_preprocessor(monkeypatch):
    """The input kinds of test_every_input_kind_gives_the_bits_of_the_contiguous_frame, through a new stager, with the preprocessor's
    constructor out of reach."""
    from PIL import Image
    from tests import jpeg_ref as J
    from vlatouch import imgprep, jpegmap

    def refuse(self, *a, **k):
        raise AssertionError("jpeg_mapping_device constructed a DevicePreprocessor")
    monkeypatch.setattr(imgprep.DevicePreprocessor, "__init__", refuse)
    monkeypatch.setattr(jpegmap, "_stagers", {})
    a = J.make_frame("noise", 19, 21)
    ref = J.jpeg_roundtrip(a, 95, "cv2")
    wide = torch.full((19, 40, 3), 77, dtype=torch.uint8, device=DEV)
    wide[:, 5:26] = torch.from_numpy(a).to(DEV)
    got = jpegmap.jpeg_mapping_device([wide[:, 5:26], Image.fromarray(a), a, torch.from_numpy(a), torch.from_numpy(a).to(DEV)], 95, "cv2")
    for k, t in enumerate(got):
        assert np.array_equal(t.cpu().numpy(), ref), f"input kind {k}"
    assert [type(s) for s in jpegmap._stagers.values()] == [imgprep.FrameStager]


def test_workspace_sizes_are_the_parents():
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        want = json.load(f)["bytes"]
    got = K.workspace_sizes(DEV)
    assert list(got) == list(want)
    diff = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
