"""CPU-only checks of the colour augmentation's host side: the numpy statement of the arithmetic (tests/imgaug_ref.py, what
csrc/vt_colorjitter.hip restates) against PIL bit for bit, the parameter draws of vlatouch/imgaug.py against their stated draw sequence
and the reference's loop, the conversion to the C record, the C entry point's argument checks (no launch happens), and the training
loop's handling of the collator's batches (vlatouch/rdt_train.py: prepare_batch, finetune) with stand-in encoders and a stub trainer."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import imgaug_ref as R


def _params(order=(0, 1, 2, 3), **kw):
    from vlatouch.imgaug import ColorJitterParams
    return ColorJitterParams(order, **kw)


def _same(arr, p):
    from PIL import Image
    want = np.asarray(R.color_jitter_pil(Image.fromarray(arr), p))
    got = R.color_jitter_np(arr, p)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = int((got != want).any(axis=-1).sum())
    assert bad == 0, f"{bad} pixels differ for {p}"


@pytest.fixture(scope="module")
def colours():
    return R.all_colours()


# ------------------------------------------------------------------------------------------------ 1. the numpy statement is PIL's arithmetic
@pytest.mark.parametrize("shift", [7, 128, 249])
def test_hue_on_all_colours(colours, shift):
    from PIL import Image
    want = np.asarray(R.hue_pil(Image.fromarray(colours), shift))
    got = R.hue_np(colours, shift)
    bad = int((got != want).any(axis=-1).sum())
    assert bad == 0, f"{bad} of 2^24 colours differ"


def test_saturation_on_all_colours(colours):
    drawn = float(torch.empty(1).uniform_(0.5, 1.5, generator=torch.Generator().manual_seed(3)))
    for f in (0.5, 1.5, drawn):
        _same(colours, _params(saturation=f))


def test_brightness_on_all_bytes():
    arr = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=-1)
    for f in (0.7, 1.0, 1.3, 1.75):
        _same(arr, _params(brightness=f))
    lifted = R.color_jitter_np(arr, _params(brightness=1.75))
    assert np.array_equal(lifted[..., 0].reshape(-1), np.minimum(255, (np.arange(256) * 7) >> 2))        # the existing lift8


def test_contrast_on_ramp_frames():
    means = set()
    for m in range(256):
        arr = R.ramp_frame(m)
        means.add(R.contrast_mean_np(arr))
        for f in (0.6, 1.4):
            _same(arr, _params(contrast=f))
    assert min(means) <= 2 and max(means) >= 252 and len(means) >= 250            # the rounded mean sweeps the byte range
    for arr in R.half_mean_frames():
        for f in (0.6, 1.4):
            _same(arr, _params(contrast=f))
    a, b, c = R.half_mean_frames()
    assert (R.contrast_mean_np(a), R.contrast_mean_np(b), R.contrast_mean_np(c)) == (11, 101, 100)       # x.5 rounds up, x.25 down


def test_all_orders_on_a_random_frame():
    g = np.random.default_rng(0)
    arr = g.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for order in itertools.permutations(range(4)):
        _same(arr, _params(order, brightness=0.83, contrast=1.31, saturation=0.61, hue=-0.021))
        _same(arr, _params(order, brightness=1.27, contrast=0.64, saturation=1.44, hue=0.03))
    _same(arr, _params((2, 0, 3, 1), contrast=1.2, hue=0.01))                      # a subset
    assert np.array_equal(R.color_jitter_np(arr, _params()), arr)                  # the empty one


# ------------------------------------------------------------------------------------------------ 2. color_jitter_params
def test_params_follow_the_stated_draw_sequence():
    from vlatouch.imgaug import color_jitter_params
    p = color_jitter_params(generator=torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    order = torch.randperm(4, generator=g).tolist()
    vals = [float(torch.empty(1).uniform_(lo, hi, generator=g)) for lo, hi in ((0.7, 1.3), (0.6, 1.4), (0.5, 1.5), (-0.03, 0.03))]
    assert list(p.order) == order and [p.brightness, p.contrast, p.saturation, p.hue] == vals
    torch.manual_seed(9)                                                           # no generator: the global one
    q = color_jitter_params()
    torch.manual_seed(9)
    order = torch.randperm(4).tolist()
    b = float(torch.empty(1).uniform_(0.7, 1.3))
    assert list(q.order) == order and q.brightness == b
    # a (lo, hi) pair is taken as given; a strength above 1 clips its lower end at zero
    r = color_jitter_params(brightness=(1.75, 1.75), contrast=1.5, generator=torch.Generator().manual_seed(1))
    assert r.brightness == 1.75 and 0.0 <= r.contrast <= 2.5


def test_params_stay_in_range():
    from vlatouch.imgaug import color_jitter_params
    g = torch.Generator().manual_seed(0)
    orders = set()
    for _ in range(1000):
        p = color_jitter_params(generator=g)
        orders.add(tuple(p.order))
        assert sorted(p.order) == [0, 1, 2, 3]
        assert 0.7 <= p.brightness <= 1.3 and 0.6 <= p.contrast <= 1.4 and 0.5 <= p.saturation <= 1.5 and -0.03 <= p.hue <= 0.03
    assert len(orders) == 24


def test_degenerate_ranges_still_consume_their_draws():
    from vlatouch.imgaug import color_jitter_params
    ga, gb = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
    a = color_jitter_params(generator=ga)
    b = color_jitter_params(brightness=0, hue=0, generator=gb)
    assert b.brightness == 1.0 and b.hue == 0.0
    assert (b.order, b.contrast, b.saturation) == (a.order, a.contrast, a.saturation)
    assert torch.equal(ga.get_state(), gb.get_state())


# ------------------------------------------------------------------------------------------------ 3. draw_image_aug
def _reference_loop(valid, rng, generator):
    """train/dataset.py:386-391, line by line, with ColorJitter's parameter draw in place of its application."""
    from vlatouch.imgaug import color_jitter_params
    chosen = []
    for v in valid:
        params = None
        if v and True and (rng.random() > 0.5):
            aug_type = rng.choice([
                "corrput_only", "color_only", "both"])
            if aug_type != "corrput_only":
                params = color_jitter_params(brightness=0.3, contrast=0.4, saturation=0.5, hue=0.03, generator=generator)
            if aug_type != "color_only":
                pass                                                               # image_corrupt: not built, draws nothing from `random`
        chosen.append(params)
    return chosen


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_draw_image_aug_consumes_the_streams_like_the_reference(seed):
    from vlatouch.imgaug import draw_image_aug
    valid = [bool(v) for v in np.random.default_rng(seed).random(200) > 0.25]
    ra, rb = random.Random(seed), random.Random(seed)
    ga, gb = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
    got, want = draw_image_aug(valid, rng=ra, generator=ga), _reference_loop(valid, rb, gb)
    assert len(got) == 200 and [p is not None for p in got] == [p is not None for p in want]
    assert got == want
    assert all(p is None for p, v in zip(got, valid) if not v)
    assert 20 < sum(p is not None for p in got) < 90                               # about a third of the valid frames
    assert ra.getstate() == rb.getstate() and torch.equal(ga.get_state(), gb.get_state())


# ------------------------------------------------------------------------------------------------ 4. the C record
def test_record_conversion():
    from vlatouch import _lib
    from vlatouch.imgaug import OP_NONE, ColorJitterParams, hue_shift
    assert hue_shift(-0.03) == 249 and hue_shift(0.03) == 7 and hue_shift(0.0) == 0 and hue_shift(0.5) == 127 and hue_shift(-0.5) == 129
    rec =_lib.ColorJitterFrame()
    ColorJitterParams((3, 1, 0, 2), brightness=0.9, contrast=None, saturation=1.25, hue=-0.03).fill_record(rec)
    assert list(rec.order) == [3, OP_NONE, 0, 2]
    assert (rec.brightness, rec.saturation, rec.hue_shift) == (float(np.float32(0.9)), 1.25, 249)
    ColorJitterParams((0, 1, 2, 3)).fill_record(rec)
    assert list(rec.order) == [OP_NONE] * 4
    with pytest.raises(ValueError):
        ColorJitterParams((0, 1, 2, 2))
    with pytest.raises(ValueError):
        ColorJitterParams((0, 1, 2, 3), hue=0.6)


def test_entry_point_rejects_bad_arguments_without_a_launch():
    """n < 1, a null source, an unknown operation id, a repeated one and a short workspace: each fails in the host-side check."""
    from vlatouch import _lib
    from vlatouch.imgaug import OP_NONE
    L = _lib.lib()
    assert L.vt_colorjitter_workspace_bytes(0) == 0 and L.vt_colorjitter_workspace_bytes(3) >= 3 * 3 * 64 * 8

    def table(n=1):
        arr = (_lib.ColorJitterFrame * n)()
        for f in arr:
            f.src, f.pitch, f.h, f.w, f.out_off = 4096, 30, 4, 10, 0
            f.order[:] = [OP_NONE] * 4
        return arr
    fake = C.c_void_p(4096)                                          # never dereferenced: every call below fails before a launch
    ws = L.vt_colorjitter_workspace_bytes(1)

    def call(arr, n=1, flags=0, ws_bytes=ws):
        return L.vt_colorjitter(arr, fake, n, flags, fake, fake, ws_bytes, None)
    cases_ = []
    cases_.append(("n < 1", call(table(), n=0)))
    a = table(); a[0].src = None
    cases_.append(("null source", call(a)))
    a = table(); a[0].order[2] = 7
    cases_.append(("unknown operation", call(a)))
    a = table(); a[0].order[1] = -1
    cases_.append(("unknown operation", call(a)))
    a = table(); a[0].order[0] = a[0].order[3] = 1
    cases_.append(("appears twice", call(a)))
    a = table(); a[0].pitch = 29
    cases_.append(("pitch", call(a)))
    cases_.append(("workspace", call(table(), ws_bytes=ws - 1)))
    cases_.append(("flag", call(table(), flags=2)))
    for what, code in cases_:
        assert code != 0, what
    assert call(table(), ws_bytes=ws - 1) != 0 and b"workspace" in L.vt_last_error()


# ------------------------------------------------------------------------------------------------ 5. the loop takes the collator's batches
class _Vision:
    hidden_size = 5

    def __init__(self):
        self.seen = []

    def __call__(self, x):
        self.seen.append(x)
        return x.reshape(x.shape[0], -1)[:, :10].reshape(x.shape[0], 2, 5).clone().requires_grad_(True)


class _Text:
    def __call__(self, input_ids, attention_mask):
        return {"last_hidden_state": (input_ids.float().unsqueeze(-1) * attention_mask.float().unsqueeze(-1)).requires_grad_(True)}


class _Pre:
    def __init__(self):
        self.calls = []

    def __call__(self, frames, jitter=None):
        self.calls.append((list(frames), jitter))
        return torch.stack([torch.full((3, 2, 2), -1.0 if f is None else float(f)) for f in frames])


def _collator(B=2, N=3, **extra):
    g = torch.Generator().manual_seed(0)
    b = dict(states=torch.randn(B, 2, 8, generator=g), actions=torch.randn(B, 4, 8, generator=g), state_elem_mask=torch.ones(B, 8),
             ctrl_freqs=torch.tensor([10.0, 25.0][:B]), lang_attn_mask=torch.ones(B, 6, dtype=torch.bool), data_indices=[0] * B)
    b.update(extra)
    return b


def test_prepare_batch_key_mapping():
    from vlatouch.rdt_train import prepare_batch
    B, N = 2, 3
    toks, emb = torch.randn(B, 6, 5), torch.randn(B, 6, 7)
    b = _collator(img_tokens=toks, lang_embeds=emb)
    kw = prepare_batch(b)
    assert set(kw) == {"lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs"}
    assert kw["img_tokens"] is toks and kw["lang_tokens"] is emb and kw["lang_attn_mask"] is b["lang_attn_mask"] and kw["ctrl_freqs"] is b["ctrl_freqs"]
    assert torch.equal(kw["state_tokens"], b["states"][:, -1:, :]) and kw["state_tokens"].shape == (B, 1, 8)
    assert kw["action_gt"] is b["actions"] and torch.equal(kw["action_mask"], b["state_elem_mask"].unsqueeze(1))
    # `images` through the vision encoder, `input_ids` through the text encoder
    vis, images, ids = _Vision(), torch.randn(B, N, 3, 2, 2), torch.arange(B * 6).reshape(B, 6)
    kw = prepare_batch(_collator(images=images, input_ids=ids), vision_encoder=vis, text_encoder=_Text())
    assert torch.equal(vis.seen[0], images.reshape(B * N, 3, 2, 2)) and kw["img_tokens"].shape == (B, N * 2, 5) and not kw["img_tokens"].requires_grad
    assert torch.equal(kw["lang_tokens"], ids.float().unsqueeze(-1)) and not kw["lang_tokens"].requires_grad
    # `frames`: B lists of N, flattened sample by sample, with the jitter list beside them (argument, batch key, flat or nested)
    frames = [[1, None, 3], [4, 5, None]]
    jit = [["a", None, "c"], ["d", "e", None]]
    for how in ("key", "argument", "flat"):
        vis, pre = _Vision(), _Pre()
        if how == "key":
            kw = prepare_batch(_collator(frames=frames, jitter=jit, lang_embeds=emb), vision_encoder=vis, preprocessor=pre)
        elif how == "argument":
            kw = prepare_batch(_collator(frames=frames, lang_embeds=emb), vision_encoder=vis, preprocessor=pre, jitter=jit)
        else:
            kw = prepare_batch(_collator(frames=frames, lang_embeds=emb), vision_encoder=vis, preprocessor=pre, jitter=sum(jit, []))
        assert pre.calls == [([1, None, 3, 4, 5, None], ["a", None, "c", "d", "e", None])], how
        assert vis.seen[0].shape == (6, 3, 2, 2) and kw["img_tokens"].shape == (B, N * 2, 5)
        assert float(kw["img_tokens"][1, 0, 0]) == 4.0 and float(kw["img_tokens"][0, 2, 0]) == -1.0
    vis, pre = _Vision(), _Pre()
    prepare_batch(_collator(frames=frames, lang_embeds=emb), vision_encoder=vis, preprocessor=pre)
    assert pre.calls[0][1] is None
    # the two random draws of a test batch pass through
    kw = prepare_batch(_collator(img_tokens=toks, lang_embeds=emb, noise=toks, timesteps=torch.tensor([1, 2])))
    assert kw["noise"] is toks and kw["timesteps"].tolist() == [1, 2]


def test_prepare_batch_errors():
    from vlatouch.rdt_train import prepare_batch
    emb, ids = torch.randn(2, 6, 7), torch.zeros(2, 6, dtype=torch.long)
    with pytest.raises(ValueError, match="a batch with `images` needs vision_encoder"):
        prepare_batch(_collator(images=torch.zeros(2, 3, 3, 2, 2), lang_embeds=emb))
    with pytest.raises(ValueError, match="a batch with `images` needs vision_encoder"):
        prepare_batch(_collator(frames=[[1], [2]], lang_embeds=emb), preprocessor=_Pre())
    with pytest.raises(ValueError, match="a batch with `frames` needs preprocessor"):
        prepare_batch(_collator(frames=[[1], [2]], lang_embeds=emb), vision_encoder=_Vision())
    with pytest.raises(ValueError, match="a batch with `input_ids` needs text_encoder"):
        prepare_batch(_collator(img_tokens=torch.zeros(2, 6, 5), input_ids=ids))
    with pytest.raises(ValueError, match="must hold B = 2 lists"):
        prepare_batch(_collator(frames=[[1], [2], [3]], lang_embeds=emb), vision_encoder=_Vision(), preprocessor=_Pre())


class _StubTrainer:
    """finetune's view of a trainer: counts optimizer steps, records what train_step got."""
    def __init__(self):
        self.global_step, self.micro_step, self.sync_gradients, self.got = 0, 0, True, []

    def train_step(self, **kw):
        self.got.append(kw)
        self.global_step += 1
        return torch.tensor(float(self.global_step))


def test_finetune_routes_by_the_states_key():
    from vlatouch.rdt_train import finetune
    toks, emb = torch.randn(2, 6, 5), torch.randn(2, 6, 7)
    plain = dict(lang_tokens=emb, lang_attn_mask=None, img_tokens=toks, state_tokens=1, action_gt=2, action_mask=3, ctrl_freqs=4, noise=5)
    coll = _collator(frames=[[1, 2], [3, None]], jitter=[None, "j", None, None], lang_embeds=emb)
    tr, vis, pre = _StubTrainer(), _Vision(), _Pre()
    losses = finetune(tr, [plain, coll, plain], max_train_steps=3, vision_encoder=vis, preprocessor=pre)
    assert [float(x) for x in losses] == [1.0, 2.0, 3.0]
    assert tr.got[0] == plain and tr.got[2] == plain and tr.got[0]["img_tokens"] is toks            # unchanged, key for key
    assert set(tr.got[1]) == {"lang_tokens", "lang_attn_mask", "img_tokens", "state_tokens", "action_gt", "action_mask", "ctrl_freqs"}
    assert pre.calls == [([1, 2, 3, None], [None, "j", None, None])] and len(vis.seen) == 1
    assert tr.got[1]["img_tokens"].shape == (2, 4, 5) and torch.equal(tr.got[1]["state_tokens"], coll["states"][:, -1:, :])
    with pytest.raises(ValueError, match="needs preprocessor"):
        finetune(_StubTrainer(), [coll], max_train_steps=1, vision_encoder=vis)
