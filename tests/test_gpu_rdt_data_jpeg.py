"""EpisodeStore(frames="jpeg") on the GPU: a recording converted with images="jpeg" and kept as bitstreams in HBM gives, for the same plans,
exactly the micro-batch of the store that keeps the Pillow-decoded pixels (frames="device", the path before this mode existed): every tensor
and every frame's bytes, with jitter / corruption lists, masked frames and pad_and_resize; it is smaller, refuses a cap below its compressed
size, and feeds `finetune`."""
import random

import numpy as np
import pytest
import torch

from tests import cases
from tests import jpegdec_ref as R
from tests import rdt_data_ref as RD
from vlatouch import convert

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPS = {1: 36, 2: 40, 3: 33}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """Three short episodes, camera1 and camera2 of 48 x 64 (episode 3 has no camera2) and the always-missing third slot, converted both ways."""
    root = tmp_path_factory.mktemp("jpeg_store")
    for e, n in STEPS.items():
        R.write_recording(str(root / "raw" / f"episode_{e}"), n, seed=10 + e, cameras=("camera1", "camera2") if e != 3 else ("camera1",), lang=(3, 96))
    convert.convert_dataset_to_hdf5(str(root / "raw"), str(root / "decoded"))
    convert.convert_dataset_to_hdf5(str(root / "raw"), str(root / "jpeg"), images="jpeg")
    return root


def _stores(dirs, **kw):
    from vlatouch.rdt_data import EpisodeStore
    args = dict(dataset_name=RD.DATASET_NAME, dataset_names=RD.DATASET_NAMES, control_freq=RD.CONTROL_FREQ, horizon=16, device=DEV)
    args.update(kw)
    return EpisodeStore(str(dirs / "decoded"), frames="device", **args), EpisodeStore(str(dirs / "jpeg"), frames="jpeg", **args)


def _rngs(seed):
    return dict(np_rng=np.random.RandomState(seed), rng=random.Random(seed), generator=torch.Generator().manual_seed(seed))


def _same_batches(a, b, shape):
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], torch.Tensor):
            assert torch.equal(a[key], b[key]), key
    assert a["data_indices"] == b["data_indices"] and a["jitter"] == b["jitter"] and a.get("corrupt") == b.get("corrupt")
    n = 0
    for fa, fb in zip(a["frames"], b["frames"]):
        assert len(fa) == len(fb) == 6
        for x, y in zip(fa, fb):
            assert (x is None) == (y is None)
            if x is not None:
                assert y.is_cuda and y.dtype == torch.uint8 and tuple(y.shape) == tuple(x.shape) == shape and torch.equal(x, y)
                n += 1
    return n


@pytest.mark.parametrize("resize", [None, 32])
def test_assemble_equals_the_store_of_the_decoded_files(dirs, resize):
    dec, jpg = _stores(dirs, pad_and_resize=resize)
    assert len(dec.episodes) == len(jpg.episodes) == 3 and dec.dataset_stat() == jpg.dataset_stat()
    draw = dict(cond_mask_prob=0.3, state_noise_snr=40, image_aug=True, image_corrupt=True, corrupt_rng=np.random.default_rng(3))
    r = _rngs(8)
    shown = hidden = jittered = corrupted = 0
    for _ in range(3):
        plans = dec.draw(4, **r, **draw)
        a, b = dec.assemble(plans), jpg.assemble(plans)
        again = jpg.assemble(plans)
        torch.cuda.synchronize()
        k = _same_batches(a, b, (48, 64, 3) if resize is None else (32, 32, 3))
        assert _same_batches(b, again, (48, 64, 3) if resize is None else (32, 32, 3)) == k
        shown, hidden = shown + k, hidden + 24 - k
        jittered += sum(j is not None for js in (b["jitter"] or []) for j in js)
        corrupted += sum(c is not None for cs in b.get("corrupt", []) for c in cs)
    assert shown >= 12 and hidden >= 12                       # masked and missing frames are the background (None) under both stores
    assert jittered >= 1 and corrupted >= 1                   # the jitter and corruption lists pass through
    assert jpg.resident_bytes < dec.resident_bytes and jpg.host_frame_bytes == 0
    if resize is None:                                        # the raw frames against their files: well under a third here (smooth synthetic frames)
        frames_dec = sum(n * 48 * 64 * 3 * (2 if e != 3 else 1) for e, n in STEPS.items())
        assert dec.resident_bytes - jpg.resident_bytes > frames_dec // 2


def test_all_frames_masked_decodes_nothing(dirs):
    dec, jpg = _stores(dirs)
    plans = dec.draw(2, **_rngs(1), cond_mask_prob=1.0)
    b = jpg.assemble(plans)
    assert all(f is None for s in b["frames"] for f in s) and torch.equal(b["actions"], dec.assemble(plans)["actions"])


def test_a_cap_below_the_compressed_size_raises(dirs):
    _, jpg = _stores(dirs)
    jpg.upload()
    frames = jpg.resident_bytes - _stores(dirs, cameras=(None, None, None))[1].upload().resident_bytes
    assert frames > 0
    _stores(dirs, max_device_bytes=frames)[1].upload()
    with pytest.raises(ValueError, match="no pinned-host spill"):
        _stores(dirs, max_device_bytes=frames - 1)[1].upload()


def test_finetune_runs_from_the_jpeg_store_as_from_the_decoded_one(dirs):
    from tests.test_gpu_rdt_data import _tower_and_preprocessor
    from tests.test_gpu_rdt_train import _runner
    from vlatouch.rdt_train import finetune
    tower, pp = _tower_and_preprocessor()
    cfg = dict(cases.RDT_TINY, img_token_dim=tower.hidden_size, img_cond_len=6 * tower.num_patches)
    dec, jpg = _stores(dirs, horizon=cfg["horizon"])
    draw = dict(cond_mask_prob=0.3, state_noise_snr=None, image_aug=True)
    losses = []
    for store in (dec, jpg):
        tr = _runner(cfg).trainer(lr=1e-3)
        torch.manual_seed(31)
        losses.append(finetune(tr, store.batches(2, **_rngs(5), **draw), max_train_steps=2, vision_encoder=tower, preprocessor=pp))
        assert tr.global_step == 2
    assert len(losses[1]) == 2 and all(bool(torch.isfinite(x)) for x in losses[1])
    assert all(torch.equal(x, y) for x, y in zip(*losses))
