"""The host half of vlatouch/ctrl_data.py (no GPU): the store's index against `ControllerDataset`, `ControllerStoreModule`'s split and
statistics against the `ControllerDataModule` it wraps, `StoreLoader`'s order against a real `torch.utils.data.DataLoader`, and the whole-
number normalisation decision the GPU tests use as their reference statement."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import cases
from residual_controller.controller_dataset import ControllerDataModule, ControllerDataset
from vlatouch import ctrl_data as CD
from vlatouch import eval as ev

EPH = os.path.join(cases.GOLDEN, "episodes_h5")
FILES = [os.path.join(EPH, f) for f in ("episode_1.h5", "episode_2.h5")]


def test_index_is_the_datasets():
    ds = ControllerDataset(EPH, file_paths=FILES, context_frames=2, horizon=8, use_images=False)
    st = CD.ControllerStore(ds, None, build=False)
    assert len(st) == len(ds) == 27 + 33
    assert st.episode_indices == [(int(e), int(s)) for e, s in ds.episode_indices]
    assert [e for e, _ in st.episode_indices].count(0) == 27 and [e for e, _ in st.episode_indices].count(1) == 33
    assert st.file_paths == ds.file_paths and (st.context_frames, st.horizon) == (2, 8)
    assert st.stats is ds.stats
    plan = st.check_index(torch.tensor([0, 26, 27, 59]))
    assert plan.dtype == np.int32 and plan.tolist() == [list(ds.episode_indices[i]) for i in (0, 26, 27, 59)]
    for bad in ([60], [-1], [], [[0]]):
        with pytest.raises(ValueError):
            st.check_index(bad)
    with pytest.raises(ValueError):
        st.check_index(np.array([0.5]))


def test_module_keeps_the_split_and_the_statistics(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    for f in FILES:
        shutil.copy(f, d)
    np.random.seed(3)
    dm = ControllerDataModule(str(d), batch_size=8, num_workers=0, context_frames=2, horizon=8, use_images=False)
    mod = CD.ControllerStoreModule(dm, None, build=False)
    assert mod.train_store.file_paths == dm.train_dataset.file_paths and mod.val_store.file_paths == dm.val_dataset.file_paths
    assert len(mod.train_store.file_paths) == 1 and len(mod.val_store.file_paths) == 1
    assert mod.stats is dm.stats and mod.train_store.stats is dm.stats and mod.val_store.stats is dm.stats      # validation normalises with the training files'
    assert set(dm.stats) == set(mod.stats) and all(np.array_equal(dm.stats[k], mod.stats[k]) for k in dm.stats)
    assert mod.train_dataset is dm.train_dataset and mod.val_dataset is dm.val_dataset and mod.batch_size == 8
    assert len(mod.train_dataloader()) == len(dm.train_dataset) // 8
    assert len(mod.val_dataloader()) == -(-len(dm.val_dataset) // 8)
    tab = mod.train_store._stats_table()
    assert tab.dtype == np.float32 and tab.shape == (4, 10)
    for row, k in enumerate(("action_mins", "action_maxs", "vla_mins", "vla_maxs")):
        assert np.array_equal(tab[row], torch.as_tensor(dm.stats[k], dtype=torch.float32).numpy())


class _Range(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class _FakeStore:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("seed", [0, 7])
def test_loader_draws_what_a_dataloader_draws(seed):
    n, bs = 27, 8
    torch.manual_seed(seed)
    dl = torch.utils.data.DataLoader(_Range(n), batch_size=bs, shuffle=True, drop_last=True)
    want = [[b.tolist() for b in dl] for _ in range(3)]
    tail_want = torch.rand(4)
    torch.manual_seed(seed)
    sl = CD.StoreLoader(_FakeStore(n), bs, shuffle=True, drop_last=True)
    got = [[b.index.tolist() for b in sl] for _ in range(3)]
    tail_got = torch.rand(4)
    assert got == want and len(sl) == len(dl) == 3
    assert want[0] != want[1] != want[2] and all(len(b) == bs for ep in got for b in ep)
    assert torch.equal(tail_got, tail_want)                              # the global generator is left where the DataLoader leaves it
    assert all(b.index.dtype == torch.int64 for b in sl)


def test_validation_loader_order_and_partial_batch():
    n, bs = 27, 8
    torch.manual_seed(5)
    dl = torch.utils.data.DataLoader(_Range(n), batch_size=bs, shuffle=False, drop_last=False)
    want = [b.tolist() for b in dl]
    tail_want = torch.rand(2)
    torch.manual_seed(5)
    sl = CD.StoreLoader(_FakeStore(n), bs, shuffle=False, drop_last=False)
    got = [b.index.tolist() for b in sl]
    assert got == want and got[-1] == [24, 25, 26] and len(sl) == len(dl) == 4
    assert torch.equal(torch.rand(2), tail_want)
    st = sl.store
    assert all(b.store is st for b in sl)


def test_decision_rule_on_either_side_of_a_half():
    """normalise iff mean(u8 / 255) >= 0.5, in whole numbers: 2 * sum >= 255 * B * P."""
    P = 28 * 28 * 3
    frame = lambda v: np.full((28, 28, 3), v, dtype=np.uint8)
    sums = lambda frames: [int(f.astype(np.uint64).sum()) for f in frames]
    bright, dark = frame(200), frame(40)
    assert CD.norm_decision(sums([bright, bright, bright, dark]), P)          # mean 0.63: all four are normalised, the dark one too
    assert not CD.norm_decision(sums([bright, dark, dark, dark]), P)          # mean 0.31: none is, the bright one neither
    assert CD.norm_decision(sums([bright]), P) and not CD.norm_decision(sums([dark]), P)
    # exactly one half: 127 and 128 average 127.5 / 255 = 0.5 -> on (the reference skips only below 0.5); one count less -> off
    assert CD.norm_decision(sums([frame(127), frame(128)]), P)
    low = frame(127).copy()
    low[0, 0, 0] = 126
    assert not CD.norm_decision(sums([low, frame(128)]), P)
    assert not CD.norm_decision(sums([frame(0)]), P)                          # an all-black frame
    for frames in ([bright, bright, bright, dark], [bright, dark, dark, dark]):
        mean = float(np.mean(np.stack(frames).astype(np.float64) / 255))
        assert CD.norm_decision(sums(frames), P) == (mean >= 0.5) and abs(mean - 0.5) > 0.01


def test_golden_fixture_batches_sit_away_from_a_half():
    """The two fixtures' camera means, over every window's image frame: 0.59 - 0.61 and 0.29 - 0.31 (the GPU tests rely on the margin)."""
    seen = []
    for path in FILES:
        ep = ev.load_episode(path, images=True)
        for k in ("camera1_resized", "camera2_resized"):
            m = ep[k].reshape(ep[k].shape[0], -1).astype(np.float64).mean(axis=1) / 255
            assert np.all(np.abs(m - 0.5) >= 0.01)
            seen.append((float(m.min()), float(m.max())))
    lo, hi = min(s[0] for s in seen), max(s[1] for s in seen)
    assert 0.28 <= lo <= 0.32 and 0.58 <= hi <= 0.62, seen
