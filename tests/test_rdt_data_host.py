"""The host half of the fine-tuning data path (vlatouch/rdt_data.py) and its fp64 statement (tests/rdt_data_ref.py) against what the
reference's own code produced on the fixture episodes (tests/golden/g19_rdt_data.npz, tools/make_golden_rdt_data.py).  No GPU.

Tolerance: arrays derived from qpos are compared within 1e-12 absolute.  The only arithmetic that differs from the reference is the 6-D
rotation (direct from the quaternion instead of scipy's Euler round trip); the two agree to 1.5e-15 on 20 000 random quaternions and to the
golden's `sixd_route_err` on the fixture, values are O(1), and the statistics are means of at most 57 such values: 1e-12 is three orders
above that.  Everything that is a decision (step, masks, frame indices, which frames are background or augmented) is compared for equality."""
import os
import random

import numpy as np
import pytest
import torch

from tests import rdt_data_ref as R

TOL = 1e-12
KEPT64 = ("episode_2", "episode_12", "episode_21")
LATE = ("episode_10", "episode_20")


@pytest.fixture(scope="module")
def G():
    return dict(np.load(R.GOLDEN))


@pytest.fixture(scope="module")
def eps():
    return {os.path.basename(p)[:-3]: R.load_episode(p) for p in R.fixture_paths()}


def _store(**kw):
    from vlatouch.rdt_data import EpisodeStore
    args = dict(dataset_name=R.DATASET_NAME, dataset_names=R.DATASET_NAMES, control_freq={R.DATASET_NAME: R.CONTROL_FREQ})
    args.update(kw)
    return EpisodeStore(R.FIXTURE_DIR, **args)


@pytest.fixture(scope="module")
def store():
    return _store()


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= TOL


# ------------------------------------------------------------------------------------------------ the fp64 statement against the golden
def test_golden_holds_what_the_tool_promises(G):
    assert list(G["names"]) == [os.path.basename(p) for p in R.fixture_paths()]
    assert float(G["sixd_route_err"]) <= 1e-14
    assert sorted(n[:-3] for n, e in zip(G["names"], G["expect"]) if e == "kept") == sorted(KEPT64)
    assert [int(G[f"pf_{n}_steps"]) for n in KEPT64] == [40, 57, 45]


@pytest.mark.parametrize("name,tag,horizon", [(n, "pf", 64) for n in KEPT64] + [(n, "pf8", 8) for n in LATE])
def test_statement_parse_file(G, eps, name, tag, horizon):
    for k, seed in enumerate(R.G19_PARSE_SEEDS):
        s = R.parse_file(eps[name], np.random.RandomState(seed), horizon=horizon)
        assert s["step_id"] == int(G[f"{tag}_{name}_step_id"][k])
        assert (s["cam_mask"] == G[f"{tag}_{name}_cam_high_mask"][k]).all()
        for key in ("state", "actions", "state_std", "state_mean", "state_norm", "state_indicator"):
            assert close(s[key], G[f"{tag}_{name}_{key}"][k]), (name, seed, key)


def test_statement_state_only_and_dataset_stat(G, eps):
    for name, want in zip(G["names"], G["so_len"]):
        state, n = R.state_only(eps[name[:-3]])
        assert n == int(want)
        if n:
            assert close(state, G[f"so_{name[:-3]}"])
    stat = R.dataset_stat([eps[n] for n in KEPT64])
    for key in ("state_mean", "state_std", "state_min", "state_max"):
        assert close(stat[key], G[f"stat_{key}"]), key


def _frames_agree(G, seed, b, inst, number_of):
    """One sample's six frames: background / frame identity / augmentation as the reference's run recorded them."""
    for q in range(6):
        bg = bool(G[f"gi_{seed}_fr_background"][b, q])
        assert (inst["frames"][q] is None) == bg, (seed, b, q)
        if not bg:
            cam, idx = inst["frame_ref"][q]
            assert list(G[f"gi_{seed}_fr_sig"][b, q]) == [number_of, cam + 1, idx], (seed, b, q)
            assert list(inst["frames"][q][6, 8]) == [number_of, cam + 1, idx]
        p = inst["jitter"][q]
        assert (p is not None) == bool(G[f"gi_{seed}_fr_jittered"][b, q]), (seed, b, q)
        if p is not None:
            assert list(p.order) == list(G[f"gi_{seed}_fr_order"][b, q]) and list(p.factors()) == list(G[f"gi_{seed}_fr_factors"][b, q])


def _number(ep) -> int:
    return int(os.path.basename(ep["path"])[len("episode_"):-3])


@pytest.mark.parametrize("seed", R.G19_SEEDS)
def test_statement_getitem_and_collate(G, seed):
    ds = R.Dataset()
    assert ds.total == int(G["gi_len"])
    w = G["gi_weights"]
    assert np.array_equal(w[w > 0], ds.weights) and [n[:-3] for n, x in zip(G["gi_files"], w) if x > 0] == list(KEPT64)
    torch.manual_seed(seed)
    np_rng, rng = np.random.RandomState(seed), random.Random(seed)
    inst = [ds.getitem(np_rng, rng, None, **R.G19_KW) for _ in range(R.G19_B)]
    batch = R.collate(inst)
    for key in ("states", "actions", "state_elem_mask", "state_norm"):
        assert close(batch[key].numpy(), G[f"gi_{seed}_{key}"]), key
    assert np.array_equal(batch["ctrl_freqs"].numpy(), G[f"gi_{seed}_ctrl_freqs"])
    assert batch["data_indices"] == list(G[f"gi_{seed}_data_indices"])
    assert np.array_equal(batch["lang_embeds"].numpy(), G[f"gi_{seed}_lang_embeds"])
    assert np.array_equal(batch["lang_attn_mask"].numpy(), G[f"gi_{seed}_lang_attn_mask"])
    for b, i in enumerate(inst):
        _frames_agree(G, seed, b, i, _number(ds.eps[i["episode"]]))


def test_golden_samples_cover_the_branches(G):
    """The seeded runs must exercise what they are there to pin: masked and unmasked conditions, background, plain and augmented frames."""
    ctrl = np.concatenate([G[f"gi_{s}_ctrl_freqs"] for s in R.G19_SEEDS])
    elem = np.concatenate([G[f"gi_{s}_state_elem_mask"].sum(axis=1) for s in R.G19_SEEDS])
    bg = np.concatenate([G[f"gi_{s}_fr_background"].reshape(-1) for s in R.G19_SEEDS])
    jit = np.concatenate([G[f"gi_{s}_fr_jittered"].reshape(-1) for s in R.G19_SEEDS])
    assert set(ctrl.tolist()) == {0, R.CONTROL_FREQ} and set(elem.tolist()) == {0.0, 10.0}
    assert bg.sum() > bg.size // 3 and (~bg).sum() >= 6 and jit.sum() >= 2 and (~jit & ~bg).sum() >= 2


# ------------------------------------------------------------------------------------------------ the product's host half
def test_store_drops_and_reports(G, store):
    assert store.report == {"episode_3.h5": "fewer than 32 steps", "episode_11.h5": "no step moves more than 1e-2 away from the first",
                            "episode_10.h5": "first_idx - 1 >= N - int(horizon / 2): no step can be drawn",
                            "episode_20.h5": "first_idx - 1 >= N - int(horizon / 2): no step can be drawn"}
    # which files the reference itself refuses: parse_file_state_only returns length 0 for the first two, and the tool saw randint raise for the others
    assert [n for n, l in zip(G["names"], G["so_len"]) if l == 0] == ["episode_3.h5", "episode_11.h5"]
    assert [os.path.basename(e.path)[:-3] for e in store.episodes] == list(KEPT64)
    assert len(store) == int(G["gi_len"])
    w = G["gi_weights"]
    assert np.array_equal(store.weights, w[w > 0])
    assert len(store) == sum(e.qpos.shape[0] - (e.first_idx - 1) for e in store.episodes)


def test_store_horizon_checks():
    from vlatouch.rdt_data import EpisodeStore
    kw = dict(dataset_name="mango", dataset_names=["mango"], control_freq=25)
    with pytest.raises(ValueError, match="horizon"):
        EpisodeStore(R.FIXTURE_DIR, horizon=2, **kw)
    with pytest.raises(ValueError, match="dataset_name"):
        EpisodeStore(R.FIXTURE_DIR, dataset_name="mango", dataset_names=["other"], control_freq=25)
    with pytest.raises(ValueError, match="frames"):
        EpisodeStore(R.FIXTURE_DIR, frames="disk", **kw)
    with pytest.raises(ValueError, match="state_indices"):
        EpisodeStore(R.FIXTURE_DIR, state_indices=[1, 2, 3], **kw)
    s8 = EpisodeStore(R.FIXTURE_DIR, horizon=8, **kw)                              # the two late episodes are usable at horizon 8
    assert [os.path.basename(e.path)[:-3] for e in s8.episodes] == ["episode_2", "episode_10", "episode_12", "episode_20", "episode_21"]
    assert sorted(s8.report) == ["episode_11.h5", "episode_3.h5"]


def test_store_tables_against_the_golden(G, store):
    for ep in store.episodes:
        n = os.path.basename(ep.path)[:-3]
        assert close(store.fill_in_state(ep.qpos[ep.first_idx - 1:]), G[f"so_{n}"])
        for row, key in enumerate(("state_std", "state_mean", "state_norm")):
            assert close(store.fill_in_state(ep.stats[row]), G[f"pf_{n}_{key}"][0]), (n, key)
        for k, step in enumerate(G[f"pf_{n}_step_id"]):                          # the rows the kernel gathers for the golden's steps
            rows = np.minimum(step + 2 + np.arange(64), ep.qpos.shape[0] - 1)
            assert close(store.fill_in_state(ep.qpos[rows]), G[f"pf_{n}_actions"][k])
            assert close(store.fill_in_state(ep.qpos[step:step + 1]), G[f"pf_{n}_state"][k])
    stat = store.dataset_stat()
    assert stat["dataset_name"] == R.DATASET_NAME and sorted(stat) == ["dataset_name", "state_max", "state_mean", "state_min", "state_std"]
    for key in ("state_mean", "state_std", "state_min", "state_max"):
        assert close(stat[key], G[f"stat_{key}"]), key


@pytest.mark.parametrize("seed", R.G19_SEEDS)
def test_draw_follows_the_reference_streams(G, store, seed):
    """The plans of a seeded draw against the reference's recorded samples: decisions equal; the state the plan stands for (the kernel's
    statement, evaluated here in numpy) within the tolerance."""
    torch.manual_seed(seed)
    plans = store.draw(R.G19_B, np_rng=np.random.RandomState(seed), rng=random.Random(seed), generator=None, **R.G19_KW)
    c = np.sqrt(10 ** (R.G19_KW["state_noise_snr"] / 10))
    mean = np.asarray(store.dataset_stat()["state_mean"])
    for b, p in enumerate(plans):
        ep = store.episodes[p.episode]
        assert p.action_id == p.step_id + 2 and p.noise.shape == (10,)
        assert p.ctrl_masked == (int(G[f"gi_{seed}_ctrl_freqs"][b]) == 0)
        assert p.elem_masked == (G[f"gi_{seed}_state_elem_mask"][b].sum() == 0)
        state = mean if p.state_masked else store.fill_in_state(ep.qpos[p.step_id] + (0.0 + (ep.stats[0] / c) * p.noise))
        assert close(state, G[f"gi_{seed}_states"][b, 0]), (seed, b, p)
        rows = np.minimum(p.action_id + np.arange(64), ep.qpos.shape[0] - 1)
        assert close(store.fill_in_state(ep.qpos[rows]), G[f"gi_{seed}_actions"][b])
        assert p.frame_idx == [max(p.step_id - 1, 0), p.step_id]
        assert p.slot_valid == [p.step_id - (ep.first_idx - 1) + 1 >= 2, True]
        number = int(os.path.basename(ep.path)[len("episode_"):-3])
        for q in range(6):
            assert p.frame_valid[q] == (not G[f"gi_{seed}_fr_background"][b, q]), (seed, b, q)
            if p.frame_valid[q]:
                assert list(G[f"gi_{seed}_fr_sig"][b, q]) == [number, q % 3 + 1, p.frame_idx[q // 3]]
            j = p.jitter[q]
            assert (j is not None) == bool(G[f"gi_{seed}_fr_jittered"][b, q])
            if j is not None:
                assert list(j.order) == list(G[f"gi_{seed}_fr_order"][b, q]) and list(j.factors()) == list(G[f"gi_{seed}_fr_factors"][b, q])


def test_draw_equals_the_statement_on_other_settings(store):
    """Streams stay in step with the fp64 statement for the defaults, for the sample-loader settings and at horizon 8 (five episodes)."""
    s8, d8 = _store(horizon=8), R.Dataset(horizon=8)
    for st, ds, kw in ((store, R.Dataset(), {}), (store, R.Dataset(), dict(cond_mask_prob=0, state_noise_snr=None, image_aug=False)),
                       (s8, d8, dict(cond_mask_prob=0.5, image_aug=True)), (s8, d8, dict(cam_ext_mask_prob=0.9, state_noise_snr=30))):
        a, b, g1, g2 = (np.random.RandomState(4), random.Random(4)), (np.random.RandomState(4), random.Random(4)), *(torch.Generator().manual_seed(4) for _ in "ab")
        plans = st.draw(7, np_rng=a[0], rng=a[1], generator=g1, **kw)
        inst = [ds.getitem(b[0], b[1], g2, **kw) for _ in range(7)]
        for p, i in zip(plans, inst):
            assert (p.episode, p.step_id) == (i["episode"], i["step_id"])
            assert p.ctrl_masked == (i["ctrl_freq"] == 0) and p.elem_masked == (i["state_elem_mask"].sum() == 0)
            assert p.frame_valid == [f is not None for f in i["frames"]]
            assert [(q % 3, p.frame_idx[q // 3]) if v else None for q, v in enumerate(p.frame_valid)] == i["frame_ref"]
            assert p.jitter == i["jitter"]
        assert a[0].randint(1 << 30) == b[0].randint(1 << 30) and a[1].random() == b[1].random()       # both consumed the same number of draws


def test_plans_are_checked_before_any_launch(store):
    from vlatouch.rdt_data import SamplePlan
    ep = store.episodes[0]
    n, lo = ep.qpos.shape[0], ep.first_idx - 1
    good = dict(episode=0, step_id=lo, ctrl_masked=False, state_masked=False, elem_masked=False, frame_idx=[lo, lo], slot_valid=[False, True],
                frame_valid=[False] * 6)
    store.check_plans([SamplePlan(**good)])
    for bad, match in ((dict(step_id=n - 32), "step_id"), (dict(step_id=lo - 1), "step_id"), (dict(episode=3), "episode"), (dict(episode=-1), "episode"),
                       (dict(action_id=lo + 3), "action_id"), (dict(frame_idx=[lo, n]), "frame index"), (dict(noise=np.zeros(9), noise_snr=40), "noise"), (dict(noise=np.zeros(10)), "noise_snr"),
                       (dict(frame_valid=[False, False, True, False, False, False]), "no camera")):
        with pytest.raises(ValueError, match=match):
            store.assemble([SamplePlan(**dict(good, **bad))])                    # a ValueError, not the missing GPU: nothing was launched
    with pytest.raises(ValueError, match="no plans"):
        store.assemble([])
