"""`ControllerStore` / `ControllerStoreModule` (vlatouch/ctrl_data.py) against the path they stand for: `ControllerDataset.__getitem__` ->
collate -> `_prepare_batch_for_diffusion` / `_prepare_batch` with the DINOv2 tower run on the batch's frames.

Tolerances.  Everything but the CLS columns is a copy or vt_action_normalize's arithmetic on the same fp32 value: bit-equal.  The decisions
must equal the encoder's own (`last_flags[:, 1]`); every batch mean used is at least 0.01 away from 0.5.  The CLS columns come from two
runs of the same fp32 tower on other batch compositions (the GEMM tiles see other row counts) and on pixels that differ by at most 1 ulp
(u8 * (1/255) against float32(u8) / 255): each side is within the project's DINO_TOL["fp32"] = 2e-4 of the reference's output
(tests/test_gpu_models.py), so they agree within 2 * 2e-4 = 4e-4.  The same bound holds between stores built with other chunk sizes."""
import os
import shutil
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import ctrl_data_ref as R
from vlatouch import ctrl_data as CD
from vlatouch import eval as ev
from vlatouch import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEAT_TOL = 2 * 2e-4
CF, H = 2, 16
EPH = os.path.join(cases.GOLDEN, "episodes_h5")
N3, BLACK = 36, 11           # the synthetic episode: 36 frames of 28 x 28, even frames bright on camera 1 and dark on camera 2, frame 11 black


def _synthetic_episode(path):
    g = np.random.default_rng(77)
    ep = R.synth_episode(N3, 3, hv=64)
    ep["ee_poses"][:, 0] = 0.05 * np.arange(N3)                 # moves from frame 1 on: windows start at 1, their images are frames 2 .. 19
    ep["gelsight_force/displacement"] = g.normal(size=(N3, 63, 2)).astype(np.float32)      # as the fixtures have it: one collate over both kinds
    even = (np.arange(N3) % 2 == 0)[:, None, None, None]
    bright = g.integers(R.BRIGHT - 10, R.BRIGHT + 11, size=(N3, 28, 28, 3))
    dark = g.integers(R.DARK - 10, R.DARK + 11, size=(N3, 28, 28, 3))
    cam1, cam2 = np.where(even, bright, dark).astype(np.uint8), np.where(even, dark, bright).astype(np.uint8)
    cam1[BLACK] = 0
    cam2[BLACK] = 0
    np.savez(path, camera1_resized=cam1, camera2_resized=cam2, **ep)


class _Env:
    pass


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from residual_controller.bridge_controller import DiffusionController
    from residual_controller.bridge_train import DiffusionControllerTrainer
    from residual_controller.controller_dataset import ControllerDataset
    d = tmp_path_factory.mktemp("ctrl_store")
    npz = str(d / "episode_3.npz")
    _synthetic_episode(npz)
    e = _Env()
    e.dir = d
    e.files = [os.path.join(EPH, "episode_1.h5"), os.path.join(EPH, "episode_2.h5"), npz]
    e.ds = ControllerDataset(str(d), file_paths=e.files, context_frames=CF, horizon=H, use_images=True)
    assert len(e.ds) == 19 + 25 + 18
    e.dm = types.SimpleNamespace(stats=e.ds.stats)
    e.ctrl = synth.build_controller(DiffusionController, "fp32", device=DEV)
    e.store = CD.ControllerStore(e.ds, e.ctrl.image_encoder)
    e.trainer = DiffusionControllerTrainer(e.ctrl, e.dm, checkpoint_dir=str(d / "ck_a"), device=DEV)
    e.index_of = {es: i for i, es in enumerate(e.store.episode_indices)}
    e.frame = lambda f: e.index_of[(2, f - (CF - 1))]          # the window of the synthetic episode whose image is frame f
    return e


def _batches(e):
    fr = e.frame
    return {
        "golden windows": ([0, 18, 19, 43, 5, 30, 30, 7], (1.0, 0.0)),
        "3 bright + 1 dark on camera 1": ([fr(2), fr(4), fr(6), fr(5)], (1.0, 0.0)),
        "1 bright + 3 dark on camera 1": ([fr(2), fr(3), fr(5), fr(7)], (0.0, 1.0)),
        "with the black frame": ([fr(BLACK), fr(2), fr(4), fr(6), fr(8)], (1.0, 0.0)),
        "the black frame alone": ([fr(BLACK)], (0.0, 0.0)),
        "golden and synthetic": ([3, fr(3), 25, fr(9), fr(13), fr(19)], (0.0, 1.0)),
    }


def test_report_and_tables(env):
    rep = env.store.report()
    d = env.store._dev
    rows = 40 + 46 + N3
    assert rep["rows"] == rows and rep["episodes"] == 3 and rep["skipped"] == {} and rep["frames_encoded"] == len(env.ds) and rep["engine_rebuilds"] == 0
    assert d["pose10"].shape == (rows, 10) and d["pose10"].dtype == torch.float64 and d["vla"].shape == (rows, 64, 10) and d["vla"].dtype == torch.float64
    assert d["forces"].shape == (rows, 3) and d["feat"].shape == (2, rows, 2, 384) and d["pix_sum"].shape == (2, rows)
    assert d["ep_off"].tolist() == [0, 40, 86, rows]
    assert rep["total_bytes"] == sum(rep["resident_bytes"].values()) == sum(t.numel() * t.element_size() for t in d.values()) and rep["build_seconds"] > 0
    ep = ev.load_episode(env.files[2], images=True)
    want = ep["camera2_resized"].reshape(N3, -1).astype(np.uint64).sum(axis=1)
    used = np.arange(2, 20)
    assert d["pix_sum"][1, 86 + used].cpu().numpy().astype(np.uint64).tolist() == want[used].tolist()
    assert int(d["pix_sum"][0, 86 + BLACK]) == 0 and int(d["pix_sum"][0, 86 + 25]) == 0          # a black frame; a frame no window shows
    assert bool((d["feat"][:, 86 + 25] == 0).all()) and bool((d["feat"][:, 86 + 2] != 0).any())
    assert not torch.equal(d["feat"][0, 86 + 2, 0], d["feat"][0, 86 + 2, 1])
    with pytest.raises(ValueError, match="max_device_bytes"):
        CD.ControllerStore(env.ds, env.ctrl.image_encoder, max_device_bytes=1000)


def test_assemble_equals_the_dataset_path(env):
    tr, dv = env.trainer, 384
    for what, (idx, want) in _batches(env).items():
        rows = [int(env.store._dev["ep_off"][e]) + s + CF - 1 for e, s in (env.store.episode_indices[i] for i in idx)]
        for c in range(2):
            m = float(env.store._dev["pix_sum"][c, rows].sum()) / (255.0 * len(idx) * 28 * 28 * 3)
            assert abs(m - 0.5) >= 0.01, (what, c, m)
        ref = tr._prepare_batch_for_diffusion(ev.collate([env.ds[i] for i in idx]))
        ref_flags = env.ctrl.image_encoder.engine.last_flags[:, 1].clone()
        got = tr._prepare_batch_for_diffusion(CD.StoreBatch(env.store, torch.tensor(idx)))
        assert set(got) == set(ref) | {"norm_flags"}
        assert torch.equal(got["norm_flags"], ref_flags) and got["norm_flags"].tolist() == list(want), (what, got["norm_flags"], ref_flags)
        assert got["obs_in"].shape == ref["obs_in"].shape and torch.equal(got["obs_in"][:, 2 * dv:], ref["obs_in"][:, 2 * dv:]), what
        for k in ("expert_act", "vla_act", "forces", "current_force"):
            assert got[k].shape == ref[k].shape and torch.equal(got[k].cpu(), ref[k].cpu()), (what, k)
        err = float((got["obs_in"][:, :2 * dv] - ref["obs_in"][:, :2 * dv]).abs().max())
        print(f"{what}: max |cls(store) - cls(dataset path)| = {err:.3e} (tol {FEAT_TOL})")
        assert err < FEAT_TOL, (what, err)
        again = env.store.assemble(idx, layout="bridge", kin=tr.trainer.mlp.kin)
        assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)
    with pytest.raises(ValueError):
        env.store.assemble([len(env.store)], layout="bridge", kin=tr.trainer.mlp.kin)
    with pytest.raises(ValueError):
        env.store.assemble([0], layout="bridge", kin=780)
    with pytest.raises(ValueError):
        env.store.assemble([0], layout="diffusion", kin=784)


def test_build_is_deterministic_and_chunking_stays_within_tolerance(env):
    a = env.store._dev
    b = CD.ControllerStore(env.ds, env.ctrl.image_encoder)._dev
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]
    c = CD.ControllerStore(env.ds, env.ctrl.image_encoder, encode_chunk=4)._dev
    assert all(torch.equal(a[k], c[k]) for k in a if k != "feat")
    err = float((a["feat"] - c["feat"]).abs().max())
    print(f"encode_chunk 64 against 4: max |feat difference| = {err:.3e} (tol {FEAT_TOL})")
    assert err < FEAT_TOL, err


def test_bridge_trainer_step_is_the_step_on_the_assembled_tensors(env):
    from residual_controller.bridge_controller import DiffusionController
    from residual_controller.bridge_train import DiffusionControllerTrainer
    mk = lambda ctrl, name: DiffusionControllerTrainer(ctrl, env.dm, checkpoint_dir=str(env.dir / name), device=DEV)
    a = mk(env.ctrl, "ck_b")
    other = synth.build_controller(DiffusionController, "fp32", device=DEV)
    b = mk(other, "ck_c")
    idx = torch.tensor([env.frame(2), 0, 20, env.frame(5), env.frame(BLACK), 41, 7, 7])
    g = torch.Generator().manual_seed(3)
    t, z = torch.rand(8, generator=g).to(DEV), torch.randn(8, H, 10, generator=g).to(DEV)
    for _ in range(2):
        la, ia = a.train_step(CD.StoreBatch(env.store, idx), t, z)
        bd = env.store.assemble(idx, layout="bridge", kin=b.trainer.mlp.kin, use_force=b.use_force)
        b.trainer.lr = b._lr()
        lb, ib = b.trainer.train_step(bd["obs_in"], bd["vla_act"], bd["expert_act"], t, z)
        b.sched_step += 1
        assert np.isfinite(la) and la == lb and ia == ib, (la, lb, ia, ib)
    ea, _ = a.eval_step(CD.StoreBatch(env.store, idx), t, z)
    eb, _ = b.trainer.get_loss(bd["obs_in"], bd["vla_act"], bd["expert_act"], t, z, backward=False)
    assert ea == eb
    with pytest.raises(ValueError, match="encoder"):                   # the store's features are another encoder object's
        b.train_step(CD.StoreBatch(env.store, idx), t, z)
    ds8 = types.SimpleNamespace(file_paths=env.ds.file_paths, episode_indices=[(0, 4)], context_frames=3, horizon=H, stats=env.ds.stats)
    with pytest.raises(ValueError, match="context_frames"):
        a.train_step(CD.StoreBatch(CD.ControllerStore(ds8, env.ctrl.image_encoder, build=False), torch.tensor([0])), t[:1], z[:1])


def test_lstm_trainer_step_is_the_step_on_the_assembled_tensors(env):
    from residual_controller.lstm_step_controller import TactileLSTMController
    from residual_controller.lstm_train import LSTMControllerTrainer
    c = synth.DINOV2_CONFIGS["small"]
    mk = lambda: TactileLSTMController(device=DEV, precision="fp32",
                                       image_state_dict=synth.torch_state_dict(synth.dinov2_shapes(c["hidden"], c["layers"]), prefix="dinov2-small."))
    ca, cb = mk(), mk()
    a = LSTMControllerTrainer(ca, env.dm, checkpoint_dir=str(env.dir / "ck_la"), device=DEV)
    b = LSTMControllerTrainer(cb, env.dm, checkpoint_dir=str(env.dir / "ck_lb"), device=DEV)
    store = CD.ControllerStore(env.ds, ca.image_encoder, encode_chunk=16)
    idx = torch.tensor([env.frame(3), 1, 22, env.frame(4), env.frame(BLACK), 40])
    ref = a._prepare_batch(ev.collate([env.ds[i] for i in idx.tolist()]))
    ref_flags = ca.image_encoder.engine.last_flags[:, 1].clone()
    bd = a._prepare_batch(CD.StoreBatch(store, idx))
    assert set(bd) == set(ref) | {"norm_flags"} and torch.equal(bd["norm_flags"], ref_flags)
    assert bd["obs_in"].shape == ref["obs_in"].shape and torch.equal(bd["obs_in"][:, 768:], ref["obs_in"][:, 768:])
    assert float((bd["obs_in"][:, :768] - ref["obs_in"][:, :768]).abs().max()) < FEAT_TOL
    for k in ("expert_act", "vla_act", "forces"):
        assert bd[k].shape == ref[k].shape and torch.equal(bd[k].cpu(), ref[k].cpu()), k
    for _ in range(2):
        la = a.train_step(CD.StoreBatch(store, idx), masks=None)
        lb = b.trainer.train_step(bd["obs_in"], bd["vla_act"], bd["forces"], bd["expert_act"], masks=None)
        assert np.isfinite(la) and la == lb, (la, lb)
    assert a.eval_step(CD.StoreBatch(store, idx)) == b.trainer.get_loss(bd["obs_in"], bd["vla_act"], bd["forces"], bd["expert_act"], masks=None, backward=False)[0]
    with pytest.raises(ValueError, match="encoder"):
        b.train_step(CD.StoreBatch(store, idx), masks=None)


def test_trainer_runs_an_epoch_from_a_store_module(tmp_path):
    from residual_controller.bridge_controller import DiffusionController
    from residual_controller.bridge_train import DiffusionControllerTrainer
    from residual_controller.controller_dataset import ControllerDataModule
    d = tmp_path / "data"
    d.mkdir()
    for f in ("episode_1.h5", "episode_2.h5"):
        shutil.copy(os.path.join(EPH, f), d)
    np.random.seed(1)
    torch.manual_seed(1)
    dm = ControllerDataModule(str(d), batch_size=8, num_workers=0, context_frames=CF, horizon=H, use_images=False)
    ctrl = synth.build_controller(DiffusionController, "fp32", device=DEV)
    mod = CD.ControllerStoreModule(dm, ctrl)
    assert mod.train_store.report()["frames_encoded"] == len(dm.train_dataset) and mod.val_store.report()["frames_encoded"] == len(dm.val_dataset)
    tr = DiffusionControllerTrainer(ctrl, mod, learning_rate=1e-4, checkpoint_dir=str(tmp_path / "ck"), device=DEV)
    best = tr.train(mod, num_epochs=1, save_interval=1, eval_interval=1, log_interval=1)
    assert np.isfinite(best)
    steps = [h for h in tr.history if "step" in h]
    assert len(steps) == len(mod.train_dataset) // 8 and len(steps) >= 2 and all(np.isfinite(h["loss"]) for h in steps)
    assert [h for h in tr.history if "val_loss" in h] and all(np.isfinite(h["val_loss"]) for h in tr.history if "val_loss" in h)
    for name in ("best_model", "epoch_1"):
        assert sorted(os.listdir(tmp_path / "ck" / name)) == ["bridge_model.pt", "controller.pt"]
