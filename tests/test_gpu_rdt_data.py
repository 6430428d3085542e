"""vt_rdt_batch (csrc/vt_rdt_data.hip) as a unit against an fp64 gather stated here, `EpisodeStore.assemble` on the fixture episodes against
the reference's recorded batches (tests/golden/g19_rdt_data.npz), and `finetune` / `sample_eval` fed by `EpisodeStore.batches` against the
same loops fed by batches assembled on the host (tests/rdt_data_ref.py).

Tolerances.  A gathered value (action rows, the unnoised state, the dataset mean, the element mask, the norms, the language rows) is one
fp64 number rounded once: it must equal float32(ref64) bit for bit.  The noised state is qpos + (0 + (std / c) * z), three fp64 operations
whose error (a few 1e-16 relative) is nine orders below fp32's half-ulp (6e-8): the result is float32(ref64) or its neighbour, so at most
1 fp32 ulp.  Against the golden (the reference's fp64 arrays) the only further difference is the 6-D rotation route, `sixd_route_err`
~1e-15, which can move a value across an fp32 rounding boundary as rarely: the same 1 ulp bound is used there for all arrays.
Outputs are NaN-filled with guard words after each buffer."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import cases
from tests import rdt_data_ref as R
from vlatouch import _lib as L
from vlatouch import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
MASK_FREQ, MASK_STATE, MASK_ELEM, NOISE = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------------ 1. the kernel as a unit
class Tables:
    """Synthetic device tables: episodes of 32, 40 and 100 steps; instructions of 1, 6 and Lmax = 9 tokens."""
    N = (32, 40, 100)
    LL = (1, 6, 9)

    def __init__(self, H, A, S, D, col_idx):
        g = np.random.default_rng(100 * H + A + S + D)
        self.H, self.A, self.S, self.D, self.col_idx = H, A, S, D, list(col_idx)
        self.qpos = [g.normal(size=(n, S)) for n in self.N]
        self.qpos[1][3, 0] = -0.0                                                 # a signed zero travels as it is
        self.stats = np.stack([np.stack([np.std(q, axis=0), np.mean(q, axis=0), np.sqrt(np.mean(q ** 2, axis=0))]) for q in self.qpos])
        self.mean = g.normal(size=S)
        self.lang = [g.normal(size=(l, D)).astype(np.float32) for l in self.LL]
        self.col_map = np.full(A, -1, dtype=np.int32)
        self.col_map[self.col_idx] = np.arange(S, dtype=np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        off = lambda xs: up(np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32))
        self.dev = dict(qpos=up(np.concatenate(self.qpos)), ep_off=off(self.qpos), stats=up(self.stats), mean=up(self.mean), col_map=up(self.col_map),
                        lang=up(np.concatenate(self.lang)), lang_off=off(self.lang))

    def fill(self, v):
        out = np.zeros(v.shape[:-1] + (self.A,))
        out[..., self.col_idx] = v
        return out

    def ref64(self, plans, z, c, freq):
        """The batch in fp64: (states, actions, elem_mask, state_norm, ctrl_freqs, lang, lang_mask)."""
        B, H = len(plans), self.H
        Lmax = max(self.LL[e] for e, _, _ in plans)
        st, ac, em, sn = np.zeros((B, 1, self.A)), np.zeros((B, H, self.A)), np.zeros((B, self.A)), np.zeros((B, self.A))
        fr, la, lm = np.zeros(B, dtype=np.int64), np.zeros((B, Lmax, self.D), dtype=np.float32), np.zeros((B, Lmax), dtype=bool)
        for b, (e, step, fl) in enumerate(plans):
            q = self.qpos[e]
            s = q[step]
            if fl & NOISE:
                s = s + (0.0 + (self.stats[e, 0] / c) * z[b])
            st[b, 0] = self.fill(self.mean if fl & MASK_STATE else s)
            ac[b] = self.fill(q[np.minimum(step + 2 + np.arange(H), len(q) - 1)])
            em[b] = self.fill(np.zeros(self.S) if fl & MASK_ELEM else np.ones(self.S))
            sn[b] = self.fill(self.stats[e, 2])
            fr[b] = 0 if fl & MASK_FREQ else freq
            la[b, :self.LL[e]], lm[b, :self.LL[e]] = self.lang[e], True
        return st, ac, em, sn, fr, la, lm, Lmax


def launch(t: Tables, plans, z, c, freq, Lmax, lang=None):
    """-> the seven outputs as numpy, after checking the guard words behind each.  lang: another device address of the language table."""
    B, H, A, S, D = len(plans), t.H, t.A, t.S, t.D
    buf = np.zeros(16 * B + 8 * B * S, dtype=np.uint8)
    buf[:16 * B].view(np.int32).reshape(B, 4)[:, :3] = plans
    buf[16 * B:].view(np.float64).reshape(B, S)[:] = z
    plan = torch.from_numpy(buf).to(DEV)
    shapes = dict(states=(B, 1, A), actions=(B, H, A), elem=(B, A), norm=(B, A), lang=(B, Lmax, D))
    bufs = {k: torch.full((int(np.prod(s)) + GUARD,), float("nan"), dtype=torch.float32, device=DEV) for k, s in shapes.items()}
    bufs["freq"] = torch.full((B + GUARD,), -7, dtype=torch.int64, device=DEV)
    bufs["lmask"] = torch.full((B * Lmax + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    d = t.dev
    code = L.lib().vt_rdt_batch(L.ptr(d["qpos"]), L.ptr(d["ep_off"]), L.ptr(d["stats"]), L.ptr(d["mean"]), L.ptr(d["col_map"]),
                                L.ptr(d["lang"]) if lang is None else C.c_void_p(lang), L.ptr(d["lang_off"]), len(t.N), S, A, H, D, Lmax, freq,
                                C.c_double(c), L.ptr(plan), B, L.ptr(bufs["states"]),
                                L.ptr(bufs["actions"]), L.ptr(bufs["elem"]), L.ptr(bufs["norm"]), L.ptr(bufs["freq"]), L.ptr(bufs["lang"]),
                                L.ptr(bufs["lmask"]), L.stream_ptr(DEV))
    L.check(code, "vt_rdt_batch")
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, s in shapes.items():
        assert np.isnan(host[k][-GUARD:]).all(), f"guard words after {k} were written"
    assert (host["freq"][-GUARD:] == -7).all() and (host["lmask"][-GUARD:] == 0xA5).all()
    out = [host[k][:-GUARD].reshape(s) for k, s in shapes.items()]
    return out[:4] + [host["freq"][:-GUARD], out[4], host["lmask"][:-GUARD].reshape(B, Lmax)]


def ulp_distance(a32, ref64):
    """|a - float32(ref)| in fp32 ulps, through the ordered integer view (both signs)."""
    ordered = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    r = ref64.astype(np.float32)
    return np.abs(ordered(np.ascontiguousarray(a32)) - ordered(r))


def bits_equal(a32, ref64):
    return np.array_equal(np.ascontiguousarray(a32).view(np.int32), ref64.astype(np.float32).view(np.int32))


def kernel_cases(t: Tables):
    """(episode, step, flags): the first drawable step, the last one (the chunk runs past the end and pads), chunks that need no padding, the
    32-step episode, each mask alone and all together, noise on and off, every instruction length."""
    h2 = t.H // 2
    last = lambda e: max(t.N[e] - h2 - 1, 0)                  # H = 64: the 32-step episode has no drawable step; the kernel takes any row of it
    free = [(2, 0, 0), (2, max(t.N[2] - t.H - 2, 0), NOISE)]                       # step + 2 + H <= N: no padding
    return [(0, 0, 0), (0, last(0), NOISE), (1, 3, MASK_FREQ), (1, last(1), MASK_STATE), (2, 5, MASK_ELEM), *free,
            (1, 7, MASK_FREQ | MASK_STATE | MASK_ELEM | NOISE), (0, 1, MASK_STATE | NOISE), (2, last(2), NOISE), (1, 0, NOISE), (0, 5, MASK_ELEM | NOISE)]


SHAPES = {"h8": (8, 128, 10, 32, R.STATE_INDICES), "h64": (64, 128, 10, 32, R.STATE_INDICES), "h4_nonmonotone": (4, 16, 3, 30, (9, 2, 5)),
          "h8_unaligned_lang": (8, 128, 10, 30, R.STATE_INDICES)}
_tables = {}


def tables(key) -> Tables:
    if key not in _tables:
        _tables[key] = Tables(*SHAPES[key])
    return _tables[key]


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_fp64_gather(shape, B):
    t = tables(shape)
    allc = kernel_cases(t)
    assert t.N[2] >= t.H + 2 and all(0 <= s < t.N[e] for e, s, _ in allc)
    g = np.random.default_rng(7 + B)
    c, freq = float(np.sqrt(10 ** (40 / 10))), 25
    for k in range(0, len(allc), B):
        plans = allc[k:k + B]
        z = g.normal(size=(len(plans), t.S))
        st, ac, em, sn, fr, la, lm, Lmax = t.ref64(plans, z, c, freq)
        got = launch(t, plans, z, c, freq, Lmax)
        again = launch(t, plans, z, c, freq, Lmax)
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "two calls differ"
        assert bits_equal(got[1], ac) and bits_equal(got[2], em) and bits_equal(got[3], sn), (shape, plans)
        assert np.array_equal(got[4], fr) and np.array_equal(got[5].view(np.int32), la.view(np.int32)) and np.array_equal(got[6], lm.astype(np.uint8))
        for b, (e, step, fl) in enumerate(plans):
            if fl & NOISE and not fl & MASK_STATE:
                d = ulp_distance(got[0][b], st[b])
                assert d.max() <= 1, (shape, plans[b], int(d.max()))
                assert bits_equal(got[0][b][0][t.col_map < 0], st[b][0][t.col_map < 0])        # the unmapped columns stay exact zeros
            else:
                assert bits_equal(got[0][b], st[b]), (shape, plans[b])


def test_language_table_at_a_misaligned_base_takes_the_scalar_path():
    """D = 32 allows 128-bit words, but a table that starts 4 bytes past a 16-byte boundary does not: same bits through the scalar copy."""
    t = tables("h8")
    plans = [(0, 0, 0), (1, 3, 0), (2, 5, 0)]
    z = np.zeros((3, t.S))
    la, lm, Lmax = t.ref64(plans, z, 1.0, 25)[5:]
    shifted = torch.zeros(t.dev["lang"].numel() + 1, dtype=torch.float32, device=DEV)
    shifted[1:] = t.dev["lang"].flatten()
    assert shifted.data_ptr() % 16 == 0
    got = launch(t, plans, z, 1.0, 25, Lmax, lang=shifted.data_ptr() + 4)
    assert np.array_equal(got[5].view(np.int32), la.view(np.int32)) and np.array_equal(got[6], lm.astype(np.uint8))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, launch(t, plans, z, 1.0, 25, Lmax)))


def test_kernel_refuses_bad_shapes_without_a_launch():
    t = tables("h8")
    d = t.dev
    out = torch.full((4096,), float("nan"), dtype=torch.float32, device=DEV)
    plan = torch.zeros(64, dtype=torch.uint8, device=DEV)
    good = dict(E=3, S=10, A=128, H=8, D=32, Lmax=2, freq=25, c=1.0, B=1, plan=plan.data_ptr(), qpos=d["qpos"].data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        o = C.c_void_p(out.data_ptr())
        return L.lib().vt_rdt_batch(C.c_void_p(a["qpos"]), L.ptr(d["ep_off"]), L.ptr(d["stats"]), L.ptr(d["mean"]), L.ptr(d["col_map"]), L.ptr(d["lang"]),
                                    L.ptr(d["lang_off"]), a["E"], a["S"], a["A"], a["H"], a["D"], a["Lmax"], a["freq"], C.c_double(a["c"]),
                                    C.c_void_p(a["plan"]), a["B"], o, o, o, o, o, o, o, L.stream_ptr(DEV))

    for bad in (dict(B=0), dict(E=0), dict(S=0), dict(A=9), dict(H=0), dict(D=0), dict(Lmax=0), dict(c=0.0), dict(c=float("nan")), dict(B=70000),
                dict(H=65533), dict(plan=plan.data_ptr() + 4), dict(plan=0), dict(qpos=0)):
        assert call(**bad) == -22, bad
        assert b"vt_rdt_batch" in L.lib().vt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ 2. assemble on the fixture store
def _store(**kw):
    from vlatouch.rdt_data import EpisodeStore
    args = dict(dataset_name=R.DATASET_NAME, dataset_names=R.DATASET_NAMES, control_freq=R.CONTROL_FREQ, device=DEV)
    args.update(kw)
    return EpisodeStore(R.FIXTURE_DIR, **args)


@pytest.fixture(scope="module")
def G():
    return dict(np.load(R.GOLDEN))


@pytest.mark.parametrize("seed", R.G19_SEEDS)
def test_assemble_equals_the_reference_batch(G, seed):
    store = _store()
    torch.manual_seed(seed)
    plans = store.draw(R.G19_B, np_rng=np.random.RandomState(seed), rng=random.Random(seed), generator=None, **R.G19_KW)
    batch = store.assemble(plans)
    again = store.assemble(plans)
    torch.cuda.synchronize()
    for key in ("states", "actions", "state_elem_mask", "state_norm"):
        got = batch[key].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == G[f"gi_{seed}_{key}"].shape
        assert ulp_distance(got, G[f"gi_{seed}_{key}"]).max() <= 1, key
        assert torch.equal(batch[key], again[key])
    assert batch["ctrl_freqs"].dtype == torch.int64 and np.array_equal(batch["ctrl_freqs"].cpu().numpy(), G[f"gi_{seed}_ctrl_freqs"])
    assert batch["data_indices"] == list(G[f"gi_{seed}_data_indices"])
    assert np.array_equal(batch["lang_embeds"].cpu().numpy(), G[f"gi_{seed}_lang_embeds"])
    assert batch["lang_attn_mask"].dtype == torch.bool and np.array_equal(batch["lang_attn_mask"].cpu().numpy(), G[f"gi_{seed}_lang_attn_mask"])
    resident = store._dev["frames"]
    for b, p in enumerate(plans):
        assert len(batch["frames"][b]) == 6
        for q, f in enumerate(batch["frames"][b]):
            if G[f"gi_{seed}_fr_background"][b, q]:
                assert f is None
                continue
            src = resident[p.episode][q % 3]
            assert f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (12, 16, 3)
            assert f.data_ptr() == src.data_ptr() + p.frame_idx[q // 3] * src.stride(0)                  # a view into the resident episode, no copy
            assert f[6, 8].tolist() == list(G[f"gi_{seed}_fr_sig"][b, q])
        jitter = batch["jitter"][b] if batch["jitter"] is not None else [None] * 6
        assert [j is not None for j in jitter] == list(G[f"gi_{seed}_fr_jittered"][b])


def test_frames_beyond_the_cap_stay_on_the_host():
    full = _store().upload()
    one = 40 * 12 * 16 * 3                                                         # episode_2's frames of one camera
    capped = _store(max_device_bytes=2 * one + 100).upload()                       # episode_2 fits; 100 bytes are left, so the later episodes do not
    hosted = _store(frames="host").upload()
    split = _store(max_device_bytes=one).upload()                                  # room for one camera of episode_2: episodes are taken whole, so none goes up
    assert split.host_frame_bytes == hosted.host_frame_bytes and all(isinstance(f, np.ndarray) for e in split._dev["frames"] for f in e if f is not None)
    assert full.host_frame_bytes == 0 and hosted.host_frame_bytes == 2 * (40 + 57 + 45) * 576 and capped.host_frame_bytes == hosted.host_frame_bytes - 2 * one
    assert full.resident_bytes - capped.resident_bytes == capped.host_frame_bytes
    plans = full.draw(4, np_rng=np.random.RandomState(1), rng=random.Random(1), cond_mask_prob=0.0)
    assert {p.episode for p in plans} == {0, 1, 2}
    a, b, c = full.assemble(plans), capped.assemble(plans), hosted.assemble(plans)
    for p, fa, fb, fc in zip(plans, a["frames"], b["frames"], c["frames"]):
        for x, y, z in zip(fa, fb, fc):
            if x is None:
                assert y is None and z is None
                continue
            assert isinstance(z, np.ndarray) and (isinstance(y, torch.Tensor) and y.is_cuda) == (p.episode == 0)
            assert np.array_equal(x.cpu().numpy(), np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)) and np.array_equal(x.cpu().numpy(), z)
    assert torch.equal(a["actions"], c["actions"])


# ------------------------------------------------------------------------------------------------ 3. the loops
def _tower_and_preprocessor():
    from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
    from vlatouch.imgprep import DevicePreprocessor
    S = 64                                                                         # the small tower of the raw-frames test of the colour jitter
    c = dict(synth.SIGLIP_CONFIGS["tiny"], image_size=S)
    vcfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"], image_size=S,
                patch_size=14)
    tower = SiglipVisionTower("synthetic", None, device=DEV, precision="fp32", state_dict=cases.sd_torch(synth.siglip_shapes(**c), prefix="siglip-tiny64."),
                              config=vcfg)
    pp = DevicePreprocessor(S, [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], DEV, torch.float32, pad=True, brightness=True, image_size=None)
    return tower, pp


def _rngs(seed):
    return dict(np_rng=np.random.RandomState(seed), rng=random.Random(seed), generator=torch.Generator().manual_seed(seed))


def test_finetune_and_sample_eval_from_the_store_equal_the_host_feed():
    """gradient_accumulation_steps = 2, two optimizer steps: four micro-batches of two samples drawn with image_aug on, cond_mask_prob 0.5 and
    no state noise.  Run a is fed by store.batches, run r by the same samples assembled on the host in fp64 (frames as host arrays): losses,
    weights and EMA weights are bit-equal; then a sample_eval visit over each feed with the sample-loader settings gives the same dict."""
    from tests.test_gpu_rdt_train import _runner
    from vlatouch.rdt_train import finetune, sample_eval
    tower, pp = _tower_and_preprocessor()
    cfg = dict(cases.RDT_TINY, img_token_dim=tower.hidden_size, img_cond_len=6 * tower.num_patches)
    store, ds = _store(horizon=cfg["horizon"]), R.Dataset(horizon=cfg["horizon"])
    assert len(store.episodes) == len(ds.eps) == 5
    draw = dict(cond_mask_prob=0.5, state_noise_snr=None, image_aug=True)
    r_rngs = _rngs(5)
    host = [R.host_batch(ds, 2, r_rngs["np_rng"], r_rngs["rng"], r_rngs["generator"], **draw) for _ in range(5)]
    flat = [f for b in host[:4] for s in b["frames"] for f in s]
    jit = [j for b in host[:4] for s in b["jitter"] for j in s]
    assert any(f is None for f in flat) and sum(f is not None for f in flat) >= 8 and 0 < sum(j is not None for j in jit) < len(jit)
    kw = dict(lr=1e-3, gradient_accumulation_steps=2)
    a, r = _runner(cfg).trainer(**kw), _runner(cfg).trainer(**kw)
    torch.manual_seed(31)                                                          # train_step's own draws (noise, timesteps) come from the device generator
    la = finetune(a, store.batches(2, **_rngs(5), **draw), max_train_steps=2, vision_encoder=tower, preprocessor=pp)
    torch.manual_seed(31)
    lr = finetune(r, host, max_train_steps=2, vision_encoder=tower, preprocessor=pp)
    assert len(la) == len(lr) == 4 and a.global_step == r.global_step == 2
    assert all(torch.equal(x, y) for x, y in zip(la, lr)), ([float(x) for x in la], [float(y) for y in lr])
    sa, sr = a.state_dict(), r.state_dict()
    assert set(sa) == set(sr) and all(torch.equal(sa[k], sr[k]) for k in sa)
    ea, er = a.ema_state_dict(), r.ema_state_dict()
    assert all(torch.equal(ea[k], er[k]) for k in ea)
    # the periodic sampling evaluation over each feed
    sample = dict(cond_mask_prob=0, state_noise_snr=None, image_aug=False)
    s_rngs = _rngs(9)
    shost = [R.host_batch(ds, 2, s_rngs["np_rng"], s_rngs["rng"], s_rngs["generator"], **sample) for _ in range(2)]
    names = {i: n for i, n in enumerate(R.DATASET_NAMES)}
    ev = dict(num_sample_batches=2, dataset_id2name=names, vision_encoder=tower, preprocessor=pp)
    torch.manual_seed(32)
    ma = sample_eval(a.sampler(), store.batches(2, **_rngs(9), **sample), **ev)
    torch.manual_seed(32)
    mr = sample_eval(a.sampler(), shost, **ev)
    assert ma == mr and set(ma) == {"mango_sample_mse", "mango_sample_l2err", "overall_avg_sample_mse", "overall_avg_sample_l2err"}
    assert all(np.isfinite(v) for v in ma.values())
