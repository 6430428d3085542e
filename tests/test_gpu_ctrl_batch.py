"""vt_ctrl_batch and vt_ctrl_pixsum (csrc/vt_ctrl_data.hip) as units, without the DINOv2 tower: hand-built tables with random CLS rows
(the two normalisation modes of a frame are different random rows, so a wrong decision shows as a wrong row) against the batch the trainers'
`_prepare_batch*` build on the host path (tests/ctrl_data_ref.py).

Tolerance: none.  Every output is a copy (features, forces, the state row: one fp64 -> fp32 rounding, as `torch.as_tensor(.., float32)`
rounds it) or the arithmetic of vt_action_normalize on a value rounded the same way, so `torch.equal` is asserted on every tensor.  Every
batch mean used is at least 0.01 away from 0.5.  Outputs carry guard words behind each buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ctrl_data_ref as R
from vlatouch import _lib as L
from vlatouch import ctrl_data as CD
from vlatouch import eval as ev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
DV, HV, FD = 384, 20, 3
P = 28 * 28 * 3
N = (40, 43, 46)
ERR_ARG = -22


class Tables:
    """Three episodes of 40, 43 and 46 frames.  Camera 1 is bright in episode 0, dark in episode 1 and alternates (even frames bright) in
    episode 2; camera 2 is the opposite.  A frame's byte sum is its level times P plus a few counts."""

    def __init__(self):
        g = np.random.default_rng(2024)
        self.eps = [R.synth_episode(n, 10 + i, HV, FD) for i, n in enumerate(N)]
        self.ep_off = np.concatenate([[0], np.cumsum(N)]).astype(np.int32)
        rows = int(self.ep_off[-1])
        self.feat = g.normal(size=(2, rows, 2, DV)).astype(np.float32)
        level = np.zeros((2, rows), dtype=np.int64)
        for e, n in enumerate(N):
            fr = np.arange(n)
            cam1 = [np.full(n, R.BRIGHT), np.full(n, R.DARK), np.where(fr % 2 == 0, R.BRIGHT, R.DARK)][e]
            level[0, self.ep_off[e]:self.ep_off[e + 1]] = cam1
            level[1, self.ep_off[e]:self.ep_off[e + 1]] = R.BRIGHT + R.DARK - cam1
        self.pix = level * P + g.integers(0, 100, size=level.shape)
        self.stats = ev.normalization_stats(self.eps)
        stab = np.stack([self.stats[k] for k in ("action_mins", "action_maxs", "vla_mins", "vla_maxs")]).astype(np.float32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        pose = np.concatenate([ev.converted_ee_pose_with_gripper(ep) for ep in self.eps])
        self.dev = dict(pose10=up(pose), vla=up(np.concatenate([ep["vla_action"] for ep in self.eps])),
                        forces=up(np.concatenate([ep["gelsight_force/forces"] for ep in self.eps]).astype(np.float32)), ep_off=up(self.ep_off),
                        feat=up(self.feat), pix_sum=up(self.pix), stats=up(stab))

    def mean(self, plan, cf, cam):
        rows = np.array([self.ep_off[e] + s + cf - 1 for e, s in plan])
        return float(self.pix[cam][rows].sum()) / (255.0 * len(plan) * P)


_t = []


def tables() -> Tables:
    if not _t:
        _t.append(Tables())
    return _t[0]


def launch(t, plan, *, cf, h, layout, use_force, kin, check=True, **over):
    """-> (code, outputs as device tensors) after checking the guard words behind each buffer."""
    B = len(plan)
    bridge = layout == "bridge"
    shapes = dict(obs_in=(B, kin), expert_act=(B, h, 10), vla_act=(B, h, 10), forces=(B, h, FD), norm_flags=(2,))
    if bridge:
        shapes["current_force"] = (B, FD)
    bufs = {k: torch.full((int(np.prod(s)) + GUARD,), 12345.0, dtype=torch.float32, device=DEV) for k, s in shapes.items()}
    plan_dev = torch.tensor(plan, dtype=torch.int32, device=DEV).reshape(B, 2)
    d = t.dev
    a = dict(pose10=d["pose10"].data_ptr(), E=len(N), rows=int(t.ep_off[-1]), Hv=HV, Fd=FD, dv=DV, P=P, cf=cf, h=h, layout=CD.LAYOUTS[layout], B=B, kin=kin,
             plan_ptr=plan_dev.data_ptr(), cur=bufs["current_force"].data_ptr() if bridge else 0, flags=bufs["norm_flags"].data_ptr())
    for k in ("cf", "h", "layout", "kin"):                    # `<name>_arg`: the value goes to the call only, the buffers keep the good size
        if k + "_arg" in over:
            a[k] = over.pop(k + "_arg")
    a.update(over)
    code = L.lib().vt_ctrl_batch(C.c_void_p(a["pose10"]), L.ptr(d["vla"]), L.ptr(d["forces"]), L.ptr(d["ep_off"]), L.ptr(d["feat"]), L.ptr(d["pix_sum"]),
                                 a["E"], C.c_longlong(a["rows"]), a["Hv"], a["Fd"], a["dv"], C.c_longlong(a["P"]), L.ptr(d["stats"]), C.c_float(1.4),
                                 a["cf"], a["h"], a["layout"], int(use_force), C.c_void_p(a["plan_ptr"]), a["B"], L.ptr(bufs["obs_in"]), a["kin"],
                                 L.ptr(bufs["expert_act"]), L.ptr(bufs["vla_act"]), L.ptr(bufs["forces"]), C.c_void_p(a["cur"]),
                                 C.c_void_p(a["flags"]), L.stream_ptr(DEV))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[-GUARD:] == 12345.0).all()), f"guard words after {k} were written"
    if check:
        L.check(code, "vt_ctrl_batch")
    return code, {k: b[:-GUARD].reshape(shapes[k]) for k, b in bufs.items()}


def reference(t, plan, **kw):
    return R.batch_reference(t.eps, plan, t.feat, t.pix, t.ep_off, P, t.stats, device=DEV, **kw)


def assert_same(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (what, k, float((got[k] - ref[k]).abs().max()))


def grid_plan(t, B, cf, h):
    """B windows over the three episodes with the first and the last valid start of an episode and one window twice; re-drawn (next seed)
    until both cameras' batch means are 0.01 away from 0.5."""
    for seed in range(100):
        g = np.random.default_rng(1000 * B + 10 * cf + h + 7919 * seed)
        plan = [(int(e), int(g.integers(0, N[e] - cf - h + 1))) for e in g.integers(0, 3, size=B)]
        if B >= 5:
            plan[0], plan[1], plan[3] = (2, 0), (2, N[2] - cf - h), plan[2]
        elif seed % 2:
            plan[0] = (1, N[1] - cf - h)
        if all(abs(t.mean(plan, cf, c) - 0.5) >= 0.01 for c in range(2)):
            return plan
    raise AssertionError("no plan away from 0.5")


@pytest.mark.parametrize("h", [8, 16])
@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_batch_equals_the_host_path(B, cf, h):
    t = tables()
    plan = grid_plan(t, B, cf, h)
    for layout in ("bridge", "lstm"):
        for use_force in (True, False):
            width = 2 * DV + 10 + (FD if layout == "bridge" and use_force else 0)
            kin = (width + 15) // 16 * 16
            kw = dict(cf=cf, h=h, layout=layout, use_force=use_force, kin=kin)
            _, got = launch(t, plan, **kw)
            assert_same(got, reference(t, plan, **kw), (layout, use_force, plan))
            assert bool((got["obs_in"][:, width:] == 0).all())
            _, again = launch(t, plan, **kw)
            assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got), "two calls differ"


def test_unpadded_row_takes_the_scalar_copy():
    """in_pad = 2 dv + 10 + Fd = 781 is no multiple of 4 floats: rows are not 16-byte aligned, the features go through the scalar loop."""
    t = tables()
    plan = [(0, 3), (1, 0), (2, 11), (2, 12), (0, 3)]
    kw = dict(cf=2, h=8, layout="bridge", use_force=True, kin=781)
    assert_same(launch(t, plan, **kw)[1], reference(t, plan, **kw), "kin 781")


@pytest.mark.parametrize("layout", ["bridge", "lstm"])
def test_decisions_are_the_batchs_not_the_frames(layout):
    t = tables()
    cf, h = 2, 8
    kw = dict(cf=cf, h=h, layout=layout, use_force=True, kin=784)
    f = lambda frame: (2, frame - (cf - 1))                    # the window of episode 2 whose image is `frame` (even: camera 1 bright, camera 2 dark)
    cases = {
        "camera 1 on, camera 2 off": ([(0, 0), (0, 5), (0, N[0] - cf - h)], (1.0, 0.0)),
        "camera 1 off, camera 2 on": ([(1, 0), (1, 7), (1, N[1] - cf - h)], (0.0, 1.0)),
        "3 bright + 1 dark on camera 1": ([f(2), f(4), f(6), f(5)], (1.0, 0.0)),
        "1 bright + 3 dark on camera 1": ([f(2), f(3), f(5), f(7)], (0.0, 1.0)),
    }
    feat = torch.from_numpy(t.feat).to(DEV)
    for what, (plan, want) in cases.items():
        means = [t.mean(plan, cf, c) for c in range(2)]
        assert all(abs(m - 0.5) >= 0.01 for m in means), (what, means)
        _, got = launch(t, plan, **kw)
        assert got["norm_flags"].tolist() == list(want), (what, means)
        assert_same(got, reference(t, plan, **kw), what)
        rows = [int(t.ep_off[e]) + s + cf - 1 for e, s in plan]
        for c in range(2):
            assert torch.equal(got["obs_in"][:, c * DV:(c + 1) * DV], feat[c, rows, int(want[c])]), (what, c)
    # the mixed batches: per frame the dark one (0.16) would go unnormalised and the bright one (0.78) normalised; the batch decides for all four
    means = [t.mean([f(5)], cf, 0), t.mean([f(2)], cf, 0)]
    assert means[0] < 0.49 and means[1] > 0.51
    assert launch(t, [f(5)], **kw)[1]["norm_flags"].tolist() == [0.0, 1.0] and launch(t, [f(2)], **kw)[1]["norm_flags"].tolist() == [1.0, 0.0]


def test_entries_outside_the_tables_read_nothing():
    """An episode outside [0, E) gives NaN rows and adds nothing to the sums; a start outside its episode is clamped into it."""
    t = tables()
    cf, h = 2, 8
    kw = dict(cf=cf, h=h, layout="bridge", use_force=True, kin=784)
    good = [(0, 4), (0, 9), (0, 11)]
    _, ref = launch(t, good, **kw)
    _, got = launch(t, [good[0], (3, 0), good[1], (-1, 5), good[2]], **kw)
    keep = [0, 2, 4]
    for k in ("obs_in", "expert_act", "vla_act", "forces", "current_force"):
        assert bool(torch.isnan(got[k][[1, 3]]).all()), k
        if k != "obs_in":
            assert torch.equal(got[k][keep], ref[k]), k
    # 3 bright frames among B = 5 entries: 2 * sum < 255 * 5 * P (0.47), so camera 1 goes unnormalised where the three alone (0.78) would not
    assert ref["norm_flags"].tolist() == [1.0, 0.0] and got["norm_flags"].tolist() == [0.0, 0.0]
    rows = [int(t.ep_off[e]) + s + cf - 1 for e, s in good]
    assert torch.equal(got["obs_in"][keep, :DV], torch.from_numpy(t.feat[0, rows, 0]).to(DEV))
    assert torch.equal(got["obs_in"][keep, DV:], ref["obs_in"][:, DV:])
    _, a = launch(t, [(1, 10 ** 6), (1, -5)], **kw)
    _, b = launch(t, [(1, N[1] - cf - h), (1, 0)], **kw)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_kernel_refuses_bad_arguments_without_a_launch():
    t = tables()
    plan = [(0, 3), (1, 4)]
    base = dict(cf=2, h=8, layout="bridge", use_force=True, kin=784, check=False)
    bads = [dict(B=0), dict(E=0), dict(rows=0), dict(Hv=0), dict(Fd=0), dict(dv=0), dict(P=0), dict(cf=0), dict(h=0), dict(Hv=7), dict(layout=2),
            dict(kin=780), dict(kin=0), dict(plan_ptr=0), dict(pose10=0), dict(flags=0), dict(cur=0), dict(B=(1 << 20) + 1),
            dict(pose10=t.dev["pose10"].data_ptr() + 8)]
    for bad in bads:
        over = {(k + "_arg" if k in ("cf", "h", "layout", "kin") else k): v for k, v in bad.items()}
        code, out = launch(t, plan, **base, **over)
        assert code == ERR_ARG, bad
        assert b"vt_ctrl_batch" in L.lib().vt_last_error()
        assert all(bool((o == 12345.0).all()) for o in out.values()), bad
    code, _ = launch(t, plan, cf=2, h=8, layout="lstm", use_force=True, kin=777, check=False)      # smaller than 2 dv + 10 (the LSTM row has no force columns)
    assert code == ERR_ARG
    code, _ = launch(t, plan, cf=2, h=8, layout="lstm", use_force=True, kin=778, check=False, cur=0)
    assert code == 0                                           # 778 is the LSTM row, and it needs no current_force


@pytest.mark.parametrize("shape", [(5, 28, 28, 3), (3, 1001), (2, 384 * 384 * 3)])
def test_pixsum_is_the_exact_byte_sum(shape):
    g = np.random.default_rng(shape[0])
    frames = g.integers(0, 256, size=shape, dtype=np.uint8)
    frames[0] = 0                                              # an all-black frame
    frames[-1] = 255
    n, p = shape[0], int(np.prod(shape[1:]))
    want = frames.reshape(n, -1).astype(np.uint64).sum(axis=1)
    dev = torch.from_numpy(frames).to(DEV)
    out = torch.full((n + GUARD,), -7, dtype=torch.int64, device=DEV)
    for _ in range(2):
        L.check(L.lib().vt_ctrl_pixsum(L.ptr(dev), C.c_longlong(p), n, L.ptr(out), L.stream_ptr(DEV)), "vt_ctrl_pixsum")
        torch.cuda.synchronize()
        assert out[:n].cpu().numpy().astype(np.uint64).tolist() == want.tolist() and bool((out[n:] == -7).all())
    assert int(want[0]) == 0 and int(want[-1]) == 255 * p
    for bad in (dict(p=0), dict(n=0), dict(src=0), dict(dst=0)):
        a = dict(dict(p=p, n=n, src=dev.data_ptr(), dst=out.data_ptr()), **bad)
        assert L.lib().vt_ctrl_pixsum(C.c_void_p(a["src"]), C.c_longlong(a["p"]), a["n"], C.c_void_p(a["dst"]), L.stream_ptr(DEV)) == ERR_ARG
