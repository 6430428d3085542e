"""tests/vit_ref.py on the CPU: pinned to the fp32 oracles, the cost of every GPU case measured (the bars of tests/test_gpu_vit.py are 3 x the
largest cost of a group), each reference mutation shown to leave the bars, and the grids' coverage of the driver's paths asserted.

Measured here (the measure of vit_ref.row_err: per row max|a - b| / max|row|):
  oracle/dinov2.py (fp32) against vit_ref (fp64): 1.1e-6 over the cases below; oracle/siglip.py: 9.6e-7.  Asserted at 10 x: 1.1e-5 / 9.6e-6.
  The oracles' pixels against `prepare`: 4.7e-7 of the largest pixel (the fp32 roundings of / 255 and of the normalisation); every decision equal.
  Costs: vit_ref.COSTS, one line per group there."""
import numpy as np
import pytest
import torch

from tests import vit_ref as R

torch.set_grad_enabled(False)
ORACLE_DINO, ORACLE_SIGLIP, ORACLE_PIXELS = 1.1e-6, 9.6e-7, 4.7e-7


def emu(prec):
    return dict(adt=R.DT[prec], cdt=R.DT[prec], acc=torch.float32)


# ------------------------------------------------------------------------------------------------ pin the reference
def _oracle_input(c):
    return c["frames"] if c["pre_scale"] != 1.0 else torch.from_numpy(c["frames"]).float()       # numpy: the reference divides by 255 itself


def test_prepare_matches_oracle_on_every_decision():
    from oracle import dinov2
    worst = 0.0
    for name, c in R.decision_cases().items():
        if c["mode"] != R.AUTO:
            continue                                                    # ON / OFF / RAW are the driver's own modes
        px, scale, norm, mx, mean = R.prepare(c["frames"], c["layout"], c["pre_scale"], R.AUTO)
        got = dinov2.prepare_images(_oracle_input(c)).double().numpy()
        e = float(np.abs(got - px).max() / np.abs(px).max())
        worst = max(worst, e)
        assert e < 10 * ORACLE_PIXELS, (name, e)                        # a decision taken differently is an error of order 1
    print(f"oracle pixels vs prepare: {worst:.2e}")
    d = {n: R.prepare(c["frames"], c["layout"], c["pre_scale"], c["mode"])[1:3] for n, c in R.decision_cases().items()}
    assert d["u8_127"] == (1 / 255.0, 0.0) and d["u8_128"] == (1 / 255.0, 1.0) and d["f32_mean_half"] == (1.0, 1.0)
    assert d["f32_max_one"] == (1.0, 0.0) and d["f32_max_next"] == (1 / 255.0, 0.0) and d["u8_zero_one"] == (1.0, 1.0)
    assert d["numpy_u8_255"] == (1 / 255.0, 1.0) and d["raw_bright_byte"] == (1.0, 0.0) and d["off_bright_byte"] == (1 / 255.0, 0.0)
    assert d["on_dark"] == (1.0, 1.0) and d["f32_tail_max"][0] == 1 / 255.0 and d["u8_tail_max"][0] == 1 / 255.0 and d["f32_unaligned_max"][0] == 1 / 255.0


@pytest.mark.parametrize("swiglu", [False, True])
def test_blocks_match_dinov2_oracle(swiglu):
    from oracle import dinov2
    worst = 0.0
    for res, B in ((28, 3), (45, 2)):
        sd = R.dino_shapes_sd(128, 2, swiglu=swiglu, image_size=res)     # the table matches the grid: the oracle does not interpolate
        f = R.frame("bright", (B, 3, res, res), np.float32, res)
        px = R.prepare(f, "nchw", 1.0, R.AUTO)[0]
        got = dinov2.dinov2_forward(sd, dinov2.prepare_images(torch.from_numpy(f)), heads=2, return_tokens=True)
        ref = R.blocks(sd, R.tokens(sd, px, res // 14, R.pos_rows(sd, res // 14)), 2)
        worst = max(worst, R.row_err(got, ref))
    print(f"oracle dinov2 vs vit_ref: {worst:.2e}")
    assert worst < 10 * ORACLE_DINO, worst


def test_blocks_match_siglip_oracle():
    from oracle import siglip
    worst = 0.0
    for res, B in R.SIGLIP_RUNS:
        sd = R.siglip_shapes_sd(res)
        px = R.siglip_pixels(B, res, seed=res + B, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
        got = siglip.siglip_forward(sd, torch.from_numpy(px), heads=R.SIGLIP_HEADS)
        ref = R.blocks(sd, R.tokens(sd, px.astype(np.float64), res // 14, R.pos_rows(sd, res // 14)), R.SIGLIP_HEADS)
        worst = max(worst, R.row_err(got, ref))
    print(f"oracle siglip vs vit_ref: {worst:.2e}")
    assert worst < 10 * ORACLE_SIGLIP, worst


# ------------------------------------------------------------------------------------------------ measure the bars
def front_run(sd, c, **kw):
    px = np.concatenate([R.prepare(f, c["layout"], 1.0, R.AUTO)[0] for f in R.front_frames(c)])
    g = c["res"] // 14
    return R.tokens(sd, px, g, R.pos_rows(sd, g), **kw)


def front_costs(prec):
    out = []
    for hidden, heads in R.FRONT_MODELS:
        sd = R.dino_shapes_sd(hidden, 1, image_size=42)
        for c in R.front_cases():
            out.append(R.row_err(front_run(sd, c, **emu(prec)), front_run(sd, c)))
    return out


def dino_block_runs():
    for name, cfg in R.BLOCK_CONFIGS.items():
        sd = R.dino_shapes_sd(cfg["hidden"], cfg["layers"], swiglu=cfg["swiglu"], image_size=42)
        for n, (res, ncams, B) in enumerate(cfg["runs"]):
            yield name, cfg, sd, res, R.block_frames(res, ncams, B, seed=n + 1)


def dino_costs(prec):
    out = {}
    for name, cfg, sd, res, frames in dino_block_runs():
        if prec in cfg["precs"]:
            pos = R.pos_rows(sd, res // 14)
            got = R.dino_reference(sd, cfg["heads"], frames, pos, **emu(prec))[1]
            out[(name, res, len(frames), len(frames[0]))] = R.row_err(got, R.dino_reference(sd, cfg["heads"], frames, pos)[1])
    return out


def siglip_costs(prec, mean=(0.5,) * 3, std=(0.5,) * 3):
    out = []
    for res, B in R.SIGLIP_RUNS:
        sd = R.siglip_shapes_sd(res)
        px = R.siglip_pixels(B, res, seed=res + B, mean=mean, std=std).astype(np.float64)
        run = lambda **kw: R.blocks(sd, R.tokens(sd, px, res // 14, R.pos_rows(sd, res // 14), **kw), R.SIGLIP_HEADS, **kw)
        out.append(R.row_err(run(**emu(prec)), run()))
    return out


@pytest.fixture
def one_thread():
    """The costs are measured on one thread: a BLAS that splits a sum over threads moves an fp32 cost by up to 15 %."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _held(group, prec, costs):
    """The literal in vit_ref.COSTS is the largest measured cost rounded up to two digits.  Held from both sides: never 1.25 x above the
    measurement (a bar may not grow unnoticed), and the measurement at most 10 % above the literal (another CPU's BLAS sums fp32 in another
    order; the bars then stay the stricter ones recorded here)."""
    m, lit = max(costs), R.COSTS[(group, prec)]
    print(f"cost {group} {prec}: max {m:.3e} over {len(costs)} cases (literal {lit:.3e}, bar {R.BARS[(group, prec)]:.3e})")
    assert m <= 1.1 * lit and lit <= 1.25 * m, (group, prec, m, lit)
    assert R.BARS[(group, prec)] == 3.0 * lit


@pytest.mark.parametrize("prec", R.PRECS)
def test_costs_front(prec, one_thread):
    _held("front", prec, front_costs(prec))


@pytest.mark.parametrize("prec", R.PRECS)
def test_costs_dino_blocks(prec, one_thread):
    _held("dino", prec, list(dino_costs(prec).values()))


@pytest.mark.parametrize("prec", R.PRECS)
def test_costs_siglip(prec, one_thread):
    _held("siglip", prec, siglip_costs(prec) + siglip_costs(prec, R.IMAGENET_MEAN, R.IMAGENET_STD))


# ------------------------------------------------------------------------------------------------ sensitivity
def test_every_mutation_leaves_the_bars():
    """Each mutation of the reference moves at least one grid case past the widest bar of its group (bf16's), so a kernel with that error fails."""
    front_bar = max(R.BARS[("front", p)] for p in R.PRECS)
    dino_bar = max(R.BARS[("dino", p)] for p in R.PRECS)
    assert set(R.MUTATIONS) == {"swap_ij", "reverse_channels", "keep_remainder", "shift_pos", "cls_other_image", "layerscale_after_add", "mean_le", "max_ge"}
    for mut in ("swap_ij", "reverse_channels", "keep_remainder", "shift_pos"):
        sd = R.dino_shapes_sd(64, 1, image_size=42)
        worst = max(R.row_err(front_run(sd, c, mut=mut), front_run(sd, c)) for c in R.front_cases())
        print(f"{mut}: {worst:.3e} (bar {front_bar:.3e})")
        assert worst > 10 * front_bar, (mut, worst)
    for mut in ("cls_other_image", "layerscale_after_add"):
        worst = 0.0
        for name, cfg, sd, res, frames in dino_block_runs():
            pos = R.pos_rows(sd, res // 14)
            worst = max(worst, R.row_err(R.dino_reference(sd, cfg["heads"], frames, pos, mut=mut)[1][:, 0], R.dino_reference(sd, cfg["heads"], frames, pos)[1][:, 0]))
        print(f"{mut}: {worst:.3e} on the CLS rows (bar {dino_bar:.3e})")
        assert worst > 10 * dino_bar, (mut, worst)
    for mut, names in (("mean_le", ("f32_mean_half",)), ("max_ge", ("f32_max_one", "u8_zero_one", "numpy_u8_255"))):
        cs = R.decision_cases()
        for n in names:                                                 # the decision flags are compared exactly: one flipped flag is a failure
            c = cs[n]
            assert R.prepare(c["frames"], c["layout"], c["pre_scale"], c["mode"], mut=mut)[1:3] != R.prepare(c["frames"], c["layout"], c["pre_scale"], c["mode"])[1:3], (mut, n)


def test_siglip_scaling_defect_is_visible():
    """Dividing ImageNet-normalised pixels by 255 (the max > 1 rule the SigLIP route must not have) is far outside the SigLIP bars."""
    res, B = 28, 3
    sd = R.siglip_shapes_sd(res)
    px = R.siglip_pixels(B, res, seed=1, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD).astype(np.float64)
    assert abs(float(px.max()) - (1 - 0.406) / 0.225) < 1e-6
    run = lambda p: R.blocks(sd, R.tokens(sd, p, 2, R.pos_rows(sd, 2)), R.SIGLIP_HEADS)
    assert R.row_err(run(px / 255.0), run(px)) > 10 * max(R.BARS[("siglip", p)] for p in R.PRECS)


# ------------------------------------------------------------------------------------------------ coverage
def test_grids_cover_the_paths():
    # statistics: the three walks, an unaligned base, an extreme in the tail alone, both exact ties, the numpy-uint8 255
    walks = set()
    for et, shape in R.LARGE.items():
        w, chain = R.stat_walks(int(np.prod(shape)), 4 if et == "f32" else 1, True)
        assert "unrolled" in w and chain == 4, (et, w, chain)            # 201 243 vectors > 3 x 65 536
        walks |= w
    dc = R.decision_cases()
    for n, c in dc.items():
        walks |= R.stat_walks(c["frames"].size, c["frames"].itemsize, not c["offset"])[0]
    assert walks == {"unrolled", "vector", "scalar"}
    assert R.stat_walks(dc["f32_unaligned_max"]["frames"].size, 4, False)[0] == {"scalar"}
    for n in ("f32_tail_max", "u8_tail_max"):
        f = dc[n]["frames"].reshape(-1)
        V = 16 // f.itemsize
        assert f.size % V and f[: f.size // V * V].max() <= 1 < f[-1], n   # the only value above 1 lies behind the last whole vector
    assert float(dc["f32_max_one"]["frames"].max()) == 1.0 and float(dc["f32_mean_half"]["frames"].astype(np.float64).mean()) == 0.5
    assert dc["numpy_u8_255"]["frames"].max() == 255 and np.float32(255) * np.float32(1 / 255.0) == np.float32(1.0)
    assert {c["mode"] for c in dc.values()} == {R.AUTO, R.ON, R.OFF, R.RAW}
    # patchify: both paths in the 16-bit modes, odd res, remainder, nhwc, uint8, misaligned base (every case also runs offset), padding columns
    fc = R.front_cases()
    paths = {(R.patchify_path(c["layout"], c["et"], p, c["res"], al), c["res"] % 2, c["layout"], c["et"], al) for c in fc for p in R.PRECS for al in (True, False)}
    assert {("two", 0, "nchw", "f32", True), ("one", 1, "nchw", "f32", True), ("one", 0, "nchw", "f32", False), ("one", 0, "nhwc", "f32", True),
            ("one", 0, "nchw", "u8", True), ("one", 1, "nhwc", "u8", False)} <= paths
    assert {c["res"] % 14 for c in fc} >= {0, 1, 3} and {c["res"] // 14 for c in fc} == {1, 2, 3}
    assert all(R.kpad(p) > 588 for p in R.PRECS)                        # padding columns exist in every mode: the 0xFF-filled workspace sees them
    assert {(c["B"], len(c["kinds"])) for c in fc} == {(1, 1), (3, 1), (1, 2), (3, 2)}
    for c in fc:                                                        # two cameras decide differently; every decision keeps its distance
        fl = [R.prepare(f, c["layout"], 1.0, R.AUTO) for f in R.front_frames(c)]
        assert all(abs(f[4] - 0.5) > 0.05 and abs(f[3] - 1.0) > 0.05 for f in fl), c
        if len(fl) == 2:
            assert fl[0][2] != fl[1][2], c
    # the pruned last block: one layer = the pruned block alone, two = one full + one pruned; Bt of 1, 3 and 6; packed fc1 and split-K shapes
    runs = {(cfg["layers"], ncams * B) for cfg in R.BLOCK_CONFIGS.values() if cfg["hidden"] == 128 and not cfg["swiglu"] for _, ncams, B in cfg["runs"]}
    assert runs == {(l, bt) for l in (1, 2) for bt in (1, 3, 6)}
    p = R.BLOCK_CONFIGS["d256_packed"]
    res, ncams, B = p["runs"][0]
    assert ncams * B * ((res // 14) ** 2 + 1) == 65 and p["hidden"] % 256 == 0 and "fp32" not in p["precs"]
    s = R.BLOCK_CONFIGS["d512_splitk"]
    res, ncams, B = s["runs"][0]
    rows, Dm = ncams * B * ((res // 14) ** 2 + 1), 4 * s["hidden"]
    assert rows == 130 and rows > 64 and rows <= 1100 and Dm >= 2048 and (Dm // 64) % 4 == 0
    assert any(cfg["swiglu"] for cfg in R.BLOCK_CONFIGS.values())
    assert {r for r, _ in R.SIGLIP_RUNS} == {28, 42} and {b for _, b in R.SIGLIP_RUNS} == {1, 3}
