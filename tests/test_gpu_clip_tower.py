"""The CLIP tower with deep visual prompts (ClipEngine on vt_dino_forward, csrc/vt_models.hip + vt_prompt_seam.hip) against the float64
statement of tests/clip_ref.py.

Shapes: patch 14, res = image_size in {28, 42} (5 and 10 tokens), D in {64, 128} (1 and 2 heads) x n_ctx in {0, 3, 8}, 3 layers; prompt depths
P in {0, 1, 2, 3 (-1)}: no prompts, drop at block 1, overwrite + gate + drop, prompts to the end with the CLS-only last block attending to the
prompt rows as keys; Bt in {1, 3}; fp32, bf16, fp16.  Compared: the pooled output (the pruned engine) and post_layernorm of every row the last
block carries (the out_all engine, prompt rows included when P = layers); and the same two at the inner block boundaries, as the towers cut
after block 1 and after block 2 put them out (clip_ref.cut: same weights, depth min(P, m); a cut tower's rows are the whole tower's residual
stream at that boundary on every row the boundary hands on).  One case at D = 512, mlp 2048, Bt (N + n) = 7 x 13 = 91 > 64 rows, so fc2 takes
the split-K + slab-reduction branch behind a quick-GELU fc1.

The measure is vit_ref.row_err.  A bar is 3 x the largest cost of the statement on the CPU with the precision's rounding points and fp32
arithmetic (clip_ref.COSTS, measured over exactly these cases, cuts included, and held by tests/test_clip_ref_host.py):

  group    cost fp32   bf16     fp16      bar fp32   bf16     fp16
  tower    1.4e-6      1.1e-2   1.2e-3    4.2e-6     3.3e-2   3.6e-3

The gate cannot be seen in any output of the tower: a gated tail is overwritten by the next block's VPT_shallow or dropped, and the last block
does not gate.  What the gate computes is held bit for bit by tests/test_gpu_prompt_seam.py.  VPT_gamma of block 1, the one gate a 3-layer
tower reads, takes each of -4, 0 and 5 over the grid (clip_ref.tower_sd rotates them); here that only proves that nothing leaks."""
import functools

import pytest
import torch

from tests import clip_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(name, res, P, B):
    """The float64 statement of one case, computed once and shared by the three precisions: (weights, pixels, pooler_output, every row)."""
    sd = R.tower_sd(name, res, P)
    px = R.pixels(B, res, seed=res + B)
    _, pool64, every64 = R.forward(sd, px, R.TOWER_CONFIGS[name]["heads"], P)
    return sd, px, pool64, every64


@functools.lru_cache(maxsize=None)
def cut_reference(name, res, P, B, m):
    sd, px, _, _ = reference(name, res, P, B)
    sd_m, P_m = R.cut(sd, m, P)
    _, pool64, every64 = R.forward(sd_m, px, R.TOWER_CONFIGS[name]["heads"], P_m)
    return sd_m, px, pool64, every64


def engines(sd, heads, P, prec, dev):
    from vlatouch.clip import ClipEngine
    return (ClipEngine(sd, heads=heads, precision=prec, device=dev, prompt_depth=P),
            ClipEngine(sd, heads=heads, precision=prec, device=dev, prompt_depth=P, out_all=True))


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("name,res,P", R.tower_cases(), ids=[f"{n}-r{r}-P{p}" for n, r, p in R.tower_cases()])
def test_tower_pooled_and_every_token(dev, name, res, P, prec):
    c = R.TOWER_CONFIGS[name]
    sd = reference(name, res, P, R.BATCHES[0])[0]
    pooled_eng, full_eng = engines(sd, c["heads"], P, prec, dev)
    depth = R.depth(R.LAYERS, P) if c["n_ctx"] else 0
    assert pooled_eng.prompt_depth == depth and pooled_eng.n_ctx == (c["n_ctx"] if depth else 0) and pooled_eng.image_size == res
    bar, fails = R.BARS[("tower", prec)], []
    for B in R.BATCHES:
        _, px, pool64, every64 = reference(name, res, P, B)
        x = torch.from_numpy(px)
        pooled = pooled_eng.forward(x).cpu()
        every = full_eng.forward_tokens(x).cpu()
        assert pooled.shape == pool64.shape and every.shape == every64.shape
        assert every.shape[1] == (res // 14) ** 2 + 1 + (c["n_ctx"] if depth == R.LAYERS else 0)
        e_pool, e_all, e_row0 = R.row_err(pooled, pool64), R.row_err(every, every64), R.row_err(every[:, 0], pool64)
        print(f"clip {name} res {res} P {P} {prec} B {B}: pooled {e_pool:.3e}, every token {e_all:.3e}, out_all row 0 {e_row0:.3e} (bar {bar:.3e})")
        if not (e_pool <= bar and e_all <= bar and e_row0 <= bar):
            fails.append((B, e_pool, e_all, e_row0, bar))
    # the inner block boundaries: the tower cut after block 1 and after block 2 (clip_ref.cut), every row and the pruned CLS row
    for m in R.CUTS:
        sd_m, P_m = R.cut(sd, m, P)
        pooled_m, full_m = engines(sd_m, c["heads"], P_m, prec, dev)
        assert full_m.layers == m and full_m.prompt_depth == (P_m if c["n_ctx"] else 0)
        for B in R.BATCHES:
            _, px, pool64, every64 = cut_reference(name, res, P, B, m)
            x = torch.from_numpy(px)
            every, pooled = full_m.forward_tokens(x).cpu(), pooled_m.forward(x).cpu()
            assert every.shape == every64.shape
            e_all, e_pool = R.row_err(every, every64), R.row_err(pooled, pool64)
            print(f"clip {name} res {res} P {P} {prec} B {B} boundary {m}: every token {e_all:.3e}, pooled {e_pool:.3e} (bar {bar:.3e})")
            if not (e_all <= bar and e_pool <= bar):
                fails.append((f"boundary {m}", B, e_all, e_pool, bar))
    assert not fails, fails


@pytest.mark.parametrize("prec", R.PRECS)
def test_split_k_fc2_behind_quick_gelu(dev, prec):
    s = R.SPLITK
    sd = R.clip_sd(s["hidden"], R.LAYERS, s["inter"], s["res"], s["n_ctx"], s["prompt_depth"])
    rows = s["B"] * ((s["res"] // 14) ** 2 + 1 + s["n_ctx"])
    assert rows > 64 and s["inter"] >= 2048 and (s["inter"] // 64) % 4 == 0 and rows <= 1100            # vt_dino_forward's split-K condition
    pooled_eng, full_eng = engines(sd, s["heads"], s["prompt_depth"], prec, dev)
    px = R.pixels(s["B"], s["res"], seed=s["res"] + s["B"])
    _, pool64, every64 = R.forward(sd, px, s["heads"], s["prompt_depth"])
    x = torch.from_numpy(px)
    e_pool, e_all = R.row_err(pooled_eng.forward(x).cpu(), pool64), R.row_err(full_eng.forward_tokens(x).cpu(), every64)
    bar = R.BARS[("tower", prec)]
    print(f"clip split-K {prec}: pooled {e_pool:.3e}, every token {e_all:.3e} (bar {bar:.3e})")
    assert e_pool <= bar and e_all <= bar, (e_pool, e_all, bar)


def test_image_0_does_not_depend_on_the_batch(dev):
    """fp32: image 0's pooled row at Bt = 3 equals its row at Bt = 1 bit for bit, with the prompt rows running to the end."""
    name, res, P = "d128_n8", 42, -1
    sd = R.tower_sd(name, res, P)
    eng, _ = engines(sd, 2, P, "fp32", dev)
    px = torch.from_numpy(R.pixels(3, res, seed=9))
    a = eng.forward(px).cpu()
    b = eng.forward(px[:1]).cpu()
    assert torch.equal(a[:1], b)


def test_refusals(dev):
    import ctypes as C
    from vlatouch import _lib as L
    from vlatouch.clip import ClipEngine, clip_pack
    sd = R.tower_sd("d64_n3", 28, 2)
    eng = ClipEngine(sd, heads=1, precision="fp32", device=dev)
    assert eng.prompt_depth == 2 and eng.n_ctx == 3                  # the depth is read off the VPT_shallow keys
    with pytest.raises(L.VtError):
        eng.forward(torch.zeros(1, 3, 42, 42))                       # res != image_size, on the host
    lib = L.lib()
    x = torch.zeros(1, 3, 42, 42, device=dev)
    out, pos = torch.zeros(1, 64, device=dev), torch.zeros(9, 64, device=dev)
    ws = torch.zeros(lib.vt_dino_workspace_bytes(eng._h, 1, 42), dtype=torch.uint8, device=dev)
    call = lambda res: lib.vt_dino_forward(eng._h, L.ptr_array([x]), 1, 0, 0, C.c_float(1.0), L.IMGNORM_RAW, 1, res, L.ptr(pos), L.ptr(out), None, L.ptr(ws),
                                           L.stream_ptr(dev))
    assert call(42) == -22 and b"image_size" in lib.vt_last_error()  # and in the driver, before any launch
    names, W, f = clip_pack(sd, heads=1, cdt=L.F32)
    Wd = [w.to(dev) for w in W]

    def create(n_weights=None, **over):
        d = L.DinoDesc()
        for k, v in f.items():
            if k != "pos_patch":
                setattr(d, k, v)
        d.cdt = d.adt = L.F32
        d.eps, d.act, d.pre_ln = 1e-5, L.ACT_QUICK_GELU, 1
        for k, v in over.items():
            setattr(d, k, v)
        h = C.c_void_p()
        rc = lib.vt_dino_create(C.byref(d), L.ptr_array(Wd), len(Wd) if n_weights is None else n_weights, C.byref(h))
        if rc == 0:
            lib.vt_dino_destroy(h)
        return rc

    assert create() == 0
    assert create(prompt_depth=4) == -22                             # prompt_depth > layers
    assert create(no_cls=1) == -22                                   # prompt rows without a CLS token
    assert create(n_prompt=-1) == -22
    assert create(n_weights=len(Wd) - 1) == -22
    torch.cuda.synchronize(dev)
