"""vt_refresh16 (csrc/vt_refresh16.hip) as a unit: one read of an fp32 master writes the 16-bit copy, its zero-padded transpose and the
fragment-packed form of each.  Every output is compared bit for bit with the passes it replaces on the same master (ops.cast, then
transpose_pad, then ops.pack_w32 of each), on masters that hold the values where a conversion can go wrong; refusals and unrequested outputs
are checked with sentinels."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VT_ERR_ARG = -22
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FORMS = ("w16", "w16t", "wp", "wtp")
SENTINEL = 0x5A5A
# (N, K, row pitch or None, packed forms requested): the smallest shapes at which each part can go wrong
SHAPES = [(64, 256, None, True),        # one column block of the small-M tile, one k-chunk
          (256, 256, None, True),       # RDT_TINY's square Linear
          (320, 512, None, True),       # more than one tile each way, N not a power of two
          (256, 768, 800, True),        # pitched master
          (68, 40, None, False),        # ragged tiles, Np = 72: zero padding is written; no packed form exists
          (2048, 256, None, True), (256, 2048, None, True)]      # the embedder shapes


def _specials(dtype):
    """+-0, subnormals of the target type (smallest, largest, and one that rounds between two of them), values that round up across a binade
    (to 2.0 exactly, and a tie going to even), the largest finite value and one that rounds to inf, +-inf and a NaN."""
    fi = torch.finfo(dtype)
    eps, tiny, big = fi.eps, fi.tiny, fi.max
    sub = fi.smallest_subnormal if hasattr(fi, "smallest_subnormal") else tiny * eps
    return torch.tensor([0.0, -0.0, sub, -sub, tiny - sub, 2.5 * sub, 1.5 * sub, 0.4 * sub, 0.6 * sub, 2.0 - eps / 4, -(2.0 - eps / 4), 1.0 + eps / 2,
                         1.0 + 3 * eps / 2, 1.0 + eps / 2 + eps / 1024, big, -big, big * (1 + eps / 4), big * (1 + eps), float("inf"), -float("inf"),
                         float("nan"), 1e-30, -3.0e38], dtype=torch.float32)


def _master(N, K, pitch, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(N, pitch or K, generator=g) * torch.exp(4 * torch.randn(N, pitch or K, generator=g))
    sp = _specials(dtype)
    idx = torch.randperm(N * K, generator=g)[: 4 * sp.numel()]
    full[idx // K, idx % K] = sp.repeat(4)
    full[0, 0], full[N - 1, K - 1], full[N - 1, 0], full[0, K - 1] = float("nan"), -0.0, float("inf"), sp[2]      # the corners of the tiling
    return full.to(DEV)[:, :K]


def _two_pass(w, dtype, packed):
    """Today's path: cast, transpose_pad, and pack_w32 of each."""
    from vlatouch import ops
    from vlatouch.rdt_train import transpose_pad
    w16 = ops.cast(w.contiguous(), dtype)
    w16t = transpose_pad(w16)
    out = {"w16": w16, "w16t": w16t}
    if packed:
        out["wp"], out["wtp"] = ops.pack_w32(w16), ops.pack_w32(w16t)
    return out


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("N,K,pitch,packed", SHAPES)
def test_every_form_equals_the_two_pass_path_bit_for_bit(N, K, pitch, packed, dname):
    from vlatouch import ops
    dtype = DTYPES[dname]
    w = _master(N, K, pitch, dtype, seed=N + K)
    assert w.stride(0) == (pitch or K) and bool(torch.isnan(w).any()) and bool(torch.isinf(w).any())
    want = _two_pass(w, dtype, packed)
    forms = FORMS if packed else FORMS[:2]
    got = ops.refresh16(w, dtype, forms)
    torch.cuda.synchronize()
    Np = (N + 7) // 8 * 8
    assert got["w16"].shape == (N, K) and got["w16t"].shape == (K, Np)
    for f in forms:
        assert torch.equal(_bits(got[f]), _bits(want[f])), f"{f}: {int((_bits(got[f]) != _bits(want[f])).sum())} of {got[f].numel()} elements differ"
    if Np > N:
        assert not bool(_bits(got["w16t"])[:, N:].any()), "the padding columns of w16t must be zero"
    # and in place over buffers of an earlier call, as the trainer refreshes
    again = ops.refresh16(w * 2, dtype, forms, out=got)
    assert all(again[f].data_ptr() == got[f].data_ptr() for f in forms)
    assert torch.equal(_bits(again["w16"]), _bits(ops.cast((w * 2).contiguous(), dtype)))


def _raw(w_ptr, ldw, N, K, dt, bufs):
    from vlatouch import _lib as L
    return L.lib().vt_refresh16(C.c_void_p(w_ptr), ldw, N, K, dt, *(L.ptr(bufs.get(f)) for f in FORMS), L.stream_ptr(torch.device(DEV)))


def _sentinels(N, K):
    Np = (N + 7) // 8 * 8
    n = {"w16": N * K, "w16t": K * Np, "wp": N * K, "wtp": K * Np}
    return {f: torch.full((n[f] + 64,), SENTINEL, dtype=torch.int16, device=DEV) for f in FORMS}


@pytest.mark.parametrize("what", ["wp for (68, 40)", "wtp for (68, 40)", "null master", "N = 0", "K = 0", "N = -1", "fp32 dtype", "unknown dtype"])
def test_refusals_give_the_error_code_and_write_nothing(what):
    from vlatouch import _lib as L
    N, K = (68, 40) if "68" in what else (64, 256)
    w = torch.randn(N, K, device=DEV)
    bufs = _sentinels(N, K)
    use = dict(bufs)
    if what.startswith("wp"):
        use.pop("wtp")
    elif what.startswith("wtp"):
        use.pop("wp")
    dt = {"fp32 dtype": L.F32, "unknown dtype": 7}.get(what, L.BF16)
    n, k = {"N = 0": (0, K), "K = 0": (N, 0), "N = -1": (-1, K)}.get(what, (N, K))
    rc = _raw(0 if what == "null master" else w.data_ptr(), K, n, k, dt, use)
    torch.cuda.synchronize()
    assert rc == VT_ERR_ARG, (what, rc)
    assert L.lib().vt_last_error().decode().startswith("vt_refresh16")
    for f, t in bufs.items():
        assert bool((t == SENTINEL).all()), f"{what}: {f} was written"


@pytest.mark.parametrize("subset", [s for r in range(5) for s in itertools.combinations(FORMS, r)], ids=lambda s: "+".join(s) or "none")
def test_outputs_that_are_not_requested_are_never_touched(subset):
    """Every subset of the four pointers on (320, 512) fp16: the requested forms hold the two-pass bits, the others and the guard behind each
    buffer keep their sentinel."""
    N, K, dtype = 320, 512, torch.float16
    w = _master(N, K, None, dtype, seed=3)
    want = _two_pass(w, dtype, True)
    bufs = _sentinels(N, K)
    from vlatouch import _lib as L
    rc = _raw(w.data_ptr(), K, N, K, L.F16, {f: bufs[f] for f in subset})
    torch.cuda.synchronize()
    assert rc == 0, L.lib().vt_last_error().decode()
    for f in FORMS:
        n = want[f].numel()
        if f in subset:
            assert torch.equal(bufs[f][:n], _bits(want[f]).reshape(-1)), f
            assert bool((bufs[f][n:] == SENTINEL).all()), f"{f}: written past its end"
        else:
            assert bool((bufs[f] == SENTINEL).all()), f"{f} was not requested and was written"


def test_pack_w32_kept_its_layout():
    """vt_pack_w32 now takes its index from the header vt_refresh16 shares (csrc/vt_pack.h): its output against the layout spelled out in torch,
    [N / 32][K / 16][2 column halves][32 rows][8]."""
    from vlatouch import ops
    for N, K in ((64, 256), (320, 48)):
        w = torch.randn(N, K, device=DEV).to(torch.bfloat16)
        want = w.view(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
        assert torch.equal(_bits(ops.pack_w32(w)), _bits(want))
