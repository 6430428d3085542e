"""What the launchers of the LDS-DMA GEMM family (csrc/vt_gemm_{pws,pw,ppk,pt,pp,fast,f32r}.hip) enqueue: one case per template instantiation a
launcher can choose, each at the smallest shape that routes there, as a sha256 digest of every output buffer plus a comparison with an fp64 product
computed on the device.  tests/golden/g26_gemm_launch_parent.json holds the digests the commit BEFORE the family's shared tile order, DMA staging and
launch table moved into csrc/vt_gemm_tile.h / vt_gemm_route.h gave on an MI355X (tools/make_golden_gemm_launch_parent.py wrote it);
tests/test_gpu_gemm_launch_parent.py recomputes them.  That refactor left every kernel's device code as it was and rewrote the launchers' host code, so
every bit must be where it was.

A case builds its block with ops.gemm_block_params, sets the fields that function does not know (Wp, cmap, hn_*, xn_*, rs_*) on the block, asserts
vt_gemm_route_of's answer BEFORE it launches (as ops.gemm_block does) and launches through vt_gemm.  One group per route (`ROUTES`):
  PWS   (67 | 97, 128, 256) on the packed copy: one ragged m-tile / two m-tiles, the second ragged; bf16 and fp16, 16-bit C and fp32 C + residual;
        head norm on one 16-bit case; slab mode (67, 128, 512), splitk = 2
  PW    (2230, 2048, 512) on the packed copy, 14 x 16 tiles, the last row tile ragged: four dtype combinations at ring depth 4, the bf16 pair also
        at depth 8; the RMSNorm hand-off: producer (fp32 C + residual + xn_out / xn_part) and consumer (2230, 2048, 2048) reading the producer's
        xn_out and xn_part, both norm forms, bf16 and fp16
  PPK   the same shape without the packed copy, four dtype combinations
  PT    (4000, 3072, 1024), 16 x 12 tiles, the last row tile ragged: 16-bit C with none / GELU-erf / GELU-tanh, fp32 C + residual + column scale,
        the fused K|V tile stream; bf16 and fp16
  PP    the same shape with what the persistent tile lacks: no bias, SiLU, fp32 C with residual and no column scale, fp16 -> fp32 C, a two-segment
        head norm, cmap 1 / 2 / 3 without head norm
  GLDS  (1500, 1024, 64): 64-row tiles, two stages; (4096, 4096, 64): 128-row tiles, one stage; bf16 and fp16, 16-bit and fp32 C, cmap 1 / 2 / 3
  F32R  (200, 260, 1056) exact fp32

Bars of the fp64 comparison (max abs error over max abs reference; the project's, from test_gemm_packed_weights_tile, set at K = 2048 and no K here
is larger): 1e-2 for 16-bit C, 2e-4 for fp32 C, 2e-5 for raw split-K slabs.  Tile-stream outputs are compared through cases.kv_tile_stream."""
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn.functional as F

from tests import cases
from tests.train16_cases import digest

GOLDEN_NAME = "g26_gemm_launch_parent.json"
ROUTES = ("PWS", "PW", "PPK", "PT", "PP", "GLDS", "F32R")
BAR_C16, BAR_F32, BAR_SLAB = 1e-2, 2e-4, 2e-5
EPS = 1e-6
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS = OrderedDict([("bf16", BF16), ("fp16", F16)])
ACTS64 = {0: lambda x: x, 1: lambda x: F.gelu(x), 2: lambda x: F.gelu(x, approximate="tanh"), 3: F.silu}
ACT_NAMES = {0: "none", 1: "gelu_erf", 2: "gelu_tanh", 3: "silu"}
KV_FILL = 7.0       # what the tile-stream buffers hold before the launch (rows >= M of the last row block keep it or take zeros: part of the digest)


def rnd(shape, seed, dev, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def rel_err(got, ref) -> float:
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-12))


class Results:
    """sha256 per output buffer and (rel_err, bar) per fp64 comparison, both keyed `<route>/<case>/<buffer>`."""

    def __init__(self):
        self.sha, self.err = OrderedDict(), OrderedDict()

    def add(self, key, buf, ref=None, bar=None, err=None):
        self.sha[key] = digest(buf)
        if ref is not None or err is not None:
            self.err[key] = (rel_err(buf, ref) if err is None else err, bar)


_problem = {}


def problem(dev, M, N, K, dt, seed=40):
    """a [M, K], w [N, K] (scaled K^-0.5), bias [N], column scale [N], the fp64 product a w^T on the device; the last problem is kept (the cases of
    one shape and type follow each other)."""
    key = (str(dev), M, N, K, dt, seed)
    if _problem.get("key") != key:
        _problem.clear()
        a, w = rnd((M, K), seed + 1, dev, dt), rnd((N, K), seed + 2, dev, dt, K ** -0.5)
        _problem.update(key=key, a=a, w=w, bias=rnd((N,), seed + 3, dev), cs=rnd((N,), seed + 4, dev) + 1.0, y=a.double() @ w.double().t())
    return _problem


def launch_block(p, route, dev) -> None:
    """ops.gemm_block for a block with extra fields set: the route is asserted before the launch."""
    from vlatouch import _lib as L
    from vlatouch import ops
    got = ops.gemm_route(p)
    assert got == route, f"the dispatcher sends this block to {got}, the case expects {route}"
    L.check(L.lib().vt_gemm(C.byref(p), L.stream_ptr(dev)), "vt_gemm")


def head_norm64(x, segs, mode):
    """per-head (64 columns) RMSNorm of the columns [c0, c1) with gains g[64] for every (g, c0, c1) in segs; mode 1 mean-square, 2 unbiased variance."""
    x = x.clone()
    for g, c0, c1 in segs:
        h = x[:, c0:c1].reshape(x.shape[0], -1, 64)
        var = h.pow(2).mean(-1, keepdim=True) if mode == 1 else h.var(-1, keepdim=True)
        x[:, c0:c1] = (h * torch.rsqrt(var + EPS) * g.double()).reshape(x.shape[0], c1 - c0)
    return x


def kv_err(kv, ref, cmap, T) -> float:
    """tile stream [H, T, 2, 64, 64] against the fp64 rows ref [M, N]: cmap 1 = all columns are K, 2 = all are V, 3 = [K | V]."""
    M, N = ref.shape
    D = N // 2 if cmap == 3 else N
    k = ref[:, :D].reshape(M, D // 64, 64)
    v = ref[:, N - D:].reshape(M, D // 64, 64)
    want = cases.kv_tile_stream(k, v, T)
    ones = torch.ones(M, D // 64, 64, dtype=torch.bool, device=ref.device)
    valid = cases.kv_tile_stream(ones, ones, T, fill=False)
    worst = 0.0
    for part in ((0,) if cmap == 1 else (1,) if cmap == 2 else (0, 1)):
        got, exp = kv[:, :, part].double()[valid[:, :, part]], want[:, :, part][valid[:, :, part]]
        worst = max(worst, float((got - exp).abs().max() / (exp.abs().max() + 1e-12)))
    return worst


def linear(res, key, dev, route, M, N, K, dt, *, odt=None, bias=True, act=0, cs=False, residual=False, hn=None, hn_mode=1, cmap=0, wp=False,
           splitk=1, seed=40) -> None:
    """One launch and its fp64 comparison: C = residual + cs * act(headnorm(a w^T + bias)).  hn = column ends of the head-norm segments: (c0,) uses
    hn_w0 on [0, c0), (c0, c1) also hn_w1 on [c0, c1)."""
    from vlatouch import ops
    pr = problem(dev, M, N, K, dt, seed)
    a, w = pr["a"], pr["w"]
    odt = odt or dt
    b = pr["bias"] if bias else None
    r = rnd((M, N), seed + 5, dev, odt) if residual else None
    ref = pr["y"] + b.double() if bias else pr["y"]
    if splitk > 1:
        out = torch.zeros(splitk, M, N, dtype=F32, device=dev)
    elif cmap:
        T = (M + 63) // 64
        out = torch.full(((N // 2 if cmap == 3 else N) // 64, T, 2, 64, 64), KV_FILL, dtype=dt, device=dev)
    else:
        out = torch.zeros(M, N, dtype=odt, device=dev)
    p = ops.gemm_block_params(a, w, out.view(-1).as_strided((M, N), (N, 1)) if cmap else out, b, act=act, colscale=pr["cs"] if cs else None, residual=r, splitk=splitk)
    if cmap:
        p.cmap, p.cmap_T = cmap, T      # C = the stream's first byte, ldc = N: what ops.gemm passes
    gains = []
    if hn:
        gains = [1.0 + 0.1 * rnd((64,), seed + 6 + i, dev) for i in range(len(hn))]
        p.hn_w0, p.hn_c0_end = gains[0].data_ptr(), hn[0]
        p.hn_w1, p.hn_c1_end = (gains[1].data_ptr() if len(hn) > 1 else 0), hn[-1]
        p.hn_eps, p.hn_mode = EPS, hn_mode
        ref = head_norm64(ref, list(zip(gains, (0,) + tuple(hn[:-1]), hn)), hn_mode)
    if wp:
        wpk = ops.pack_w32(w)
        p.Wp = wpk.data_ptr()
    launch_block(p, route, dev)
    torch.cuda.synchronize(dev)
    if splitk > 1:
        return res.add(f"{route}/{key}/slabs", out, err=rel_err(out.double().sum(0), pr["y"]), bar=BAR_SLAB)
    if cmap:
        return res.add(f"{route}/{key}/kv", out, err=kv_err(out, ref, cmap, T), bar=BAR_C16)
    ref = ACTS64[act](ref)
    if cs:
        ref = ref * pr["cs"].double()
    if residual:
        ref = ref + r.double()
    res.add(f"{route}/{key}/C", out, ref, BAR_F32 if odt == F32 else BAR_C16)


def _pws(res, dev) -> None:
    from vlatouch import _lib as L
    for M in (67, 97):
        for n, dt in DTS.items():
            linear(res, f"M{M}/{n}_c16", dev, "PWS", M, 128, 256, dt, wp=True)
            linear(res, f"M{M}/{n}_f32_residual", dev, "PWS", M, 128, 256, dt, odt=F32, residual=True, cs=True, wp=True)
    linear(res, "M67/bf16_c16_headnorm", dev, "PWS", 67, 128, 256, BF16, hn=(128,), hn_mode=L.NORM_RMS_MEANSQ, wp=True)
    for n, dt in DTS.items():
        linear(res, f"M67/{n}_slabs", dev, "PWS", 67, 128, 512, dt, odt=F32, bias=False, splitk=2, wp=True)


PW_SHAPE = (2230, 2048, 512)


def _pw_pair(res, dev, n, dt, mode) -> None:
    """RMSNorm hand-off: C = residual + cs * (a W1^T + b1) (fp32) with xn_out = C * gain and xn_part on the side; then rmsnorm(C) * gain @ W2^T + b2."""
    from vlatouch import ops
    M, N, K = PW_SHAPE
    pr = problem(dev, M, N, K, dt)
    r, gain = rnd((M, N), 45, dev), 1.0 + 0.1 * rnd((N,), 46, dev)
    c = torch.zeros(M, N, dtype=F32, device=dev)
    xn, part = torch.zeros(M, N, dtype=dt, device=dev), torch.zeros(M, 2 * N // 128, 2, dtype=F32, device=dev)
    p = ops.gemm_block_params(pr["a"], pr["w"], c, pr["bias"], colscale=pr["cs"], residual=r)
    wp1 = ops.pack_w32(pr["w"])
    p.Wp, p.xn_out, p.xn_ld, p.xn_gain, p.xn_part, p.rs_mode = wp1.data_ptr(), xn.data_ptr(), xn.stride(0), gain.data_ptr(), part.data_ptr(), mode
    launch_block(p, "PW", dev)
    torch.cuda.synchronize(dev)
    c64 = r.double() + pr["cs"].double() * (pr["y"] + pr["bias"].double())
    key = f"PW/handoff_{n}_mode{mode}"
    res.add(f"{key}/producer_C", c, c64, BAR_F32)
    res.add(f"{key}/producer_xn_out", xn, c64 * gain.double(), BAR_C16)
    sums = c64.reshape(M, -1, 64).sum(-1)
    res.add(f"{key}/producer_xn_part_sums", part[:, :, 1].contiguous(), sums, BAR_F32)
    res.sha[f"{key}/producer_xn_part"] = digest(part)
    w2, b2 = rnd((N, N), 47, dev, dt, N ** -0.5), rnd((N,), 48, dev)
    out = torch.zeros(M, N, dtype=dt, device=dev)
    q = ops.gemm_block_params(xn, w2, out, b2)
    wp2 = ops.pack_w32(w2)
    q.Wp, q.rs_part, q.rs_n, q.rs_inv_k, q.rs_eps, q.rs_mode = wp2.data_ptr(), part.data_ptr(), part.shape[1], 1.0 / N, EPS, mode
    launch_block(q, "PW", dev)
    torch.cuda.synchronize(dev)
    var = c64.pow(2).mean(-1, keepdim=True) if mode == 1 else c64.var(-1, keepdim=True)
    ref = (c64 * torch.rsqrt(var + EPS) * gain.double()) @ w2.double().t() + b2.double()
    res.add(f"{key}/consumer_C", out, ref, BAR_C16)


def _pw(res, dev) -> None:
    from vlatouch import _lib as L
    lib = L.lib()
    M, N, K = PW_SHAPE
    try:
        for ring in (4, 8):
            L.check(lib.vt_tune(1, ring), "vt_tune")
            for n, dt in (DTS.items() if ring == 4 else [("bf16", BF16)]):
                linear(res, f"ring{ring}/{n}_c16_gelu_tanh", dev, "PW", M, N, K, dt, act=L.ACT_GELU_TANH, wp=True)
                linear(res, f"ring{ring}/{n}_f32_residual", dev, "PW", M, N, K, dt, odt=F32, residual=True, cs=True, wp=True)
    finally:
        lib.vt_tune(1, 0)
    for n, dt in DTS.items():
        for mode in (L.NORM_RMS_MEANSQ, L.NORM_RMS_VAR):
            _pw_pair(res, dev, n, dt, mode)


def _ppk(res, dev) -> None:
    M, N, K = PW_SHAPE
    for n, dt in DTS.items():
        linear(res, f"{n}_c16", dev, "PPK", M, N, K, dt)
        linear(res, f"{n}_f32_residual", dev, "PPK", M, N, K, dt, odt=F32, residual=True, cs=True)


SQ_SHAPE = (4000, 3072, 1024)


def _pt(res, dev) -> None:
    from vlatouch import _lib as L
    M, N, K = SQ_SHAPE
    for n, dt in DTS.items():
        for act in (L.ACT_NONE, L.ACT_GELU_ERF, L.ACT_GELU_TANH):
            linear(res, f"{n}_p16_{ACT_NAMES[act]}", dev, "PT", M, N, K, dt, act=act)
        linear(res, f"{n}_r32", dev, "PT", M, N, K, dt, odt=F32, residual=True, cs=True)
        linear(res, f"{n}_kv", dev, "PT", M, N, K, dt, cmap=3, hn=(N // 2,), hn_mode=L.NORM_RMS_MEANSQ)


def _pp(res, dev) -> None:
    from vlatouch import _lib as L
    M, N, K = SQ_SHAPE
    linear(res, "bf16_no_bias", dev, "PP", M, N, K, BF16, bias=False)
    linear(res, "bf16_silu", dev, "PP", M, N, K, BF16, act=L.ACT_SILU)
    linear(res, "bf16_f32_residual", dev, "PP", M, N, K, BF16, odt=F32, residual=True)
    for cmap in (1, 2, 3):
        linear(res, f"bf16_cmap{cmap}", dev, "PP", M, N, K, BF16, cmap=cmap)
    linear(res, "fp16_f32", dev, "PP", M, N, K, F16, odt=F32)
    linear(res, "fp16_headnorm_two_segments", dev, "PP", M, N, K, F16, hn=(1024, 2048), hn_mode=L.NORM_RMS_VAR)
    linear(res, "fp16_cmap3", dev, "PP", M, N, K, F16, cmap=3)


def _glds(res, dev) -> None:
    for tag, (M, N, K) in (("bm64_two_stages", (1500, 1024, 64)), ("bm128_one_stage", (4096, 4096, 64))):
        for n, dt in DTS.items():
            linear(res, f"{tag}/{n}_c16", dev, "GLDS", M, N, K, dt)
            linear(res, f"{tag}/{n}_f32", dev, "GLDS", M, N, K, dt, odt=F32, residual=True, cs=True)
            for cmap in ((1, 2, 3) if dt == BF16 else (3,)):
                linear(res, f"{tag}/{n}_cmap{cmap}", dev, "GLDS", M, N, K, dt, cmap=cmap)


def _f32r(res, dev) -> None:
    linear(res, "exact_fp32", dev, "F32R", 200, 260, 1056, F32)


GROUPS = OrderedDict([("PWS", _pws), ("PW", _pw), ("PPK", _ppk), ("PT", _pt), ("PP", _pp), ("GLDS", _glds), ("F32R", _f32r)])


def gemm_launch_cases(dev, routes=None) -> Results:
    res = Results()
    with torch.no_grad():
        for r in (routes or ROUTES):
            GROUPS[r](res, dev)
            torch.cuda.synchronize(dev)
    _problem.clear()
    return res
