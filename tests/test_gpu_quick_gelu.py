"""VT_ACT_QUICK_GELU (7): x * sigmoid(1.702 x) as the element-wise epilogue of vt_gemm and vt_mlp, against an fp64 product on the device.

One case per route the fc1 of a ViT FFN (16-bit or fp32 C, bias, activation) can take, at the smallest tile-crossing shape of
tests/gemm_launch_cases.py that routes there: REG (fp32 and 16-bit operands), PWS on the packed copy, GLDS, PPK, PT (its own template
instantiation of the activation) and PP (the persistent tile switched off).  The activations are scaled so that a w^T + bias spans more than
+-12: both tails of the sigmoid (exp overflow side included) are met; the test asserts that span on the reference.

vt_gemm is measured PER ELEMENT against a tolerance that follows from the arithmetic alone (the fp64 reference takes the same, already
rounded operands):
  tol_ij = 1.1 (K + 2) 2^-24 S_ij   fp32 accumulation of the K products and the bias in any order, S_ij = sum_k |a_ik w_jk| + |b_j| (computed in
                                    fp64 on the device), carried through the activation, whose slope is at most 1.1
         + 8 2^-24 |ref_ij|         the epilogue's hardware exp2 and reciprocal (1 ulp each) and its two products
         + u (|ref_ij| + the above) one rounding to the output type: u = 2^-8 (bf16), 2^-11 (fp16), 0 (fp32)
The figure printed and asserted is the largest |out - ref| / tol over the elements (<= 1).  So that another activation cannot pass for this
one, the same figure is formed for tanh-GELU and for SiLU of the same pre-activations in place of the device's output, and must exceed 3.

vt_mlp (three Linears, two activations, hidden activations stored in the mode's type) is measured by row_err against the float64 chain; its
bar is 3 x the cost of the same chain on the CPU in fp32 arithmetic with the mode's rounding points, measured in the test before the device
is asked.  In fp32 the chain with tanh-GELU in place of quick-GELU must lie more than 3 bars away.  In the 16-bit modes it does not (2.0e-3
against bars of 1.9e-2 and 2.1e-3: at most 0.02 of absolute difference under rows that reach beyond 12), so there the figure is printed
only; what tells the activations apart in 16 bits is the per-element test above, on the same vt_gemm launches vt_mlp makes."""
import ctypes as C

import pytest
import torch

from tests import gemm_launch_cases as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
UNIT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}      # half an ulp: 8 / 11 significand bits
ACT = 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def quick_gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def operands(dev, M, N, K, dt, seed=70):
    """-> a, w, bias, the fp64 pre-activations, and the per-element tolerance of the docstring for an output of type dt."""
    a = G.rnd((M, K), seed + 1, dev, dt, 4.0)                       # a w^T ~ N(0, 16): spans +-12 and beyond
    w, b = G.rnd((N, K), seed + 2, dev, dt, K ** -0.5), G.rnd((N,), seed + 3, dev)
    pre = a.double() @ w.double().t() + b.double()
    assert float(pre.min()) < -12.0 and float(pre.max()) > 12.0, (float(pre.min()), float(pre.max()))
    S = a.double().abs() @ w.double().abs().t() + b.double().abs()
    ref = quick_gelu64(pre)
    fp32_side = 1.1 * (K + 2) * 2.0 ** -24 * S + 8 * 2.0 ** -24 * ref.abs()
    tol = fp32_side + UNIT[dt] * (ref.abs() + fp32_side)
    return a, w, b, pre, ref, tol


CASES = [
    ("REG", 67, 128, 256, F32, False), ("REG", 67, 128, 256, BF16, False), ("REG", 67, 128, 256, F16, False),
    ("PWS", 67, 128, 256, BF16, True), ("PWS", 97, 128, 256, F16, True),
    ("GLDS", 1500, 1024, 64, BF16, False), ("GLDS", 1500, 1024, 64, F16, False),
    ("PPK", 2230, 2048, 512, BF16, False), ("PPK", 2230, 2048, 512, F16, False),
    ("PT", 4000, 3072, 1024, BF16, False), ("PT", 4000, 3072, 1024, F16, False),
    ("PP", 4000, 3072, 1024, BF16, False),
]


@pytest.mark.parametrize("route,M,N,K,dt,packed", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{str(c[4]).split('.')[-1]}" for c in CASES])
def test_gemm_quick_gelu(dev, route, M, N, K, dt, packed):
    from vlatouch import _lib as L
    from vlatouch import ops
    assert L.ACT_QUICK_GELU == ACT
    a, w, b, pre, ref, tol = operands(dev, M, N, K, dt)
    # another activation in this one's place must be far outside the tolerance: the test can tell them apart
    others = {"gelu_tanh": torch.nn.functional.gelu(pre, approximate="tanh"), "silu": torch.nn.functional.silu(pre)}
    apart = {n: float(((o - ref).abs() / tol).max()) for n, o in others.items()}
    assert min(apart.values()) > 3.0, apart
    out = torch.zeros(M, N, dtype=dt, device=dev)
    p = ops.gemm_block_params(a, w, out, b, act=ACT)
    if packed:
        wpk = ops.pack_w32(w)
        p.Wp = wpk.data_ptr()
    lib = L.lib()
    if route == "PP":
        L.check(lib.vt_tune(8, 0), "vt_tune")                       # every PT becomes PP
    try:
        G.launch_block(p, route, dev)
        torch.cuda.synchronize(dev)
    finally:
        if route == "PP":
            lib.vt_tune(8, 1)
    assert bool(torch.isfinite(out).all())
    e = float(((out.double() - ref).abs() / tol).max())
    print(f"quick-gelu {route} {M}x{N}x{K} {dt}: worst |out - ref| / tol = {e:.3f}; tanh-GELU would give {apart['gelu_tanh']:.1f}, SiLU {apart['silu']:.1f}")
    assert e <= 1.0, (route, e)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_mlp_quick_gelu(dev, prec):
    """vt_mlp: Linear, quick-GELU, Linear, quick-GELU, Linear (the last without activation), 67 rows, hidden activations in the mode's type."""
    from vlatouch.engine import MlpEngine
    dt = {"fp32": F32, "bf16": BF16, "fp16": F16}[prec]
    dims = (256, 128, 192, 64)
    sd = {}
    for j in range(3):
        sd[f"{2 * j}.weight"] = G.rnd((dims[j + 1], dims[j]), 80 + j, "cpu", F32, (4.0 if j == 0 else 1.0) * dims[j] ** -0.5)
        sd[f"{2 * j}.bias"] = G.rnd((dims[j + 1],), 90 + j, "cpu")
    from tests.vit_ref import rnd, row_err
    x = G.rnd((67, 256), 99, "cpu", dt, 4.0)

    def chain(act, acc, rdt):
        h = x.to(acc)
        for j in range(3):
            h = h @ rnd(sd[f"{2 * j}.weight"].to(acc), rdt).t() + sd[f"{2 * j}.bias"].to(acc)
            if j == 0 and acc == torch.float64:
                assert float(h.min()) < -12.0 and float(h.max()) > 12.0
            if j < 2:
                h = rnd(act(h), rdt)                                 # the hidden activations are stored in the mode's type
        return h

    rdt = None if prec == "fp32" else dt
    ref = chain(quick_gelu64, torch.float64, None)
    cost = row_err(chain(quick_gelu64, torch.float32, rdt), ref)     # what the format alone costs, on the CPU
    bar = 3.0 * cost
    other = row_err(chain(lambda t: torch.nn.functional.gelu(t, approximate="tanh"), torch.float64, None), ref)
    if prec == "fp32":                                               # only fp32 resolves the two activations through two more Linears (see the module's text)
        assert other > 3.0 * bar, (other, bar)
    eng = MlpEngine(sd, act=ACT, precision=prec, device=dev)
    got = eng(x.to(dev), torch.float32)
    e = row_err(got.cpu(), ref)
    print(f"vt_mlp quick-gelu {prec}: {e:.3e} (CPU cost {cost:.3e}, bar {bar:.3e}; tanh-GELU would give {other:.3e})")
    assert e <= bar, (prec, e, bar)
