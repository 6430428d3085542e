"""Which GEMM kernel a parameter block takes (csrc/vt_gemm_route.hip through vt_gemm_route_of / vt_gemm_route_split).  Host code only: no GPU.

EXPECTED was not produced by the code under test: it is the decision of the commit BEFORE the routing function existed, taken by calling that
build's exported eligibility predicates through ctypes in the order its three launchers evaluated them (the differential sweep of the change that
introduced vt_gemm_route: 200 000 seeded random blocks, every outcome reached, no mismatch).  A route that changes here is a behaviour change of
the dispatcher and needs its own measurement; it is never fixed by editing the table alone.
"""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vla-touch_amd"))

from vlatouch import _lib as L  # noqa: E402

PTR = 4096      # any non-null pointer: the route depends on which pointers are set, never on where they point


def blk(M, N, K, dt=L.BF16, cdt=None, wdt=None, wp=False, bias=True, res=False, cs=False, act=L.ACT_NONE, **fields):
    """A Linear's block as the drivers' lin() builds it; `fields` sets anything else by name (pointer fields: True -> PTR)."""
    p = L.GemmParams()
    p.A = p.W = p.C = PTR
    p.M, p.N, p.K = M, N, K
    p.lda, p.ldw, p.ldc = K, K, N
    p.groups = p.splitk = 1
    p.a_dtype = dt
    p.w_dtype = dt if wdt is None else wdt
    p.c_dtype = dt if cdt is None else cdt
    p.act = act
    if wp:
        p.Wp = PTR
    if bias:
        p.bias = PTR
    if res:
        p.residual, p.ldr = PTR, N
    if cs:
        p.colscale = PTR
    for k, v in fields.items():
        setattr(p, k, PTR if v is True else v)
    return p


def cases():
    c = {}
    # RDT-1B (hidden 2048): the Linears of one denoise step on M = 67 * B rows, with and without the fragment-packed copy of the weights
    D = 2048
    for B in (1, 2, 8, 32):
        for wp in (False, True):
            tag = f"B={B}{' Wp' if wp else ''}"
            M = 67 * B
            c[f"rdt qkv {tag}"] = blk(M, 3 * D, D, wp=wp)
            c[f"rdt proj {tag}"] = blk(M, D, D, cdt=L.F32, res=True, wp=wp)
            c[f"rdt cross-q {tag}"] = blk(M, D, D, wp=wp)
            c[f"rdt fc1 {tag}"] = blk(M, D, D, act=L.ACT_GELU_TANH, wp=wp)
            c[f"rdt fc2 {tag}"] = blk(M, D, D, cdt=L.F32, res=True, wp=wp)
    # the same at batch 1 as the small-batch split of the denoise loop issues them: fp32 slabs, 4 k-slices, epilogue left to the slab reduction
    c["rdt qkv B=1 slabs Wp"] = blk(67, 3 * D, D, cdt=L.F32, bias=False, wp=True, splitk=4, c_slab=67 * 3 * D)
    c["rdt qkv B=1 slabs"] = blk(67, 3 * D, D, cdt=L.F32, bias=False, splitk=4, c_slab=67 * 3 * D)
    # RMSNorm hand-off at batch 32: producer (residual Linear) and consumer sides; a block the weights-in-registers tile does not fit is unsupported
    hand = dict(xn_out=True, xn_ld=D, xn_gain=True, xn_part=True)
    c["rdt proj B=32 Wp hand-off producer"] = blk(2144, D, D, cdt=L.F32, res=True, wp=True, **hand)
    c["rdt qkv B=32 Wp hand-off consumer"] = blk(2144, 3 * D, D, wp=True, rs_part=True, rs_n=32, rs_inv_k=1.0 / D, rs_eps=1e-6)
    c["hand-off producer, M=3000 does not fit pw"] = blk(3000, D, D, cdt=L.F32, res=True, wp=True, **hand)
    c["hand-off producer without packed weights"] = blk(2144, D, D, cdt=L.F32, res=True, **hand)
    c["hand-off consumer, rs_n=34"] = blk(2144, 3 * D, D, wp=True, rs_part=True, rs_n=34)
    # cached-condition K|V projection (cmap 3, K half head-normed) on the image condition of 32 samples, and on one sample's language tokens
    R = 32 * 4374
    c["rdt cond K|V 32 x 4374 rows"] = blk(R, 2 * D, D, cmap=3, cmap_T=(R + 63) // 64, hn_w0=True, hn_c0_end=D, hn_c1_end=D, hn_eps=1e-6, hn_mode=1)
    c["rdt cond K|V cmap 3, 120 rows"] = blk(120, 2 * D, D, cmap=3, cmap_T=2)
    # DINOv2-B (hidden 768, fp16) at 64 images: M = 64 * 257; fc1's ragged last row block is split off
    Dd, Md = 768, 16448
    c["dino-b qkv"] = blk(Md, 3 * Dd, Dd, dt=L.F16)
    c["dino-b proj"] = blk(Md, Dd, Dd, dt=L.F16, cdt=L.F32, res=True, cs=True)
    c["dino-b fc1"] = blk(Md, 4 * Dd, Dd, dt=L.F16, act=L.ACT_GELU_ERF)
    c["dino-b fc1 Wp"] = blk(Md, 4 * Dd, Dd, dt=L.F16, act=L.ACT_GELU_ERF, wp=True)
    c["dino-b fc1 64-row remainder"] = blk(64, 4 * Dd, Dd, dt=L.F16, act=L.ACT_GELU_ERF)
    c["dino-b fc1 64-row remainder Wp"] = blk(64, 4 * Dd, Dd, dt=L.F16, act=L.ACT_GELU_ERF, wp=True)
    c["dino-b fc2"] = blk(Md, Dd, 4 * Dd, dt=L.F16, cdt=L.F32, res=True, cs=True)
    c["dino-b fc2 batch 1 (514 rows)"] = blk(514, Dd, 4 * Dd, dt=L.F16, cdt=L.F32, res=True, cs=True)
    c["dino-b fc2 batch 1 slabs"] = blk(514, Dd, 4 * Dd, dt=L.F16, cdt=L.F32, bias=False, splitk=4, c_slab=514 * Dd)
    # SigLIP so400m (hidden 1152, FFN 4304) on 6 images x 729 patches, and on 32 samples of them
    Ds, Fs = 1152, 4304
    for Ms in (4374, 32 * 4374):
        c[f"siglip qkv M={Ms}"] = blk(Ms, 3 * Ds, Ds, dt=L.F16)
        c[f"siglip proj M={Ms}"] = blk(Ms, Ds, Ds, dt=L.F16, cdt=L.F32, res=True)
        c[f"siglip fc1 M={Ms}"] = blk(Ms, Fs, Ds, dt=L.F16, act=L.ACT_GELU_TANH)
        c[f"siglip fc2 M={Ms}"] = blk(Ms, Ds, Fs, dt=L.F16, cdt=L.F32, res=True)
    # exact fp32 either side of the ring kernel's `tiles of 128 x 128 < 1024`, split-bf16 (x3), a conv product, fp32 activations on bf16 weights
    c["fp32 4096 x 3968 x 4096 (992 tiles)"] = blk(4096, 3968, 4096, dt=L.F32)
    c["fp32 4096 x 4096 x 4096 (1024 tiles)"] = blk(4096, 4096, 4096, dt=L.F32)
    c["x3 512 x 512 x 1280"] = blk(512, 512, 1280, dt=L.F32, wdt=L.F32X3)
    c["x3 512 x 512 x 1288 (K % 64)"] = blk(512, 512, 1288, dt=L.F32, wdt=L.F32X3)
    c["x3 conv 5 taps x 256 channels"] = blk(512, 512, 1280, dt=L.F32, wdt=L.F32X3, taps=5, cin=256, tout=16, tin=16, stride=1, off0=-2, tstep=1)
    c["x3 conv 5 taps x 24 channels, 4 slices"] = blk(512, 256, 120, dt=L.F32, wdt=L.F32X3, bias=False, taps=5, cin=24, tout=16, tin=16, stride=1, off0=-2,
                                                      tstep=1, splitk=4, c_slab=512 * 256)
    c["fp32 A x bf16 W"] = blk(64, 256, 256, dt=L.F32, wdt=L.BF16, cdt=L.F32)
    c["bf16 tiny M"] = blk(2, 2048, 256)
    # what two GPU tests state in their docstrings but can only check numerically
    c["(3000, 2048, 2048) Wp keeps the old tiles"] = blk(3000, 2048, 2048, wp=True)
    c["(8193, 6144, 512) head norm is not split"] = blk(8193, 6144, 512, hn_w0=True, hn_c0_end=2048, hn_w1=True, hn_c1_end=4096, hn_eps=1e-6, hn_mode=1)
    c["(8193, 6144, 512) plain"] = blk(8193, 6144, 512)
    # rejected blocks
    c["K % 8"] = blk(256, 256, 20)
    c["split-K into 16-bit C"] = blk(256, 256, 256, splitk=2)
    c["bf16 x bf16 -> fp16"] = blk(64, 256, 256, cdt=L.F16)
    c["head norm outside the LDS-DMA family"] = blk(64, 256, 256, hn_w0=True, hn_c0_end=256, hn_c1_end=256)
    return c


# label -> route; a ROWSPLIT names the routes of its two launches (full 256-row blocks + remaining rows)
EXPECTED = {
    'rdt qkv B=1': 'REG',
    'rdt proj B=1': 'REG',
    'rdt cross-q B=1': 'REG',
    'rdt fc1 B=1': 'REG',
    'rdt fc2 B=1': 'REG',
    'rdt qkv B=1 Wp': 'PWS',
    'rdt proj B=1 Wp': 'PWS',
    'rdt cross-q B=1 Wp': 'PWS',
    'rdt fc1 B=1 Wp': 'PWS',
    'rdt fc2 B=1 Wp': 'PWS',
    'rdt qkv B=2': 'GLDS',
    'rdt proj B=2': 'REG',
    'rdt cross-q B=2': 'REG',
    'rdt fc1 B=2': 'REG',
    'rdt fc2 B=2': 'REG',
    'rdt qkv B=2 Wp': 'PWS',
    'rdt proj B=2 Wp': 'PWS',
    'rdt cross-q B=2 Wp': 'PWS',
    'rdt fc1 B=2 Wp': 'PWS',
    'rdt fc2 B=2 Wp': 'PWS',
    'rdt qkv B=8': 'PPK',
    'rdt proj B=8': 'REG',
    'rdt cross-q B=8': 'REG',
    'rdt fc1 B=8': 'REG',
    'rdt fc2 B=8': 'REG',
    'rdt qkv B=8 Wp': 'PPK',
    'rdt proj B=8 Wp': 'REG',
    'rdt cross-q B=8 Wp': 'REG',
    'rdt fc1 B=8 Wp': 'REG',
    'rdt fc2 B=8 Wp': 'REG',
    'rdt qkv B=32': 'PT',
    'rdt proj B=32': 'PPK',
    'rdt cross-q B=32': 'PPK',
    'rdt fc1 B=32': 'PPK',
    'rdt fc2 B=32': 'PPK',
    'rdt qkv B=32 Wp': 'PW',
    'rdt proj B=32 Wp': 'PW',
    'rdt cross-q B=32 Wp': 'PW',
    'rdt fc1 B=32 Wp': 'PW',
    'rdt fc2 B=32 Wp': 'PW',
    'rdt qkv B=1 slabs Wp': 'PWS',
    'rdt qkv B=1 slabs': 'REG',
    'rdt proj B=32 Wp hand-off producer': 'PW',
    'rdt qkv B=32 Wp hand-off consumer': 'PW',
    'hand-off producer, M=3000 does not fit pw': 'UNSUPPORTED',
    'hand-off producer without packed weights': 'UNSUPPORTED',
    'hand-off consumer, rs_n=34': 'UNSUPPORTED',
    'rdt cond K|V 32 x 4374 rows': 'PT',
    'rdt cond K|V cmap 3, 120 rows': 'UNSUPPORTED',
    'dino-b qkv': 'PT',
    'dino-b proj': 'PT',
    'dino-b fc1': 'ROWSPLIT: PT + REG',
    'dino-b fc1 Wp': 'ROWSPLIT: PT + PWS',
    'dino-b fc1 64-row remainder': 'REG',
    'dino-b fc1 64-row remainder Wp': 'PWS',
    'dino-b fc2': 'PT',
    'dino-b fc2 batch 1 (514 rows)': 'REG',
    'dino-b fc2 batch 1 slabs': 'REG',
    'siglip qkv M=4374': 'PT',
    'siglip proj M=4374': 'PPK',
    'siglip fc1 M=4374': 'GLDS',
    'siglip fc2 M=4374': 'REG',
    'siglip qkv M=139968': 'PT',
    'siglip proj M=139968': 'PP',
    'siglip fc1 M=139968': 'PP',
    'siglip fc2 M=139968': 'REG',
    'fp32 4096 x 3968 x 4096 (992 tiles)': 'F32R',
    'fp32 4096 x 4096 x 4096 (1024 tiles)': 'REG',
    'x3 512 x 512 x 1280': 'F32R',
    'x3 512 x 512 x 1288 (K % 64)': 'REG',
    'x3 conv 5 taps x 256 channels': 'F32R',
    'x3 conv 5 taps x 24 channels, 4 slices': 'REG',
    'fp32 A x bf16 W': 'REG',
    'bf16 tiny M': 'REG',
    '(3000, 2048, 2048) Wp keeps the old tiles': 'GLDS',
    '(8193, 6144, 512) head norm is not split': 'PP',
    '(8193, 6144, 512) plain': 'ROWSPLIT: PT + REG',
    'K % 8': 'BAD_ARG',
    'split-K into 16-bit C': 'BAD_ARG',
    'bf16 x bf16 -> fp16': 'UNSUPPORTED',
    'head norm outside the LDS-DMA family': 'UNSUPPORTED',
}
# the entries that differ with vt_tune(2, 0) (weights-in-registers tile off) / vt_tune(8, 0) (persistent tile off), from the same source
EXPECTED_KNOB_2_OFF = {
    'rdt qkv B=32 Wp': 'PT',
    'rdt proj B=32 Wp': 'PPK',
    'rdt cross-q B=32 Wp': 'PPK',
    'rdt fc1 B=32 Wp': 'PPK',
    'rdt fc2 B=32 Wp': 'PPK',
    'rdt proj B=32 Wp hand-off producer': 'UNSUPPORTED',
    'rdt qkv B=32 Wp hand-off consumer': 'UNSUPPORTED',
}
EXPECTED_KNOB_8_OFF = {
    'rdt qkv B=32': 'PP',
    'rdt cond K|V 32 x 4374 rows': 'PP',
    'dino-b qkv': 'PP',
    'dino-b proj': 'GLDS',
    'dino-b fc1': 'ROWSPLIT: PP + REG',
    'dino-b fc1 Wp': 'ROWSPLIT: PP + PWS',
    'dino-b fc2': 'PP',
    'siglip qkv M=4374': 'PP',
    'siglip qkv M=139968': 'PP',
    '(8193, 6144, 512) plain': 'ROWSPLIT: PP + REG',
}


def route(p):
    lib = L.lib()
    r = L.ROUTE_NAMES[lib.vt_gemm_route_of(C.addressof(p))]
    head, tail = C.c_int(-1), C.c_int(-1)
    rc = lib.vt_gemm_route_split(C.addressof(p), C.byref(head), C.byref(tail))
    if r != "ROWSPLIT":
        assert rc != 0
        return r
    assert rc == 0
    return f"ROWSPLIT: {L.ROUTE_NAMES[head.value]} + {L.ROUTE_NAMES[tail.value]}"


def test_table_covers_every_case():
    assert sorted(cases()) == sorted(EXPECTED)
    assert {e.split(":")[0] for e in EXPECTED.values()} == set(L.ROUTE_NAMES), "every outcome of the dispatcher appears in the table"


@pytest.mark.parametrize("label", sorted(EXPECTED))
def test_route(label):
    assert route(cases()[label]) == EXPECTED[label]


def test_docstring_cases_of_the_gpu_tests():
    assert EXPECTED["(3000, 2048, 2048) Wp keeps the old tiles"] != "PW"
    assert not EXPECTED["(8193, 6144, 512) head norm is not split"].startswith("ROWSPLIT")
    assert EXPECTED["(8193, 6144, 512) plain"].startswith("ROWSPLIT")       # the head norm is what keeps the block whole
    assert EXPECTED["hand-off producer, M=3000 does not fit pw"] == "UNSUPPORTED"


def test_null_block_is_a_bad_argument():
    assert L.ROUTE_NAMES[L.lib().vt_gemm_route_of(None)] == "BAD_ARG"


def routes_with(knob, value):
    lib = L.lib()
    try:
        assert lib.vt_tune(knob, value) == 0
        got = {k: route(p) for k, p in cases().items()}
    finally:
        assert lib.vt_tune(knob, 1) == 0
    assert {k: route(p) for k, p in cases().items()} == EXPECTED      # restored
    return got


def test_knob_2_off_routes_nothing_to_pw():
    assert "PW" in EXPECTED.values()
    got = routes_with(2, 0)
    assert not [k for k, r in got.items() if "PW" in r.replace("PWS", "")]
    assert got == {**EXPECTED, **EXPECTED_KNOB_2_OFF}
    assert sorted(EXPECTED_KNOB_2_OFF) == sorted(k for k, r in EXPECTED.items() if r == "PW")      # and nothing else moves
    # no other kernel has the RMSNorm hand-off
    assert all(r == "UNSUPPORTED" for k, r in EXPECTED_KNOB_2_OFF.items() if cases()[k].xn_out or cases()[k].rs_part)


def test_knob_8_off_turns_every_pt_into_pp():
    assert any("PT" in r for r in EXPECTED.values())
    got = routes_with(8, 0)
    assert not [k for k, r in got.items() if "PT" in r]
    assert got == {**EXPECTED, **EXPECTED_KNOB_8_OFF}
    assert sorted(EXPECTED_KNOB_8_OFF) == sorted(k for k, r in EXPECTED.items() if "PT" in r)      # and nothing else moves
    # PT becomes PP, except one round of 160 .. 256 tiles (DINOv2-B's output projection: 65 x 3), which only the persistent kernel claims for the
    # 256-square family: without it the block falls through to the narrower tiles
    one_round = ["dino-b proj"]
    assert all(r == EXPECTED[k].replace("PT", "PP") for k, r in EXPECTED_KNOB_8_OFF.items() if k not in one_round)
    assert all("PP" not in EXPECTED_KNOB_8_OFF[k] for k in one_round)
