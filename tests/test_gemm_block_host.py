"""ops.gemm_block_params / ops.groupnorm_block_params (the block builders of tests/test_gpu_gemm_blocks.py) on the host: their default path — one group,
contiguous operands — fills a block field for field as ops.gemm / ops.conv1d_cl / ops.groupnorm_cl do for the same tensors, and groups, group strides
and pitches follow from the tensors' strides.  Host code only: CPU tensors stand in for device memory, nothing is launched."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vla-touch_amd"))

from vlatouch import _lib as L, ops  # noqa: E402


class _Capture:
    """Stands in for the loaded library: keeps a copy of the block a wrapper would have launched."""

    def __init__(self, struct):
        self.struct, self.block = struct, None

    def _take(self, ref, stream):
        self.block = self.struct.from_buffer_copy(bytes(ref._obj))
        return 0

    vt_gemm = vt_groupnorm = _take


@pytest.fixture
def captured(monkeypatch):
    def go(struct, fn, *args, **kw):
        cap = _Capture(struct)
        monkeypatch.setattr(L, "lib", lambda: cap)
        monkeypatch.setattr(L, "stream_ptr", lambda device=None: None)
        out = fn(*args, **kw)
        monkeypatch.undo()
        return cap.block, out
    return go


def fields(p, skip=()):
    return {name: getattr(p, name) for name, _ in p._fields_ if name not in skip}


def same_block(got, want, skip=()):
    g, w = fields(got, skip), fields(want, skip)
    assert g == w, {k: (g[k], w[k]) for k in g if g[k] != w[k]}


@pytest.mark.parametrize("adt,wdt,odt", [(torch.float32, torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16, torch.float32),
                                         (torch.float16, torch.float16, torch.float16), (torch.float32, torch.bfloat16, torch.bfloat16)])
def test_default_path_equals_ops_gemm(captured, adt, wdt, odt):
    M, N, K = 70, 100, 64
    a, w = torch.zeros(M, K, dtype=adt), torch.zeros(N, K, dtype=wdt)
    bias, cs, res, out = torch.zeros(N), torch.zeros(N), torch.zeros(M, N, dtype=odt), torch.empty(M, N, dtype=odt)
    want, _ = captured(L.GemmParams, ops.gemm, a, w, bias, act=L.ACT_MISH, colscale=cs, residual=res, out=out, out_dtype=odt)
    same_block(ops.gemm_block_params(a, w, out, bias, act=L.ACT_MISH, colscale=cs, residual=res), want)
    want, _ = captured(L.GemmParams, ops.gemm, a, w, out=out, out_dtype=odt)
    same_block(ops.gemm_block_params(a, w, out), want)
    # a row-pitched A, as ops.gemm takes it
    wide = torch.zeros(M, K + 32, dtype=adt)
    want, _ = captured(L.GemmParams, ops.gemm, wide[:, :K], w, out=out, out_dtype=odt)
    same_block(ops.gemm_block_params(wide[:, :K], w, out), want)


def test_default_path_equals_ops_gemm_slabs_and_conv(captured):
    M, N, K, S = 64, 96, 160, 3
    a, w, slabs = torch.zeros(M, K), torch.zeros(N, K), torch.empty(S, M, N)
    want, _ = captured(L.GemmParams, ops.gemm, a, w, out=slabs, splitk=S)
    same_block(ops.gemm_block_params(a, w, slabs, splitk=S), want)
    B, T, cin, cout, k = 3, 16, 32, 40, 5
    x, wp, bias = torch.zeros(B, T, cin), torch.zeros(cout, k * cin), torch.zeros(cout)
    conv = dict(taps=k, cin=cin, tout=8, stride=2, off0=-2)
    want, out = captured(L.GemmParams, ops.conv1d_cl, x, wp, bias, **conv)
    got = ops.gemm_block_params(x, wp, out.reshape(B * 8, cout), bias, conv=conv)
    same_block(got, want, skip=("act",))
    assert got.act == L.ACT_NONE
    want, out = captured(L.GemmParams, ops.conv1d_cl, x, wp, None, splitk=2, **conv)
    same_block(ops.gemm_block_params(x, wp, out.reshape(2, B * 8, cout), splitk=2, conv=conv), want)


def test_strides_become_group_strides_and_pitches():
    G, M, N, K = 4, 10, 16, 24
    a = torch.zeros(G, M, 40)[:, :, :K]                                   # lda 40 > K
    w = torch.zeros(N, K).expand(G, N, K)                                 # shared: w_gs 0
    bias = torch.zeros(G + 1, N)[:G]
    res = torch.zeros(M, 20)[:, :N].expand(G, M, N)                       # shared, ldr 20
    buf = torch.zeros(G, M + 1, 48)
    out = buf[:, :M, 32:48]                                               # ldc 48, a gap row between groups, a column offset
    p = ops.gemm_block_params(a, w, out, bias, residual=res, w_code=L.F32X3)
    assert (p.groups, p.splitk, p.M, p.N, p.K) == (G, 1, M, N, K)
    assert (p.a_gs, p.lda, p.w_gs, p.ldw) == (M * 40, 40, 0, K)
    assert (p.c_gs, p.ldc, p.C) == ((M + 1) * 48, 48, buf.data_ptr() + 32 * 4)
    assert (p.bias_gs, p.r_gs, p.ldr) == (N, 0, 20)
    assert (p.a_dtype, p.w_dtype, p.c_dtype) == (L.F32, L.F32X3, L.F32)
    slabs = torch.zeros(3, G, M + 1, N)[:, :, :M]
    p = ops.gemm_block_params(a, w, slabs, splitk=3)
    assert (p.groups, p.splitk, p.c_gs, p.c_slab, p.ldc) == (G, 3, (M + 1) * N, G * (M + 1) * N, N)
    x = torch.zeros(G, 3, 8, 16)
    p = ops.gemm_block_params(x, torch.zeros(G, N, 5 * 16), torch.zeros(G, 3 * 8, N), conv=dict(taps=5, cin=16, tout=8, off0=-2))
    assert (p.groups, p.a_gs, p.lda, p.tin, p.tout, p.taps, p.cin, p.stride, p.off0, p.tstep, p.M, p.K) == (G, 3 * 8 * 16, 16, 8, 8, 5, 16, 1, -2, 1, 24, 80)


def test_groupnorm_block_with_one_net_equals_ops_groupnorm_cl(captured):
    S, B, T, Cc = 3, 2, 4, 64
    slabs = torch.zeros(S, B * T, Cc)
    bias, gamma, beta = torch.zeros(Cc), torch.zeros(Cc), torch.zeros(Cc)
    film, res = torch.zeros(B, 2 * Cc), torch.zeros(B * T, Cc, dtype=torch.bfloat16)
    per_net = ("p_gs", "vec_gs", "film_gs", "r_gs", "o_gs")                   # strides between nets: not read when nets == 1
    for kw in (dict(film=film), dict(residual=res, out_dtype=torch.bfloat16)):
        want, out = captured(L.GnParams, ops.groupnorm_cl, slabs, bias, gamma, beta, B=B, T=T, ngroups=4, **kw)
        got = ops.groupnorm_block_params(slabs[:, None], bias[None], gamma[None], beta[None], out[None], B=B, T=T, ngroups=4,
                                         film=None if "film" not in kw else film[None], residual=None if "residual" not in kw else res[None])
        same_block(got, want, skip=per_net)
        assert got.nets == 1


def test_groupnorm_block_strides():
    S, nets, B, T, Cc = 2, 2, 3, 4, 16
    M = B * T
    slabs = torch.zeros(S, nets + 1, M + 2, Cc + 8)[:, :nets, :M, :Cc]
    vecs = torch.zeros(nets, 3, Cc + 4)
    film = torch.zeros(nets, B + 1, 5 * Cc)[:, :B]
    res = torch.zeros(nets, M + 3, Cc + 12)[:, :M, :Cc]
    out = torch.zeros(nets, M + 1, Cc + 24)[:, :M, :Cc]
    p = ops.groupnorm_block_params(slabs, vecs[:, 0, :Cc], vecs[:, 1, :Cc], vecs[:, 2, :Cc], out, B=B, T=T, ngroups=4, film=film, film_off=2 * Cc, residual=res)
    assert (p.nslabs, p.slab_stride, p.p_gs, p.ldp) == (S, 3 * (M + 2) * (Cc + 8), (M + 2) * (Cc + 8), Cc + 8)
    assert (p.vec_gs, p.film_gs, p.film_ld, p.film_off) == (3 * (Cc + 4), (B + 1) * 5 * Cc, 5 * Cc, 2 * Cc)
    assert (p.r_gs, p.ldr, p.o_gs, p.ldo) == ((M + 3) * (Cc + 12), Cc + 12, (M + 1) * (Cc + 24), Cc + 24)
    assert (p.nets, p.B, p.T, p.C, p.ngroups) == (nets, B, T, Cc, 4)
    assert p.gamma - p.bias == (Cc + 4) * 4 and p.beta - p.gamma == (Cc + 4) * 4
