"""GPU parity of the cross-attention against a cached condition (csrc/vt_attn_kvt.hip) through the C ABI: attn_kvt_ring_kernel, the key-range
split merged by attn_combine_kernel, and retile_kv_kernel.  Reference: softmax(scale q k^T, masked keys at -inf) v in float64 on the CPU, per
(batch, head), from the same 16-bit q, k and v.

The tile stream is built in torch from the layout documented at the top of vt_attn_kvt.hip (cases.kv_tile_stream), never by the library.
The inputs are shaped so that a dropped, doubled or leaked key moves the output well past the bars:
  V    column 0 = 1: the output is exactly 1.0 wherever a row has a valid key (the row sum is taken from the same 16-bit P through the same
       MFMA as P V); columns 1..16 = indicators of the keys of each part of the split; 17 / 18 = of the sample's first / last tile; 19 / 20 =
       of the first / last key of a sample (a neighbour's key across a sample boundary lands in 19 or 20); the rest N(0, 1)
  q.k  needle: per query row one key 8 above the rest (the sample's first key, its last key, the first key of its second tile, or a key
       inside its last part); near-uniform: small q; floor: every score at -bound (the fp16 P of the fixed form near the subnormals)
Rows past B * Nk of the stream hold 16-bit NaN in both halves, T exceeds the tiles the rows need (the head stride comes from T), Q is a
strided view of a fused buffer and O has its own row stride; sentinels around O and after the split buffer must survive every call."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BAR_REL = {"bf16": 1.5e-2, "f16": 2e-3}      # random columns: max|out - ref| / max|ref| (the bars of test_attention)
BAR_ABS = {"bf16": 1e-2, "f16": 2e-3}        # indicator columns: max|out - ref|
LIMIT = {"bf16": 40.0, "f16": 10.0}          # the largest fixed_max vt_attn_kvt_launch admits; above it the online form runs
SCALE = 0.125
C_PART, C_FIRST_TILE, C_LAST_TILE, C_FIRST_KEY, C_LAST_KEY, C_RAND = 1, 17, 18, 19, 20, 21
SENT16, SENT32 = 0x7E5A, 0x5AA5A55A
GUARD = 8 << 20                              # sentinel bytes after the split buffer

# B, Nk, Nq, parts, H.  parts None: Nq spans more than one query block, or a shape the split never sees -> the unsplit path only
SHAPES = [
    (1, 1, 1, 2, 1),            # one key: every part but the first empty
    (2, 7, 11, 5, 2),           # both samples inside one tile, 4 empty parts
    (3, 63, 16, 2, 3),
    (5, 64, 32, 5, 2),          # tile-aligned samples
    (3, 65, 33, 16, 4),         # more parts than tiles
    (2, 130, 67, 2, 2),
    (5, 130, 128, 5, 1),        # 8 waves, one query block
    (1, 2100, 11, 16, 4),       # RDT horizon 8 at batch 1 (4 waves: 64 partial rows per part)
    (3, 2100, 67, 16, 3),
    (1, 4374, 67, 16, 32),      # RDT-1B at batch 1
    (2, 4374, 1, 5, 2),
    (2, 4374, 200, None, 2),    # two query blocks of 7 waves
    (3, 130, 129, None, 3),     # two query blocks of 5 waves
    (5, 65, 67, None, 1),
    (1, 2100, 200, None, 4),
]
MASKS = ("none", "trail", "lead", "last", "onepart", "sample")
REGIMES = ("needle", "uniform", "floor")


def _grid():
    """Every shape in every (dtype, softmax form) twice; within a (dtype, form) the 30 items walk all 18 (mask, regime) pairs."""
    items = []
    for ci, (dname, form) in enumerate(itertools.product(DT, ("online", "fixed"))):
        for n, (si, rep) in enumerate(itertools.product(range(len(SHAPES)), range(2))):
            B, Nk, Nq, parts, H = SHAPES[si]
            pair = (n * 7 + ci * 5) % 18
            mask, regime = MASKS[pair // 3], REGIMES[pair % 3]
            items.append(pytest.param(dname, form, B, Nk, Nq, parts, H, mask, regime, 1000 * si + 10 * rep + ci,
                                      id=f"{dname}-{form}-B{B}-Nk{Nk}-Nq{Nq}-p{parts or 1}-H{H}-{mask}-{regime}"))
    return items


@pytest.fixture(scope="module")
def dev():
    from vlatouch import _lib as L
    lib = L.lib()
    L.check(lib.vt_tune(6, 1), "vt_tune")            # the fixed-maximum form admitted (the default)
    return torch.device("cuda:0")


def part_of_row(B, Nk, parts):
    """Part of its own sample's split that every stream row m < B * Nk falls in (vt_attn_kvt.hip: `per` tiles per part, from the sample's first tile)."""
    m = torch.arange(B * Nk)
    row0 = m // Nk * Nk
    t_first, t_last = row0 // 64, (row0 + Nk - 1) // 64
    per = (t_last - t_first + parts) // parts
    return (m // 64 - t_first) // per


def make_inputs(dname, B, H, Nq, Nk, parts, regime, seed):
    """q [B, Nq, H, 64], k / v [B * Nk, H, 64] (stream rows), all in the 16-bit type `dname`."""
    g = torch.Generator().manual_seed(seed)
    M = B * Nk
    m = torch.arange(M)
    row0 = m // Nk * Nk
    part = part_of_row(B, Nk, parts)
    v = torch.randn(M, H, 64, generator=g)
    v[:, :, 0] = 1.0
    v[:, :, C_PART:C_PART + 16] = (part[:, None] == torch.arange(16)).float()[:, None, :]
    v[:, :, C_FIRST_TILE] = (m // 64 == row0 // 64).float()[:, None]
    v[:, :, C_LAST_TILE] = (m // 64 == (row0 + Nk - 1) // 64).float()[:, None]
    v[:, :, C_FIRST_KEY] = (m == row0).float()[:, None]
    v[:, :, C_LAST_KEY] = (m == row0 + Nk - 1).float()[:, None]
    if regime == "uniform":
        k = torch.randn(M, H, 64, generator=g)
        q = torch.randn(B, Nq, H, 64, generator=g) * 0.05
    elif regime == "floor":                                  # every scaled score exactly -limit
        k = torch.zeros(M, H, 64)
        k[:, :, 0] = 1.0
        q = torch.zeros(B, Nq, H, 64)
        q[..., 0] = -LIMIT[dname] / SCALE
    else:                                                    # needle: channel 60 + j of q meets needle key j of the sample (score +8)
        k = torch.zeros(M, H, 64)
        q = torch.zeros(B, Nq, H, 64)
        k[:, :, :56] = torch.randn(M, H, 56, generator=g)
        q[..., :56] = torch.randn(B, Nq, H, 56, generator=g) * 0.15
        for b in range(B):
            r0 = b * Nk
            second_tile = 64 - r0 % 64
            last_part = (part[r0:r0 + Nk] == part[r0 + Nk - 1]).nonzero().flatten()
            for j, l in enumerate((0, Nk - 1, second_tile if second_tile < Nk else Nk // 2, int(last_part[len(last_part) // 2]))):
                k[r0 + l, :, 60 + j] = 1.0
        j_row = (torch.arange(Nq)[None, :, None] + torch.arange(B)[:, None, None] + torch.arange(H)[None, None, :]) % 4
        q[..., 60:] = 64.0 * F.one_hot(j_row, 4).float()
    dt = DT[dname]
    return q.to(dt), k.to(dt), v.to(dt)


def make_mask(kind, B, Nk, part):
    """[B, Nk] bool (True = attend) or None."""
    if kind == "none":
        return None
    keep = torch.ones(B, Nk, dtype=torch.bool)
    n = min(max(1, Nk // 3), Nk - 1)
    if kind == "trail":
        keep[:, Nk - n:] = False
    elif kind == "lead":
        keep[:, :n] = False
    elif kind == "last":
        keep[:, :-1] = False
    elif kind == "onepart":                                  # the keys of the part that holds the middle key
        p = part.reshape(B, Nk)
        keep = p == p[:, Nk // 2:Nk // 2 + 1]
    elif kind == "sample":                                   # the middle sample fully masked, its neighbours fully valid
        keep[B // 2] = False
    return keep


def reference(q, k, v, keep, B, Nk):
    """float64 softmax(scale q k^T) v per (batch, head) -> (out [B, Nq, H, 64], the unmasked scaled scores [B, H, Nq, Nk])."""
    H = q.shape[2]
    kd, vd = k.double().reshape(B, Nk, H, 64), v.double().reshape(B, Nk, H, 64)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), kd) * SCALE
    sm = s if keep is None else s.masked_fill(~keep[:, None, None, :], float("-inf"))
    p = torch.softmax(sm, -1).nan_to_num(0.0)               # a fully masked row has no softmax: the kernel writes zeros and flags it
    return torch.einsum("bhqk,bkhd->bqhd", p, vd), s


class KvtCall:
    """Device buffers of one shape; call() runs vt_attention_kvt once and checks the sentinels around its outputs."""

    def __init__(self, dev, dt, q, kv, T, keep, B, Nk):
        from vlatouch import _lib as L
        self.L, self.lib, self.dev, self.dt = L, L.lib(), dev, dt
        self.B, self.Nq, self.H = q.shape[0], q.shape[1], q.shape[2]
        self.Nk, self.T = Nk, T
        B, Nq, H = self.B, self.Nq, self.H
        self.q_rs = 3 * H * 64 + 64                          # Q = the middle third of a fused [B][Nq + 1][q_rs] buffer
        self.qbuf = torch.full((B, Nq + 1, self.q_rs), float("nan"), dtype=dt, device=dev)
        self.qbuf[:, :Nq, H * 64:2 * H * 64] = q.reshape(B, Nq, H * 64).to(dev)
        self.o_rs = H * 64 + 48                              # O = columns 16 .. 16 + 64 H of [B][Nq + 2][o_rs]
        self.obuf = torch.empty(B, Nq + 2, self.o_rs, dtype=dt, device=dev)
        self.region = torch.zeros(B, Nq + 2, self.o_rs, dtype=torch.bool, device=dev)
        self.region[:, :Nq, 16:16 + H * 64] = True
        self.kv = kv
        self.kmask = None if keep is None else keep.to(torch.uint8).contiguous().to(dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(self, fixed_max, parts):
        L, B, Nq, H = self.L, self.B, self.Nq, self.H
        self.obuf.view(torch.int16).fill_(SENT16)
        self.flag.zero_()
        p = L.AttnKvtParams()
        p.Q = self.qbuf[:, :, H * 64:].data_ptr()
        p.KV, p.O = self.kv.data_ptr(), self.obuf[:, :, 16:].data_ptr()
        p.q_bs, p.q_rs = (Nq + 1) * self.q_rs, self.q_rs
        p.o_bs, p.o_rs = (Nq + 2) * self.o_rs, self.o_rs
        p.kmask = None if self.kmask is None else self.kmask.data_ptr()
        p.B, p.H, p.Nq, p.Nk, p.T = B, H, Nq, self.Nk, self.T
        p.scale, p.fixed_max, p.dtype = SCALE, fixed_max, L.dt_code(self.dt)
        p.range_flag = self.flag.data_ptr()
        ws, nb = None, 0
        if parts:
            nb = self.lib.vt_attention_kvt_part_bytes(B, H, Nq, parts)
            assert nb > 0 and nb % 4 == 0
            ws = torch.full(((nb + GUARD) // 4,), SENT32, dtype=torch.int32, device=self.dev)
            p.parts, p.part_ws = parts, ws.data_ptr()
        L.check(self.lib.vt_attention_kvt(C.byref(p), L.stream_ptr(self.dev)), "vt_attention_kvt")
        torch.cuda.synchronize(self.dev)
        if ws is not None:
            hit = int((ws[nb // 4:] != SENT32).sum())
            assert hit == 0, f"{hit} words written past the {nb} bytes of vt_attention_kvt_part_bytes"
        hit = int((self.obuf.view(torch.int16)[~self.region] != SENT16).sum())
        assert hit == 0, f"{hit} elements written outside O (rows >= Nq, or outside the heads' columns)"
        out = self.obuf[:, :Nq, 16:16 + H * 64].reshape(B, Nq, H, 64).clone()
        return out, int(self.flag.item())


def check_against_reference(out, flag, ref, keep, dname, what):
    """-> (relative error of the random columns, absolute error of the indicator columns)."""
    from vlatouch import _lib as L
    o = out.double().cpu()
    empty = torch.zeros(o.shape[0], dtype=torch.bool) if keep is None else ~keep.any(-1)
    if bool(empty.any()):
        assert float(o[empty].abs().max()) == 0.0, f"{what}: a sample without valid keys must come out as exact zeros"
        assert flag == L.RANGE_ATTN_EMPTY, f"{what}: range flag {flag}, want RANGE_ATTN_EMPTY for the empty rows"
    else:
        assert flag == 0, f"{what}: range flag {flag} although every row has a valid key"
    if bool(empty.all()):
        return 0.0, 0.0
    o, r = o[~empty], ref[~empty]
    assert bool((o[..., 0] == 1.0).all()), f"{what}: the ones column is not exactly 1: {o[..., 0][o[..., 0] != 1.0][:8].tolist()}"
    e_rel = float((o[..., C_RAND:] - r[..., C_RAND:]).abs().max() / r[..., C_RAND:].abs().max())
    e_ind = float((o[..., 1:C_RAND] - r[..., 1:C_RAND]).abs().max())
    assert e_rel <= BAR_REL[dname], f"{what}: random columns {e_rel:.3e} > {BAR_REL[dname]}"
    assert e_ind <= BAR_ABS[dname], f"{what}: indicator columns {e_ind:.3e} > {BAR_ABS[dname]}"
    return e_rel, e_ind


@pytest.mark.parametrize("dname,form,B,Nk,Nq,parts,H,mask,regime,seed", _grid())
def test_cached_cross_attention_vs_float64(dev, dname, form, B, Nk, Nq, parts, H, mask, regime, seed):
    dt = DT[dname]
    nominal = parts or 4                                     # the unsplit-only shapes still get part indicators (of a 4-way split)
    q, k, v = make_inputs(dname, B, H, Nq, Nk, nominal, regime, seed)
    keep = make_mask(mask, B, Nk, part_of_row(B, Nk, nominal))
    ref, s = reference(q, k, v, keep, B, Nk)
    if regime == "needle" and Nk > 1:                        # the input is what it claims: the needle stands at least 6 above every other key
        top2 = s.topk(2, dim=-1).values
        assert float((top2[..., 0] - top2[..., 1]).min()) >= 6.0
    T = (B * Nk + 63) // 64 + 1
    kv = cases.kv_tile_stream(k.to(dev), v.to(dev), T, fill=float("nan"))
    call = KvtCall(dev, dt, q, kv, T, keep, B, Nk)
    if form == "fixed":
        bound = LIMIT[dname] if regime == "floor" else 1.02 * float(s.abs().max())
        assert 0.0 < bound <= LIMIT[dname], bound          # admitted: the fixed form really runs
    else:
        bound = 0.0
    paths = ([parts] if parts else []) + [None]
    report = []
    for pp in paths:
        what = f"{'split ' + str(pp) if pp else 'unsplit'} fixed_max {bound:g}"
        out, flag = call.call(bound, pp)
        again, _ = call.call(bound, pp)
        assert torch.equal(out.view(torch.int16), again.view(torch.int16)), f"{what}: two calls differ"
        e_rel, e_ind = check_against_reference(out, flag, ref, keep, dname, what)
        report.append(f"{'split' if pp else 'unsplit'} rel {e_rel:.2e} ind {e_ind:.2e}")
        if form == "fixed":                                  # just above the admission limit the launcher runs the online form
            above = float(np.nextafter(np.float32(LIMIT[dname]), np.float32(np.inf)))
            o_above, _ = call.call(above, pp)
            o_online, _ = call.call(0.0, pp)
            assert torch.equal(o_above.view(torch.int16), o_online.view(torch.int16)), f"{what}: fixed_max {above} is not the online form"
    print(f"[kvt {dname} {form} B{B} Nk{Nk} Nq{Nq} parts {parts} H{H} {mask} {regime}] " + "; ".join(report))


@pytest.mark.parametrize("M", [1, 63, 64, 65, 2100])
def test_retile_kv_matches_torch_tile_stream(dev, M):
    """vt_retile_kv on a row-major K | V product (ld = 2 * H * 64, as the RDT condition cache uses it) == the tile stream built in torch, bit for bit,
    on every row < M; nothing past the last head's T tiles is written."""
    from vlatouch import _lib as L
    lib = L.lib()
    H = 3
    T = (M + 63) // 64 + 1
    for dname, dt in DT.items():
        g = torch.Generator().manual_seed(M)
        kvs = torch.randn(M, 2 * H * 64, generator=g).to(dt).to(dev)
        out = torch.full((H * T + 1, 2, 64, 64), SENT16, dtype=torch.int16, device=dev)
        L.check(lib.vt_retile_kv(L.ptr(kvs), C.c_void_p(kvs.data_ptr() + H * 64 * 2), 2 * H * 64, L.ptr(out), M, T, H, L.stream_ptr(dev)),
                "vt_retile_kv")
        want = cases.kv_tile_stream(kvs[:, :H * 64].reshape(M, H, 64), kvs[:, H * 64:].reshape(M, H, 64), T).view(torch.int16)
        ones = torch.ones(M, H, 64, dtype=torch.bool, device=dev)
        valid = cases.kv_tile_stream(ones, ones, T, fill=False)
        got = out[:H * T].reshape(H, T, 2, 64, 64)
        assert torch.equal(got[valid], want[valid]), dname
        assert bool((out[H * T:] == SENT16).all()), dname
