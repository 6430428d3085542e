"""vt_prompt_seam and vt_prompt_compact (csrc/vt_prompt_seam.hip) as units against numpy, bit for bit in fp32.

The seam's statement, per element of the last n rows of each image and in this order: gate v = fl(fl(g v) + fl(fl(1 - g) before)), save
before = v, overwrite v = VPT_shallow.  numpy's float32 arithmetic rounds every operation once, which is what the kernel does (no fused
multiply-add), so the comparison is exact.  Every combination of (gate, save, overwrite) that does something, Bt in {1, 5}, n in {1, 8},
D in {4, 68, 1024}; the stream, `before` and a guard band around both are filled with a sentinel pattern and every element outside the tail must
keep it.  The compaction out of place and in place, for rows and n that are multiples of nothing."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def guarded(a: np.ndarray, dev):
    """a on the device inside a buffer with GUARD sentinel floats on both sides (16-byte aligned) -> (view, whole buffer, the sentinel)."""
    sent = np.float32(-12345.5)
    buf = torch.full((a.size + 2 * GUARD,), float(sent), dtype=torch.float32, device=dev)
    v = buf[GUARD:GUARD + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v, buf, sent


def guard_ok(buf, sent) -> bool:
    h = buf.cpu().numpy()
    return bool((h[:GUARD] == sent).all() and (h[-GUARD:] == sent).all())


ROWS = 7                                                            # rows per image with the tail; n = 8 uses 11


@pytest.mark.parametrize("Bt,n,D", list(itertools.product((1, 5), (1, 8), (4, 68, 1024))))
def test_seam_equals_numpy_bit_for_bit(dev, Bt, n, D):
    from vlatouch import _lib as L
    lib = L.lib()
    rows = ROWS if n == 1 else 11
    g = np.random.Generator(np.random.PCG64(1000 * Bt + 10 * n + D))
    for gate, save, over in itertools.product((False, True), repeat=3):
        if not (gate or save or over):
            continue
        tok0 = g.standard_normal((Bt, rows, D)).astype(np.float32)
        bef0 = g.standard_normal((Bt, n, D)).astype(np.float32)
        shallow = g.standard_normal((n, D)).astype(np.float32)
        gv = np.float32(g.uniform(0.01, 0.99))
        tok, tok_buf, s1 = guarded(tok0, dev)
        bef, bef_buf, s2 = guarded(bef0, dev)
        sh = torch.from_numpy(shallow).to(dev)
        gd = torch.tensor([gv], dtype=torch.float32, device=dev)
        L.check(lib.vt_prompt_seam(L.ptr(tok), Bt, rows, n, D, L.ptr(gd) if gate else None, L.ptr(bef), int(save), L.ptr(sh) if over else None,
                                   L.stream_ptr(dev)), "vt_prompt_seam")
        torch.cuda.synchronize(dev)
        want_tok, want_bef = tok0.copy(), bef0.copy()
        v = want_tok[:, rows - n:].copy()
        if gate:
            v = gv * v + (np.float32(1.0) - gv) * bef0                # float32 throughout: one rounding per operation
            assert v.dtype == np.float32
        if save:
            want_bef = v.copy()
        if over:
            v = np.broadcast_to(shallow, v.shape).copy()
        want_tok[:, rows - n:] = v
        what = (Bt, n, D, gate, save, over)
        assert np.array_equal(tok.cpu().numpy().view(np.uint32), want_tok.view(np.uint32)), what      # the tail as stated, every other row untouched
        assert np.array_equal(bef.cpu().numpy().view(np.uint32), want_bef.view(np.uint32)), what
        assert guard_ok(tok_buf, s1) and guard_ok(bef_buf, s2), what


@pytest.mark.parametrize("Bt,rows,n,D", [(1, 7, 3, 4), (5, 7, 3, 68), (5, 13, 1, 68), (3, 11, 8, 1024), (5, 258, 1, 68), (4, 265, 8, 1024)])
def test_compaction_out_of_place_and_in_place(dev, Bt, rows, n, D):
    from vlatouch import _lib as L
    lib = L.lib()
    g = np.random.Generator(np.random.PCG64(rows * 100 + n))
    src0 = g.standard_normal((Bt, rows, D)).astype(np.float32)
    want = np.ascontiguousarray(src0[:, : rows - n])
    src, src_buf, s1 = guarded(src0, dev)
    dst, dst_buf, s2 = guarded(np.zeros_like(want), dev)
    L.check(lib.vt_prompt_compact(L.ptr(src), L.ptr(dst), Bt, rows, n, D, L.stream_ptr(dev)), "vt_prompt_compact")
    torch.cuda.synchronize(dev)
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(src.cpu().numpy().view(np.uint32), src0.view(np.uint32)) and guard_ok(src_buf, s1) and guard_ok(dst_buf, s2)
    # in place: the first Bt * (rows - n) * D floats become the compact stream, what lies behind them is not written
    L.check(lib.vt_prompt_compact(L.ptr(src), L.ptr(src), Bt, rows, n, D, L.stream_ptr(dev)), "vt_prompt_compact (in place)")
    torch.cuda.synchronize(dev)
    flat = src.cpu().numpy().reshape(-1)
    assert np.array_equal(flat[: want.size].view(np.uint32), want.reshape(-1).view(np.uint32))
    if Bt > 1:
        assert np.array_equal(flat[want.size:].view(np.uint32), src0.reshape(-1)[want.size:].view(np.uint32))
    assert guard_ok(src_buf, s1)


def test_refusals(dev):
    from vlatouch import _lib as L
    lib = L.lib()
    t = torch.zeros(2, 5, 8, device=dev)
    b = torch.zeros(2, 2, 8, device=dev)
    s = torch.zeros(2, 8, device=dev)
    g = torch.zeros(1, device=dev)
    st = L.stream_ptr(dev)
    assert lib.vt_prompt_seam(L.ptr(t), 2, 5, 2, 8, L.ptr(g), L.ptr(b), 1, L.ptr(s), st) == 0
    for args in ((None, 2, 5, 2, 8, L.ptr(g), L.ptr(b), 1, L.ptr(s)), (L.ptr(t), 0, 5, 2, 8, None, None, 0, L.ptr(s)), (L.ptr(t), 2, 5, 6, 8, None, None, 0, L.ptr(s)),
                 (L.ptr(t), 2, 5, 2, 6, None, None, 0, L.ptr(s)), (L.ptr(t), 2, 5, 2, 8, L.ptr(g), None, 0, None), (L.ptr(t), 2, 5, 2, 8, None, None, 1, None),
                 (L.ptr(t), 2, 5, 2, 8, None, None, 0, None)):
        assert lib.vt_prompt_seam(*args, st) == -22, args
    d = torch.zeros(2, 3, 8, device=dev)
    assert lib.vt_prompt_compact(L.ptr(t), L.ptr(d), 2, 5, 2, 8, st) == 0
    for args in ((None, L.ptr(d), 2, 5, 2, 8), (L.ptr(t), None, 2, 5, 2, 8), (L.ptr(t), L.ptr(d), 0, 5, 2, 8), (L.ptr(t), L.ptr(d), 2, 5, 0, 8),
                 (L.ptr(t), L.ptr(d), 2, 5, 5, 8), (L.ptr(t), L.ptr(d), 2, 5, 2, 6)):
        assert lib.vt_prompt_compact(*args, st) == -22, args
    off = torch.zeros(2 * 5 * 8 + 1, device=dev)[1:]                 # 4 bytes past an allocation's base
    assert off.data_ptr() % 16 == 4
    assert lib.vt_prompt_seam(L.ptr(off), 2, 5, 2, 8, None, None, 0, L.ptr(s), st) == -22
    assert lib.vt_prompt_seam(L.ptr(t), 2, 5, 2, 8, None, L.ptr(off), 1, None, st) == -22
    assert lib.vt_prompt_compact(L.ptr(off), L.ptr(d), 2, 5, 2, 8, st) == -22 and lib.vt_prompt_compact(L.ptr(t), L.ptr(off), 2, 5, 2, 8, st) == -22
    torch.cuda.synchronize(dev)
