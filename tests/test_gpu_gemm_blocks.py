"""GPU parity of vt_gemm / vt_groupnorm parameter blocks that only the library's own drivers fill: grouped launches (groups, a_gs, w_gs, c_gs, bias_gs,
r_gs, c_slab), pitched operands (lda, ldw, ldc, ldr, in place), the split-bf16 ("x3") arithmetic, and vt_groupnorm over several nets.

Every launch goes through ops.gemm_block_params / ops.groupnorm_block_params (strides -> block fields), states the kernel it holds to account by asserting
vt_gemm_route_of's answer BEFORE it launches, is compared with an fp64 product of the same (rounded) operands, and writes into a window of a larger buffer
pre-filled with a NaN bit pattern: everything outside the windows (the gap row after each group, the columns [N, ld), the slack before the first and after
the last group) must keep that pattern bit for bit.  A row that a kernel "computes but never stores", or a group stride that is off by a row, fails there
even where the numbers inside the windows are right.

Bars (none of them measured on the code under test):
  exact fp32 on the ring kernel 2e-6, on the register-staged kernel 2e-5; 16-bit operands 2e-3 into fp32, 1e-2 into bf16 (the bars of test_gpu_primitives);
  x3, against fp64:   |out - ref| / (|a| |w|^T) < 2^-16 per component — the kernel header's claim; a CPU emulation of the three-term product on row-scaled
                      operands gives 5.3e-7 .. 4.2e-6 for K = 64 .. 2560 and 1.8e-4 .. 1.3e-3 with either lo term dropped;
  x3, against the emulation a_hi w_hi + a_lo w_hi + a_hi w_lo (hi = bf16(x), lo = bf16(x - hi), summed in fp64): 2e-6 of each output row's max norm — the
                      exact-fp32 bar: it pins the arithmetic (an extra a_lo w_lo term, a lo taken from the wrong hi), not only its accuracy.
Each figure is printed before it is asserted (pytest -s / -rP shows them)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vlatouch import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


ACTS = {0: lambda x: x, 1: lambda x: F.gelu(x), 2: lambda x: F.gelu(x, approximate="tanh"), 3: F.silu, 4: F.mish}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
X3_BAR, EMU_BAR = 2.0 ** -16, 2e-6


# ---------------------------------------------------------------------------------------- assertions (every figure is printed first)
def below(value, bar, what):
    print(f"[gemm_blocks] {what}: {value:.3e} (bar {bar:.3e})")
    assert value < bar, (what, value, bar)          # a NaN (a sentinel left inside a window) fails here too


def same_bits(a, b, what):
    it = torch.int32 if a.element_size() == 4 else torch.int16
    assert a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it)), what


def group_rel_err(out, ref):
    """rel_err (max abs error over max abs reference) of every group on its own; the worst group.  Computed where the tensors live."""
    d = (out.double() - ref).abs().flatten(-2).amax(-1)
    return float((d / (ref.abs().flatten(-2).amax(-1) + 1e-12)).max())


def row_rel_err(out, ref):
    """max abs error over max abs reference of every output row on its own (rows of the x3 operands differ by up to 2^24); the worst row."""
    return float(((out.double() - ref).abs().amax(-1) / (ref.abs().amax(-1) + 1e-300)).max())


# ---------------------------------------------------------------------------------------- guarded outputs
SENTINEL = {F32: (torch.int32, 0x7FC12345), BF16: (torch.int16, 0x7FC1), F16: (torch.int16, 0x7E01)}      # NaNs with a payload
LEAD = 64      # sentinel elements before the first and after the last group (keeps the windows 16-byte aligned)


class Guard:
    """S slabs x G groups of M x N output windows inside one sentinel-filled buffer: group g of slab s starts at ((s * G + g) * (M + 1)) * ld + col0, so
    c_gs = (M + 1) * ld leaves one sentinel row after every group and c_slab = G * c_gs."""

    def __init__(self, dev, dtype, M, N, G=None, S=1, ld=None, col0=0):
        ld = N if ld is None else ld
        assert col0 + N <= ld
        self.dtype, self.grouped, self.S = dtype, G is not None, S
        G = 1 if G is None else G
        it, self.bits = SENTINEL[dtype]
        n = S * G * (M + 1) * ld
        self.flat = torch.full((LEAD + n + LEAD,), self.bits, dtype=it, device=dev)
        self.win = self.flat[LEAD:LEAD + n].view(S, G, M + 1, ld)[:, :, :M, col0:col0 + N]
        self.outside = torch.ones(self.flat.shape, dtype=torch.bool, device=dev)
        self.outside[LEAD:LEAD + n].view(S, G, M + 1, ld)[:, :, :M, col0:col0 + N] = False

    def out(self):
        """The windows as the output operand of ops.gemm_block_params: [S,][G,] M, N."""
        v = self.win.view(self.dtype)
        if not self.grouped:
            v = v[:, 0]
        return v if self.S > 1 else v[0]

    def result(self):
        """fp64 [G,] M, N: the windows, split-K slabs summed."""
        v = self.win.view(self.dtype).double().sum(0)
        return v if self.grouped else v[0]

    def check(self, what):
        kept = self.flat[self.outside]
        assert torch.equal(kept, torch.full_like(kept, self.bits)), f"{what}: written outside the output windows"


def launch(route, a, w, out, bias=None, **fields):
    """Launch the block on the kernel `route` names; ops.gemm_block asserts vt_gemm_route_of's answer before it launches."""
    from vlatouch import ops
    assert ops.gemm_block(a, w, out, bias, route=route, **fields) == route


# ---------------------------------------------------------------------------------------- section 1: split-bf16 products
def randn_rows_scaled(shape, gen, scale=1.0):
    """randn whose rows (last dimension) are scaled by 2^e, e uniform in -12 .. 12: the lo half of a split value depends on the value's own exponent, so a
    fault in one row shows in that row."""
    x = torch.randn(shape, generator=gen, device=gen.device) * scale
    e = torch.randint(-12, 13, tuple(shape[:-1]) + (1,), generator=gen, device=gen.device)
    return x * torch.exp2(e.float())


def split_bf16(x):
    hi = x.to(BF16).float()
    lo = (x - hi).to(BF16).float()
    return hi.double(), lo.double()


def x3_refs(a, w):
    """a [.., M, K], w [.., N, K] fp32 -> fp64 (a w^T, the three-term emulation, |a| |w|^T).  Every product of two bf16 values is exact in fp32, so forming
    the terms in fp64 from the split halves equals forming them in fp32 and summing in fp64."""
    ah, al = split_bf16(a)
    wh, wl = split_bf16(w)
    t = lambda m: m.transpose(-1, -2)
    ref = a.double() @ t(w.double())
    emu = ah @ t(wh) + al @ t(wh) + ah @ t(wl)
    den = a.double().abs() @ t(w.double().abs())
    return ref, emu, den


def x3_checks(out, refs, what):
    ref, emu, den = refs
    below(float(((out - ref).abs() / den).max()), X3_BAR, f"{what}: componentwise error against fp64")
    below(row_rel_err(out, emu), EMU_BAR, f"{what}: per-row error against the three-term emulation")


@functools.lru_cache(maxsize=None)
def x3_problem(M, N, K):
    """CPU operands and references of one plain x3 product, shared by the tests that use the shape; never modified."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a, w = randn_rows_scaled((M, K), g), randn_rows_scaled((N, K), g, K ** -0.5)
    bias = torch.randn(N, generator=g)
    return a, w, bias, x3_refs(a, w)


X3_PLAIN = [  # M, N, K, splitk, bias, route
    (70, 100, 64, 1, True, "F32R"),        # ragged M and N, N % 4 == 0
    (200, 260, 1088, 1, True, "F32R"),     # 34 k-tiles
    (512, 512, 2560, 3, False, "F32R"),    # uneven slices, slabs
    (200, 260, 1064, 1, False, "REG"),     # K % 64 == 40: 64 x 64 tile, ragged last k-tile, hi and lo planes
    (20, 260, 1064, 1, False, "REG"),      # 32 x 64 tile (M <= 32)
    (70, 100, 40, 1, False, "REG"),        # fewer k than one tile
    (257, 36, 160, 2, False, "REG"),       # raw slabs, narrow N
]


@pytest.mark.parametrize("M,N,K,splitk,with_bias,route", X3_PLAIN)
def test_x3_product(dev, M, N, K, splitk, with_bias, route):
    """a_dtype F32, w_dtype F32X3, fp32 out.  The product is held to both x3 bars without a bias; the bias launch of the same block must then equal
    fp32(product + bias) BIT FOR BIT (both kernels add the bias to the finished accumulator), which is stronger than any tolerance — and is how a bias of
    unit size can be checked next to products of rows scaled down to 2^-24, where the componentwise measure of the sum would only see the bias' own rounding.
    The biased output is also held to the componentwise bar with the bias in the denominator."""
    from vlatouch import _lib as L
    a, w, bias, refs = x3_problem(M, N, K)
    what = f"x3 {route} ({M}, {N}, {K}) splitk {splitk}"
    g = Guard(dev, F32, M, N, S=splitk)
    launch(route, a.to(dev), w.to(dev), g.out(), w_code=L.F32X3, splitk=splitk)
    g.check(what)
    x3_checks(g.result().cpu(), refs, what)
    if with_bias:
        gb = Guard(dev, F32, M, N)
        launch(route, a.to(dev), w.to(dev), gb.out(), bias.to(dev), w_code=L.F32X3)
        gb.check(what + " + bias")
        same_bits(gb.out(), g.out() + bias.to(dev), what + ": bias launch == fp32(product + bias)")
        ref, _, den = refs
        err = (gb.result().cpu() - (ref + bias.double())).abs() / (den + bias.double().abs())
        below(float(err.max()), X3_BAR, what + " + bias: componentwise error against fp64")


@pytest.mark.parametrize("act", [4, 1, 3], ids=["mish", "gelu", "silu"])
def test_x3_epilogue_on_the_register_staged_kernel(dev, act):
    """(200, 260, 1088) with bias, activation, column scale and residual: the ring has no such epilogue, so the shape lands on REG.  The epilogue is applied
    in fp64 to the fp64 product; max-norm bar of test_gemm_plain's fp32 epilogue."""
    from vlatouch import _lib as L
    M, N, K = 200, 260, 1088
    a, w, bias, (ref, _, _) = x3_problem(M, N, K)
    gen = torch.Generator().manual_seed(77 + act)
    cs, res = torch.randn(N, generator=gen) + 1.0, torch.randn(M, N, generator=gen)
    g = Guard(dev, F32, M, N)
    launch("REG", a.to(dev), w.to(dev), g.out(), bias.to(dev), w_code=L.F32X3, act=act, colscale=cs.to(dev), residual=res.to(dev))
    g.check("x3 epilogue")
    want = res.double() + cs.double() * ACTS[act](ref + bias.double())
    below(rel_err(g.result(), want), 2e-5, f"x3 REG epilogue act {act}: max-norm error against fp64")


def test_x3_ring_and_register_staged_kernels_agree(dev):
    """The same (200, 260, 1088) product from F32R and from REG (a column scale of ones takes the block off the ring)."""
    from vlatouch import _lib as L
    M, N, K = 200, 260, 1088
    a, w, _, refs = x3_problem(M, N, K)
    ring, reg = Guard(dev, F32, M, N), Guard(dev, F32, M, N)
    launch("F32R", a.to(dev), w.to(dev), ring.out(), w_code=L.F32X3)
    launch("REG", a.to(dev), w.to(dev), reg.out(), w_code=L.F32X3, colscale=torch.ones(N, device=dev))
    ring.check("x3 ring"), reg.check("x3 reg")
    x3_checks(reg.result().cpu(), refs, "x3 REG (200, 260, 1088) colscale 1")
    below(row_rel_err(ring.result(), reg.result()), EMU_BAR, "x3 F32R against REG, per row")


def im2col(x, taps, tout, stride, off0):
    """x [.., B, Tin, cin] -> the kernel's implicit A' [.., B * tout, taps * cin]: A'[(b, t), tap * cin + c] = x[b, t * stride + off0 + tap, c] or 0 outside."""
    B, tin, cin = x.shape[-3:]
    cols = []
    for tap in range(taps):
        rows = torch.arange(tout) * stride + off0 + tap
        ok = (rows >= 0) & (rows < tin)
        piece = x[..., rows.clamp(0, tin - 1), :] * ok[:, None].to(x.dtype)
        cols.append(piece)
    return torch.cat(cols, -1).reshape(*x.shape[:-3], B * tout, taps * cin)


X3_CONV = [  # B, T, cin, cout, k, stride, splitk, route
    (3, 16, 256, 256, 5, 1, 4, "F32R"),     # padding taps read the zero page, grouped slabs
    (3, 8, 512, 512, 5, 1, 4, "REG"),       # M = 24
    (3, 16, 24, 64, 5, 1, 1, "REG"),        # cin not a multiple of the k-tile: a tile spans taps
    (5, 16, 64, 96, 3, 2, 1, "F32R"),       # strided (M = 5 x 8 = 40: the ring wants 32 rows)
]


@pytest.mark.parametrize("B,T,cin,cout,k,stride,splitk,route", X3_CONV)
def test_x3_conv_two_groups(dev, B, T, cin, cout, k, stride, splitk, route):
    """The implicit conv1d of the U-Net drivers (two nets = two groups) in x3 arithmetic.  fp64 reference: F.conv1d; the componentwise measure and the
    emulation use the im2col of the same operands (checked against F.conv1d here, in fp64)."""
    from vlatouch import _lib as L
    G, pad = 2, k // 2
    tout = (T + 2 * pad - k) // stride + 1
    gen = torch.Generator().manual_seed(31 * cin + cout + stride)
    x = randn_rows_scaled((G, B, T, cin), gen)
    w = randn_rows_scaled((G, cout, cin * k), gen, (cin * k) ** -0.5).reshape(G, cout, cin, k)
    wp = w.permute(0, 1, 3, 2).reshape(G, cout, k * cin).contiguous()                  # tap-major: W'[co, tap * cin + ci] = w[co, ci, tap]
    what = f"x3 conv {route} B {B} T {T} cin {cin} cout {cout} k {k} stride {stride} splitk {splitk}"
    g = Guard(dev, F32, B * tout, cout, G=G, S=splitk)
    launch(route, x.to(dev), wp.to(dev), g.out(), w_code=L.F32X3, splitk=splitk, conv=dict(taps=k, cin=cin, tout=tout, stride=stride, off0=-pad))
    g.check(what)
    refs = x3_refs(im2col(x, k, tout, stride, -pad), wp)
    conv = torch.stack([F.conv1d(x[i].double().transpose(1, 2), w[i].double(), None, stride=stride, padding=pad).transpose(1, 2).reshape(B * tout, cout)
                        for i in range(G)])
    assert group_rel_err(refs[0], conv) < 1e-13, "the test's own im2col"
    x3_checks(g.result().cpu(), (conv, refs[1], refs[2]), what)


# ---------------------------------------------------------------------------------------- sections 2 and 3: grouped and pitched launches
def _operand(gen, G, rows, cols, ld, dtype, shared, scale=1.0, x3=False, quiet=True):
    """[G, rows, cols] view (row stride ld >= cols) of fresh device data; shared: one [rows, cols] expanded over the groups (group stride 0).  Groups 1 and
    G - 1 of a per-group operand are scaled by 1/16 when `quiet` (a group of small values must not hide behind the others)."""
    lead = () if (G is None or shared) else (G,)
    t = randn_rows_scaled(lead + (rows, ld), gen, scale) if x3 else torch.randn(lead + (rows, ld), generator=gen, device=gen.device) * scale
    if lead and quiet:
        t[1] *= 1.0 / 16
        t[G - 1] *= 1.0 / 16
    v = t.to(dtype)[..., :cols]
    return v.expand(G, rows, cols) if (G is not None and shared) else v


def run_block(dev, route, M, N, K, G, adt, odt, *, wdt=None, x3=False, shared_a=False, shared_w=False, bias=None, res=None, act=0, splitk=1,
              lda=None, ldw=None, ldc=None, ldr=None, col0=0):
    """One grouped (G = None: plain) block against fp64, its guard regions checked.  bias / res: None | "per" | "shared" | (res only) "inplace"; returns the
    Guard and the operands for follow-up launches."""
    from vlatouch import _lib as L
    wdt = adt if wdt is None else wdt
    gen = torch.Generator(device=dev)
    gen.manual_seed(7919 * M + 31 * N + K)
    a = _operand(gen, G, M, K, lda or K, adt, shared_a, x3=x3)
    w = _operand(gen, G, N, K, ldw or K, wdt, shared_w, K ** -0.5, x3=x3, quiet=shared_a)      # a shared A: the quiet groups are W's
    b = None if bias is None else _operand(gen, G, 1, N, N, F32, bias == "shared", quiet=False)[..., 0, :]
    g = Guard(dev, odt, M, N, G=G, S=splitk, ld=ldc, col0=col0)
    r = None
    if res == "inplace":
        g.out().copy_(_operand(gen, G, M, N, N, odt, False, quiet=False))
        r = g.out()
    elif res is not None:
        r = _operand(gen, G, M, N, ldr or N, odt, res == "shared", quiet=False)
    r_init = None if r is None else r.clone()          # the residual as it is before the launch (an in-place launch overwrites it)
    r0 = None if r is None else r_init.double()
    fields = dict(act=act, splitk=splitk, residual=r)
    if x3:
        fields["w_code"] = L.F32X3
    what = f"{route} {str(adt)[6:]} x {'x3' if x3 else str(wdt)[6:]} -> {str(odt)[6:]} ({M}, {N}, {K}) G {G} splitk {splitk} ld a/w/c/r {lda}/{ldw}/{ldc}/{ldr} col0 {col0}"
    launch(route, a, w, g.out(), b, **fields)
    g.check(what)
    out = g.result()
    a_r = a.to(BF16) if (adt == F32 and wdt == BF16) else a          # fp32 activations on bf16 weights are rounded to bf16 at staging
    if x3:
        assert b is None and r is None and act == 0
        x3_checks(out, x3_refs(a, w), what)
    else:
        want = a_r.double() @ w.double().transpose(-1, -2)
        if b is not None:
            want = want + b.double().unsqueeze(-2)
        want = ACTS[act](want)
        if r0 is not None:
            want = want + r0
        exact = adt == F32 and wdt == F32
        tol = (2e-6 if route == "F32R" else 2e-5) if exact else (2e-3 if odt == F32 else 1e-2)
        below(group_rel_err(out, want), tol, what + ": worst group's max-norm error against fp64")
    if G is not None and route in ("GLDS", "PPK", "PP") and res != "inplace":
        # the group index changes addresses, not arithmetic: where one group alone still takes the same kernel, the grouped output equals it bit for bit
        from vlatouch import ops
        one = Guard(dev, odt, M, N, ld=ldc, col0=col0)
        if ops.gemm_route(ops.gemm_block_params(a[0], w[0], one.out(), None if b is None else b[0], act=act, residual=None if r is None else r[0])) == route:
            for i in range(G):
                one = Guard(dev, odt, M, N, ld=ldc, col0=col0)
                launch(route, a[i], w[i], one.out(), None if b is None else b[i], act=act, residual=None if r is None else r[i])
                same_bits(one.out(), g.out()[i], f"{what}: group {i} alone")
    return g, dict(a=a, w=w, bias=b, residual=r_init, what=what)


GROUPED = {
    # the DINO patch-embed form: one group per image, shared W / bias / residual, c_gs skips a row between groups
    "glds f16->f32 shared W, bias, residual": dict(route="GLDS", M=130, N=384, K=64, G=16, adt=F16, odt=F32, shared_w=True, bias="shared", res="shared"),
    "glds bf16->bf16 per-group W, bias": dict(route="GLDS", M=130, N=384, K=128, G=16, adt=BF16, odt=BF16, bias="per"),
    # the RDT image-adaptor form: M % 160 == 40 gives every group a clamped last row tile
    "ppk bf16->bf16 shared W, residual": dict(route="PPK", M=200, N=256, K=512, G=25, adt=BF16, odt=BF16, shared_w=True, bias="shared", res="shared"),
    "ppk bf16->f32 shared W, residual": dict(route="PPK", M=200, N=256, K=512, G=25, adt=BF16, odt=F32, shared_w=True, bias="shared", res="shared"),
    # M % 256 == 1: 255 clamped rows sit above the next group
    "pp bf16->bf16 per-group W": dict(route="PP", M=257, N=256, K=1024, G=96, adt=BF16, odt=BF16, bias="per"),
    "pp bf16->bf16 shared W, gelu_tanh": dict(route="PP", M=300, N=512, K=512, G=128, adt=BF16, odt=BF16, shared_w=True, bias="shared", act=2),
    # K % 64 != 0 keeps the block off the LDS-DMA family: 2 x 3 x 16 = 96 tiles of 128 x 128 -> the 64 x 64 register tile, 192 tiles -> the 128 x 128 one
    "reg bf16->f32 K=72": dict(route="REG", M=130, N=384, K=72, G=16, adt=BF16, odt=F32, bias="per"),
    "reg bf16->f32 K=72, 128x128 tile": dict(route="REG", M=130, N=384, K=72, G=32, adt=BF16, odt=F32, bias="per"),
    "reg f32 x bf16 -> f32": dict(route="REG", M=200, N=384, K=64, G=16, adt=F32, wdt=BF16, odt=F32, bias="per"),
    # the first film_tables Linear: both nets read the same A
    "reg f32 shared A, mish": dict(route="REG", M=3, N=1024, K=256, G=2, adt=F32, odt=F32, shared_a=True, bias="per", act=4),
    # slabs at C + grp * c_gs + slice * c_slab, c_slab = G * c_gs (conv_slabs' layout)
    "f32r exact splitk 4": dict(route="F32R", M=64, N=512, K=1280, G=2, adt=F32, odt=F32, splitk=4),
    "f32r x3 splitk 5": dict(route="F32R", M=96, N=512, K=2560, G=2, adt=F32, odt=F32, x3=True, splitk=5),
    "reg x3 splitk 5": dict(route="REG", M=24, N=512, K=2560, G=2, adt=F32, odt=F32, x3=True, splitk=5),
}


@pytest.mark.parametrize("label", list(GROUPED))
def test_grouped_launch(dev, label):
    """Every kernel that takes groups, c_gs = (M + 1) * ldc; every group has its own data, error per group."""
    run_block(dev, **GROUPED[label])


PITCHED = {
    "glds lda 128, ldc 448": dict(route="GLDS", M=130, N=384, K=64, G=16, adt=F16, odt=F32, shared_w=True, bias="shared", lda=128, ldc=448),
    "ppk ldc 320, ldr 256": dict(route="PPK", M=200, N=256, K=512, G=25, adt=BF16, odt=F32, shared_w=True, bias="shared", res="per", ldc=320, ldr=256),
    "pp ldc 576": dict(route="PP", M=300, N=512, K=512, G=128, adt=BF16, odt=BF16, shared_w=True, bias="shared", ldc=576),
    # the second film_tables Linear writes an N-wide product into a column block of a wider table
    "reg f32 ldc 512, columns 0..": dict(route="REG", M=5, N=256, K=1024, G=2, adt=F32, odt=F32, bias="per", ldc=512, col0=0),
    "reg f32 ldc 512, columns 256..": dict(route="REG", M=5, N=256, K=1024, G=2, adt=F32, odt=F32, bias="per", ldc=512, col0=256),
    "f32r lda 96, ldw 80": dict(route="F32R", M=70, N=100, K=64, G=None, adt=F32, odt=F32, bias="per", lda=96, ldw=80),
    # ldc % 4 != 0 leaves the LDS-DMA family and takes the scalar-store epilogue
    "reg f16->f32 ldc 386": dict(route="REG", M=130, N=384, K=64, G=16, adt=F16, odt=F32, shared_w=True, bias="shared", ldc=386),
    "reg bf16->bf16 ldc 386": dict(route="REG", M=130, N=384, K=64, G=16, adt=BF16, odt=BF16, bias="per", ldc=386),
    # N % 4 != 0, residual with an odd pitch
    "reg f32 N 101, ldc 103, ldr 105": dict(route="REG", M=70, N=101, K=64, G=2, adt=F32, odt=F32, bias="per", res="per", ldc=103, ldr=105),
    "reg bf16->bf16 N 102, ldc 103, ldr 105": dict(route="REG", M=70, N=102, K=64, G=2, adt=BF16, odt=BF16, bias="per", res="per", ldc=103, ldr=105),
}


@pytest.mark.parametrize("label", list(PITCHED))
def test_pitched_launch(dev, label):
    """lda > K, ldw > K, ldc > N, ldr != ldc, a column offset: the columns outside the window keep the sentinel."""
    run_block(dev, **PITCHED[label])


IN_PLACE = {
    "reg f32": dict(route="REG", M=70, N=256, K=64, G=2, adt=F32, odt=F32, bias="per", ldc=320, col0=64),
    "reg bf16->f32": dict(route="REG", M=70, N=256, K=128, G=2, adt=BF16, odt=F32, bias="per", ldc=320),
    "ppk bf16->f32": dict(route="PPK", M=200, N=256, K=512, G=25, adt=BF16, odt=F32, shared_w=True, bias="shared", ldc=320),
}


@pytest.mark.parametrize("label", list(IN_PLACE))
def test_residual_in_place(dev, label):
    """residual and C are the same pitched fp32 buffer (RDT writes `out` over `residual`): equal, bit for bit, to the launch that reads the same residual
    from a buffer of its own."""
    cfg = IN_PLACE[label]
    g, io = run_block(dev, res="inplace", **cfg)          # compared with fp64 on the residual as it was before the launch
    sep = Guard(dev, F32, cfg["M"], cfg["N"], G=cfg["G"], ld=cfg["ldc"], col0=cfg.get("col0", 0))
    launch(cfg["route"], io["a"], io["w"], sep.out(), io["bias"], residual=io["residual"])
    sep.check(io["what"] + " out of place")
    same_bits(g.out(), sep.out(), io["what"] + ": in place == out of place")


# ---------------------------------------------------------------------------------------- section 4: vt_groupnorm over several nets
def gn_reference(slabs, bias, gamma, beta, B, T, ngroups, eps, film, film_off, residual):
    """fp64 group_norm -> mish -> FiLM -> + residual, per net.  slabs [S, nets, B*T, C] ... -> [nets, B*T, C]."""
    S, nets, M, Cc = slabs.shape
    outs = []
    for n in range(nets):
        y = (slabs[:, n].double().sum(0) + bias[n].double()).reshape(B, T, Cc).transpose(1, 2)
        y = F.mish(F.group_norm(y, ngroups, gamma[n].double(), beta[n].double(), eps))
        if film is not None:
            f = film[n].double()
            y = f[:, film_off:film_off + Cc, None] * y + f[:, film_off + Cc:film_off + 2 * Cc, None]
        y = y.transpose(1, 2).reshape(M, Cc)
        outs.append(y if residual is None else y + residual[n].double())
    return torch.stack(outs)


GN_CASES = [  # T, C, ngroups, nslabs, epilogue, out dtype
    (16, 256, 8, 1, "film", F32),
    (16, 256, 8, 5, "residual", F32),
    (16, 256, 8, 8, "film", BF16),
    (16, 256, 8, 11, "residual", BF16),      # past GN_MAX_SLABS: the tail loop
    (16, 256, 4, 11, "film", F32),           # 64 channels x 16 steps = 1024 values per unit
    (16, 256, 32, 5, "residual", F32),       # 8 x 16 = 128 values: half the block idles
    (4, 512, 8, 8, "residual", F32),
    (4, 512, 8, 11, "film", BF16),
    (12, 64, 8, 5, "film", F32),             # 8 x 12 = 96 values per unit: not a multiple of the 256 threads
    (12, 64, 8, 11, "residual", BF16),
    (12, 64, 8, 1, "both", F32),
]


@pytest.mark.parametrize("T,Cc,ngroups,S,epi,odt", GN_CASES)
def test_groupnorm_two_nets(dev, T, Cc, ngroups, S, epi, odt):
    """nets = 2, B = 3 with every per-net stride set so that the nets are NOT back to back (a gap after each net's slabs, vectors, FiLM rows, residual and
    output), a FiLM table wider than 2C read at a column offset, ldr != ldo > C.  Net 1's pre-norm values carry a common offset of 50 (std 1): the
    two-pass variance must not lose them."""
    from vlatouch import ops
    nets, B = 2, 3
    M = B * T
    gen = torch.Generator(device=dev)
    gen.manual_seed(1009 * T + Cc + 7 * ngroups + S)
    rn = lambda *shape: torch.randn(shape, generator=gen, device=dev)
    slabs = rn(S, nets + 1, M + 2, Cc + 8)[:, :nets, :M, :Cc]           # p_gs = (M + 2) * (C + 8), ldp = C + 8, slab_stride = 3 * p_gs
    slabs[:, 1] += 50.0 / S
    vecs = rn(nets, 3, Cc + 4)                                         # vec_gs = 3 * (C + 4)
    bias, gamma, beta = vecs[:, 0, :Cc], vecs[:, 1, :Cc], vecs[:, 2, :Cc]
    gamma += 1.0
    film_off = 2 * Cc + 8
    film = rn(nets, B + 1, 5 * Cc + 16)[:, :B] if epi in ("film", "both") else None      # film_ld = 5C + 16, film_gs = (B + 1) * film_ld
    res = rn(nets, M + 3, Cc + 12).to(odt)[:, :M, :Cc] if epi in ("residual", "both") else None      # ldr = C + 12, r_gs = (M + 3) * ldr
    g = Guard(dev, odt, M, Cc, G=nets, ld=Cc + 24)                      # ldo = C + 24, o_gs = (M + 1) * ldo
    ops.groupnorm_block(slabs, bias, gamma, beta, g.out(), B=B, T=T, ngroups=ngroups, film=film, film_off=film_off, residual=res)
    what = f"groupnorm nets 2 T {T} C {Cc} ngroups {ngroups} nslabs {S} {epi} -> {str(odt)[6:]}"
    g.check(what)
    want = gn_reference(slabs, bias, gamma, beta, B, T, ngroups, 1e-5, film, film_off, res)
    below(group_rel_err(g.result(), want), 2e-5 if odt == F32 else 1e-2, what + ": worst net's max-norm error against fp64")


def test_groupnorm_unit_larger_than_lds_is_refused(dev):
    """C = 2048, ngroups = 1, T = 16: a unit of 128 KiB does not fit the 64 KiB of LDS -> VT_ERR_UNSUPPORTED, nothing launched (the output keeps the sentinel)."""
    from vlatouch import ops, _lib as L
    nets, B, T, Cc = 2, 1, 16, 2048
    slabs = torch.zeros(1, nets, B * T, Cc, device=dev)
    vec = torch.ones(nets, Cc, device=dev)
    g = Guard(dev, F32, B * T, Cc, G=nets)
    p = ops.groupnorm_block_params(slabs, vec, vec, vec, g.out(), B=B, T=T, ngroups=1)
    assert L.lib().vt_groupnorm(C.byref(p), L.stream_ptr(dev)) == -95
    torch.cuda.synchronize()
    assert torch.equal(g.flat, torch.full_like(g.flat, g.bits))
