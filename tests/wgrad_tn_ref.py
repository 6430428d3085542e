"""The statement of vt_gemm_tn (csrc/vt_gemm_tn.hip) and the case lists of its tests.

dW[N, K] = sum_m dy[m, n] x[m, k] and db[N] = sum_m dy[m, n] for 16-bit dy [M, N], x [M, K]: `ref` is that product in fp64 of the inputs as they
are stored (already rounded to bf16 or fp16), so the only error of a correct kernel is its fp32 summation.  With small integers as inputs every
partial sum is an integer below 2^24 and ANY summation order gives the fp64 result exactly: the exact cases are the structural test."""
import ctypes as C

import torch

M_STEP = 32           # the kernel's reduction step; rows_per_split is a multiple of it
TILE = 128            # the workgroup's tile of dW on both axes

# (M, N, K).  Against the 128 x 128 tile and the 32-row m-step: N ragged in 8, 80, 96, 264 and exact in 256, 128; K ragged in 8, 96, 80, 136 and
# exact in 2048, 256; N crosses a tile in 256, 264 and K in 2048, 136, 256, 264; M crosses the m-step in 201, 268, 530 and is ragged in all of the first six.
# None of those six has M a multiple of the m-step, so (96, 136, 264) is added: three full m-steps, ragged and crossing on N and K.
KERNEL_CASES = [(1, 8, 8), (3, 256, 2048), (8, 80, 96), (201, 96, 80), (268, 264, 136), (530, 128, 256), (96, 136, 264)]


def plan(M, N, K):
    """vt_gemm_tn_plan -> (return code, splits, rows_per_split, m_step, ws_bytes).  Host only."""
    from vlatouch import _lib as L
    p = L.GemmTnPlan()
    rc = L.lib().vt_gemm_tn_plan(M, N, K, C.byref(p))
    return rc, p.splits, p.rows_per_split, p.m_step, p.ws_bytes


def split_case(N=128, K=128, want=3, limit=1 << 16):
    """The smallest M whose plan for [N, K] has at least `want` row splits -> (M, N, K)."""
    for M in range(1, limit):
        rc, S, _, _, _ = plan(M, N, K)
        assert rc == 0
        if S >= want:
            return (M, N, K)
    raise AssertionError(f"no M below {limit} gives {want} splits for N = {N}, K = {K}")


def trainer_widths():
    """(N, K) of every Linear weight of the test models and of RDT-1B."""
    from tests import cases
    out = set()
    for cfg in (cases.RDT_TINY, cases.RDT_WIDE):
        out |= {tuple(v.shape) for k, v in cases.rdt_sd(cfg).items() if k.endswith(".weight") and v.dim() == 2}
    D = 2048                                                      # RDT-1B: hidden 2048, T5-XXL 4096, SigLIP 1152, state 128 + mask
    out |= {(3 * D, D), (2 * D, D), (D, D), (4 * D, D), (D, 4 * D), (D, 4096), (D, 1152), (D, 256), (128, D), (D, 256)}
    return sorted(out)


def ref(dy, x):
    """fp64 (dW, db) of the 16-bit-rounded inputs."""
    d, xx = dy.double().cpu(), x.double().cpu()
    return d.t() @ xx, d.sum(0)


def units(dy, x):
    """The error units: max over elements of sum_m |dy x| and of sum_m |dy|."""
    d, xx = dy.double().cpu().abs(), x.double().cpu().abs()
    return float((d.t() @ xx).max()), float(d.sum(0).max())


def exact_inputs(M, N, K, dtype, seed=0, pitch_dy=None, pitch_x=None):
    """Integers in {-2 .. 2} stored in `dtype`, optionally as the leading columns' worth of wider buffers."""
    g = torch.Generator().manual_seed(seed + M * 7 + N * 3 + K)
    dy = torch.randint(-2, 3, (M, pitch_dy or N), generator=g).to(dtype)
    x = torch.randint(-2, 3, (M, pitch_x or K), generator=g).to(dtype)
    return dy, x


def random_inputs(M, N, K, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed + M * 7 + N * 3 + K)
    return torch.randn(M, N, generator=g).to(dtype), torch.randn(M, K, generator=g).to(dtype)
