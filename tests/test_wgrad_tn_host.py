"""vt_gemm_tn_plan (csrc/vt_gemm_tn.hip) without a GPU: the row splits of the transpose-free weight-gradient GEMM are a pure function of
(M, N, K) that covers rows 0 .. M - 1 exactly once in order, in runs that are multiples of the kernel's m-step, with the workspace the header
states; bad shapes are refused."""
import pytest

from tests import wgrad_tn_ref as W

VT_ERR_ARG = -22


def _rows():
    return sorted({1, 3, 32, 33, 64, 127, 128, 129, 4374 * 4, 4374 * 32, 17496 * 4} | {67 * B for B in range(1, 33)} | set(range(1, 33)))


def test_plan_over_the_trainers_shapes():
    widths = W.trainer_widths() + [(n, k) for (_, n, k) in W.KERNEL_CASES]
    assert (4096, 2048) in widths and (256, 96) in widths and (256, 80) in widths       # the K|V product of RDT-1B, RDT_TINY's adaptors
    seen_split = seen_single = 0
    for N, K in widths:
        for M in _rows():
            rc, S, rps, step, ws = W.plan(M, N, K)
            assert rc == 0, (M, N, K)
            assert step == W.M_STEP and S >= 1 and rps >= step and rps % step == 0, (M, N, K, S, rps)
            # split s owns rows [s rps, min(M, (s + 1) rps)): in order, disjoint, none empty, together 0 .. M - 1
            assert (S - 1) * rps < M <= S * rps, (M, N, K, S, rps)
            if S == 1:
                assert ws == 0, (M, N, K, ws)
                seen_single += 1
            else:
                assert ws == (S * (N * K + N) * 4 + 255) // 256 * 256, (M, N, K, S, ws)
                seen_split += 1
            assert W.plan(M, N, K) == (rc, S, rps, step, ws), "the plan must be a pure function of its arguments"
    assert seen_split and seen_single


def test_plan_depends_on_nothing_seen_before():
    """The same arguments give the same plan whatever was asked in between."""
    first = {c: W.plan(*c) for c in [(530, 128, 256), (67 * 4, 2048, 2048), (4374 * 4, 4096, 2048), (4, 2048, 256)]}
    for c in reversed(list(first)):
        W.plan(1, 8, 8), W.plan(4374 * 32, 4096, 2048)
        assert W.plan(*c) == first[c]


def test_the_split_rule_as_the_header_states_it():
    for M, N, K in [(1, 8, 8), (127, 128, 128), (128, 128, 128), (353, 128, 128), (67 * 32, 2048, 256), (67 * 4, 2048, 2048), (4374 * 32, 2048, 1152),
                    (4374 * 4, 4096, 2048), (32, 2048, 256), (5000, 8, 8)]:
        tiles = -(-N // 128) * -(-K // 128)
        steps = -(-M // 32)
        S = max(1, min(-(-256 // tiles), steps // 4, 16))
        rps = -(-steps // S) * 32
        S = -(-M // rps)
        assert W.plan(M, N, K)[1:3] == (S, rps), (M, N, K)
    assert W.plan(4374 * 4, 4096, 2048)[1] == 1              # 512 tiles already fill the chip: no workspace for the largest product
    assert W.plan(5000, 8, 8)[1] == 16                       # the cap


def test_the_split_case_of_the_gpu_test():
    M, N, K = W.split_case()
    rc, S, rps, _, ws = W.plan(M, N, K)
    assert rc == 0 and S >= 3 and M % rps != 0 and ws > 0, (M, S, rps)
    assert W.plan(M - 1, N, K)[1] < 3


@pytest.mark.parametrize("M,N,K", [(0, 8, 8), (-1, 8, 8), (4, 12, 8), (4, 8, 20), (4, 0, 8), (4, 8, 0), (4, 7, 9)])
def test_bad_arguments(M, N, K):
    from vlatouch import _lib as L
    rc, S, rps, _, ws = W.plan(M, N, K)
    assert rc == VT_ERR_ARG and (S, rps, ws) == (0, 0, 0)
    assert "vt_gemm_tn_plan" in L.lib().vt_last_error().decode()
    assert L.lib().vt_gemm_tn_plan(8, 8, 8, None) == VT_ERR_ARG
