"""vt_attention_bwd_mfma without a GPU: its statement (tests/attn_bwd_mfma_ref.py: P and dS rounded once to bf16) holds the project's bf16
attention-backward bar on every kernel case, so the bar of tests/test_gpu_attn_bwd_mfma.py is reachable;
the workspace query is positive, monotone and refuses what the kernel refuses."""
import pytest
import torch

from tests import attn_bwd_mfma_ref as M


@pytest.mark.parametrize("B,Nq,Nk,H,cross", M.KERNEL_CASES)
def test_statement_holds_the_bf16_bar(B, Nq, Nk, H, cross):
    """Per gradient, max-abs error against fp64 autograd of the same bf16-rounded inputs <= 1.5 x that of torch's bf16 CPU backward."""
    bufs, views, do, _ = M.make_case(B, Nq, Nk, H, cross, seed=Nk)
    ref, tb = M.refs((B, Nq, Nk, H, cross, "plain"), bufs, views, do, None)
    q, k, v = views(*bufs)
    got = M.statement(q, k, v, do)[:3]
    for i, name in enumerate(("dq", "dk", "dv")):
        e, et = float((got[i].double() - ref[i]).abs().max()), float((tb[i] - ref[i]).abs().max())
        print(f"[statement {Nq}x{Nk} H{H}] {name}: max err {e:.3e}; torch bf16 on the CPU {et:.3e}")
        assert e <= 1.5 * et, (name, e, et)


def test_statement_masks():
    """A masked key gets zero dK and dV, a batch element without live keys zero gradients, everything finite, and the bar holds."""
    B, Nq, Nk, H = 2, 33, 65, 2
    mask = torch.ones(B, Nk, dtype=torch.bool)
    mask[0, Nk - 3:] = False
    mask[1, :] = False
    bufs, views, do, _ = M.make_case(B, Nq, Nk, H, True, seed=Nk)
    ref, tb = M.refs((B, Nq, Nk, H, True, "tail+dead"), bufs, views, do, mask)
    q, k, v = views(*bufs)
    got = M.statement(q, k, v, do, mask=mask)[:3]
    for i in range(3):
        assert bool(torch.isfinite(got[i]).all())
        assert float(got[i][1].abs().max()) == 0.0
        assert float((got[i].double() - ref[i]).abs().max()) <= 1.5 * float((tb[i] - ref[i]).abs().max())
    assert float(got[1][0, Nk - 3:].abs().max()) == 0.0 and float(got[2][0, Nk - 3:].abs().max()) == 0.0


def test_workspace_query():
    from vlatouch import _lib as L
    f = L.lib().vt_attention_bwd_mfma_ws_bytes
    for B, Nq, Nk, H, _ in M.KERNEL_CASES:
        n = f(B, H, Nq, Nk)
        assert n > 0
        assert f(B + 1, H, Nq, Nk) >= n and f(B, H + 1, Nq, Nk) >= n and f(B, H, Nq, Nk + 1) >= n and f(B, H, Nq, Nk + 64 * M.RUN_TILES) > n
    assert f(2, 2, 129, 64) < 0 and f(2, 2, 0, 64) < 0 and f(2, 2, 67, 0) < 0 and f(2048, 32, 67, 64) < 0      # Nq cap, empty shapes, B * H > 65535
    assert f(4, 32, 67, 4374) == 4 * 32 * 18 * 67 * 67 * 4                                                       # 18 runs of (3 + 64) floats per row
