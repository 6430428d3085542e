"""The host drivers after their shared idioms (element size of a dtype code, the workspace carver, the `create` preamble and weight cursor) moved
into csrc/vt_host.h: every weight count, workspace size, derived-copy size and fused-plan size of tests/host_sizing_cases.py's grid is, byte
for byte, what a build of the commit before gave (tests/golden/g24_host_sizing_parent.json, written by
tools/make_golden_host_sizing_parent.py and never regenerated to make this pass), and each `create` still refuses a wrong count and a null
weight with the text callers saw before.  No GPU: the handles stand on fake pointers, which sizing never dereferences."""
import json
import os

import pytest

from tests import cases
from tests import host_sizing_cases as K
from vlatouch import _lib as L


def test_sizes_are_the_parents():
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        want = json.load(f)["bytes"]
    got = K.sizing()
    assert list(got) == list(want)
    diff = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


def test_the_grid_takes_both_sides_of_the_rdt_carvers_branches():
    """On the recorded numbers: the split-K slabs (M <= 512: 16 * M * 3D * 4 bytes) are in B = 1 and out of B = 32 of the wide model, and the
    row-major K | V scratch of a small condition is in RDT-1B's B = 1 and out of its B = 32."""
    with open(os.path.join(cases.GOLDEN, K.GOLDEN_NAME)) as f:
        w = json.load(f)["bytes"]
    D, N = cases.RDT_WIDE["hidden"], cases.RDT_WIDE["horizon"] + 3
    slabs = 16 * N * 3 * D * 4
    assert w["rdt_wide/bf16/B1_L12/workspace"] > slabs                                  # B = 1: M = 67 <= 512, the slabs alone are 26 MB
    assert w["rdt_wide/bf16/B32_L12/workspace"] < 32 * (w["rdt_wide/bf16/B1_L12/workspace"] - slabs) + slabs      # B = 32: M = 2144, no slabs
    # the row-major K | V scratch of a condition too small for the large-GEMM path, read off what one more language token costs RDT-1B in bf16 (a = 2 bytes):
    # B = 1 (12 and 32 tokens pad to the same 64 cache rows): the adapted token D * a + its scratch row 2 * D * a;
    # B = 32 (384 and 1024 rows are whole 64s): the adapted token + its K | V cache rows in the 14 language blocks, and NO scratch row
    D, a, lang_blocks = K.RDT_1B["hidden"], 2, (K.RDT_1B["depth"] + 1) // 2
    per_tok_1 = (w["rdt_1b/bf16/B1_L32/workspace"] - w["rdt_1b/bf16/B1_L12/workspace"]) // 20
    per_tok_32 = (w["rdt_1b/bf16/B32_L32/workspace"] - w["rdt_1b/bf16/B32_L12/workspace"]) // (32 * 20)
    assert per_tok_1 == D * a + 2 * D * a
    assert per_tok_32 == D * a + lang_blocks * 2 * D * a


CREATES = [("unet", lambda: K.unet_desc(L.F32X3, L.F32), "weight pointers"), ("dino", lambda: K.dino_desc("small", L.BF16), "weights"),
           ("t5", lambda: K.t5_desc(L.BF16), "weights"), ("lstm", lambda: K.lstm_desc(L.F32), "weights"),
           ("rdt", lambda: K.rdt_desc(cases.RDT_TINY, L.BF16), "weights")]


@pytest.mark.parametrize("prefix,desc,noun", CREATES, ids=[c[0] for c in CREATES])
def test_create_refuses_a_wrong_count_and_a_null_weight_with_the_same_words(prefix, desc, noun):
    lib = L.lib()
    rc, _, n = K.create(prefix, desc(), n=3)
    assert rc != 0 and lib.vt_last_error().decode() == f"vt_{prefix}_create: expected {n} {noun}, got 3"
    rc, h, n = K.create(prefix, desc(), null_at=5)
    if prefix == "unet":        # its residual-conv slots are null where a block keeps its width: a null entry is data, not an error
        assert rc == 0
        lib.vt_unet_destroy(h)
    else:
        assert rc != 0 and lib.vt_last_error().decode() == f"vt_{prefix}_create: weight 5 is null"
    assert getattr(lib, f"vt_{prefix}_create")(None, None, 0, None) != 0 and lib.vt_last_error().decode() == f"vt_{prefix}_create: null argument"
