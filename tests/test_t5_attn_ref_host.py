"""The fp64 statement of T5's bias attention (tests/t5_attn_ref.py) against the attention inside t5_ref.encode(dtype=float64), which
test_t5_host.py pins to HF; the coverage of the GPU grid; the structure of the needle inputs; what the number formats alone cost over the grid
(printed, and the only source of the GPU test's bars); and the proof that the grid's inputs catch a wrong kernel: five mutations of the
reference, each of which must leave the bars."""
import itertools

import pytest
import torch

from tests import t5_attn_ref as T
from tests import t5_ref

torch.set_grad_enabled(False)
GRID = T.gpu_grid()
_CACHE = {}


def tensors_and_reference(i):
    """The inputs of grid case i and their reference, computed once for the whole module and never written to."""
    if i not in _CACHE:
        t = T.case_tensors(GRID[i])
        _CACHE[i] = t + (T.reference(*t),)
    return _CACHE[i]


@pytest.mark.parametrize("cfg", T.BUCKETS)
@pytest.mark.parametrize("mask,B,L", [("none", 1, 17), ("trail", 2, 65), ("holes", 3, 70), ("lead", 1, 130), ("per_sample", 3, 33)])
def test_reference_is_the_attention_of_t5_ref_in_float64(cfg, mask, B, L):
    """One layer with o = identity, wo = 0 and unit final norm: encode returns rms(x + attention), and q, k, v are the same Linears of the same
    normed rows, so the two attentions see the same values."""
    H, D = 2, 128
    nb, md = cfg
    c = dict(vocab_size=40, d_model=D, num_heads=H, d_kv=64, d_ff=64, num_layers=1, relative_attention_num_buckets=nb,
             relative_attention_max_distance=md, layer_norm_epsilon=1e-6)
    g = torch.Generator().manual_seed(L + nb)
    a, f = "encoder.block.0.layer.0.", "encoder.block.0.layer.1."
    sd = {"shared.weight": torch.randn(40, D, generator=g, dtype=torch.float64),
          a + "layer_norm.weight": torch.rand(D, generator=g, dtype=torch.float64) + 0.5,
          a + "SelfAttention.relative_attention_bias.weight": torch.randn(nb, H, generator=g, dtype=torch.float64),
          a + "SelfAttention.o.weight": torch.eye(D, dtype=torch.float64),
          f + "layer_norm.weight": torch.ones(D, dtype=torch.float64),
          f + "DenseReluDense.wi_0.weight": torch.randn(64, D, generator=g, dtype=torch.float64),
          f + "DenseReluDense.wi_1.weight": torch.randn(64, D, generator=g, dtype=torch.float64),
          f + "DenseReluDense.wo.weight": torch.zeros(D, 64, dtype=torch.float64),
          "encoder.final_layer_norm.weight": torch.ones(D, dtype=torch.float64)}
    for n in "qkv":
        sd[a + f"SelfAttention.{n}.weight"] = torch.randn(D, D, generator=g, dtype=torch.float64) * (0.3 if n != "v" else 1.0) / D ** 0.5
    ids = torch.randint(0, 40, (B, L), generator=g)
    keep = T.make_mask(mask, B, L)
    want = t5_ref.encode(sd, c, ids, None if keep is None else keep.long(), dtype=torch.float64)
    x = sd["shared.weight"][ids]
    h = t5_ref._rms(x, sd[a + "layer_norm.weight"], 1e-6)
    q, k, v = (torch.nn.functional.linear(h, sd[a + f"SelfAttention.{n}.weight"]).view(B, L, H, 64) for n in "qkv")
    att = T.reference(q, k, v, sd[a + "SelfAttention.relative_attention_bias.weight"], T.rel_buckets(L, nb, md), keep)
    got = t5_ref._rms(x + att.reshape(B, L, D), sd["encoder.final_layer_norm.weight"], 1e-6)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((att.reshape(B, L, D) - 0).abs().max()) > 0.1                      # the attention term is not lost in x


def test_the_grid_covers_what_the_gpu_test_claims():
    assert len({tuple(sorted(c.items())) for c in GRID}) == len(GRID)
    assert {s[0] for s in T.SHAPES} == {1, 3} and {s[1] for s in T.SHAPES} == {1, 3, 6}
    for c in GRID:
        shape = (c["B"], c["H"], c["L"])
        assert shape in T.SHAPES or shape == T.LONG
        assert T.mask_ok(c["mask"], c["B"], c["L"]) and (c["num_buckets"], c["max_distance"]) in T.BUCKETS
    for dname in T.DT:
        mine = [c for c in GRID if c["dname"] == dname]
        assert {c["L"] for c in mine if c["mask"] == "none"} == {1, 15, 16, 17, 63, 64, 65, 128, 129, 200, 1024}
        assert [(c["B"], c["H"]) for c in mine if c["L"] == 1024] == [(1, 2)] * 2         # the two bias regimes of (126, 1000), nothing else
        assert {(c["mask"], c["regime"]) for c in mine if c["mask"] != "none"} == set(itertools.product(T.MASKS[1:], T.REGIMES))
        assert {c["regime"] for c in mine if c["mask"] == "none"} == set(T.REGIMES)
        for cfg in T.BUCKETS:                       # both bias regimes where the configuration's saturated last bucket is reached
            for regime in T.BIAS_REGIMES:
                assert any(c["regime"] == regime and (c["num_buckets"], c["max_distance"]) == cfg and c["L"] > T.last_bucket_from(*cfg)
                           for c in mine), (dname, cfg, regime)
        keeps = [T.make_mask(c["mask"], c["B"], c["L"]) for c in mine if c["mask"] != "none"]
        assert all(bool(k.any(-1).all()) and not bool(k.all()) for k in keeps)              # a key in every sample, and something masked
        assert any(c["mask"] == "per_sample" and 1 in T.make_mask("per_sample", c["B"], c["L"]).sum(-1).tolist() for c in mine)
        assert any(c["mask"] in ("lead", "first_tile") and c["L"] > 64 and not bool(T.make_mask(c["mask"], c["B"], c["L"])[:, :64].any())
                   for c in mine)                                                           # a leading tile without a valid key
        seen = {(h + c["seed"]) % 6 for c in mine if c["regime"] == "bias_needle" for h in range(c["H"])}
        assert seen == set(range(6))                # every needle position: rel 0, +1, -1, +max_exact, -max_distance, +(L - 1)


def test_bucket_tables_of_the_configurations():
    for nb, md in T.BUCKETS:
        bk = T.rel_buckets(1024, nb, md)
        assert int(bk.min()) == 0 and int(bk.max()) == nb - 1
        half, exact = nb // 2, nb // 2 // 2
        assert T.bucket_of(0, nb, md) == 0 and T.bucket_of(1, nb, md) == half + 1 and T.bucket_of(-1, nb, md) == 1
        assert T.bucket_of(exact, nb, md) == half + exact and T.bucket_of(exact - 1, nb, md) == half + exact - 1
        assert T.bucket_of(-md, nb, md) == half - 1 == T.bucket_of(-1023, nb, md) and T.bucket_of(1023, nb, md) == nb - 1
        assert T.last_bucket_from(nb, md) <= md


def test_structure_of_the_inputs():
    """Ones and tile columns of the reference sum to one; ascending / descending tile maxima move as the regime says, bias included; and every
    needle row whose needle keys exist unmasked has at least 0.9 of its weight on them, which the one-hot columns show."""
    needle_rows = 0
    for i, c in enumerate(GRID):
        q, k, v, rb, bk, keep, ref = tensors_and_reference(i)
        B, H, L = c["B"], c["H"], c["L"]
        assert float((ref[..., T.C_ONE] - 1.0).abs().max()) <= 1e-12
        assert float((ref[..., T.C_TILE:T.C_TILE + 4].sum(-1) - 1.0).abs().max()) <= 1e-12
        assert float((ref[..., T.C_HOT:T.C_HOT + 8].sum(-1) - 1.0).abs().max()) <= 1e-12
        s, _ = T._scores(q, k, rb, bk, keep)
        assert float(s[torch.isfinite(s)].abs().max()) <= 16.0
        if c["regime"] in ("ascending", "descending") and c["mask"] == "none" and L > T.KT:
            d = torch.stack([s[..., t:t + T.KT].amax(-1) for t in range(0, L, T.KT)], -1).diff(dim=-1)
            assert bool((d > 0).all()) if c["regime"] == "ascending" else bool((d < 0).all())
        if c["regime"] != "bias_needle":
            continue
        p = torch.softmax(s, -1)                                                    # [B, H, L, L]; every sample of the grid has a valid key
        hot = ref[..., T.C_HOT:T.C_HOT + 8]                                           # [B, L, H, 8]
        for h, nbk in enumerate(T.needle_bucket_of_head(H, L, c["num_buckets"], c["max_distance"], c["seed"])):
            on = (bk == nbk)[None].expand(B, L, L)
            if keep is not None:
                on = on & keep[:, None, :]
            rows = on.any(-1)                                                       # [B, L]: rows with a needle key
            if not bool(rows.any()):
                continue
            mass = (p[:, h] * on).sum(-1)
            assert float(mass[rows].min()) >= 0.9, (c, h, float(mass[rows].min()))
            single = on.sum(-1) == 1
            if bool(single.any()):                                                  # one needle key: its one-hot column carries the weight
                col = on.float().argmax(-1) % 8                                     # [B, L]
                w = hot[:, :, h].gather(-1, col[..., None])[..., 0]
                assert float(w[single].min()) >= 0.9, (c, h)
            needle_rows += int(rows.sum())
    assert needle_rows > 1000


def test_cost_of_the_number_formats_over_the_grid():
    """Prints, per dtype, the worst max|reference_rounded_p - reference| over the grid (random columns relative to max|reference| of the (batch,
    head) slice / structured columns absolute) and the same for the fp32-arithmetic statement, and holds the GPU test's bars to them.
    Measured: bf16 4.5e-3 / 3.1e-3 (both statements: the bf16 rounding of P and of the output is all there is); fp32 rounded P 7.2e-8 / 5.0e-8,
    fp32 arithmetic 1.2e-6 / 2.3e-6.  The bars are 3 x these: bf16 1.35e-2 / 9.3e-3, below test_gpu_attention.py's 1.5e-2 / 1e-2 and lowered to
    it.  For fp32, 3 x the cost of rounding P (2e-7) is less than one fp32 rounding of a 64-term dot product of O(10) scores leaves, so fp32's cost
    is taken from the fp32-arithmetic statement: 3.7e-6 / 6.8e-6 instead of 3e-5."""
    worst = {d: {"rounded_p": [0.0, 0.0], "f32_arithmetic": [0.0, 0.0]} for d in T.DT}
    for i, c in enumerate(GRID):
        q, k, v, rb, bk, keep, ref = tensors_and_reference(i)
        for name, fn in (("rounded_p", T.reference_rounded_p), ("f32_arithmetic", T.reference_f32_arithmetic)):
            e = T.slice_errors(fn(q, k, v, rb, bk, keep), ref)
            w = worst[c["dname"]][name]
            w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])
    for d, w in worst.items():
        print(f"[t5 attention format cost {d}] " + "; ".join(f"{n}: random {e[0]:.2e} structured {e[1]:.2e}" for n, e in w.items()))
    cost = {"bf16": worst["bf16"]["rounded_p"], "f32": [max(a, b) for a, b in zip(worst["f32"]["rounded_p"], worst["f32"]["f32_arithmetic"])]}
    for d in T.DT:
        for bar, c3, issue in ((T.BAR_REL[d], 3 * cost[d][0], T.ISSUE_BAR_REL[d]), (T.BAR_ABS[d], 3 * cost[d][1], T.ISSUE_BAR_ABS[d])):
            assert bar <= issue and 0.98 * c3 <= bar <= 1.02 * c3, (d, bar, c3)          # the bar is 3 x the measured cost, to its two digits


def _bars_hold(d, out, ref):
    e_rel, e_abs = T.slice_errors(out, ref)
    return e_rel <= T.BAR_REL[d] and e_abs <= T.BAR_ABS[d]


def _shifted(bk_of_rel, L, by):
    rel = (torch.arange(L)[None, :] - torch.arange(L)[:, None] + by).clamp(-T.REL_SPAN, T.REL_SPAN)
    return bk_of_rel[rel + T.REL_SPAN]


MUTATIONS = ("bias_i_minus_j", "bias_one_off", "last_ragged_key_dropped", "mask_ignored", "scale_one_eighth")


def _mutated(name, c, q, k, v, rb, bk, keep):
    """-> the mutated reference, or None where the mutation does not exist on this case."""
    B, L = c["B"], c["L"]
    if name == "bias_i_minus_j":
        return T.reference(q, k, v, rb, bk.t(), keep) if L > 1 else None
    if name == "bias_one_off":
        tab = torch.from_numpy(T.bucket_table(c["num_buckets"], c["max_distance"])).long()
        return T.reference(q, k, v, rb, _shifted(tab, L, 1), keep) if L > 1 else None
    if name == "last_ragged_key_dropped":
        if L % T.KT == 0 or L == 1 or (keep is not None and (not bool(keep[:, L - 1].any()) or int(keep.sum(-1).min()) < 2)):
            return None
        drop = torch.ones(B, L, dtype=torch.bool) if keep is None else keep.clone()
        drop[:, L - 1] = False
        return T.reference(q, k, v, rb, bk, drop)
    if name == "mask_ignored":
        return None if keep is None else T.reference(q, k, v, rb, bk, None)
    return T.reference(q.double() / 8, k, v, rb, bk, keep) if L > 1 else None      # scale_one_eighth


def _must_catch(name, c, rb, bk, keep):
    """Whether the case is built against the mutation, from its construction alone.  A softmax over a single valid key (`one_key`, or
    `first_tile` at L = 65) shows neither bias nor scale.  The bias mutations belong to the bias regimes, where the bias they read differs from the true one on a pair of valid keys
    (a needle on rel = 0 is its own transpose; a needle this length does not reach leaves the bias zero).  A dropped last key shows where that
    key has weight: not under `descending`, nor under a needle elsewhere.  An ignored mask shows where masked keys would have weight: the two
    regimes of flat scores."""
    if keep is not None and int(keep.sum(-1).max()) == 1:
        return name == "mask_ignored"
    if name in ("bias_i_minus_j", "bias_one_off"):
        if c["regime"] not in T.BIAS_REGIMES:
            return False
        tab = torch.from_numpy(T.bucket_table(c["num_buckets"], c["max_distance"])).long()
        other = bk.t() if name == "bias_i_minus_j" else _shifted(tab, c["L"], 1)
        valid = torch.ones(c["B"], c["L"], dtype=torch.bool) if keep is None else keep
        differs = (rb[bk] != rb[other]).any(-1)[None] & valid[:, None, :]            # [B, L, L]
        return bool(differs.any())
    if name == "last_ragged_key_dropped":
        return c["regime"] in ("uniform", "ascending", "bias_random")
    if name == "mask_ignored":
        return c["regime"] in ("uniform", "bias_random")
    return True


@pytest.mark.parametrize("name", MUTATIONS)
def test_a_wrong_kernel_leaves_the_bars(name):
    """Each mutation of the reference is a kernel bug the grid must catch: its result is held to the GPU test's own bars against the true
    reference, and must leave them on every case built against it (_must_catch), in both dtypes."""
    caught = {d: 0 for d in T.DT}
    for i, c in enumerate(GRID):
        q, k, v, rb, bk, keep, ref = tensors_and_reference(i)
        mut = _mutated(name, c, q, k, v, rb, bk, keep)
        if mut is None:
            continue
        ok = _bars_hold(c["dname"], mut, ref)
        caught[c["dname"]] += not ok
        if _must_catch(name, c, rb, bk, keep):
            assert not ok, (name, c, T.slice_errors(mut, ref))
    print(f"[t5 attention mutation {name}] cases that leave the bars: {caught}")
    assert all(n >= 10 for n in caught.values()), caught
