"""The fp64 statement of vt_attention (tests/attn_ref.py) against torch's scaled_dot_product_attention in fp64, the structure of the inputs the
GPU test relies on, what rounding P to the storage type costs per regime and dtype (printed: the only source a widened bar may have), and the
coverage of the GPU grid against the launcher's routing as attn_ref.route restates it."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import attn_ref as A

torch.set_grad_enabled(False)


def _sdpa64(q, k, v, mask, scale):
    am = None if mask is None else mask[:, None, None, :]
    o = F.scaled_dot_product_attention(q.double().transpose(1, 2), k.double().transpose(1, 2), v.double().transpose(1, 2), attn_mask=am, scale=scale)
    return o.transpose(1, 2)


@pytest.mark.parametrize("dname", list(A.DT))
@pytest.mark.parametrize("mask,B,Nq,Nk,hd", [("none", 1, 17, 65, 64), ("none", 3, 5, 7, 96), ("trail", 3, 17, 130, 64), ("holes", 3, 16, 193, 96),
                                             ("first_tile", 1, 9, 130, 64), ("middle_tile", 3, 9, 193, 64), ("one_key", 3, 4, 65, 96),
                                             ("sample", 3, 9, 70, 64), ("lead", 1, 3, 2, 64)])
def test_reference_is_torch_sdpa_in_float64(dname, mask, B, Nq, Nk, hd):
    H = 2
    for regime in A.REGIMES:
        q, k, v = A.make_inputs(dname, B, H, Nq, Nk, hd, regime, seed=Nk + Nq)
        keep = A.make_mask(mask, B, Nk)
        ref = A.reference(q, k, v, keep, A.scale_of(hd))
        want = _sdpa64(q, k, v, keep, A.scale_of(hd))
        empty = torch.zeros(B, dtype=torch.bool) if keep is None else ~keep.any(-1)
        assert bool(torch.isfinite(ref).all())
        if bool(empty.any()):                                        # no softmax there: NaN in torch before 2.5, zeros since; the statement has zeros
            assert mask == "sample" and bool((torch.isnan(want[empty]) | (want[empty] == 0)).all())
            assert float(ref[empty].abs().max()) == 0.0
        assert not bool(torch.isnan(want[~empty]).any())
        assert float((ref[~empty] - want[~empty]).abs().max()) <= 1e-12, (regime, float((ref[~empty] - want[~empty]).abs().max()))


@pytest.mark.parametrize("B,H,Nq,Nk,hd", [(1, 1, 1, 257, 64), (3, 3, 17, 65, 96), (1, 3, 64, 130, 80), (3, 1, 8, 577, 64), (3, 1, 15, 1, 64), (1, 3, 16, 7, 96)])
def test_structure_of_the_inputs(B, H, Nq, Nk, hd):
    scale, real = A.scale_of(hd), A.REAL[hd]
    for dname, regime, mask in itertools.product(A.DT, A.REGIMES, ("none", "holes", "sample", "first_tile")):
        if not A.mask_ok(mask, B, Nk):
            continue
        q, k, v = A.make_inputs(dname, B, H, Nq, Nk, hd, regime, seed=3)
        assert all(float(t[..., real:].abs().max() if real < hd else 0.0) == 0.0 for t in (q, k, v))
        keep = A.make_mask(mask, B, Nk)
        ref = A.reference(q, k, v, keep, scale)
        s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
        assert float(s.abs().max()) <= 12.0, (dname, regime, float(s.abs().max()))
        valid = torch.ones(B, dtype=torch.bool) if keep is None else keep.any(-1)
        assert float((ref[valid][..., A.C_ONE] - 1.0).abs().max()) <= 1e-12            # the ones column, to fp64 rounding
        assert float((ref[valid][..., A.C_TILE:A.C_TILE + 4].sum(-1) - 1.0).abs().max()) <= 1e-12
        assert float(ref[~valid].abs().max() if bool((~valid).any()) else 0.0) == 0.0
        assert float(ref[..., real:].abs().max() if real < hd else 0.0) == 0.0
        if regime == "needle" and mask == "none":                    # more than 0.9 of a row's mass on its needle
            p = torch.softmax(s, -1)                                 # [B, H, Nq, Nk]
            at = torch.tensor(A.needle_keys(Nk))[A.needle_of_row(B, H, Nq)].permute(0, 2, 1)
            assert float(p.gather(-1, at[..., None]).min()) > 0.9
            if Nk > 1:
                top2 = s.topk(2, dim=-1).values
                assert float((top2[..., 0] - top2[..., 1]).min()) >= 6.0
        if regime in ("ascending", "descending") and mask == "none" and Nk > A.KT:   # the tile maxima move as the regime says
            tiles = [s[..., t:t + A.KT].amax(-1) for t in range(0, Nk, A.KT)]
            d = torch.stack(tiles, -1).diff(dim=-1)
            assert bool((d > 0).all()) if regime == "ascending" else bool((d < 0).all())


def test_masks():
    for kind, B, Nk in itertools.product(A.MASKS[1:], (1, 3), (1, 7, 65, 130, 577)):
        if not A.mask_ok(kind, B, Nk):
            continue
        keep = A.make_mask(kind, B, Nk)
        assert keep.shape == (B, Nk) and keep.dtype == torch.bool and not bool(keep.all())
        alive = keep.any(-1)
        if kind == "sample":
            assert alive.tolist() == [True, False, True] and bool(keep[0].all()) and bool(keep[2].all())
        else:
            assert bool(alive.all())
        if kind == "one_key":
            assert keep.sum(-1).tolist() == [1] * B and not bool(keep[:, 0].any())
        if kind == "first_tile":
            assert not bool(keep[:, :64].any()) and bool(keep[:, 64:].all())
        if kind == "middle_tile":
            t = (Nk + 63) // 64 // 2
            assert 0 < t < (Nk + 63) // 64 - 1 and not bool(keep[:, t * 64:(t + 1) * 64].any()) and int((~keep).sum()) == 64 * B


def test_cost_of_rounding_p_per_regime_and_dtype():
    """Prints max|reference_rounded_p - reference| / max|reference| over the random columns of a (batch, head) and the absolute distance over the
    structured columns, at the largest grid shape by keys (10 tiles) and at 257 keys; and holds them under the bars of the GPU test with the factor
    of 2 that the order of summation and the hardware exp2 are given: where this fails, the bar is tighter than the number format."""
    bar_rel = {"f32": 3e-5, "bf16": 1.5e-2, "f16": 2e-3}
    bar_abs = {"f32": 3e-5, "bf16": 1e-2, "f16": 2e-3}
    for (B, H, Nq, Nk, hd), dname, regime in itertools.product(((1, 3, 96, 577, 64), (3, 3, 257, 257, 96)), A.DT, A.REGIMES):
        q, k, v = A.make_inputs(dname, B, H, Nq, Nk, hd, regime, seed=11)
        ref = A.reference(q, k, v, None, A.scale_of(hd))
        line = []
        for sum_rounded in (True, False):
            rp = A.reference_rounded_p(q, k, v, None, A.scale_of(hd), sum_rounded=sum_rounded)
            c0, c1 = A.C_RAND, A.REAL[hd]
            rel = float(((rp - ref)[..., c0:c1].abs().amax((1, 3)) / ref[..., c0:c1].abs().amax((1, 3))).max())
            ab = float((rp - ref)[..., :c0].abs().max())
            line.append(f"rel {rel:.2e} abs {ab:.2e}")
            assert 2 * rel <= bar_rel[dname] and 2 * ab <= bar_abs[dname], (dname, regime, Nk, rel, ab)
        print(f"[rounded P {dname} {regime} Nk{Nk} hd{hd}] row sum of the rounded P: {line[0]}; of the unrounded: {line[1]}")


def test_the_grid_reaches_every_branch():
    grid = A.gpu_grid()
    assert len({tuple(sorted(c.items())) for c in grid}) == len(grid)
    for c in grid:
        assert c["B"] in (1, 3) and c["H"] in (1, 3) and (c["B"], c["H"], c["Nq"], c["Nk"]) in A.SHAPES
        assert A.mask_ok(c["mask"], c["B"], c["Nk"])
        assert c["hd"] != 80 or (c["dname"] != "f32" and c["mask"] == "none" and c["o"] != "stride2")
    assert {s[2] for s in A.SHAPES} >= {1, 15, 16, 17, 64, 67, 80, 96, 100, 128, 129, 257}
    assert {s[3] for s in A.SHAPES} == {1, 7, 63, 64, 65, 128, 130, 192, 193, 257, 577}
    for dname in A.DT:
        mine = [c for c in grid if c["dname"] == dname]
        assert {(c["mask"], c["regime"]) for c in mine} == set(itertools.product(A.MASKS, A.REGIMES))
        assert {c["qkv"] for c in mine} == set(A.QKV_LAYOUTS) and {c["o"] for c in mine} == set(A.O_LAYOUTS)
        assert any(c["km_pad"] for c in mine) and any(c["mask"] != "none" and not c["km_pad"] for c in mine)
        assert {c["Nk"] for c in mine if c["Nq"] == 1 and c["o"] == "compact"} == {257, 577}
        for hd in (64, 96):                                          # masks over several tiles and wholly masked tiles at both head dimensions
            assert {c["mask"] for c in mine if c["hd"] == hd and c["mask"] != "none"} >= {"first_tile", "middle_tile", "sample", "one_key"}
        assert any(c["o"] == "stride2" and A.route(dname, c["hd"], False, c["Nq"], c["Nk"], A.o_row_stride("stride2", c["H"], c["hd"]))[0] == "attn"
                   for c in mine if c["mask"] == "none")
    for dname in ("bf16", "f16"):
        seen = set()
        for c in grid:
            if c["dname"] != dname or c["mask"] != "none":
                continue
            for knob in A.knobs_of(dname, c["hd"], c["mask"], c["Nq"], c["o"]):
                kern, G, nw = A.route(dname, c["hd"], False, c["Nq"], c["Nk"], A.o_row_stride(c["o"], c["H"], c["hd"]), knob)
                seen.add((kern, G, c["hd"], nw, A.tile_class(c["Nk"])))
        unmasked = {(hd, nw, t) for kern, G, hd, nw, t in seen if kern != "attn"}
        # 8 waves below 512 keys exist only as 3 query groups per wave (64- and 80-wide heads); 96-wide heads reach 8 waves at 4 or more tiles only
        want = set(itertools.product((64, 80, 96), (4, 5, 6, 7), (1, 2, 3, 4))) | {(hd, 8, 4) for hd in (64, 80, 96)}
        want |= {(hd, 8, t) for hd in (64, 80) for t in (1, 2, 3)}
        assert unmasked >= want, sorted(want - unmasked)
        for hd in (64, 80):
            assert {(G, nw) for kern, G, h, nw, t in seen if kern == "attn16g" and h == hd} >= {(3, 4), (3, 6), (3, 8), (6, 4)}
        assert {t for kern, G, h, nw, t in seen if kern == "attn16g"} == {1, 2, 3, 4}


def test_route_restates_the_launcher_on_known_points():
    """The points DESIGN.md and the launcher's comments name."""
    assert A.block_waves(67, 4374) == 5 and A.block_waves(64, 64) == 4 and A.block_waves(96, 1) == 6 and A.block_waves(100, 1) == 7
    assert A.block_waves(128, 511) == 4 and A.block_waves(128, 512) == 8 and A.block_waves(729, 729) == 8 and A.block_waves(257, 257) == 6
    assert A.route("bf16", 64, False, 257, 257, 768) == ("attn16g", 6, 4)            # DINOv2 @224: one block of 4 waves x 6 groups
    assert A.route("bf16", 80, False, 729, 729, 1280) == ("attn16u", 1, 8)           # SigLIP stays on attn16u_kernel
    assert A.route("bf16", 80, False, 729, 729, 1280, knob=3) == ("attn16g", 3, 8)
    assert A.route("f16", 64, False, 257, 257, 768, knob=0) == ("attn16u", 1, 6)
    assert A.route("bf16", 64, True, 257, 257, 768)[0] == "attn" and A.route("f32", 64, False, 257, 257, 768)[0] == "attn"
    assert A.route("bf16", 64, False, 257, 257, 770)[0] == "attn"
