"""Host side of the block-wise 8-bit AdamW state (vlatouch/adam8.py, the `optimizer` argument of RdtTrainer) against the numpy statement
(tests/adam8_ref.py): the known answers of DESIGN.md §8, the product's tables bit for bit, the code rule on every table value, the round-trip
bound, the moment store's checkpoint round trip and refusals on the CPU, and a CPU toy that holds the statement's
8-bit step against fp32 AdamW on an ill-scaled least-squares problem."""
import os

import numpy as np
import pytest
import torch

from tests import adam8_ref as A
from tests import cases  # noqa: F401  (puts the package on sys.path)

F = np.float32


@pytest.fixture(autouse=True)
def _the_products_tables_are_the_statements():
    """Every test here speaks about the product through the statement: they are only worth running where the product's tables are these."""
    from vlatouch import adam8
    ts, tu = adam8.code_tables()
    assert np.array_equal(ts.view(np.int32), A.TS.view(np.int32)) and np.array_equal(tu.view(np.int32), A.TU.view(np.int32))


def test_known_answers_of_the_statement():
    ts, tu = A.TS, A.TU
    assert ts.dtype == tu.dtype == F and ts.shape == tu.shape == (256,)
    assert len(np.unique(ts)) == 256 and len(np.unique(tu)) == 256
    assert bool(np.all(np.diff(ts) > 0)) and bool(np.all(np.diff(tu) > 0))
    assert int(np.where(ts == 0)[0][0]) == 127 and int(np.where(tu == 0)[0][0]) == 0
    assert ts[128] == F(5.5e-7) and tu[1] == F(3.25e-7)
    assert list(ts[:3]) == [F(-0.99296874), F(-0.9789063), F(-0.96484375)]
    assert list(ts[-3:]) == [F(0.9789063), F(0.99296874), F(1.0)]
    assert list(tu[:3]) == [F(0.0), F(3.25e-7), F(7.75e-7)]
    assert list(tu[-3:]) == [F(0.98945314), F(0.9964844), F(1.0)]
    assert -1.0 not in ts                                        # 127 negatives, 127 positives, 0 and 1
    assert A.BS.shape == A.BU.shape == (255,)


def test_product_tables_equal_the_statement_bit_for_bit():
    from vlatouch import adam8
    ts, tu = adam8.code_tables()
    for got, want in ((ts, A.TS), (tu, A.TU), (adam8.boundaries(ts), A.BS), (adam8.boundaries(tu), A.BU)):
        assert got.dtype == F and np.array_equal(got.view(np.int32), want.view(np.int32))
    buf = adam8.tables_buffer()
    assert buf.dtype == F and buf.shape == (1024,)
    want = np.concatenate([A.TS, A.TU, A.BS, [np.inf], A.BU, [np.inf]]).astype(F)
    assert np.array_equal(buf.view(np.int32), want.view(np.int32))
    assert (adam8.BLOCK, adam8.MIN_8BIT_SIZE, adam8.ZERO_CODE_SIGNED, adam8.ZERO_CODE_UNSIGNED) == (A.BLOCK, A.MIN_8BIT_SIZE, 127, 0)
    sizes = [1, 255, 4095, 4096, 4097, 70001]
    assert adam8.state_bytes(sizes) == sum(8 * n if n < 4096 else 2 * n + 8 * ((n + 255) // 256) for n in sizes)


@pytest.mark.parametrize("signed", [True, False])
def test_every_table_value_is_its_own_code_and_ties_go_down(signed):
    t, b = (A.TS, A.BS) if signed else (A.TU, A.BU)
    assert np.array_equal(A.code(t, b), np.arange(256, dtype=np.uint8))
    assert np.array_equal(A.code(b, b), np.arange(255, dtype=np.uint8)), "a value on a boundary takes the lower index"
    assert np.array_equal(A.code(np.nextafter(b, F(np.inf)), b), np.arange(1, 256).astype(np.uint8))


@pytest.mark.parametrize("signed", [True, False])
def test_round_trip_error_is_at_most_half_the_local_gap(signed):
    rng = np.random.default_rng(3)
    n = 70001
    x = (rng.standard_normal(n) * np.exp(2.0 * rng.standard_normal(n))).astype(F)
    if not signed:
        x = x * x
    x[5 * 256:6 * 256] = 0                                       # an all-zero block
    codes, absmax, _ = A.quantize(x, signed)
    assert absmax.shape == ((n + 255) // 256,) and absmax[5] == 0
    assert bool(np.all(codes[5 * 256:6 * 256] == (127 if signed else 0)))
    back = A.dequantize(codes, absmax, signed, np.float64)
    t = (A.TS if signed else A.TU).astype(np.float64)
    gap = np.diff(t)
    lo = np.concatenate([gap[:1], gap])[codes]                   # distance to the neighbours of the chosen value
    hi = np.concatenate([gap, gap[-1:]])[codes]
    scale = np.repeat(absmax.astype(np.float64), 256)[:n]
    r = x.astype(np.float64) / np.where(scale == 0, 1, scale)
    # the signed table has no -1: below its first entry the error is the distance to that entry, not half a gap
    inside = r >= t[0]
    err = np.abs(back - x.astype(np.float64))
    bound = 0.5 * np.maximum(lo, hi) * scale * (1 + 2.0 ** -22)
    assert bool(np.all(err[inside] <= bound[inside])), float((err - bound)[inside].max())
    assert bool(np.all(err[~inside] <= (1.0 + t[0]) * scale[~inside] * (1 + 2.0 ** -22)))


def test_unknown_optimizer_raises():
    from vlatouch.rdt_train import OPTIMIZERS, RdtTrainer
    assert OPTIMIZERS == ("adamw", "adamw8bit")
    with pytest.raises(ValueError, match="optimizer"):
        RdtTrainer({}, heads=2, horizon=4, action_dim=8, optimizer="adam8", device="cpu")


STORE_SHAPES = {"small": (255,), "edge.weight": (64, 64), "big.weight": (3, 1400), "scalar": ()}      # 255 | 4096 | 4200 (17 blocks, the last partial) | 1


def _store_tensors(st):
    return {f"{part}.{k}": t.clone() for part in ("m", "v", "am", "av") for k, t in getattr(st, part).items()}


def _equal_tensors(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def test_store_zero_state_round_trips_through_a_checkpoint_on_the_cpu(tmp_path):
    """Moments8 without a GPU: the zero state (codes 127 / 0, zero scales; fp32 zeros below MIN_8BIT_SIZE), saved before and after it is held,
    loads into a second store with equal tensors; byte counts are the count from the shapes either way."""
    from safetensors.torch import load_file
    from vlatouch import adam8
    a = adam8.Moments8(STORE_SHAPES, "cpu")
    want_bytes = 8 * 255 + 8 * 1 + (2 * 4096 + 8 * 16) + (2 * 4200 + 8 * 17)    # fp32 m, v | two codes per element + two scales per block
    assert not a.m and a.nbytes() == want_bytes == adam8.state_bytes([255, 4096, 4200, 1])
    os.makedirs(tmp_path / "early" / "checkpoint")
    a.save(str(tmp_path / "early"))                              # before the first step: the file holds the zero state
    a.zero()
    assert a.m and a.nbytes() == want_bytes and a.state_json == {"optimizer": "adamw8bit", "block": 256}
    assert set(a.am) == set(a.av) == {"edge.weight", "big.weight"} and set(a.m) == set(a.v) == set(STORE_SHAPES)
    assert a.m["small"].dtype == torch.float32 and not a.m["small"].any() and a.m["scalar"].shape == (1,)
    assert bool((a.m["big.weight"] == 127).all()) and bool((a.v["big.weight"] == 0).all()) and a.m["big.weight"].dtype == a.v["big.weight"].dtype == torch.uint8
    assert a.am["big.weight"].shape == (17,) and not a.am["big.weight"].any() and not a.av["edge.weight"].any()
    os.makedirs(tmp_path / "held" / "checkpoint")
    a.save(str(tmp_path / "held"))
    early, held = (load_file(str(tmp_path / d / "checkpoint" / "adam8.safetensors")) for d in ("early", "held"))
    assert _equal_tensors(early, held)
    assert np.array_equal(held["table_signed"].numpy().view(np.int32), A.TS.view(np.int32))
    assert np.array_equal(held["table_unsigned"].numpy().view(np.int32), A.TU.view(np.int32))
    a.am["big.weight"][3], a.m["big.weight"][700], a.v["small"][9] = 0.25, 200, 1.5          # a state that is not the zero one
    a.save(str(tmp_path / "held"))
    b = adam8.Moments8(STORE_SHAPES, "cpu")
    b.load(str(tmp_path / "held"), a.state_json)
    assert _equal_tensors(_store_tensors(a), _store_tensors(b))
    m, v = b.moments("small")
    assert torch.equal(v, a.v["small"]) and v.data_ptr() != b.v["small"].data_ptr()


@pytest.mark.parametrize("what", ["missing key", "element count", "dtype", "code table bit", "block"])
def test_store_refuses_a_mismatched_checkpoint_and_stays_as_it_was(what, tmp_path):
    from safetensors.torch import load_file, save_file
    from vlatouch import adam8
    a = adam8.Moments8(STORE_SHAPES, "cpu")
    a.zero()
    os.makedirs(tmp_path / "checkpoint")
    a.save(str(tmp_path))
    f = str(tmp_path / "checkpoint" / "adam8.safetensors")
    st, js = load_file(f), a.state_json
    if what == "missing key":
        del st["av.big.weight"]
    elif what == "element count":
        st["am.big.weight"] = torch.zeros(16)
    elif what == "dtype":
        st["m8.edge.weight"] = st["m8.edge.weight"].to(torch.int8)
    elif what == "code table bit":
        st["table_unsigned"] = (st["table_unsigned"].view(torch.int32) ^ torch.tensor([0] * 200 + [1] + [0] * 55, dtype=torch.int32)).view(torch.float32)
    else:
        js = dict(js, block=128)
    save_file(st, f)
    b = adam8.Moments8(STORE_SHAPES, "cpu")
    b.zero()
    b.m["big.weight"][5], b.av["edge.weight"][2], b.m["small"][1] = 3, 0.5, -2.0               # recognisably its own state
    before, held = _store_tensors(b), {part: dict(getattr(b, part)) for part in ("m", "v", "am", "av")}
    with pytest.raises(ValueError):
        b.load(str(tmp_path), js)
    assert _equal_tensors(before, _store_tensors(b))
    assert all(getattr(b, part)[k] is t for part, d in held.items() for k, t in d.items()), "the store holds other tensors than before"
    fresh = adam8.Moments8(STORE_SHAPES, "cpu")
    with pytest.raises(ValueError):
        fresh.load(str(tmp_path), js)
    assert not (fresh.m or fresh.v or fresh.am or fresh.av)


def _toy(seed):
    """256 x 8192 least squares with log-normal column scales -> (A, y).  sigma = 0.5: the second moment goes with the square of a column's
    scale, so 8192 draws (out to 3.7 sigma either way) spread it over e^(4 x 3.7 x 0.5) = 1.6e3 inside a block, well inside the unsigned
    table's range of 1 : 3.25e-7.  At sigma = 1 the spread reaches 2.7e6, elements fall on code 0 (an exactly zero second moment, their
    history lost) and the 8-bit run can overshoot where such an element's gradient passes through zero (seen on one seed of five, 1.2 x the
    first loss at step 20): the statement has no guard against it, and the toy is not about that regime."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((256, 8192)) * np.exp(0.5 * rng.standard_normal(8192))).astype(F)
    w = rng.standard_normal(8192).astype(F)
    return a, (a @ w).astype(F)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_cpu_toy_8bit_follows_fp32_adamw(seed):
    """lr 1e-2, both runs from w = 0 on the same problem.  At the step where the fp32 loss first passes 0.05 of its first value, the loss of
    the statement's 8-bit step is at most 1.5 x it (this toy, seeds 0 - 4: 1.02 - 1.05 x)."""
    a, y = _toy(seed)
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 1e-2

    def loss_grad(w):
        r = a @ w - y
        return float(np.mean(r.astype(np.float64) ** 2)), ((2.0 / r.size) * (a.T @ r)).astype(F)

    w32, w8 = np.zeros(8192, F), np.zeros(8192, F)
    s32, s8 = {"m": np.zeros(8192, F), "v": np.zeros(8192, F)}, A.zero_state(8192)
    assert "m8" in s8
    first = None
    for step in range(1, 3001):
        hy = A.hyper(lr, b1, b2, step, 0.0)
        l32, g32 = loss_grad(w32)
        l8, g8 = loss_grad(w8)
        first = l32 if first is None else first
        if l32 <= 0.05 * first:
            break
        w32, _, s32, _ = A.step8(w32, g32, s32, None, hy, b1, b2, eps, wd)
        w8, _, s8, _ = A.step8(w8, g8, s8, None, hy, b1, b2, eps, wd)
    else:
        pytest.fail(f"fp32 AdamW did not reach 0.05 of its first loss in 3000 steps ({l32 / first:.3f})")
    print(f"[adam8 toy seed {seed}] step {step}: fp32 loss {l32 / first:.4f} of the first, 8-bit {l8 / first:.4f} ({l8 / l32:.3f} x)")
    assert l8 <= 1.5 * l32, (step, l8, l32)
