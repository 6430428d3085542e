"""vt_tactile_head (csrc/vt_tactile_head.hip) against the float64 statement of tests/clip_ref.py: video feature, cosine similarities, top-k.

Grid: b in {1, 3}, l in {1, 5, 10}, D in {64, 1024}, (R, k) in clip_ref.HEAD_RK (R in {1, 7, 300}, k in {1, 3, 16}, k <= R).
Bar: 3 x the cost of the statement in fp32 arithmetic on the CPU over this grid (clip_ref.COSTS["head", "fp32"] = 2.0e-7, measured and held by
tests/test_clip_ref_host.py) = 6.0e-7; `video` by row_err, `sims` absolutely (a cosine is at most 1).
Top-k: the indices equal torch.topk's on the float64 similarities.  clip_ref.head_data draws every bank so that a video's k + 1 largest
similarities lie at least HEAD_GAP = 1e-4 apart, which is more than 100 x the measured fp32 error; the test asserts that gap on the reference
before it looks at the device's answer, so no case can hide behind a tie.  One constructed exact tie checks that the lower index wins, a zero
bank row gives similarity 0 (not NaN), and a video's results do not depend on how many videos the call carries."""
import numpy as np
import pytest
import torch

from tests import clip_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BAR = R.BARS[("head", "fp32")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def run(dev, pooled, bank, k):
    from vlatouch.clip import TactileHeads
    h = TactileHeads(dev)
    h.set_bank(torch.as_tensor(bank))
    video, sims, idx, val = h.retrieve(torch.as_tensor(pooled), k)
    torch.cuda.synchronize(dev)
    return video.cpu(), sims.cpu(), idx.cpu(), val.cpu()


@pytest.mark.parametrize("D", R.HEAD_D)
@pytest.mark.parametrize("l", R.HEAD_L)
def test_video_sims_topk(dev, l, D):
    worst_v = worst_s = 0.0
    for b in R.HEAD_B:
        for Rn, k in R.HEAD_RK:
            pooled, bank = R.head_data(b, l, D, Rn, k)
            v64 = R.video_feature(pooled)
            s64 = R.cosine(bank, v64)
            top = torch.topk(s64, k, dim=-1)
            srt = s64.sort(dim=-1, descending=True).values[:, : k + 1]
            if srt.shape[1] > 1:
                assert float((srt[:, :-1] - srt[:, 1:]).min()) > 100 * R.COSTS[("head", "fp32")], (b, l, D, Rn, k)      # the gap, on the reference, first
            video, sims, idx, val = run(dev, pooled, bank, k)
            e_v, e_s = R.row_err(video, v64), float((sims.double() - s64).abs().max())
            worst_v, worst_s = max(worst_v, e_v), max(worst_s, e_s)
            what = (b, l, D, Rn, k)
            assert e_v <= BAR and e_s <= BAR, (what, e_v, e_s, BAR)
            assert torch.equal(idx.long(), top.indices), (what, idx, top.indices)
            assert torch.equal(val, sims.gather(1, idx.long())), what                     # the values are the similarities at those indices
    print(f"tactile head l {l} D {D}: video {worst_v:.3e}, sims {worst_s:.3e} (bar {BAR:.3e})")


def test_tie_goes_to_the_lower_index_and_zero_row_is_zero(dev):
    g = np.random.Generator(np.random.PCG64(5))
    D = 64
    pooled = (g.standard_normal((2, 5, D)) + 0.5).astype(np.float32)
    bank = g.standard_normal((9, D)).astype(np.float32)
    bank[6] = bank[2]                                                # an exact tie: the same bits give the same similarity
    bank[4] = 0.0
    bank[2] *= 4.0                                                   # a power of two: the cosine of rows 2 and 6 stays bit-equal
    bank[6] *= 0.5
    video, sims, idx, val = run(dev, pooled, bank, 9)
    assert bool(torch.isfinite(sims).all()) and float(sims[:, 4].abs().max()) == 0.0
    assert torch.equal(sims[:, 2], sims[:, 6])
    for j in range(2):
        order = idx[j].tolist()
        assert sorted(order) == list(range(9))
        assert order.index(2) + 1 == order.index(6), order           # equal values: neighbours, the lower index first
        assert all(val[j, i] >= val[j, i + 1] for i in range(8))


def test_results_do_not_depend_on_the_number_of_videos(dev):
    pooled, bank = R.head_data(3, 10, 1024, 300, 16)
    v3, s3, i3, t3 = run(dev, pooled, bank, 16)
    v1, s1, i1, t1 = run(dev, pooled[1:2], bank, 16)
    assert torch.equal(v3[1:2], v1) and torch.equal(s3[1:2], s1) and torch.equal(i3[1:2], i1) and torch.equal(t3[1:2], t1)


def test_video_only_and_refusals(dev):
    from vlatouch import _lib as L
    from vlatouch.clip import TactileHeads
    pooled, bank = R.head_data(3, 5, 64, 7, 3)
    h = TactileHeads(dev)
    v = h.video(torch.from_numpy(pooled))
    assert R.row_err(v.cpu(), R.video_feature(pooled)) <= BAR
    lib, st = L.lib(), L.stream_ptr(dev)
    p, bk = torch.from_numpy(pooled).to(dev), torch.from_numpy(bank).to(dev)
    bn, vid, sims = torch.zeros(7, device=dev), torch.zeros(3, 64, device=dev), torch.zeros(3, 7, device=dev)
    idx, val = torch.zeros(3, 16, dtype=torch.int32, device=dev), torch.zeros(3, 16, device=dev)
    good = [L.ptr(p), 3, 5, 64, L.ptr(bk), L.ptr(bn), 7, 3, L.ptr(vid), L.ptr(sims), L.ptr(idx), L.ptr(val)]
    assert lib.vt_tactile_bank_norms(L.ptr(bk), 7, 64, L.ptr(bn), st) == 0 and lib.vt_tactile_head(*good, st) == 0
    for pos, bad in ((0, None), (8, None), (5, None), (9, None), (10, None), (11, None), (7, 8), (7, 17), (7, -1), (6, 0), (3, 66), (1, 0), (2, 0)):
        a = list(good)
        a[pos] = bad
        assert lib.vt_tactile_head(*a, st) == -22, (pos, bad)
    a = list(good)
    a[6], a[7] = 300, 17                                             # k > 16 with R large enough
    assert lib.vt_tactile_head(*a, st) == -22
    assert lib.vt_tactile_bank_norms(None, 7, 64, L.ptr(bn), st) == -22 and lib.vt_tactile_bank_norms(L.ptr(bk), 7, 66, L.ptr(bn), st) == -22
    with pytest.raises(ValueError):
        h.retrieve(torch.from_numpy(pooled), k=1)                    # no bank
    h.set_bank(torch.from_numpy(bank))
    for k in (8, 17, -1):
        with pytest.raises(ValueError):
            h.retrieve(torch.from_numpy(pooled), k=k)
    v2 = h.video(torch.from_numpy(pooled))                           # one return shape, bank or no bank
    assert isinstance(v2, torch.Tensor) and torch.equal(v2, v)
    off = torch.zeros(7 * 64 + 1, device=dev)[1:].view(7, 64)        # 4 bytes past an allocation's base: float4 loads would be misaligned
    assert off.data_ptr() % 16 == 4
    a = list(good)
    a[4] = L.ptr(off)
    assert lib.vt_tactile_head(*a, st) == -22 and lib.vt_tactile_bank_norms(L.ptr(off), 7, 64, L.ptr(bn), st) == -22
    torch.cuda.synchronize(dev)


def test_bank_is_uploaded_once_per_tensor(dev):
    from vlatouch.clip import TactileHeads
    pooled, bank = R.head_data(1, 5, 64, 7, 3)
    t = torch.from_numpy(bank)
    h = TactileHeads(dev)
    h.set_bank(t)
    first = h.bank
    h.set_bank(t)
    assert h.bank is first                                           # the same unmodified tensor: nothing is uploaded again
    t[0] *= 2.0
    h.set_bank(t)
    assert h.bank is not first and torch.equal(h.bank.cpu(), t)      # modified in place: uploaded again
    h.set_bank(t.clone())
    assert torch.equal(h.bank.cpu(), t)


def test_zero_video_gives_nan_similarities_and_valid_indices(dev):
    """The reference divides the mean by its norm without an eps: a zero mean feature is NaN, and so is every similarity.  The indices stay
    inside the bank: the lowest k, in order."""
    _, bank = R.head_data(1, 5, 64, 7, 3)
    pooled = np.zeros((2, 5, 64), dtype=np.float32)
    pooled[1] = R.head_data(1, 5, 64, 7, 3)[0][0]
    video, sims, idx, val = run(dev, pooled, bank, 3)
    assert bool(torch.isnan(video[0]).all()) and bool(torch.isnan(sims[0]).all()) and bool(torch.isnan(val[0]).all())
    assert idx[0].tolist() == [0, 1, 2]
    assert bool(torch.isfinite(sims[1]).all()) and torch.equal(idx[1].long(), torch.topk(sims[1], 3).indices)
