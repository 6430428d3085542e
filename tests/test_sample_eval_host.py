"""Host-side checks of fine-tuning's periodic sampling evaluation (no GPU): the fp64 restatement
of `log_sample_res` (tests/sample_eval_ref.py) against the reference's own run (tests/golden/g18_sample_eval.npz,
tools/make_golden_sample_eval.py), and the host logic of vlatouch.rdt_train.sample_eval / finetune."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import sample_eval_ref as S


def _g18():
    return np.load(f"{cases.GOLDEN}/g18_sample_eval.npz")


def _golden(run):
    g = _g18()
    return {str(k): float(v) for k, v in zip(g[f"{run}_keys"], g[f"{run}_values"])}


def test_declaration_cites_the_reference_lines_it_restates():
    assert "sample.py:55-86" in open(f"{cases.ROOT}/include/vlatouch.h").read()


def test_golden_covers_what_it_is_meant_to_pin():
    """The inputs the golden was taken on: sparse masks, exact zeros in state_norm under the mask, a single-element sample, a dataset that occurs
    in one batch only, one that never occurs, and in `nanmask` one sample without any unmasked element."""
    assert "UNPINNED" in str(_g18()["sampler"])
    b = S.golden_batches("main")
    assert [x["actions"].shape for x in b] == [(3, 8, 128)] * 2 and [x["data_indices"] for x in b] == [[0, 1, 0], [1, 2, 1]]
    for x in b:
        m, sn = x["state_elem_mask"], x["state_norm"]
        assert 0 < float(m.mean()) < 0.2 and bool((m.sum(1) >= 1).all()) and float(m[0].sum()) == 1
        assert bool(((sn == 0) & (m == 1)).any(1).all()), "every sample has an unmasked element whose state_norm is exactly 0"
    z = S.golden_batches("nanmask")
    assert float(z[1]["state_elem_mask"][0].sum()) == 0 and all(float(x["state_elem_mask"][s].sum()) > 0 for j, x in enumerate(z) for s in range(3) if (j, s) != (1, 0))


@pytest.mark.parametrize("run", list(S.G18_RUNS))
def test_restatement_matches_the_references_own_run(run):
    """Every key of g18 within 0.5e-4 + 2e-6 |value|: the reference's round(., 4) plus its fp32 arithmetic (about 5e-6 on values near 50).  Same
    key set, in the same order; NaN exactly where the golden has it."""
    gold = _golden(run)
    batches = S.golden_batches(run)
    got = S.log_sample_res_restated(batches, [b["pred"] for b in batches], S.G18_ID2NAME, S.G18_RUNS[run][2])
    assert list(got) == list(gold)
    assert S.same_nan_places(got, gold)
    assert any(np.isnan(v) for v in gold.values()) == (run == "nanmask")
    worst = 0.0
    for k, want in gold.items():
        if np.isnan(want):
            continue
        err, bar = abs(got[k] - want), 0.5e-4 + 2e-6 * abs(want)
        worst = max(worst, err / bar)
        assert err <= bar, (k, got[k], want)
    print(f"[g18 {run}] worst |fp64 restatement - reference| = {worst:.3f} of the bar")
    assert "never_sampled_sample_mse" not in gold and "bridge_sample_mse" in gold
    if run == "nanmask":
        assert {k for k, v in gold.items() if np.isnan(v)} == {"rh20t_sample_mse", "rh20t_sample_l2err"}
        assert np.isfinite(gold["overall_avg_sample_mse"]) and np.isfinite(gold["overall_avg_sample_l2err"])


def test_overall_divisor_is_num_sample_batches_when_the_loader_ends_early():
    main, short = _golden("main"), _golden("short")
    for k in ("overall_avg_sample_mse", "overall_avg_sample_l2err"):
        assert abs(short[k] - main[k] * 2 / 3) <= 1e-4, k              # both rounded to 4 decimals
    assert all(short[k] == main[k] for k in main if not k.startswith("overall_avg_"))


def _sums(run):
    """acc / count as vt_sample_metrics leaves them (rows in dataset_id2name's key order), from the fp64 restatement."""
    batches = S.golden_batches(run)
    dev_batches = [dict(pred=b["pred"], target=b["actions"], mask=b["state_elem_mask"], state_norm=b["state_norm"],
                        dataset_idx=torch.tensor(b["data_indices"])) for b in batches]
    return S.running_sums(dev_batches, len(S.G18_ID2NAME))[-1]


def test_means_of_the_device_sums_use_the_references_divisors():
    """sample_eval_means on the sums of `main`: per-dataset rows divided by their counts, the overall row by num_sample_batches (2, and 3 when
    the iterable ended early); a dataset that never occurred has no key, so its zero count divides nothing."""
    from vlatouch.rdt_train import sample_eval_means
    acc, count = _sums("main")
    keys = {"agilex_sample_mse": (0, 0), "rh20t_sample_l2err": (1, 1), "bridge_sample_mse": (2, 0), "overall_avg_sample_mse": (4, 0),
            "overall_avg_sample_l2err": (4, 1)}
    assert list(count) == [2, 3, 1, 0, 2]
    for nsb, run in ((2, "main"), (3, "short")):
        got, gold = sample_eval_means(torch.from_numpy(acc), torch.from_numpy(count), keys, nsb), _golden(run)
        assert set(got) == set(keys)
        for k, v in got.items():
            assert abs(v - gold[k]) <= 0.5e-4 + 2e-6 * abs(gold[k]), (run, k, v, gold[k])


class _NoDevice:
    device = "cuda"

    def predict_action(self, **kw):
        raise AssertionError("the indices are checked before anything is sampled")


def test_out_of_range_data_indices_raise_before_the_device_is_touched():
    from vlatouch.rdt_train import sample_eval
    b = dict(S.golden_batches("main")[0])
    for bad in ([0, 1, 4], [0, -1, 0]):
        b["data_indices"] = bad
        with pytest.raises(ValueError, match="data_indices"):
            sample_eval(_NoDevice(), [b], num_sample_batches=2, dataset_id2name=S.G18_ID2NAME)
    with pytest.raises(ValueError):
        sample_eval(_NoDevice(), [b], num_sample_batches=0, dataset_id2name=S.G18_ID2NAME)
    assert sample_eval(_NoDevice(), [], num_sample_batches=2, dataset_id2name=S.G18_ID2NAME) == {}     # no batch: the reference returns {}


def test_finetune_with_sample_period_needs_batches_and_names():
    from vlatouch.rdt_train import finetune
    with pytest.raises(ValueError, match="sample_period"):
        finetune(None, [], max_train_steps=1, sample_period=2)
    with pytest.raises(ValueError, match="sample_period"):
        finetune(None, [], max_train_steps=1, sample_period=2, sample_batches=[])
    with pytest.raises(ValueError, match="sample_period"):
        finetune(None, [], max_train_steps=1, sample_period=2, dataset_id2name=S.G18_ID2NAME)
    assert finetune(None, [], max_train_steps=1, sample_period=-1) == []            # unset: today's loop


def test_mirror_package_has_the_references_signature():
    import inspect
    import train.sample
    from train.sample import log_sample_res
    assert train.sample.__file__.startswith(cases.PKG), "the product's mirror, not another `train` on sys.path"
    assert list(inspect.signature(log_sample_res).parameters) == ["text_encoder", "vision_encoder", "rdt", "args", "accelerator", "weight_dtype",
                                                                   "dataset_id2name", "dataloader", "logger"]
