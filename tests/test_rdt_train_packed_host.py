"""The host half of `RdtTrainer(small_batch_linear=...)`: the keyword's refusals (raised before anything touches a device), the field the
ranks of a process group compare, and the host-only sizing calls of the entry points the option adds.  No GPU."""
import pytest

from tests import cases  # noqa: F401  (puts the package on sys.path)


def _new(**kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer({}, heads=2, horizon=8, action_dim=16, **kw)


def test_packed_with_fp32_is_refused_at_construction():
    from vlatouch.rdt_train import SMALL_BATCH_LINEARS
    assert SMALL_BATCH_LINEARS == ("gemm", "packed")
    with pytest.raises(ValueError, match="small_batch_linear='packed'.*precision='bf16' or 'fp16'"):
        _new(small_batch_linear="packed")                       # precision defaults to fp32
    with pytest.raises(ValueError, match="small_batch_linear"):
        _new(small_batch_linear="packed", precision="fp32")


@pytest.mark.parametrize("bad", ["pws", "PACKED", "", None, True])
def test_an_unknown_value_is_refused(bad):
    for precision in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="small_batch_linear must be one of"):
            _new(small_batch_linear=bad, precision=precision)


def test_the_process_group_comparison_names_the_field(monkeypatch):
    """Two ranks that differ in small_batch_linear alone: dist.differing_field, fed what each rank's constructor hands it
    (RdtTrainer.group_fields), names that field with both values; identical ranks give None.  The all-gather is replaced by the two ranks'
    dictionaries, so no process group is needed."""
    import torch.distributed as dist
    from vlatouch import dist as D
    from vlatouch.rdt_train import RdtTrainer
    common = ("digest", 2, "bf16", "adamw", "fp32", "mfma", "tn")
    ranks = [RdtTrainer.group_fields(*common, sbl, None) for sbl in ("gemm", "packed")]
    assert list(ranks[0]) == list(ranks[1]) and "small_batch_linear" in ranks[0]

    def fake_gather(peers):
        def all_gather_object(out, obj, group=None):
            out[:] = peers
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: len(peers))
        monkeypatch.setattr(dist, "all_gather_object", all_gather_object)

    fake_gather(ranks)
    for mine in ranks:                                          # every rank gets the same answer
        assert D.differing_field(mine, "group") == ("small_batch_linear", ["gemm", "packed"])
    fake_gather([ranks[1], dict(ranks[1])])
    assert D.differing_field(ranks[1], "group") is None
    # a field listed before it still wins, as for the other keywords
    other = RdtTrainer.group_fields("digest", 2, "fp16", "adamw", "fp32", "mfma", "tn", "packed", None)
    fake_gather([ranks[0], other])
    assert D.differing_field(ranks[0], "group")[0] == "precision"


def test_the_split_k_scratch_is_sized_by_the_library():
    """Host-only calls: the slab area is what the inference engine's workspace reserves for the same rows (16 slabs of M x N fp32 up to 512 rows,
    nothing above), and refusals of vt_refresh16 that need no device are refusals here too."""
    from vlatouch import _lib as L
    lib = L.lib()
    assert lib.vt_splitk_slab_bytes(512, 768) == 16 * 512 * 768 * 4 and lib.vt_splitk_slab_bytes(513, 768) == 0 and lib.vt_splitk_slab_bytes(0, 768) == 0
    assert lib.vt_splitk_counters() >= 6 * (6144 // 64)            # one per 96 x 64 tile of the widest RDT-1B Linear at 512 rows
    assert lib.vt_refresh16(None, 8, 8, 8, L.BF16, None, None, None, None, None) == -22
    assert lib.vt_last_error().decode().startswith("vt_refresh16")
