"""T5 v1.1 text encoder, host side (no GPU): bucket table, packing plan, local loader, and the plain-torch restatement pinned to g15."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cases, t5_ref
from vlatouch import synth
from vlatouch import t5 as T5

G15 = os.path.join(cases.GOLDEN, "g15_t5.npz")
CASES = {"tiny_b3": "tiny", "small_b2": "small_like", "tiny_l200": "tiny"}


def test_bucket_table_matches_golden():
    tab = T5.bucket_table(32, 128)
    assert tab.dtype == np.int8 and tab.shape == (2047,)
    assert np.array_equal(tab, np.load(G15)["buckets"])
    assert tab[1023] == 0 and tab.min() == 0 and tab.max() == 31


def test_bucket_table_matches_hf_for_every_rel():
    transformers = pytest.importorskip("transformers")
    from transformers.models.t5.modeling_t5 import T5Attention
    rel = torch.arange(-1023, 1024, dtype=torch.long)
    for nb, md in ((32, 128), (32, 64), (16, 32)):
        hf = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=nb, max_distance=md)
        assert np.array_equal(T5.bucket_table(nb, md), hf.numpy().astype(np.int8)), (nb, md)
    del transformers


def test_pack_plan_key_map_and_shapes():
    for name in ("tiny", "small_like", "xxl"):
        cfg = synth.t5_config(name)
        c = T5.t5_config(cfg)
        shapes = synth.t5_shapes(**cfg)
        plan = T5.pack_plan(c, shapes.keys())
        n = c["num_layers"]
        assert len(plan) == 2 + 6 * n + 1
        assert [p[0] for p in plan[:2]] == ["shared", "rel_bias"] and plan[-1][0] == "final_ln"
        want = T5.slot_shapes(c)
        for slot, keys, kind in plan:      # concatenating the source shapes along dim 0 gives the slot's packed shape
            got = (sum(shapes[k][0] for k in keys),) + tuple(shapes[keys[0]][1:])
            assert got == want[slot], (name, slot)
            assert kind == ("f32" if slot.split(".")[0] in ("rel_bias", "ln1", "ln2", "final_ln") else "w")
        qkv = dict((p[0], p[1]) for p in plan)["qkv.1"]
        assert qkv == [f"encoder.block.1.layer.0.SelfAttention.{x}.weight" for x in "qkv"]
        assert dict((p[0], p[1]) for p in plan)["wi.0"] == ["encoder.block.0.layer.1.DenseReluDense.wi_0.weight",
                                                            "encoder.block.0.layer.1.DenseReluDense.wi_1.weight"]
    c = T5.t5_config(synth.t5_config("small_like"))
    assert T5.slot_shapes(c)["qkv.0"] == (3 * 384, 512) and T5.slot_shapes(c)["o.0"] == (512, 384)      # inner != d_model


def test_pack_plan_embedding_key_tied_or_untied():
    cfg = T5.t5_config(synth.t5_config("tiny"))
    keys = set(synth.t5_shapes(**synth.t5_config("tiny")))
    assert T5.pack_plan(cfg, keys)[0][1] == ["shared.weight"]
    untied = (keys - {"shared.weight"}) | {"encoder.embed_tokens.weight"}
    assert T5.pack_plan(cfg, untied)[0][1] == ["encoder.embed_tokens.weight"]
    with pytest.raises(KeyError):
        T5.pack_plan(cfg, keys - {"shared.weight"})
    with pytest.raises(KeyError):
        T5.pack_plan(cfg, keys - {"encoder.block.1.layer.1.DenseReluDense.wo.weight"})


def test_config_rejects_non_gated_and_other_head_widths():
    for ffp in ("relu", "gated-relu", "gelu"):
        with pytest.raises(ValueError, match="gated-gelu"):
            T5.t5_config(synth.t5_config("tiny", feed_forward_proj=ffp))
    with pytest.raises(ValueError, match="d_kv"):
        T5.t5_config(synth.t5_config("tiny", d_kv=128))
    with pytest.raises(ValueError, match="fp16"):
        T5.T5Engine({}, synth.t5_config("tiny"), precision="fp16")


def _write_checkpoint(d, name="tiny", untied=False):
    from safetensors.torch import save_file
    sd = t5_ref.t5_sd(name)
    if untied:
        sd["encoder.embed_tokens.weight"] = sd.pop("shared.weight")
    sd["decoder.final_layer_norm.weight"] = torch.ones(4)        # a full T5 checkpoint also carries the decoder: ignored
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    json.dump(dict(synth.t5_config(name), model_type="t5"), open(os.path.join(d, "config.json"), "w"))
    return sd


def test_loader_reads_local_directory(tmp_path):
    sd = _write_checkpoint(str(tmp_path))
    assert T5.resolve_local(str(tmp_path)) == str(tmp_path)
    got = T5.local_state_dict(str(tmp_path))
    cfg = T5.t5_config(json.load(open(os.path.join(str(tmp_path), "config.json"))))
    plan = T5.pack_plan(cfg, got.keys())
    for _, keys, _ in plan:
        for k in keys:
            assert torch.equal(got[k], sd[k])


def test_loader_reads_sharded_and_bin_forms(tmp_path):
    from safetensors.torch import save_file
    sd = t5_ref.t5_sd("tiny")
    keys = sorted(sd)
    halves = (keys[: len(keys) // 2], keys[len(keys) // 2:])
    a, b = tmp_path / "sharded", tmp_path / "bins"
    a.mkdir()
    b.mkdir()
    wmap = {}
    for i, ks in enumerate(halves):
        f = f"model-{i + 1:05d}-of-00002.safetensors"
        save_file({k: sd[k].contiguous() for k in ks}, str(a / f))
        wmap.update({k: f for k in ks})
    json.dump({"weight_map": wmap}, open(a / "model.safetensors.index.json", "w"))
    torch.save(sd, str(b / "pytorch_model.bin"))
    for d in (a, b):
        got = T5.local_state_dict(str(d))
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in keys)


def test_loader_finds_hf_cache_snapshot_and_never_fetches(tmp_path, monkeypatch):
    import socket

    def no_network(*a, **k):
        raise AssertionError("the T5 loader tried to open a network connection")

    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError, match="google/t5-v1_1-xxl"):
        T5.load_t5_encoder("google/t5-v1_1-xxl", device="cuda")
    snap = tmp_path / "hub" / "models--google--t5-v1_1-xxl" / "snapshots" / "abc123"
    snap.mkdir(parents=True)
    _write_checkpoint(str(snap))
    (tmp_path / "hub" / "models--google--t5-v1_1-xxl" / "refs").mkdir()
    (tmp_path / "hub" / "models--google--t5-v1_1-xxl" / "refs" / "main").write_text("abc123")
    assert T5.resolve_local("google/t5-v1_1-xxl") == str(snap)


@pytest.mark.parametrize("case", sorted(CASES))
def test_t5_ref_matches_golden(case):
    """g15 holds the reference's encoder run in float64 (stored as fp32).  The restatement in float64 must reproduce it to 2e-5; that pins the
    formula independently of any machine's BLAS summation order.  In fp32, the precision the GPU tests use it in, it must stay within fp32's own
    error on this unscaled encoder (HF's fp32 run is up to 4e-5 from the float64 answer)."""
    g = np.load(G15)
    name = CASES[case]
    ids, mask, ref = torch.from_numpy(g[f"{case}_ids"]), torch.from_numpy(g[f"{case}_mask"]), torch.from_numpy(g[f"{case}_out"]).double()
    sd, cfg = t5_ref.t5_sd(name), synth.t5_config(name)
    out64 = t5_ref.encode(sd, cfg, ids, mask, dtype=torch.float64)
    assert float((out64 - ref).abs().max()) < 2e-5
    out32 = t5_ref.encode(sd, cfg, ids, mask)
    assert float((out32.double() - ref).abs().max()) < 1e-4
