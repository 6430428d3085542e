"""CPU-only: the surface and the loader of the tactile-encoder mirror (octopi_s/utils/encoder.py) on a temporary directory the test writes,
the CLIP engine's weight order (vlatouch.clip.clip_pack, plain CPU code) and the refusals that are decided on the host."""
import os
import warnings

import pytest
import torch
import yaml

from tests import clip_ref as R

torch.set_grad_enabled(False)
CFG = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=3, num_attention_heads=1, image_size=28, patch_size=14)
PROMPT = dict(use_clip="synthetic-clip", num_context_vision=3, prompt_depth_vision=2, gate_prior=0.0, dim_context_vision=64)


def tower_sd():
    return R.clip_sd(64, 3, 256, 28, 3, 2)


def write_exp(tmp_path, with_prompt=True, vificlip_prefix="module.clip_model.vision_model.", skip=()):
    from vlatouch import synth
    os.makedirs(tmp_path, exist_ok=True)
    with open(os.path.join(tmp_path, "run.yaml"), "w") as f:
        yaml.safe_dump(dict(dim_context_vision=64, residual_ratio=0.5, frame_size=28, flip_p=0.0), f)
    if with_prompt:
        with open(os.path.join(tmp_path, "prompt_learning.yaml"), "w") as f:
            yaml.safe_dump(PROMPT, f)
    sd = tower_sd()
    vf = {vificlip_prefix + k: v for k, v in sd.items()}
    vf["module.clip_model.text_model.final_layer_norm.weight"] = torch.ones(8)      # a text-tower key and the logit scales: ignored
    vf["module.logit_scale_tactile"] = torch.tensor(2.0)
    heads = synth.tactile_head_shapes(64, 48)
    files = {"tactile_vificlip.pt": vf}
    for name, kind in (("dotted_tactile_adapter.pt", "adapter"), ("plain_tactile_adapter.pt", "adapter"), ("property_classifier.pt", "property_classifier"),
                       ("project.pt", "project")):
        files[name] = {("module." if name.startswith("dotted") else "") + k: torch.from_numpy(v)
                       for k, v in synth.fill_state_dict(heads[kind], prefix=name + ".").items()}
    for name, d in files.items():
        if name not in skip:
            torch.save(d, os.path.join(tmp_path, name))
    return sd, files


def test_surface_matches_the_reference():
    import inspect
    from octopi_s.utils import encoder as E
    for name in ("CLIPVisionEncoder", "ViFiCLIP", "Adapter", "PropertyClassifier", "load_encoder", "TactileProjector", "rag_topk"):
        assert hasattr(E, name), name
    assert list(inspect.signature(E.ViFiCLIP.forward).parameters)[1:] == ["frames", "texts", "attention_masks"]
    assert list(inspect.signature(E.ViFiCLIP.__init__).parameters)[1:] == ["clip_model", "freeze_text_encoder", "use_positional_embeds"]
    assert list(inspect.signature(E.Adapter.__init__).parameters)[1:4] == ["input_size", "output_size", "residual_ratio"]
    assert list(inspect.signature(E.PropertyClassifier.__init__).parameters)[1:2] == ["input_size"]
    assert list(inspect.signature(E.load_encoder).parameters)[:2] == ["configs", "device"]
    assert list(inspect.signature(E.CLIPVisionEncoder.forward).parameters)[1:] == ["frames"]


def test_loader_reads_the_experiment_directory(tmp_path, capsys):
    from octopi_s.utils import encoder as E
    sd, files = write_exp(str(tmp_path))
    base = {k: torch.zeros_like(v) for k, v in sd.items() if "VPT" not in k}          # the "pretrained" CLIP: no prompt keys, other values
    vifi, dotted, plain, prop, cfgs = E.load_encoder(dict(load_exp_path=str(tmp_path), use_clip=None), "cuda:0", state_dict=base, clip_config=CFG)
    out = capsys.readouterr().out
    for line in ("Loaded tactile ViFi-CLIP!", "Loaded dotted tactile adapter!", "Loaded plain tactile adapter!", "Loaded property regression model!"):
        assert line in out
    assert cfgs["dim_context_vision"] == 64 and cfgs["residual_ratio"] == 0.5
    tower = vifi.clip_model
    assert set(tower.sd) == set(sd) and all(torch.equal(tower.sd[k], sd[k]) for k in sd)      # prefixes and `module.` stripped, text keys dropped
    assert tower._complete_prompts() == 2 and tower.prompt_configs["num_context_vision"] == 3
    assert torch.equal(dotted.state_dict()["rfc.0.weight"], files["dotted_tactile_adapter.pt"]["module.rfc.0.weight"])      # `module.` stripped
    assert torch.equal(plain.state_dict()["rfc.2.bias"], files["plain_tactile_adapter.pt"]["rfc.2.bias"])
    assert torch.equal(prop.state_dict()["hardness_fc.weight"], files["property_classifier.pt"]["hardness_fc.weight"])
    proj = E.TactileProjector(E.CLIPVisionEncoder(tower), 48)
    assert proj.load(str(tmp_path)) and torch.equal(proj.state_dict()["2.weight"], files["project.pt"]["2.weight"])
    with pytest.raises(RuntimeError):
        dotted.load_state_dict({"rfc.0.weight": torch.zeros(512, 64)}, strict=True)


@pytest.mark.parametrize("prefix", ["vision_model.", "clip_model.vision_model.", "module.vision_model.", ""])
def test_key_prefixes(prefix):
    from vlatouch.clip import clip_vision_sd
    sd = tower_sd()
    got = clip_vision_sd({prefix + k: v for k, v in sd.items()} | ({"text_model.x": torch.zeros(1)} if prefix else {}))
    assert set(got) == set(sd)


def test_missing_files_warn_with_the_references_words(tmp_path):
    from octopi_s.utils import encoder as E
    write_exp(str(tmp_path), skip=("tactile_vificlip.pt", "plain_tactile_adapter.pt", "property_classifier.pt"))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        vifi, dotted, plain, prop, _ = E.load_encoder(dict(load_exp_path=str(tmp_path), use_clip=None), "cuda:0", state_dict=tower_sd(), clip_config=CFG)
    said = [str(x.message) for x in w if x.category is UserWarning]
    assert said == ["No trained tactile ViFi-CLIP model found!", "No trained plain tactile adapter found!", "No trained property regression model found!"]
    assert float(plain.state_dict()["rfc.0.weight"].abs().max()) == 0.0


def test_no_weights_is_a_file_not_found_error(tmp_path, monkeypatch):
    from octopi_s.utils import encoder as E
    write_exp(str(tmp_path))
    monkeypatch.delenv("VLATOUCH_SYNTH_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError, match="no CLIP weights for 'synthetic-clip': pass state_dict=, point use_clip at a local HF directory"):
        E.load_encoder(dict(load_exp_path=str(tmp_path), use_clip=None), "cuda:0")
    monkeypatch.setenv("VLATOUCH_SYNTH_WEIGHTS", "1")
    vifi = E.load_encoder(dict(load_exp_path=str(tmp_path), use_clip=None), "cuda:0", clip_config=CFG)[0]
    assert vifi.clip_model.sd["VPT"].shape == (3, 64)                                  # the file's prompts over the synthetic set


def test_texts_are_refused():
    from octopi_s.utils import encoder as E
    vifi = E.ViFiCLIP(E.ClipVisionTower("x", state_dict=tower_sd(), config=CFG))
    with pytest.raises(NotImplementedError, match="text tower is not built"):
        vifi.forward(torch.zeros(1, 2, 3, 28, 28), torch.zeros(1, 4, dtype=torch.long), None)
    with pytest.raises(NotImplementedError):
        E.Adapter(64, 32, 0.5)
    with pytest.raises(ValueError):
        E.rag_topk(torch.zeros(1, 2, 3, 28, 28), vifi, torch.zeros(4, 64), k=5)        # k > R, decided before the GPU is touched
    with pytest.raises(ValueError):
        E.rag_topk(torch.zeros(1, 2, 3, 28, 28), vifi, torch.zeros(40, 64), k=17)      # k > 16


def test_engine_weight_order():
    from vlatouch import _lib as L
    from vlatouch.clip import clip_pack
    sd = tower_sd()
    for cdt, kpad in ((L.F32, 592), (L.BF16, 640)):
        names, W, f = clip_pack(sd, heads=1, cdt=cdt)
        assert names[:3] == ["patch_w", "patch_b", "cls_pos0"]
        per = ["ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2"]
        assert names[3:3 + 42] == [f"{i}.{n}" for i in range(3) for n in per]
        assert names[45:] == ["lnf_w", "lnf_b", "pre_w", "pre_b", "VPT", "1.VPT_shallow", "gates"]
        assert len(W) == 3 + 14 * 3 + 2 + 2 + 1 + 1 + 1
        by = dict(zip(names, W))
        assert by["patch_w"].shape == (64, kpad) and float(by["patch_w"][:, 588:].abs().max()) == 0.0 and float(by["patch_b"].abs().max()) == 0.0
        assert torch.equal(by["cls_pos0"], sd["embeddings.class_embedding"] + sd["embeddings.position_embedding.weight"][0])
        assert by["0.qkv_w"].shape == (192, 64) and torch.equal(by["0.qkv_w"][64:128].float(), sd["encoder.layers.0.self_attn.k_proj.weight"].to(by["0.qkv_w"].dtype).float())
        assert torch.equal(by["1.ls1"], torch.ones(64)) and torch.equal(by["2.ls2"], torch.ones(64))
        assert torch.equal(by["gates"], torch.sigmoid(torch.tensor([-4.0, 0.0, 0.0])).where(torch.tensor([True, True, False]), torch.tensor(0.5)))
        assert f["n_prompt"] == 3 and f["prompt_depth"] == 2 and f["image_size"] == 28 and f["mlp_dim"] == 256 and f["kpad"] == kpad
        assert torch.equal(f["pos_patch"], sd["embeddings.position_embedding.weight"][1:])
    # depth 0: no prompt weights, whatever the checkpoint carries
    names, W, f = clip_pack(sd, heads=1, cdt=L.F32, prompt_depth=0)
    assert names[-1] == "pre_b" and f["n_prompt"] == 0 and f["prompt_depth"] == 0
    with pytest.raises(L.VtError):
        clip_pack(sd, heads=1, cdt=L.F32, prompt_depth=4)                              # prompt_depth > layers
    with pytest.raises(L.VtError):
        clip_pack(sd, heads=2, cdt=L.F32)                                              # 32-wide heads
