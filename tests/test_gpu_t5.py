"""T5 v1.1 text encoder on the MI355X (vlatouch.t5 / csrc/vt_t5.hip) against HF's own output (g15) and the plain-torch restatement."""
import os

import numpy as np
import pytest
import torch

from tests import cases, t5_ref
from vlatouch import synth
from vlatouch import t5 as T5

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G15 = os.path.join(cases.GOLDEN, "g15_t5.npz")
CASES = {"tiny_b3": "tiny", "small_b2": "small_like", "tiny_l200": "tiny"}
# fp32: 2e-4 absolute on final-normed outputs of scale O(1), against g15's float64 run of the reference.  bf16 (bf16 weights and GEMM operands, fp32 residual stream): these synthetic
# weights give unscaled attention logits of std ~8, so a one-ulp operand change moves whole softmax rows; the CPU restatement with the
# engine's rounding points (t5_ref.encode(operands=bf16)) is itself 0.22 - 0.39 from the fp32 golden, HF's own bf16 run 0.38 - 0.44.
# The bf16 bar is therefore "no further from the fp32 result than the reference's own bf16 execution" (g15 keeps that run) where it
# exists, and BAR["bf16"] (measured 0.20 at XXL width) elsewhere; the mean error is held to 0.05.
BAR = {"fp32": 2e-4, "bf16": 0.3}
BF16_MEAN = 0.05


def hf_bf16_err(g, case):
    hf = torch.from_numpy(g[f"{case}_out_hf_bf16"].view(np.int16)).view(torch.bfloat16).float()
    return float((hf - torch.from_numpy(g[f"{case}_out"])).abs().max())
_ENG = {}


def engine(name, prec):
    if (name, prec) not in _ENG:
        _ENG[(name, prec)] = T5.T5Engine(t5_ref.t5_sd(name), synth.t5_config(name), precision=prec, device=DEV)
    return _ENG[(name, prec)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_engine_matches_golden(case, prec):
    g = np.load(G15)
    e = engine(CASES[case], prec)
    out = e.forward(torch.from_numpy(g[f"{case}_ids"]), torch.from_numpy(g[f"{case}_mask"]))
    torch.cuda.synchronize()
    d = (out.cpu() - torch.from_numpy(g[f"{case}_out"])).abs()      # every row, padded positions included
    err = float(d.max())
    if prec == "fp32":
        assert np.isfinite(err) and err <= BAR[prec], (case, prec, err)
    else:
        assert np.isfinite(err) and err <= hf_bf16_err(g, case) and float(d.mean()) <= BF16_MEAN, (case, prec, err, hf_bf16_err(g, case))


def test_l1024_against_t5_ref():
    cfg = synth.t5_config("tiny")
    g = torch.Generator().manual_seed(15)
    ids = torch.randint(2, cfg["vocab_size"], (1, 1024), generator=g)
    mask = torch.ones(1, 1024, dtype=torch.long)
    mask[0, 900:] = 0
    ref = t5_ref.encode(t5_ref.t5_sd("tiny"), cfg, ids, mask, dtype=torch.float64)       # float64: the reference's own fp32 error stays out of the bar
    out = engine("tiny", "fp32").forward(ids, mask)
    assert float((out.cpu().double() - ref).abs().max()) <= BAR["fp32"]


def _edge_mask(kind, B, L):
    """[B, L] long attention_mask.  lead: left padding (a leading masked run of L // 3); holes: every third token out, shifted by the sample;
    per_sample: valid lengths L, 1, L // 2."""
    if kind == "none":
        return None
    pos, b = torch.arange(L)[None, :], torch.arange(B)[:, None]
    if kind == "lead":
        keep = (pos >= max(1, L // 3)).expand(B, L)
    elif kind == "holes":
        keep = (pos + b) % 3 != 1
    else:
        keep = pos < torch.tensor([(L, 1, max(1, L // 2))[i % 3] for i in range(B)])[:, None]
    return keep.long()


@pytest.mark.parametrize("B,L,kind", [(1, 1, "none"), (1, 64, "lead"), (1, 64, "holes"), (2, 65, "lead"), (2, 65, "holes"), (2, 65, "per_sample"),
                                      (3, 129, "lead"), (3, 129, "holes"), (3, 129, "per_sample")])
def test_fp32_engine_edges_against_t5_ref(B, L, kind):
    """Lengths at the attention kernel's seams (one row; one full tile; one key past it; three tiles and blocks) under masks that are no suffix:
    left padding, holes, and per-sample lengths down to 1.  Every position is compared, padded ones included."""
    cfg = synth.t5_config("tiny")
    ids = torch.randint(2, cfg["vocab_size"], (B, L), generator=torch.Generator().manual_seed(100 * B + L))
    mask = _edge_mask(kind, B, L)
    assert mask is None or (bool(mask.sum(-1).min() >= 1) and not bool(mask.all()))
    ref = t5_ref.encode(t5_ref.t5_sd("tiny"), cfg, ids, mask, dtype=torch.float64)
    out = engine("tiny", "fp32").forward(ids, mask).cpu().double()
    err = float((out - ref).abs().max())
    print(f"[t5 fp32 edges B{B} L{L} {kind}] {err:.2e}")
    assert np.isfinite(err) and err <= BAR["fp32"], (B, L, kind, err)


_TAME = {}


def _tame_sd():
    """The tiny weights with every q projection scaled by 1/8 (exact in bf16): attention logits of O(1), as 1/sqrt(d)-trained weights give."""
    if not _TAME:
        _TAME.update({k: v / 8 if k.endswith("SelfAttention.q.weight") else v for k, v in t5_ref.t5_sd("tiny").items()})
    return _TAME


@pytest.mark.parametrize("case,rows", [("tiny_b3", 3), ("tiny_l200", 1)])
def test_bf16_engine_with_tame_logits_within_three_times_the_formats_cost(case, rows):
    """The bf16 bars above are as wide as the format's cost under logits of std ~8.  With logits of O(1) that cost, taken on the CPU as
    max|t5_ref.encode(float64, operands=bf16) - t5_ref.encode(float64)|, is 0.052 (3 x 37, g15's mask) and 0.058 (1 x 200), mean 0.0069 and
    0.0086; scaling q further does not lower it (0.044 / 0.040 at 1/128: what is left is the bf16 GEMM operands).  The engine is held to 3 x that
    cost, maximum and mean, against float64: 0.16 and 0.17 instead of 0.3, 0.021 and 0.026 instead of 0.05.
    Measured, engine against float64: maximum 0.050 and 0.053, mean 0.0069 and 0.0085."""
    g = np.load(G15)
    ids, mask = torch.from_numpy(g[f"{case}_ids"])[:rows], torch.from_numpy(g[f"{case}_mask"])[:rows]
    cfg, sd = synth.t5_config("tiny"), _tame_sd()
    ref64 = t5_ref.encode(sd, cfg, ids, mask, dtype=torch.float64)
    cost = (t5_ref.encode(sd, cfg, ids, mask, dtype=torch.float64, operands=torch.bfloat16) - ref64).abs()
    assert float(cost.max()) <= 0.3 / 4                                        # far below BAR["bf16"], or this test adds nothing
    e = T5.T5Engine(sd, cfg, precision="bf16", device=DEV)
    d = (e.forward(ids, mask).cpu().double() - ref64).abs()
    print(f"[t5 bf16 tame {case}] cost max {float(cost.max()):.3e} mean {float(cost.mean()):.3e}; engine max {float(d.max()):.3e} mean {float(d.mean()):.3e}")
    assert bool(torch.isfinite(d).all()) and float(d.max()) <= 3 * float(cost.max()) and float(d.mean()) <= 3 * float(cost.mean()), \
        (case, float(d.max()), float(cost.max()), float(d.mean()), float(cost.mean()))


def _xxl_sd(layers):
    cfg = synth.t5_config("xxl", num_layers=layers)
    return cfg, synth.fill_state_dict_device(synth.t5_shapes(**cfg), DEV, torch.bfloat16, seed=5)


def test_xxl_width_two_layers_against_t5_ref():
    cfg, sd = _xxl_sd(2)
    e = T5.T5Engine(sd, cfg, precision="bf16", device=DEV)
    g = torch.Generator().manual_seed(16)
    ids = torch.randint(2, cfg["vocab_size"], (2, 32), generator=g)
    mask = torch.ones(2, 32, dtype=torch.long)
    mask[1, 20:] = 0
    out = e.forward(ids, mask).cpu()
    ref = t5_ref.encode({k: v.float().cpu() for k, v in sd.items()}, cfg, ids, mask)
    del e, sd
    assert float((out - ref).abs().max()) <= BAR["bf16"] and float((out - ref).abs().mean()) <= BF16_MEAN


def test_xxl_full_depth_finite():
    cfg, sd = _xxl_sd(24)
    e = T5.T5Engine(sd, cfg, precision="bf16", device=DEV)
    del sd
    ids = torch.randint(2, cfg["vocab_size"], (1, 32), generator=torch.Generator().manual_seed(17))
    out = e.forward(ids)
    assert out.shape == (1, 32, 4096) and bool(torch.isfinite(out).all())


def test_repeatable_and_padding_independent():
    g = np.load(G15)
    ids, mask = torch.from_numpy(g["tiny_b3_ids"]), torch.from_numpy(g["tiny_b3_mask"])
    for prec in ("fp32", "bf16"):
        e = engine("tiny", prec)
        a, b = e.forward(ids, mask).clone(), e.forward(ids, mask).clone()
        assert torch.equal(a, b)
        n = int(mask[1].sum())
        alone = e.forward(ids[1:2, :n])
        assert float((a[1, :n] - alone[0]).abs().max()) <= {"fp32": 2e-4, "bf16": 2e-2}[prec], prec


def test_invalid_inputs_are_errors():
    from vlatouch._lib import VtError
    e = engine("tiny", "fp32")
    with pytest.raises((VtError, ValueError)):
        e.forward(torch.zeros(1, 1025, dtype=torch.long))
    with pytest.raises(VtError, match="no valid token"):
        e.forward(torch.ones(2, 4, dtype=torch.long), torch.tensor([[1, 1, 0, 0], [0, 0, 0, 0]]))
    with pytest.raises(VtError, match="outside"):
        e.forward(torch.full((1, 4), 100000, dtype=torch.long))


class _Tok:
    """Tokenizer stand-in: the g15 ids of the instructions it knows (T5 tokenizer call signature)."""

    def __init__(self, table):
        self.table = table

    def __call__(self, texts, max_length=None, padding="longest", truncation=True, return_tensors="pt", **_):
        texts = [texts] if isinstance(texts, str) else list(texts)
        seqs = [self.table[t] for t in texts]
        n = max(len(s) for s in seqs)
        ids = torch.zeros(len(seqs), n, dtype=torch.long)
        mask = torch.zeros(len(seqs), n, dtype=torch.long)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.tensor(s)
            mask[i, :len(s)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def _tok_tiny():
    g = np.load(G15)
    ids, mask = g["tiny_b3_ids"], g["tiny_b3_mask"]
    return _Tok({f"instr{i}": ids[i, : int(mask[i].sum())].tolist() for i in range(3)}), g


def test_t5_embedder_mirror():
    from models.multimodal_encoder.t5_encoder import T5Embedder
    tok, g = _tok_tiny()
    for dt, bar in ((torch.bfloat16, hf_bf16_err(g, "tiny_b3")), (torch.float32, BAR["fp32"])):
        emb = T5Embedder(DEV, "google/t5-v1_1-xxl", torch_dtype=dt, state_dict=t5_ref.t5_sd("tiny"), config=synth.t5_config("tiny"), tokenizer=tok)
        embs, mask = emb.get_text_embeddings(["instr0", "instr1", "instr2"])
        assert embs.shape == (3, 37, 128) and embs.dtype == dt and embs.device.type == "cuda"
        assert torch.equal(mask.cpu(), torch.from_numpy(g["tiny_b3_mask"]).long())
        ref = torch.from_numpy(g["tiny_b3_out"])
        rounding = float(ref.abs().max()) * 2.0 ** -8 if dt == torch.bfloat16 else 0.0       # the bf16 output's own rounding
        assert float((embs.float().cpu() - ref).abs().max()) <= bar + rounding
        ids = tok("instr1")["input_ids"]
        o1 = emb.model(ids.to(DEV))
        o2 = emb.model(input_ids=ids.to(DEV), attention_mask=torch.ones_like(ids).to(DEV))
        assert torch.equal(o1.last_hidden_state, o1["last_hidden_state"]) and torch.equal(o1.last_hidden_state, o2.last_hidden_state)
        assert o1.last_hidden_state.shape == (1, 5, 128) and o1.last_hidden_state.dtype == dt


def test_robot_wrapper_encode_instruction_feeds_step():
    from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
    from models.multimodal_encoder.t5_encoder import T5Embedder
    from scripts.franka_model_eef import RoboticDiffusionTransformerModel
    from tests.test_siglip import ARGS, _pil_frames
    args = {k: dict(v) for k, v in ARGS.items()}
    args["model"]["lang_token_dim"] = 128                       # = the tiny T5 width
    c = synth.SIGLIP_CONFIGS["tiny"]
    cfg = dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
               image_size=c["image_size"], patch_size=14)
    tower = SiglipVisionTower("synthetic", None, device=DEV, precision="fp32", state_dict=cases.siglip_sd("tiny"), config=cfg)
    tok, _ = _tok_tiny()
    emb = T5Embedder(DEV, "google/t5-v1_1-xxl", torch_dtype=torch.float32, state_dict=t5_ref.t5_sd("tiny"), config=synth.t5_config("tiny"), tokenizer=tok)
    m = RoboticDiffusionTransformerModel(args, device=DEV, dtype=torch.float32, control_frequency=10, vision_model=tower,
                                         text_model=emb.model, text_tokenizer=emb.tokenizer)
    text = m.encode_instruction("instr1", device=DEV)
    ids = torch.tensor([tok.table["instr1"]])
    ref_text = t5_ref.encode(t5_ref.t5_sd("tiny"), synth.t5_config("tiny"), ids)
    assert text.shape == (1, 5, 128) and float((text.cpu() - ref_text).abs().max()) <= BAR["fp32"]
    proprio = torch.randn(1, 10, generator=torch.Generator().manual_seed(3))
    torch.manual_seed(11)
    a = m.step(proprio, _pil_frames(), text)
    torch.manual_seed(11)
    b = m.step(proprio, _pil_frames(), ref_text)
    assert a.shape == (1, 8, 10) and float((a - b).abs().max()) <= 1e-3
    plain = RoboticDiffusionTransformerModel(args, device=DEV, dtype=torch.float32, control_frequency=10, vision_model=tower, policy=m.policy)
    with pytest.raises(NotImplementedError):
        plain.encode_instruction("instr1")
