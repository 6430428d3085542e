"""The tactile-encoder mirror (octopi_s/utils/encoder.py) end to end on synthetic weights at a small config against the float64 statement of
tests/clip_ref.py: CLIPVisionEncoder, ViFiCLIP, Adapter, PropertyClassifier, TactileProjector and rag_topk.

Config (clip_ref.API): hidden 128, 2 heads, 3 layers, 28 px, n_ctx 3, depth 2, E = 192; 2 videos of 3 frames; a bank of 9 whose
similarities to each video lie at least 0.07 apart (clip_ref.api_bank), so rag_topk's indices must equal torch.topk's on the float64
similarities in every mode.  ViFiCLIP.forward is called again after rag_topk on the same object.
Bars: 3 x the largest CPU-measured cost of the six outputs per mirror mode (clip_ref.COSTS["api", ...], held by tests/test_clip_ref_host.py):

  mode                                              cost      bar
  fp32                                              9.6e-7    2.9e-6
  fp16  (precision "bf16": fp16 tower, bf16 heads)  6.3e-3    1.9e-2
  bf16  (after the range guard's fall-back)         1.0e-2    3.0e-2

The range guard: an fc1 bias of 2e5 in one channel makes quick-GELU's output inf in fp16, NaN in the residual stream, and the final norm
raises VT_RANGE_NONFINITE; the tower rebuilds itself with bf16 storage, warns, and its result is then held to the bf16 bar."""
import pytest
import torch

from tests import clip_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CFG = dict(hidden_size=R.API["hidden"], intermediate_size=R.API["inter"], num_hidden_layers=R.API["layers"], num_attention_heads=R.API["heads"],
           image_size=R.API["image_size"], patch_size=14)
PROMPT = dict(num_context_vision=R.API["n_ctx"], prompt_depth_vision=R.API["prompt_depth"], gate_prior=0.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def problem():
    sd, heads, frames, bank = R.api_weights()
    return sd, heads, frames, bank, R.api_reference(sd, heads, frames, bank)


def mirror(sd, heads, dev, precision):
    from octopi_s.utils import encoder as E
    a = R.API
    tower = E.ClipVisionTower("synthetic", PROMPT, device=dev, precision=precision, state_dict={"module.clip_model.vision_model." + k: v for k, v in sd.items()},
                              config=CFG)
    vifi = E.ViFiCLIP(tower)
    enc = E.CLIPVisionEncoder(tower)
    ad = E.Adapter(a["hidden"], a["hidden"], 0.5, device=dev, precision=precision)
    ad.load_state_dict(heads["adapter"])
    pc = E.PropertyClassifier(a["hidden"], device=dev, precision=precision)
    pc.load_state_dict({"module." + k: v for k, v in heads["property_classifier"].items()})
    proj = E.TactileProjector(enc, a["llm_dim"], dtype=torch.float32 if precision == "fp32" else torch.bfloat16, device=dev, precision=precision)
    proj.load_state_dict(heads["project"])
    return E, tower, vifi, enc, ad, pc, proj


def errors(E, vifi, enc, ad, pc, proj, frames, bank, ref):
    a = R.API
    feats = enc(frames)
    assert tuple(feats.shape) == (a["b"], a["l"], a["hidden"]) and feats.dtype == torch.float32
    video, t, li, lt = vifi(frames, None, None)
    assert t is None and li is None and lt is None
    idx, val = E.rag_topk(frames, vifi, bank, a["k"])
    sims = vifi.heads.retrieve(feats, a["k"])[1]
    again = vifi(frames, None, None)                                 # after a retrieval on the same object: still (video_features, None, None, None)
    assert isinstance(again[0], torch.Tensor) and torch.equal(again[0], video) and again[1:] == (None, None, None)
    bank_on_device = vifi.heads.bank
    E.rag_topk(frames, vifi, bank, a["k"])
    assert vifi.heads.bank is bank_on_device                         # the same bank tensor is not uploaded twice
    flat = feats.reshape(a["b"] * a["l"], -1)
    tokens = proj(frames)
    assert tuple(tokens.shape) == (a["b"], a["l"], a["llm_dim"]) and tokens.dtype == proj.dtype
    got = dict(feats=feats, video=video, sims=sims, adapter=ad(flat), prop=pc(flat), project=tokens.reshape(a["b"] * a["l"], -1))
    torch.cuda.synchronize()
    errs = {k: (float((got[k].cpu().double() - ref[k]).abs().max()) if k == "sims" else R.row_err(got[k].float().cpu(), ref[k])) for k in ref}
    want = torch.topk(ref["sims"], a["k"], dim=-1)
    srt = ref["sims"].sort(dim=-1, descending=True).values[:, : a["k"] + 1]
    return errs, idx.cpu(), want.indices, float((srt[:, :-1] - srt[:, 1:]).min())


@pytest.mark.parametrize("precision,mode", [("fp32", "fp32"), ("bf16", "fp16")])
def test_mirror_end_to_end(dev, problem, precision, mode, monkeypatch):
    from vlatouch import _lib as L
    monkeypatch.delenv("VLATOUCH_CLIP_PRECISION", raising=False)
    sd, heads, frames, bank, ref = problem
    E, tower, vifi, enc, ad, pc, proj = mirror(sd, heads, dev, precision)
    errs, idx, want, gap = errors(E, vifi, enc, ad, pc, proj, frames, bank, ref)
    bar = R.BARS[("api", mode)]
    print(f"mirror {precision}: {({k: f'{v:.2e}' for k, v in errs.items()})} (bar {bar:.2e}); top-k gap {gap:.2e}")
    assert tower.engine.adt == (L.F32 if precision == "fp32" else L.F16) and tower.engine.prompt_depth == 2 and tower.engine.n_ctx == 3
    assert gap >= R.API_GAP > 2 * max(R.BARS.values())               # asserted on the reference first: the order is decided far above any mode's error
    assert max(errs.values()) <= bar, (errs, bar)
    assert torch.equal(idx, want), (idx, want)
    assert tuple(idx.shape) == (R.API["b"], R.API["k"]) and idx.dtype == torch.int64


def test_range_guard_falls_back_to_bf16(dev, problem, monkeypatch):
    from vlatouch import _lib as L
    monkeypatch.delenv("VLATOUCH_CLIP_PRECISION", raising=False)
    sd, heads, frames, bank, _ = problem
    sd = {k: v.clone() for k, v in sd.items()}
    sd["encoder.layers.1.mlp.fc1.bias"][7] = 2.0e5
    ref = R.api_reference(sd, heads, frames, bank)
    E, tower, vifi, enc, ad, pc, proj = mirror(sd, heads, dev, "bf16")
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        feats = enc(frames)
    assert tower.engine.adt == L.BF16 and tower._range.fell_back and tower._range.bits & L.RANGE_NONFINITE
    assert bool(torch.isfinite(feats).all())
    e = R.row_err(feats.cpu(), ref["feats"])
    bar = R.BARS[("api", "bf16")]
    print(f"mirror after the fall-back: frame features {e:.3e} (bar {bar:.3e})")
    assert e <= bar, (e, bar)
    errs = errors(E, vifi, enc, ad, pc, proj, frames, bank, ref)[0]
    print(f"mirror after the fall-back: {({k: f'{v:.2e}' for k, v in errs.items()})}")
    assert max(errs.values()) <= bar, (errs, bar)
