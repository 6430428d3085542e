"""CPU-only: the float64 statement of Octopi's tactile encoder (tests/clip_ref.py) against what it can be held to on this side.

PINNED to the installed `transformers` (5.x): `CLIPVisionModel` with a small random `CLIPVisionConfig` (hidden_act "quick_gelu").  With prompt
depth 0 the statement in fp32 equals HF's `pooler_output` and `last_hidden_state` within 1e-5 of each row's maximum.  For depth > 0 the block
arithmetic is held to HF's own `CLIPEncoderLayer` modules, called layer by layer with the statement's prompt steps applied between them.

UNPINNED against the reference's own classes: octopi_s/utils/encoder.py imports `CLIPVisionTransformer` and `_create_4d_causal_attention_mask`
from `transformers.models.clip.modeling_clip`, which this `transformers` no longer has (the reference pins 4.45.1, which is not installed), so
`PromptLearningCLIPEncoderLayer` cannot be imported here.  The ORDER of the prompt steps is therefore held by known answers on a toy block
(below), written from the description of the reference's forward.

The bars of the GPU tests (clip_ref.COSTS) are measured here on the CPU and the literals held to the measurement."""
import numpy as np
import pytest
import torch

from tests import clip_ref as R

torch.set_grad_enabled(False)
HF_TOL = 1e-5


def hf_model(hidden, heads, inter, layers, image_size, seed=0):
    from transformers import CLIPVisionConfig, CLIPVisionModel
    torch.manual_seed(seed)
    cfg = CLIPVisionConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads, image_size=image_size,
                           patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5, attn_implementation="eager")
    m = CLIPVisionModel(cfg).eval()
    for p in m.parameters():                                        # HF's init leaves biases 0 and gains 1: every term must matter
        p.add_(0.05 * torch.randn_like(p))
    return m


def rel_sd(m):
    """Keys relative to the vision transformer (transformers 5.x saves them so; 4.x under `vision_model.`)."""
    pre = "vision_model."
    return {(k[len(pre):] if k.startswith(pre) else k): v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("hidden,heads,res,B", [(64, 1, 28, 1), (128, 2, 42, 3)])
def test_depth_0_equals_hf_clip_vision_model(hidden, heads, res, B):
    m = hf_model(hidden, heads, 4 * hidden, 3, res)
    px = torch.from_numpy(R.pixels(B, res, seed=res + B))
    out = m(pixel_values=px)
    last, pooled, _ = R.forward(rel_sd(m), px, heads, 0, acc=torch.float32)
    e_last, e_pool = R.row_err(last, out.last_hidden_state), R.row_err(pooled, out.pooler_output)
    print(f"depth 0 d{hidden} res {res} B {B}: last_hidden_state {e_last:.2e}, pooler_output {e_pool:.2e}")
    assert e_last <= HF_TOL and e_pool <= HF_TOL


@pytest.mark.parametrize("P", [1, 2, -1])
def test_blocks_equal_hf_encoder_layers_between_the_prompt_steps(P):
    """The statement's own block against HF's CLIPEncoderLayer under the same prompt steps, every block's input included (`trace`)."""
    hidden, heads, res, B, n, layers = 128, 2, 28, 3, 3, 3
    m = hf_model(hidden, heads, 512, layers, res, seed=P + 5)
    sd = rel_sd(m)
    g = torch.Generator().manual_seed(11)
    depth = R.depth(layers, P)
    sd["VPT"] = torch.randn(n, hidden, generator=g)
    for i in range(layers):
        if 1 <= i < depth:
            sd[f"encoder.layers.{i}.VPT_shallow"] = torch.randn(n, hidden, generator=g)
        if i != layers - 1:
            sd[f"encoder.layers.{i}.VPT_gamma"] = torch.tensor((-4.0, 0.0, 5.0)[i % 3])
    px = torch.from_numpy(R.pixels(B, res, seed=3))
    mine_trace, hf_trace = [], []
    last, pooled, _ = R.forward(sd, px, heads, P, acc=torch.float32, trace=mine_trace)
    vm = getattr(m, "vision_model", m)
    t = R.tokens(sd, px, depth, acc=torch.float32)

    def hf_block(i, x):
        y = vm.encoder.layers[i](x, attention_mask=None)
        return y[0] if isinstance(y, tuple) else y

    t = R.run_layers(t, layers, depth, n, hf_block, lambda i: sd[f"encoder.layers.{i}.VPT_shallow"],
                     lambda i: torch.sigmoid(sd[f"encoder.layers.{i}.VPT_gamma"]), hf_trace)
    assert [x.shape for x in mine_trace] == [x.shape for x in hf_trace]
    errs = [R.row_err(a, b) for a, b in zip(mine_trace, hf_trace)] + [R.row_err(last, t), R.row_err(pooled, vm.post_layernorm(t[:, 0]))]
    print(f"P {P}: block inputs, last_hidden_state, pooler_output: {[f'{e:.1e}' for e in errs]}")
    assert max(errs) <= HF_TOL
    rows = [x.shape[1] for x in mine_trace]
    assert rows == [5 + n if i < depth else 5 for i in range(layers)]


# ------------------------------------------------------------------------------------------------ known answers for the prompt order
def _toy(P, layers, gates, n=1):
    """Two rows per image (one ordinary row = 1, one prompt row: VPT = 2), D = 1.  Block i maps every value x to x + 10^i, VPT_shallow_i =
    1000 (i + 1).  -> (the rows every block received, the rows every block handed on after its gate step).
    The gated tail never reaches an output of the tower: the next block overwrites it (i + 1 < P) or drops it (i + 1 == P), and the last block
    does not gate.  It lives on only as the next block's `before`, so the known answers read it from `after`."""
    t = torch.tensor([[[1.0], [2.0]]], dtype=torch.float64)
    trace, after = [], []
    R.run_layers(t, layers, P, n, lambda i, x: x + 10.0 ** i, lambda i: torch.full((n, 1), 1000.0 * (i + 1), dtype=torch.float64),
                 lambda i: torch.tensor(gates[i], dtype=torch.float64), trace, after)
    return [x.flatten().tolist() for x in trace], [x.flatten().tolist() for x in after]


def test_gate_1_keeps_the_blocks_output():
    trace, after = _toy(P=4, layers=4, gates={1: 1.0, 2: 1.0})
    # block 1 receives tail 3, overwrites it with 2000, puts out 2010; gate 1 keeps 2010.  Block 2 likewise: 3000 -> 3100.
    assert trace == [[1.0, 2.0], [2.0, 2000.0], [12.0, 3000.0], [112.0, 4000.0]]
    assert after == [[2.0, 3.0], [12.0, 2010.0], [112.0, 3100.0], [1112.0, 5000.0]]


def test_gate_0_restores_the_tail_as_it_arrived():
    trace, after = _toy(P=4, layers=4, gates={1: 0.0, 2: 0.0})
    # `before` of block 1 is the tail AS IT ARRIVED (3 = VPT + block 0), not the overwritten 2000; block 2's `before` is what block 1's gate left
    assert trace == [[1.0, 2.0], [2.0, 2000.0], [12.0, 3000.0], [112.0, 4000.0]]
    assert after == [[2.0, 3.0], [12.0, 3.0], [112.0, 3.0], [1112.0, 5000.0]]


def test_gate_mixes_with_before_and_carries_over():
    _, after = _toy(P=4, layers=4, gates={1: 0.25, 2: 0.5})
    t1 = 0.25 * 2010.0 + 0.75 * 3.0                                  # 504.75
    t2 = 0.5 * 3100.0 + 0.5 * t1                                     # block 2 gates against block 1's GATED tail
    assert after[1] == [12.0, t1] and after[2] == [112.0, t2] and after[3] == [1112.0, 5000.0]


def test_block_0_never_overwrites_and_depth_shortens_the_sequence():
    trace, after = _toy(P=1, layers=3, gates={})
    assert trace == [[1.0, 2.0], [2.0], [12.0]] and after[-1] == [112.0]      # block 0 sees VPT itself and does not gate; block 1 == P drops the tail
    trace, after = _toy(P=2, layers=3, gates={1: 0.0})
    assert trace == [[1.0, 2.0], [2.0, 2000.0], [12.0]] and after == [[2.0, 3.0], [12.0, 3.0], [112.0]]      # block 1 < P gates, block 2 == P drops
    trace, after = _toy(P=3, layers=4, gates={1: 1.0, 2: 1.0})
    assert [len(x) for x in trace] == [2, 2, 2, 1] and after[-1] == [1112.0]
    trace, after = _toy(P=0, layers=2, gates={}, n=0)
    assert trace == [[1.0, 2.0], [2.0, 3.0]] and after[-1] == [12.0, 13.0]    # no prompts: nothing is touched


def test_last_layer_never_gates():
    trace, after = _toy(P=2, layers=2, gates={1: 0.0})                        # gate 0 would restore 3; the last block keeps its output
    assert trace == [[1.0, 2.0], [2.0, 2000.0]] and after == [[2.0, 3.0], [12.0, 2010.0]]
    trace, after = _toy(P=3, layers=3, gates={1: 0.0, 2: 0.0})
    assert after == [[2.0, 3.0], [12.0, 3.0], [112.0, 3100.0]]


# ------------------------------------------------------------------------------------------------ heads against torch
def test_heads_equal_torch():
    g = torch.Generator().manual_seed(5)
    pooled = torch.randn(3, 5, 64, generator=g, dtype=torch.float64)
    bank = torch.randn(7, 64, generator=g, dtype=torch.float64)
    bank[2] = 0.0
    v = R.video_feature(pooled)
    want = pooled.mean(dim=1)
    want = want / want.norm(p=2, dim=-1, keepdim=True)
    assert torch.equal(v, want)
    cos = torch.nn.CosineSimilarity(dim=1, eps=1e-8)
    s = R.cosine(bank, v)
    for j in range(3):
        assert torch.allclose(s[j], cos(bank, v[j:j + 1]), rtol=0, atol=1e-15)
        assert torch.equal(torch.topk(s[j], 3).indices, torch.topk(cos(bank, v[j:j + 1]), 3).indices)
    assert float(s[:, 2].abs().max()) == 0.0

    D, E = 64, 48
    ad = torch.nn.Sequential(torch.nn.Linear(D, 512), torch.nn.GELU(), torch.nn.Linear(512, D)).double()
    x = torch.randn(4, D, generator=g, dtype=torch.float64)
    sd = {f"rfc.{k}": p for k, p in ad.state_dict().items()}
    assert torch.allclose(R.adapter(sd, x), x + ad(x), rtol=0, atol=1e-13)
    fc = torch.nn.Sequential(torch.nn.Linear(D, 512), torch.nn.GELU(), torch.nn.Linear(512, 256), torch.nn.GELU()).double()
    hard, rough = torch.nn.Linear(256, 1).double(), torch.nn.Linear(256, 1).double()
    sd = {**{f"fc.{k}": p for k, p in fc.state_dict().items()}, **{f"hardness_fc.{k}": p for k, p in hard.state_dict().items()},
          **{f"roughness_fc.{k}": p for k, p in rough.state_dict().items()}}
    assert torch.allclose(R.property_classifier(sd, x), torch.cat([hard(fc(x)), rough(fc(x))], dim=1), rtol=0, atol=1e-13)
    pr = torch.nn.Sequential(torch.nn.Linear(D, E), torch.nn.GELU(), torch.nn.Linear(E, E)).double()
    assert torch.allclose(R.project(pr.state_dict(), x), pr(x), rtol=0, atol=1e-13)


def test_quick_gelu_is_hf_quick_gelu():
    from transformers.activations import ACT2FN
    x = torch.linspace(-12, 12, 97, dtype=torch.float64)
    assert torch.allclose(R.quick_gelu(x), ACT2FN["quick_gelu"](x), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ the bars
def tower_costs():
    cost = {p: 0.0 for p in R.PRECS}
    runs = [(R.tower_sd(name, res, P), R.TOWER_CONFIGS[name]["heads"], P, res, B) for name, res, P in R.tower_cases() for B in R.BATCHES]
    s = R.SPLITK
    runs.append((R.clip_sd(s["hidden"], R.LAYERS, s["inter"], s["res"], s["n_ctx"], s["prompt_depth"]), s["heads"], s["prompt_depth"], s["res"], s["B"]))
    for sd, heads, P, res, B in list(runs[:-1]):                   # the inner block boundaries: the same towers cut after block 1 and block 2
        for m in R.CUTS:
            sd_m, P_m = R.cut(sd, m, P)
            runs.append((sd_m, heads, P_m, res, B))
    for sd, heads, P, res, B in runs:
        px = R.pixels(B, res, seed=res + B)
        _, pool64, every64 = R.forward(sd, px, heads, P)
        for prec in R.PRECS:
            _, pool, every = R.forward(sd, px, heads, P, adt=R.DT[prec], cdt=R.DT[prec], acc=torch.float32)
            cost[prec] = max(cost[prec], R.row_err(pool, pool64), R.row_err(every, every64))
    return cost


def head_cost():
    worst = 0.0
    for b, l, D, Rn, k in R.head_cases():
        pooled, bank = R.head_data(b, l, D, Rn, k)
        v64, v32 = R.video_feature(pooled), R.video_feature(pooled, acc=torch.float32)
        s64, s32 = R.cosine(bank, v64), R.cosine(bank, v32, acc=torch.float32)
        worst = max(worst, R.row_err(v32, v64), float((s32.double() - s64).abs().max()))
    return worst


def _held(measured: float, literal: float):
    """The literal is the measurement rounded up to two digits: never below it, and not more than 15 % above."""
    return measured <= literal <= 1.15 * measured + 1e-12


def test_tower_bars_are_the_measured_costs():
    cost = tower_costs()
    print("tower costs:", {p: f"{v:.3e}" for p, v in cost.items()})
    for prec, v in cost.items():
        assert _held(v, R.COSTS[("tower", prec)]), (prec, v, R.COSTS[("tower", prec)])


def test_head_bar_is_the_measured_cost():
    v = head_cost()
    print(f"head cost (video rows by row_err, sims absolute): {v:.3e}")
    assert _held(v, R.COSTS[("head", "fp32")]), (v, R.COSTS[("head", "fp32")])
    assert R.HEAD_GAP > 100 * v


def api_costs():
    sd, heads, frames, bank = R.api_weights()
    ref = R.api_reference(sd, heads, frames, bank)
    cost = {}
    for mode, (tdt, hdt) in R.API_MODES.items():
        got = R.api_reference(sd, heads, frames, bank, tdt, hdt, acc=torch.float32)
        if hdt is not None:
            got["project"] = R.rnd(got["project"], torch.bfloat16)      # TactileProjector hands its tokens over in the LLM's dtype
        cost[mode] = max(float((got[k].double() - ref[k]).abs().max()) if k == "sims" else R.row_err(got[k], ref[k]) for k in ref)
    return cost


def test_api_bars_are_the_measured_costs():
    cost = api_costs()
    print("api costs:", {p: f"{v:.3e}" for p, v in cost.items()})
    for mode, v in cost.items():
        assert _held(v, R.COSTS[("api", mode)]), (mode, v, R.COSTS[("api", mode)])
