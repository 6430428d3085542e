"""Octopi's tactile encoder stated in float64 on the CPU (torch-double only): the CLIP vision tower with deep visual prompts and gated prompt
carry-over, and the heads that consume its pooled features.  Written from the description of the computation, not from the reference's code;
nothing here imports the product's code (the synthetic weights come from vlatouch.synth's deterministic rule, as data).

  tokens      patch conv WITHOUT bias, class_embedding prepended, position_embedding added (never interpolated), the n_ctx rows of VPT appended
              after the patch tokens when the prompt depth P != 0, then pre_layrnorm of every row, the prompt rows included
  run_layers  the prompt steps around block i (the tail = the last n_ctx rows of each image), `block` being any function (i, t) -> t:
                i != last           remember `before` = the tail as it arrives
                1 <= i < P          overwrite the tail with VPT_shallow_i (not normed)
                i == P (P >= 1)     drop the tail: 1 + g^2 + n_ctx rows become 1 + g^2 for the remaining blocks
                after the block, 1 <= i < P and i != last:   tail = s * tail + (1 - s) * before,  s = sigmoid(VPT_gamma_i)
              block 0 neither overwrites nor gates; the last block never gates.
  block       pre-LN attention and pre-LN MLP, quick_gelu(x) = x * sigmoid(1.702 x), no LayerScale, LayerNorm eps 1e-5
  forward     -> (last_hidden_state, pooler_output = post_layernorm(row 0), post_layernorm of every row: what the driver's out_all hands out)
  heads       video = mean over the l frames then / its L2 norm (no eps); cosine similarity (eps 1e-8) of a bank against it, top-k;
              Adapter x + rfc(x); PropertyClassifier; project.  GELU is the erf form.

`acc` is the arithmetic type and `adt` / `cdt` the rounding points of the driver's 16-bit modes, exactly as in tests/vit_ref.py (whose `rnd`,
`_ln`, `_attend` and `row_err` are reused): `adt` rounds patches, normalised activations, q | k | v, the packed attention probabilities, the
attention output and the FFN hidden; `cdt` rounds the GEMM weights.  The residual stream, the prompt rows, biases and gains stay unrounded."""
import math

import numpy as np
import torch

from tests.vit_ref import DT, PATCH, PRECS, _attend, _gelu_erf, _ln, rnd, row_err      # noqa: F401  (re-exported for the tests)

EPS = 1e-5


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def depth(layers: int, prompt_depth: int) -> int:
    return layers if prompt_depth == -1 else prompt_depth


def n_layers(sd) -> int:
    L = 0
    while f"encoder.layers.{L}.layer_norm1.weight" in sd:
        L += 1
    return L


def _sd(sd, key, acc):
    return sd[key].detach().to(acc)


# ------------------------------------------------------------------------------------------------ front
def tokens(sd, pixels, P: int, *, adt=None, cdt=None, acc=torch.float64, pre_ln: bool = True) -> torch.Tensor:
    """pixels [Bt, 3, S, S] (CLIP-normalised) -> the rows block 0 receives [Bt, 1 + g^2 (+ n_ctx), D]."""
    x = torch.as_tensor(pixels).to(acc)
    Bt, _, res, _ = x.shape
    g = res // PATCH
    pos = _sd(sd, "embeddings.position_embedding.weight", acc)
    assert pos.shape[0] == 1 + g * g, "res must equal image_size: the position table is never interpolated"
    p = x[:, :, : g * PATCH, : g * PATCH].reshape(Bt, 3, g, PATCH, g, PATCH).permute(0, 2, 4, 1, 3, 5)
    p = rnd(p.reshape(Bt, g * g, 3 * PATCH * PATCH), adt)
    w = rnd(_sd(sd, "embeddings.patch_embedding.weight", acc).reshape(-1, 3 * PATCH * PATCH), cdt)
    t = torch.cat((_sd(sd, "embeddings.class_embedding", acc).expand(Bt, 1, -1), p @ w.T), dim=1) + pos[None]
    if P != 0:
        t = torch.cat((t, _sd(sd, "VPT", acc).expand(Bt, -1, -1)), dim=1)
    if pre_ln:
        t = _ln(t, _sd(sd, "pre_layrnorm.weight", acc), _sd(sd, "pre_layrnorm.bias", acc), EPS)
    return t


# ------------------------------------------------------------------------------------------------ prompt steps
def run_layers(t, layers: int, P: int, n: int, block, shallow, gate, trace=None, after=None):
    """t [Bt, rows, D]; block(i, t) -> t; shallow(i) -> [n, D] for 1 <= i < P; gate(i) -> sigmoid(VPT_gamma_i) for 1 <= i < P, i != last.
    `trace` (a list) receives the rows every block receives, after its prompt steps; `after` the rows it hands on, after its gate step."""
    last = layers - 1
    for i in range(layers):
        before = t[:, t.shape[1] - n:] if (i != last and P != 0 and n) else None
        add = 1 <= i < P and n > 0
        if add:
            t = torch.cat((t[:, : t.shape[1] - n], shallow(i).expand(t.shape[0], -1, -1)), dim=1)
        elif i == P and P >= 1 and n > 0:
            t = t[:, : t.shape[1] - n]
        if trace is not None:
            trace.append(t)
        t = block(i, t)
        if add and i != last:
            s = gate(i)
            t = torch.cat((t[:, : t.shape[1] - n], s * t[:, t.shape[1] - n:] + (1 - s) * before), dim=1)
        if after is not None:
            after.append(t)
    return t


# ------------------------------------------------------------------------------------------------ block
def block(sd, i: int, t, heads: int, *, adt=None, cdt=None, acc=torch.float64):
    G = lambda k: _sd(sd, f"encoder.layers.{i}.{k}", acc)
    lin = lambda x, k: x @ rnd(G(k + ".weight"), cdt).T + G(k + ".bias")
    Bt, N, D = t.shape
    hd = D // heads
    h = rnd(_ln(t, G("layer_norm1.weight"), G("layer_norm1.bias"), EPS), adt)
    q, k, v = (rnd(lin(h, f"self_attn.{n}_proj"), adt).reshape(Bt, N, heads, hd).transpose(1, 2) for n in ("q", "k", "v"))
    a = rnd(_attend(q, k, v, hd, adt).transpose(1, 2).reshape(Bt, N, D), adt)
    t = t + lin(a, "self_attn.out_proj")
    h = rnd(_ln(t, G("layer_norm2.weight"), G("layer_norm2.bias"), EPS), adt)
    return t + lin(rnd(quick_gelu(lin(h, "mlp.fc1")), adt), "mlp.fc2")


def forward(sd, pixels, heads: int, prompt_depth: int, *, adt=None, cdt=None, acc=torch.float64, trace=None):
    """-> (last_hidden_state [Bt, rows, D], pooler_output [Bt, D], post_layernorm of every row [Bt, rows, D])."""
    L = n_layers(sd)
    P = depth(L, prompt_depth)
    n = sd["VPT"].shape[0] if P != 0 else 0
    kw = dict(adt=adt, cdt=cdt, acc=acc)
    t = tokens(sd, pixels, P, **kw)
    t = run_layers(t, L, P, n, lambda i, x: block(sd, i, x, heads, **kw),
                   lambda i: _sd(sd, f"encoder.layers.{i}.VPT_shallow", acc),
                   lambda i: torch.sigmoid(_sd(sd, f"encoder.layers.{i}.VPT_gamma", torch.float32)).to(acc), trace)      # the gate is formed in fp32 at load
    every = _ln(t, _sd(sd, "post_layernorm.weight", acc), _sd(sd, "post_layernorm.bias", acc), EPS)
    return t, every[:, 0], every


# ------------------------------------------------------------------------------------------------ heads
def video_feature(pooled, acc=torch.float64):
    """pooled [b, l, D] -> [b, D]: the mean over the frames, then / its L2 norm (no eps)."""
    v = torch.as_tensor(pooled).to(acc).mean(dim=1)
    return v / v.norm(p=2, dim=-1, keepdim=True)


def cosine(bank, video, acc=torch.float64, eps: float = 1e-8):
    """bank [R, D], video [b, D] -> [b, R]: x . y / (max(|x|, eps) max(|y|, eps)); a zero bank row gives 0."""
    bank, video = torch.as_tensor(bank).to(acc), torch.as_tensor(video).to(acc)
    return (video @ bank.T) / (video.norm(dim=-1).clamp_min(eps)[:, None] * bank.norm(dim=-1).clamp_min(eps)[None])


def mlp_chain(sd, x, keys, *, adt=None, cdt=None, acc=torch.float64, act_last: bool = False):
    """Linear, GELU(erf), Linear, ... over `keys` (module paths whose .weight / .bias are read); the hidden activations are stored in adt."""
    x = rnd(torch.as_tensor(x).to(acc), adt)
    for j, k in enumerate(keys):
        x = x @ rnd(_sd(sd, k + ".weight", acc), cdt).T + _sd(sd, k + ".bias", acc)
        if j < len(keys) - 1 or act_last:
            x = rnd(_gelu_erf(x), adt)
    return x


def adapter(sd, x, **kw):
    """x + rfc(x), rfc = Linear, GELU, Linear (no `align`: input and output sizes agree)."""
    return torch.as_tensor(x).to(kw.get("acc", torch.float64)) + mlp_chain(sd, x, ("rfc.0", "rfc.2"), **kw)


def property_classifier(sd, x, **kw):
    """fc = Linear, GELU, Linear, GELU; then [hardness_fc | roughness_fc] -> [B, 2]."""
    h = mlp_chain(sd, x, ("fc.0", "fc.2"), act_last=True, **kw)
    acc, cdt = kw.get("acc", torch.float64), kw.get("cdt")
    outs = [h @ rnd(_sd(sd, f"{n}.weight", acc), cdt).T + _sd(sd, f"{n}.bias", acc) for n in ("hardness_fc", "roughness_fc")]
    return torch.cat(outs, dim=-1)


def project(sd, x, **kw):
    return mlp_chain(sd, x, ("0", "2"), **kw)


# ------------------------------------------------------------------------------------------------ synthetic weights, frames
def clip_sd(hidden: int, layers: int, inter: int, image_size: int, n_ctx: int, prompt_depth: int, gammas=(-4.0, 0.0, 5.0), salt: str = ""):
    """Synthetic tower weights; VPT_gamma_i cycles through `gammas` (sigmoid = 0.018, 0.5, 0.993) so the gate's both ends and its middle are met.
    VPT and VPT_shallow are scaled up to the size of the normalised rows beside them (the rule's 1/sqrt(D) would make the gate invisible)."""
    from tests import cases
    from vlatouch import synth
    sd = cases.sd_torch(synth.clip_shapes(hidden, layers, inter, image_size=image_size, n_ctx=n_ctx, prompt_depth=prompt_depth),
                        prefix=f"clip-test-{hidden}-{layers}-{n_ctx}-{prompt_depth}{salt}.")
    for k in list(sd):
        if k.endswith("VPT_gamma"):
            sd[k] = torch.tensor(float(gammas[int(k.split(".")[2]) % len(gammas)]))
        elif k.endswith("VPT") or k.endswith("VPT_shallow"):
            sd[k] = sd[k] * math.sqrt(hidden)
    return sd


def pixels(B: int, res: int, seed: int) -> np.ndarray:
    """What get_frames hands the encoder: (u8 / 255 - mean) / std with CLIP's statistics, fp32."""
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.integers(0, 256, (B, 3, res, res)).astype(np.float64) / 255.0
    mean, std = np.array((0.48145466, 0.4578275, 0.40821073)), np.array((0.26862954, 0.26130258, 0.27577711))
    return ((u - mean.reshape(1, 3, 1, 1)) / std.reshape(1, 3, 1, 1)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the tower grid and its bars
# name -> hidden, heads, inter, n_ctx; every config has 3 layers and runs res in RES, P in DEPTHS (3 = -1 = to the end), Bt in BATCHES
TOWER_CONFIGS = {f"d{D}_n{n}": dict(hidden=D, heads=D // 64, inter=4 * D, n_ctx=n) for D in (64, 128) for n in (0, 3, 8)}
GAMMAS = (-4.0, 0.0, 5.0)
CUTS = (1, 2)                                                         # the towers cut after block 1 and after block 2: the inner block boundaries
LAYERS = 3
RES = (28, 42)
DEPTHS = (0, 1, 2, -1)
BATCHES = (1, 3)
SPLITK = dict(hidden=512, heads=8, inter=2048, n_ctx=3, res=42, prompt_depth=2, B=7)      # Bt (N + n) = 7 x 13 = 91 > 64 rows: split-K fc2 under quick-GELU


def tower_cases():
    out = []
    for name, c in TOWER_CONFIGS.items():
        for res in RES:
            for P in DEPTHS:
                if c["n_ctx"] == 0 and P != 0:
                    continue                                      # no prompt rows: only the plain tower
                out.append((name, res, P))
    return out


def tower_sd(name: str, res: int, P: int):
    """The gammas are rotated from case to case, so the one gate a 3-layer tower reads (block 1's) takes each of -4, 0 and 5 over the grid."""
    c = TOWER_CONFIGS[name]
    rot = (res // PATCH + c["n_ctx"] + P) % 3
    return clip_sd(c["hidden"], LAYERS, c["inter"], res, c["n_ctx"], P if c["n_ctx"] else 0, gammas=GAMMAS[rot:] + GAMMAS[:rot])


def cut(sd, m: int, prompt_depth: int):
    """The tower's first m blocks as a tower of its own -> (weights, its prompt depth).  What it puts out (every row through post_layernorm)
    is the residual stream at the boundary between block m-1 and block m of the whole tower, on every row that boundary hands on: its own
    last block does not gate, and the whole tower's gate there touches only rows the next block overwrites or drops."""
    L = n_layers(sd)
    d = depth(L, prompt_depth)
    keep = {k: v for k, v in sd.items() if not k.startswith("encoder.layers.") or int(k.split(".")[2]) < m}
    return keep, min(d, m)


# ------------------------------------------------------------------------------------------------ the tactile-head grid
HEAD_B, HEAD_L, HEAD_D = (1, 3), (1, 5, 10), (64, 1024)
HEAD_RK = ((1, 1), (7, 1), (7, 3), (300, 1), (300, 3), (300, 16))      # (R, k) of R in {1, 7, 300} x k in {1, 3, 16} with k <= R
HEAD_GAP = 1e-4                                                       # smallest distance between neighbours among a video's k + 1 largest similarities


def head_cases():
    return [(b, l, D, R, k) for b in HEAD_B for l in HEAD_L for D in HEAD_D for R, k in HEAD_RK]


def head_data(b: int, l: int, D: int, R: int, k: int):
    """pooled [b, l, D] and a bank [R, D], fp32: drawn again (next seed) until every video's k + 1 largest float64 similarities lie at least
    HEAD_GAP apart, so the order of the top k is decided far above fp32 rounding and no case can hide behind a tie."""
    seed = 7919 * b + 104729 * l + 31 * D + 17 * R + k
    for attempt in range(200):
        g = np.random.Generator(np.random.PCG64(seed + 1_000_003 * attempt))
        pooled = (g.standard_normal((b, l, D)) + 0.5).astype(np.float32)
        bank = (g.standard_normal((R, D)) * g.uniform(0.5, 2.0, (R, 1))).astype(np.float32)
        s = cosine(bank, video_feature(pooled)).sort(dim=-1, descending=True).values[:, : k + 1]
        if s.shape[1] < 2 or float((s[:, :-1] - s[:, 1:]).min()) >= HEAD_GAP:
            return pooled, bank
    raise AssertionError(("no bank with the gap found", b, l, D, R, k))


# ------------------------------------------------------------------------------------------------ the mirror end to end
API = dict(hidden=128, heads=2, inter=512, layers=3, image_size=28, n_ctx=3, prompt_depth=2, llm_dim=192, b=2, l=3, R=9, k=3)
# mirror precision -> (tower rounding, head rounding): "bf16" stores the tower in IEEE fp16 and the heads in bf16; after the range guard's
# fall-back the tower is bf16 too
API_MODES = {"fp32": (None, None), "fp16": (torch.float16, torch.bfloat16), "bf16": (torch.bfloat16, torch.bfloat16)}


def api_weights():
    """(tower weights, {file: head weights}, frames [b, l, 3, S, S], bank [R, D])."""
    from tests import cases
    from vlatouch import synth
    a = API
    sd = clip_sd(a["hidden"], a["layers"], a["inter"], a["image_size"], a["n_ctx"], a["prompt_depth"], salt="api")
    hs = synth.tactile_head_shapes(a["hidden"], a["llm_dim"])
    heads = {k: cases.sd_torch(v, prefix=f"clip-api-{k}.") for k, v in hs.items()}
    frames = torch.from_numpy(pixels(a["b"] * a["l"], a["image_size"], seed=77)).reshape(a["b"], a["l"], 3, a["image_size"], a["image_size"])
    return sd, heads, frames, api_bank(sd, frames)


API_GAP = 0.07                                                       # between neighbours among a video's k + 1 largest similarities: above 2 x the widest api bar


def api_bank(sd, frames):
    """A bank [R, D] whose similarities to the videos of `frames` are far apart: row r = cos(t_r) v0 + sin(t_r) n_r with v0 the float64 feature
    of video 0, n_r unit noise orthogonal to every video feature, and cos(t_r) = 0.95 - 0.1 rank(r) under a fixed permutation.  Video 0 sees
    steps of 0.1, video j steps of 0.1 (v0 . vj)."""
    a = API
    b, l = frames.shape[:2]
    feats = forward(sd, frames.reshape(b * l, *frames.shape[2:]), a["heads"], a["prompt_depth"])[1].reshape(b, l, -1)
    v = video_feature(feats)                                         # [b, D] float64, unit rows
    g = np.random.Generator(np.random.PCG64(78))
    noise = torch.from_numpy(g.standard_normal((a["R"], a["hidden"])))
    q, _ = torch.linalg.qr(v.T)                                      # an orthonormal basis of the videos' span
    noise = noise - (noise @ q) @ q.T
    noise = noise / noise.norm(dim=-1, keepdim=True)
    rank = torch.from_numpy(g.permutation(a["R"]))
    c = 0.95 - 0.1 * rank.double()
    return (c[:, None] * v[0][None] + torch.sqrt(1 - c * c)[:, None] * noise).float()


def api_reference(sd, heads, frames, bank, tower_dt=None, head_dt=None, acc=torch.float64):
    """What the mirror's classes return, as the statement: frame features, video feature, similarities, Adapter, PropertyClassifier, project."""
    a = API
    b, l = frames.shape[:2]
    feats = forward(sd, frames.reshape(b * l, *frames.shape[2:]), a["heads"], a["prompt_depth"], adt=tower_dt, cdt=tower_dt, acc=acc)[1].reshape(b, l, -1)
    if acc != torch.float64:
        feats = feats.float()                                        # the tower hands fp32 features to every head
    kw = dict(adt=head_dt, cdt=head_dt, acc=acc)
    video = video_feature(feats, acc)
    flat = feats.reshape(b * l, -1)
    return dict(feats=feats, video=video, sims=cosine(bank, video, acc), adapter=adapter(heads["adapter"], flat, **kw),
                prop=property_classifier(heads["property_classifier"], flat, **kw), project=project(heads["project"], flat, **kw))


# The bars: 3 x the largest cost of a group, as in tests/vit_ref.py.  (tower: the whole towers and their CUTS.)  A cost is the distance (row_err) between the float64 statement and the
# statement in fp32 arithmetic (fp32) or with the 16-bit rounding points and fp32 arithmetic (bf16, fp16), the largest over the group's cases
# and over pooled / every-token outputs; tests/test_clip_ref_host.py measures the costs on the CPU and holds these literals to them.
#   tower = tower_cases() x BATCHES and the SPLITK case;  head = the tactile-head grid of tests/test_gpu_tactile_head.py (video and sims, fp32)
#   api = the six outputs of api_reference at API, by mirror mode (API_MODES); `sims` absolutely, `project` with its output stored in bf16
COSTS = {
    ("tower", "fp32"): 1.4e-6, ("tower", "bf16"): 1.1e-2, ("tower", "fp16"): 1.2e-3,
    ("head", "fp32"): 2.0e-7,
    ("api", "fp32"): 9.6e-7, ("api", "fp16"): 6.3e-3, ("api", "bf16"): 1.0e-2,
}
BARS = {k: 3.0 * v for k, v in COSTS.items()}
