"""What the host drivers size without touching a GPU: `vt_X_num_weights`, `vt_X_workspace_bytes`, the derived weight copies' sizes and the
fused U-Net plan, over handles created on fake non-null pointers (never dereferenced: sizing is host arithmetic).  Shared by
tools/make_golden_host_sizing_parent.py, which recorded tests/golden/g24_host_sizing_parent.json from a build of the commit before the
drivers' carver, element-size table and `create` preamble moved into csrc/vt_host.h, and tests/test_host_sizing_parent.py.

Grid: every precision each `create` admits (the U-Net's checks none: the six (weights, activations) pairs UNetEngine can ask for); B in
{1, 3, 32}; unet T in {8, 16, 48, 68}; dino res in {28, 224} on DINOv2-small, DINOv2-base (the packed fc1 copy) and the SigLIP form of the
descriptor; t5 L in {1, 32, 120}; rdt cases.RDT_TINY, cases.RDT_WIDE and RDT-1B with lang_len in {1, 12, 32}.  With N = horizon + 3 rows per
sample that grid takes both sides of the RDT carver's branches: M = B * N <= 512 (the split-K slabs) at B = 1 and not at B = 32 of the wide
models; B * heads < 512 and N <= 128 (key-range parts) at B = 1 and not at B = 32; and the row-major K | V scratch of a condition too small
for the large-GEMM path (present for both conditions of RDT_TINY and for RDT-1B's language tokens at B = 1, absent in fp32 and at B = 32)."""
import ctypes as C
from collections import OrderedDict

from tests import cases
from vlatouch import _lib as L
from vlatouch import synth

GOLDEN_NAME = "g24_host_sizing_parent.json"
FAKE = 0x1000
BATCHES = (1, 3, 32)
RDT_1B = dict(hidden=2048, depth=28, heads=32, horizon=64, action_dim=128, lang_token_dim=4096, img_token_dim=1152, state_token_dim=128,
              max_lang_cond_len=1024, img_cond_len=4374)
DT = OrderedDict([("fp32", L.F32), ("bf16", L.BF16), ("fp16", L.F16)])


def unet_desc(cdt, adt, dims=(256, 512, 512)):
    d = L.UnetDesc()
    d.nets, d.input_dim, d.input_pad, d.cond_dim, d.dsed, d.n_groups, d.ksize, d.n_levels = 2, 10, 16, 256, 256, 8, 5, len(dims)
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.cdt, d.adt = cdt, adt
    return d


def dino_desc(size, dt):
    c = synth.DINOV2_CONFIGS[size]
    d = L.DinoDesc()
    d.hidden, d.layers, d.heads, d.patch, d.kpad = c["hidden"], c["layers"], c["heads"], 14, 592 if dt == L.F32 else 640
    d.cdt, d.adt, d.eps = dt, dt, 1e-6
    return d


def siglip_desc(dt):
    c = synth.SIGLIP_CONFIGS["tiny"]
    d = L.DinoDesc()
    d.hidden, d.layers, d.heads, d.patch, d.kpad = c["hidden"], c["layers"], c["heads"], 14, 592 if dt == L.F32 else 640
    d.cdt, d.adt, d.eps = dt, dt, 1e-6
    d.no_cls, d.act, d.head_dim, d.mlp_dim, d.out_all = 1, L.ACT_GELU_TANH, 96 if dt == L.F32 else 80, (c["inter"] + 63) // 64 * 64, 1
    d.attn_scale = 72.0 ** -0.5
    return d


def t5_desc(dt):
    c = synth.t5_config("tiny")
    return L.T5Desc(c["vocab_size"], c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"], c["num_layers"], 32, 128, 1e-6, dt, dt)


def lstm_desc(cdt):
    d = L.LstmDesc()
    d.state_dim, d.hidden, d.layers, d.force_dim, d.force_pad, d.in_pad, d.cdt = 10, 256, 2, 3, 16, 144, cdt
    return d


def rdt_desc(cfg, dt):
    d = L.RdtDesc()
    d.hidden, d.depth, d.heads, d.horizon, d.out_dim, d.state_dim = cfg["hidden"], cfg["depth"], cfg["heads"], cfg["horizon"], cfg["action_dim"], cfg["state_token_dim"]
    d.lang_dim, d.img_dim, d.max_lang_len, d.img_len = cfg["lang_token_dim"], cfg["img_token_dim"], cfg["max_lang_cond_len"], cfg["img_cond_len"]
    d.n_lang, d.n_img, d.n_state = 2, 2, 3
    d.cdt = d.adt = dt
    d.rms_mode = L.NORM_RMS_MEANSQ
    return d


def create(prefix, desc, n=None, null_at=None):
    """(return code, handle, n) of vt_<prefix>_create over fake pointers; `n` overrides the count, `null_at` zeroes one entry."""
    lib = L.lib()
    want = getattr(lib, f"vt_{prefix}_num_weights")(C.byref(desc))
    n = want if n is None else n
    w = (C.c_void_p * max(n, 1))(*([FAKE] * max(n, 1)))
    if null_at is not None:
        w[null_at] = 0
    h = C.c_void_p()
    return getattr(lib, f"vt_{prefix}_create")(C.byref(desc), w, n, C.byref(h)), h, want


def _handle(out, key, prefix, desc):
    rc, h, n = create(prefix, desc)
    assert rc == 0, (key, L.lib().vt_last_error().decode())
    out[f"{key}/num_weights"] = n
    return h


def sizing() -> "OrderedDict[str, int]":
    lib = L.lib()
    out = OrderedDict()
    for cn, cdt in (("fp32", L.F32), ("bf16", L.BF16), ("x3", L.F32X3)):
        for an, adt in (("fp32", L.F32), ("bf16", L.BF16)):
            key = f"unet/w_{cn}/a_{an}"
            h = _handle(out, key, "unet", unet_desc(cdt, adt))
            out[f"{key}/fused_bytes"] = lib.vt_unet_fused_bytes(h)
            for B in BATCHES:
                for T in (8, 16, 48, 68):
                    out[f"{key}/B{B}_T{T}/workspace"] = lib.vt_unet_workspace_bytes(h, B, T)
                    out[f"{key}/B{B}_T{T}/fused_plan_10"] = lib.vt_unet_fused_plan_bytes(h, B, T, 10)
            lib.vt_unet_destroy(h)
    for dn, dt in DT.items():
        for name, desc in (("dino_small", dino_desc("small", dt)), ("dino_base", dino_desc("base", dt)), ("siglip_tiny", siglip_desc(dt))):
            key = f"{name}/{dn}"
            h = _handle(out, key, "dino", desc)
            out[f"{key}/packed_bytes"] = lib.vt_dino_packed_bytes(h)
            for B in BATCHES:
                for res in (28, 224):
                    out[f"{key}/B{B}_res{res}/workspace"] = lib.vt_dino_workspace_bytes(h, B, res)
            lib.vt_dino_destroy(h)
    for dn in ("fp32", "bf16"):
        key = f"t5_tiny/{dn}"
        h = _handle(out, key, "t5", t5_desc(DT[dn]))
        for B in BATCHES:
            for Lq in (1, 32, 120):
                out[f"{key}/B{B}_L{Lq}/workspace"] = lib.vt_t5_workspace_bytes(h, B, Lq)
        lib.vt_t5_destroy(h)
    for cn, cdt in (("fp32", L.F32), ("bf16", L.BF16), ("x3", L.F32X3)):
        key = f"lstm_h256/{cn}"
        h = _handle(out, key, "lstm", lstm_desc(cdt))
        for B in BATCHES:
            out[f"{key}/B{B}/workspace"] = lib.vt_lstm_workspace_bytes(h, B)
        lib.vt_lstm_destroy(h)
    for mn, cfg in (("rdt_tiny", cases.RDT_TINY), ("rdt_wide", cases.RDT_WIDE), ("rdt_1b", RDT_1B)):
        for dn, dt in DT.items():
            key = f"{mn}/{dn}"
            h = _handle(out, key, "rdt", rdt_desc(cfg, dt))
            out[f"{key}/packed_bytes"] = lib.vt_rdt_packed_bytes(h)
            for B in BATCHES:
                for Lq in (1, 12, 32):
                    out[f"{key}/B{B}_L{Lq}/workspace"] = lib.vt_rdt_workspace_bytes(h, B, Lq)
            lib.vt_rdt_destroy(h)
    return out
