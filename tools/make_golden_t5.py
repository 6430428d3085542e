#!/usr/bin/env python
"""G15: instruction embeddings of the REFERENCE's T5Embedder, imported read-only in this container.

    python tools/make_golden_t5.py      # writes tests/golden/g15_t5.npz

models/multimodal_encoder/t5_encoder.py::T5Embedder is instantiated with `T5EncoderModel.from_pretrained` patched to build HF's
module from an explicit T5Config (synth.T5_CONFIGS) holding the build's deterministic synthetic weights (tests/t5_ref.py::t5_sd), and
`AutoTokenizer.from_pretrained` patched to a word-hash tokenizer stand-in (no hub access; the ids and masks are stored, so tests
need no tokenizer).  `get_text_embeddings(texts)` (padding="longest") is what is stored: once with the model in float64, rounded to fp32 on
storage (`*_out`: the exact answer to 3e-7; HF's own fp32 run is up to 4e-5 away from it — fp32's own error on this unscaled encoder, which
depends on the BLAS summation order of the machine), once in bf16 (HF's own bf16 execution, kept for the record), plus the relative-position
bucket table."""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import cases  # noqa: E402
from tests import t5_ref  # noqa: E402
import ref_import  # noqa: E402
from vlatouch import synth  # noqa: E402
from vlatouch.t5 import bucket_table  # noqa: E402

torch.set_grad_enabled(False)
ref_import.setup()
import transformers  # noqa: E402
from transformers import T5Config, T5EncoderModel  # noqa: E402

sys.path.insert(0, os.path.join(ref_import.REF, "VLA"))
CUR = {}


def fake_model_from_pretrained(name, *a, **k):
    c = synth.t5_config(CUR["name"])
    cfg = T5Config(**{kk: v for kk, v in c.items() if kk not in ("is_gated_act", "dense_act_fn")}, dropout_rate=0.0, is_encoder_decoder=False,
                   use_cache=False)
    m = T5EncoderModel(cfg).eval()
    sd = t5_ref.t5_sd(CUR["name"])
    full = m.state_dict()
    for kk in full:
        src = "shared.weight" if kk == "encoder.embed_tokens.weight" else kk
        full[kk] = sd[src]
    m.load_state_dict(full)
    return m.to(k.get("torch_dtype") or torch.float32)


class WordHashTokenizer:
    """Stand-in for AutoTokenizer: every whitespace word -> 2 + sha256(word) mod (vocab - 2), then </s> = 1; pad = 0, right padding."""

    def __init__(self, vocab):
        self.vocab = vocab

    def __call__(self, texts, max_length=None, padding="longest", truncation=True, return_attention_mask=True, add_special_tokens=True,
                 return_tensors="pt"):
        texts = [texts] if isinstance(texts, str) else list(texts)
        seqs = []
        for t in texts:
            s = [2 + int(hashlib.sha256(w.encode()).hexdigest(), 16) % (self.vocab - 2) for w in t.split()]
            if truncation and max_length:
                s = s[:max_length - 1]
            seqs.append(s + [1])
        n = max(len(s) for s in seqs)
        ids = torch.zeros(len(seqs), n, dtype=torch.long)
        mask = torch.zeros(len(seqs), n, dtype=torch.long)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.tensor(s)
            mask[i, :len(s)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def words(n, seed):
    return " ".join(f"w{seed}_{i}" for i in range(n))


T5EncoderModel.from_pretrained = staticmethod(fake_model_from_pretrained)
transformers.AutoTokenizer.from_pretrained = staticmethod(lambda *a, **k: WordHashTokenizer(synth.T5_CONFIGS[CUR["name"]]["vocab_size"]))
from models.multimodal_encoder import t5_encoder  # noqa: E402  (the reference's file)

CASES = {
    "tiny_b3": ("tiny", [words(36, 1), words(4, 2), ""]),                 # lengths 37, 5, 1 under padding="longest"
    "small_b2": ("small_like", [words(18, 3), words(11, 4)]),             # inner 384 != d_model 512
    "tiny_l200": ("tiny", [words(199, 5), words(142, 6)]),                # past max_distance 128
}
out = {"buckets": bucket_table(32, 128)}
for case, (name, texts) in CASES.items():
    CUR["name"] = name
    for prec, dt in (("fp64", torch.float64), ("bf16", torch.bfloat16)):
        emb = t5_encoder.T5Embedder(device="cpu", from_pretrained="google/t5-v1_1-xxl", torch_dtype=dt, model_max_length=1024)
        e, mask = emb.get_text_embeddings(texts)
        ids = emb.tokenizer(texts, max_length=1024, padding="longest")["input_ids"]
        if prec == "fp64":
            out[f"{case}_ids"] = ids.numpy().astype(np.int32)
            out[f"{case}_mask"] = mask.numpy().astype(np.uint8)
            out[f"{case}_out"] = e.float().numpy()
        else:
            out[f"{case}_out_hf_bf16"] = e.contiguous().view(torch.int16).numpy().view(np.uint16)   # HF's own bf16 run, raw bf16 bits, for the record
        print(case, prec, tuple(e.shape), float(e.float().abs().max()))
np.savez_compressed(os.path.join(cases.GOLDEN, "g15_t5.npz"), **out)
print("done", os.path.getsize(os.path.join(cases.GOLDEN, "g15_t5.npz")))
