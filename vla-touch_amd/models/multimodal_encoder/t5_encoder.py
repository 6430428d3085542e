"""Mirror of models/multimodal_encoder/t5_encoder.py (T5Embedder) of the reference: the T5 v1.1 text encoder that turns instructions into
RDT's lang_tokens, used by scripts/encode_lang*.py and data/franka_data/2_precompute_instruction.py.  Same constructor and
`get_text_embeddings(texts) -> (embs, attention_mask)`; `tokenizer` and `model` are the same two attributes the reference scripts use.
The encoder runs in the HIP engine (vlatouch.t5.T5Engine).  There is no hub access: the checkpoint comes from `state_dict=` + `config=`,
a local HF directory, or the local HF cache (vlatouch.t5.load_t5_encoder raises FileNotFoundError otherwise).  The tokenizer
(transformers.AutoTokenizer, local files only) is host-side string processing, loaded on first use; `tokenizer=` replaces it."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from vlatouch import t5 as T5


class _Output(dict):
    """HF BaseModelOutput stand-in: readable as `.last_hidden_state` and as `["last_hidden_state"]`."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


class T5EncoderHIP:
    """`model(ids)` / `model(input_ids=, attention_mask=)` -> output with last_hidden_state [B, L, d_model] in `torch_dtype`."""

    def __init__(self, engine: T5.T5Engine, torch_dtype=torch.bfloat16):
        self.engine = engine
        self.dtype = torch_dtype

    def eval(self):
        return self

    @property
    def device(self):
        return self.engine.device

    @property
    def config(self):
        import types
        return types.SimpleNamespace(**self.engine.cfg)

    @torch.no_grad()
    def __call__(self, input_ids=None, attention_mask=None, **_):
        out = self.engine.forward(input_ids, attention_mask, out_dtype=self.dtype)
        return _Output(last_hidden_state=out)

    forward = __call__


class T5Embedder:
    available_models = ["google/t5-v1_1-xxl"]

    def __init__(self, device, from_pretrained=None, *, cache_dir=None, hf_token=None, use_text_preprocessing=True, t5_model_kwargs=None,
                 torch_dtype=None, use_offload_folder=None, model_max_length=120, local_files_only=False,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, config=None, tokenizer=None):
        self.device = torch.device(device)
        self.torch_dtype = torch_dtype or torch.bfloat16
        self.cache_dir = cache_dir
        self.use_text_preprocessing = use_text_preprocessing
        self.hf_token = hf_token
        self.model_max_length = model_max_length
        self.from_pretrained = from_pretrained
        # use_offload_folder / t5_model_kwargs / local_files_only: accepted for the reference's signature; the whole encoder lives on the card
        # and nothing is ever fetched
        precision = "fp32" if self.torch_dtype == torch.float32 else "bf16"
        if state_dict is not None:
            if config is None:
                raise ValueError("T5Embedder: state_dict= needs config= (an HF T5Config or its dict)")
            engine = T5.T5Engine(state_dict, config, precision=precision, device=self.device)
        else:
            if from_pretrained is None:
                raise ValueError("T5Embedder: pass from_pretrained (a local directory or a cached repo id) or state_dict= + config=")
            engine = T5.load_t5_encoder(from_pretrained, precision=precision, device=self.device, cache_dir=cache_dir)
        self.model = T5EncoderHIP(engine, self.torch_dtype)
        self._tokenizer = tokenizer

    @property
    def tokenizer(self):
        if self._tokenizer is None:
            from transformers import AutoTokenizer
            path = T5.resolve_local(self.from_pretrained, self.cache_dir)
            self._tokenizer = AutoTokenizer.from_pretrained(path, model_max_length=self.model_max_length, local_files_only=True)
        return self._tokenizer

    @tokenizer.setter
    def tokenizer(self, tok):
        self._tokenizer = tok

    def get_text_embeddings(self, texts):
        text_tokens_and_mask = self.tokenizer(texts, max_length=self.model_max_length, padding="longest", truncation=True,
                                              return_attention_mask=True, add_special_tokens=True, return_tensors="pt")
        input_ids = text_tokens_and_mask["input_ids"].to(self.device)
        attention_mask = text_tokens_and_mask["attention_mask"].to(self.device)
        with torch.no_grad():
            text_encoder_embs = self.model(input_ids=input_ids, attention_mask=attention_mask)["last_hidden_state"].detach()
        return text_encoder_embs, attention_mask
