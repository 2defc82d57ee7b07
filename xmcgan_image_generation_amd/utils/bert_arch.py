"""Architecture of the caption encoder: ``bert_en_uncased_L-12_H-768_A-12`` as the reference uses it
(``preprocess_data.py:29-33,55``): embeddings + LayerNorm, then ``layers`` post-LN transformer blocks; the sequence output is
what the reference stores, the pooler is never read.

Parameters are a flat dict of NumPy arrays under the state-dict names of a Hugging Face ``BertModel`` (dense weights
``(out, in)``), the layout a user gets from one ``np.savez`` of ``model.state_dict()``.
"""
from __future__ import annotations

from typing import Dict, NamedTuple

import numpy as np

HEAD_DIM = 64
LN_EPS = 1e-12
MAX_ATTENTION_T = 32          # xmc_bert_attention's domain
MAX_ATTENTION_T_LONG = 64     # xmc_bert_attention_long's (Localized Narratives captions)

EMBEDDING_KEYS = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                  "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias")
LAYER_DENSE = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
               "intermediate.dense", "output.dense")
LAYER_NORMS = ("attention.output.LayerNorm", "output.LayerNorm")


class BertDims(NamedTuple):
    layers: int
    hidden: int
    ffn: int
    vocab: int
    max_pos: int
    heads: int


def layer_keys(i: int):
    """every key of layer ``i``"""
    pre = f"encoder.layer.{i}."
    return [pre + n + s for n in LAYER_DENSE + LAYER_NORMS for s in (".weight", ".bias")]


def expected_shapes(dims: BertDims) -> Dict[str, tuple]:
    h, f = dims.hidden, dims.ffn
    out = {EMBEDDING_KEYS[0]: (dims.vocab, h), EMBEDDING_KEYS[1]: (dims.max_pos, h), EMBEDDING_KEYS[2]: (None, h),
           EMBEDDING_KEYS[3]: (h,), EMBEDDING_KEYS[4]: (h,)}
    for i in range(dims.layers):
        pre = f"encoder.layer.{i}."
        for n in LAYER_DENSE:
            o, k = (f, h) if n == "intermediate.dense" else (h, f) if n == "output.dense" else (h, h)
            out[pre + n + ".weight"], out[pre + n + ".bias"] = (o, k), (o,)
        for n in LAYER_NORMS:
            out[pre + n + ".weight"], out[pre + n + ".bias"] = (h,), (h,)
    return out


def init_bert(seed: int, layers: int = 12, hidden: int = 768, ffn: int = 3072, vocab: int = 30522, max_pos: int = 512,
              type_vocab: int = 2) -> Dict[str, np.ndarray]:
    """Random float32 weights (tests and benchmarks; embeddings from them mean nothing).  Scales keep every activation O(1):
    dense weights N(0, 1 / in), biases and LayerNorm offsets N(0, 0.1^2), LayerNorm gains 1 + N(0, 0.1^2), tables N(0, 1)."""
    assert hidden % HEAD_DIM == 0
    rng = np.random.default_rng(seed)
    dims = BertDims(layers, hidden, ffn, vocab, max_pos, hidden // HEAD_DIM)
    p = {}
    for key, shape in expected_shapes(dims).items():
        shape = tuple(type_vocab if s is None else s for s in shape)
        if key.endswith("LayerNorm.weight"):
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        elif key.endswith(".bias"):
            a = 0.1 * rng.standard_normal(shape)
        elif key.startswith("embeddings."):
            a = rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / np.sqrt(shape[1])
        p[key] = a.astype(np.float32)
    return p
