"""Caption encoder: text in, the three tensors the generator is conditioned on out (the reference's
``preprocess_data.py:36-58``, ``get_bert_for_captions``: WordPiece ids -> ``bert_en_uncased_L-12_H-768_A-12`` -> sequence
output, its masked-length mean and the lengths).

``bert_model`` reads the weights: an ``.npz`` whose keys are the state-dict names of a Hugging Face ``BertModel`` (one
``np.savez(path, **{k: v.numpy() for k, v in model.state_dict().items()})``).  Nothing is downloaded.
``BertEncoder`` is the network on the HIP kernels of ``csrc/bert.hip`` and ``ops.gemm``; ``TextEncoder`` is the public
interface (tokenizer + network + the reference's return convention).
"""
from __future__ import annotations

import os
import re
import warnings

import numpy as np
import torch

from . import bert_arch as arch
from ..libml import wordpiece


def infer_dims(params) -> arch.BertDims:
    """layer count from the keys, hidden size from the word table, heads = hidden // 64"""
    word = arch.EMBEDDING_KEYS[0]
    if word not in params:
        raise ValueError(f"BERT checkpoint: missing key {word}")
    w = np.asarray(params[word])
    if w.ndim != 2 or w.shape[1] % arch.HEAD_DIM:
        raise ValueError(f"BERT checkpoint: {word} has shape {w.shape}; expected (vocab, hidden) with hidden a multiple of 64")
    idx = [int(m.group(1)) for k in params for m in [re.match(r"encoder\.layer\.(\d+)\.", k)] if m]
    if not idx:
        raise ValueError("BERT checkpoint: missing key encoder.layer.0.attention.self.query.weight")
    ffn_key = "encoder.layer.0.intermediate.dense.weight"
    if ffn_key not in params:
        raise ValueError(f"BERT checkpoint: missing key {ffn_key}")
    pos = arch.EMBEDDING_KEYS[1]
    if pos not in params:
        raise ValueError(f"BERT checkpoint: missing key {pos}")
    return arch.BertDims(max(idx) + 1, int(w.shape[1]), int(np.asarray(params[ffn_key]).shape[0]), int(w.shape[0]),
                         int(np.asarray(params[pos]).shape[0]), int(w.shape[1]) // arch.HEAD_DIM)


def validate(params) -> arch.BertDims:
    """every key present and of its shape, else ``ValueError`` naming the key"""
    dims = infer_dims(params)
    for key, shape in arch.expected_shapes(dims).items():
        if key not in params:
            raise ValueError(f"BERT checkpoint: missing key {key}")
        got = tuple(np.asarray(params[key]).shape)
        ok = len(got) == len(shape) and all(s is None and g >= 1 or s == g for s, g in zip(shape, got))
        if not ok:
            want = tuple("n" if s is None else s for s in shape)
            raise ValueError(f"BERT checkpoint: {key} has shape {got}, expected {want}")
    return dims


def bert_model(checkpoint_path, seed: int = 0, **init_kw):
    """-> dict of float32 NumPy arrays under the Hugging Face ``BertModel`` state-dict names (``pooler.*`` and buffers such
    as ``embeddings.position_ids`` are ignored).  ``checkpoint_path``: an ``.npz`` (read with ``allow_pickle=False``); a path
    that does not exist raises ``FileNotFoundError``, a missing or mis-shaped key ``ValueError`` naming it.  ``None`` is the
    explicit opt-in to ``bert_arch.init_bert(seed, **init_kw)`` random weights (tests, benchmarks)."""
    if checkpoint_path is None:
        return arch.init_bert(seed, **init_kw)
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"{checkpoint_path}: BERT checkpoint not found (np.savez the state_dict() of a Hugging Face "
                                f"BertModel of bert-base-uncased; None = random weights)")
    with np.load(checkpoint_path, allow_pickle=False) as z:
        raw = {k: z[k] for k in z.files if not k.startswith("pooler.")}
    dims = validate(raw)
    keep = arch.expected_shapes(dims)
    return {k: np.ascontiguousarray(raw[k], dtype=np.float32) for k in keep}


def check_ids(ids, max_len, vocab, max_pos, max_t=arch.MAX_ATTENTION_T):
    """host-side domain check of a batch of id rows; raises ``ValueError`` before anything is launched.  ``max_t``: the longest
    row the caller's attention kernel serves (``MAX_ATTENTION_T_LONG`` where ``xmc_bert_attention_long`` is behind it)"""
    ids, max_len = np.asarray(ids), np.asarray(max_len)
    if ids.ndim != 2 or max_len.shape != (ids.shape[0],):
        raise ValueError(f"ids must be (N, T) and max_len (N,), got {ids.shape} and {max_len.shape}")
    t = ids.shape[1]
    if not 2 <= t <= min(max_t, max_pos):
        raise ValueError(f"max_text_length {t} outside 2..{min(max_t, max_pos)}")
    if ids.size and (ids.min() < 0 or ids.max() >= vocab):
        bad = ids[(ids < 0) | (ids >= vocab)]
        raise ValueError(f"token id {int(bad[0])} outside the vocabulary 0..{vocab - 1}")
    if max_len.size and (max_len.min() < 2 or max_len.max() > t):
        raise ValueError(f"max_len must lie in 2..{t}")


class BertEncoder:
    """``(ids (N, T) int, max_len (N,) int) -> embedding (N, T, hidden) float32`` (NumPy) on the HIP kernels.

    Per layer: GEMM (q | k | v as one hidden -> 3 hidden product), ``xmc_bert_attention`` (``_long`` for 32 < T <= 64), GEMM, ``xmc_bias_residual_ln``,
    GEMM, ``xmc_bias_gelu``, GEMM, ``xmc_bias_residual_ln``; ``xmc_bert_embed_ln`` in front.  The GEMMs get no split-K
    workspace and every other kernel works row by row or caption by caption, so a caption's embedding does not depend on
    what shares its chunk.  Captions are processed ``chunk`` at a time; the activation buffers are allocated once per chunk
    size and reused.  ``fast=True`` (opt-in) rounds the GEMM operands to bf16 for the bf16 MFMA (``ops.gemm(fast=True)``: the
    operator table must be the bf16 one); everything else stays float32."""

    def __init__(self, ops, params, fast=False, chunk=1024):
        if fast and ops.dtype != torch.bfloat16:
            raise ValueError("fast=True needs HipOps(dtype=torch.bfloat16): ops.gemm(fast=True) is the float32 GEMM otherwise")
        self.ops, self.fast, self.chunk = ops, bool(fast), int(chunk)
        self.dims = validate(params)
        self.launches = 0                            # kernels launched so far (tests: a rejected batch launches none)
        dev = ops.device

        def up(a):
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        self.emb = [up(params[k]) for k in arch.EMBEDDING_KEYS]
        self.layers = []
        for i in range(self.dims.layers):
            pre = f"encoder.layer.{i}."
            qkv = [pre + f"attention.self.{n}" for n in ("query", "key", "value")]
            layer = {"w_qkv": up(np.concatenate([params[k + ".weight"] for k in qkv], axis=0)),
                     "b_qkv": up(np.concatenate([params[k + ".bias"] for k in qkv], axis=0))}
            for short, name in (("ao", "attention.output.dense"), ("ln1", "attention.output.LayerNorm"),
                                ("ff1", "intermediate.dense"), ("ff2", "output.dense"), ("ln2", "output.LayerNorm")):
                layer["w_" + short], layer["b_" + short] = up(params[pre + name + ".weight"]), up(params[pre + name + ".bias"])
            self.layers.append(layer)
        self._bufs = {}

    def buffers(self, n, t):
        key = (n, t)
        b = self._bufs.get(key)
        if b is None:
            ops, d = self.ops, self.dims
            rows, f32 = n * t, torch.float32
            b = {"ids": ops.empty((rows,), torch.int32), "max_len": ops.empty((n,), torch.int32),
                 "h": ops.empty((rows, d.hidden), f32), "h1": ops.empty((rows, d.hidden), f32),
                 "proj": ops.empty((rows, d.hidden), f32), "ctx": ops.empty((rows, d.hidden), f32),
                 "qkv": ops.empty((rows, 3 * d.hidden), f32), "ff": ops.empty((rows, d.ffn), f32),
                 "sentence": ops.empty((n, d.hidden), f32)}
            self._bufs[key] = b
        return b

    def _gemm(self, x, w, out):
        self.launches += 1
        return self.ops.gemm(x, w, tb=True, out=out, fast=self.fast, split_k=False)

    def forward_device(self, ids, max_len):
        """one chunk -> (embedding (n * t, hidden), sentence (n, hidden), max_len int32 (n,)): float32 device tensors owned by
        this object, valid until the next call of the same shape"""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        ml = np.ascontiguousarray(max_len, dtype=np.int64)
        check_ids(ids, ml, self.dims.vocab, self.dims.max_pos, max_t=arch.MAX_ATTENTION_T_LONG)
        ops, (n, t) = self.ops, ids.shape
        b = self.buffers(n, t)
        ml32 = ml.astype(np.int32)
        b["ids"].copy_(torch.as_tensor(ids.astype(np.int32).reshape(-1)))
        b["max_len"].copy_(torch.as_tensor(ml32))
        word, pos, typ, g, be = self.emb
        h, h1 = b["h"], b["h1"]
        attention = ops.bert_attention if t <= arch.MAX_ATTENTION_T else ops.bert_attention_long     # 64-token narratives
        ops.bert_embed_ln(b["ids"], word, pos, typ, g, be, h, t, eps=arch.LN_EPS)
        self.launches += 1
        for L in self.layers:
            self._gemm(h, L["w_qkv"], b["qkv"])
            attention(b["qkv"], L["b_qkv"], b["max_len"], ml32, b["ctx"], t)
            self._gemm(b["ctx"], L["w_ao"], b["proj"])
            ops.bias_residual_ln(b["proj"], L["b_ao"], h, L["w_ln1"], L["b_ln1"], out=h1, eps=arch.LN_EPS)
            self._gemm(h1, L["w_ff1"], b["ff"])
            ops.bias_gelu(b["ff"], L["b_ff1"], out=b["ff"])
            self._gemm(b["ff"], L["w_ff2"], b["proj"])
            ops.bias_residual_ln(b["proj"], L["b_ff2"], h1, L["w_ln2"], L["b_ln2"], out=h, eps=arch.LN_EPS)
            self.launches += 4
        ops.bert_sentence(h, b["max_len"], t, out=b["sentence"])
        self.launches += 1
        return h, b["sentence"], b["max_len"]

    def encode(self, ids, max_len):
        """-> (embedding (N, T, hidden), sentence_embedding (N, hidden)) float32 NumPy, chunk by chunk"""
        ids, max_len = np.asarray(ids), np.asarray(max_len)
        check_ids(ids, max_len, self.dims.vocab, self.dims.max_pos,          # the WHOLE list first: nothing runs on a bad one
                  max_t=arch.MAX_ATTENTION_T_LONG)
        n, t = ids.shape
        emb = np.empty((n, t, self.dims.hidden), np.float32)
        sent = np.empty((n, self.dims.hidden), np.float32)
        for lo in range(0, n, self.chunk):
            hi = min(lo + self.chunk, n)
            e, s, _ = self.forward_device(ids[lo:hi], max_len[lo:hi])
            emb[lo:hi] = e.cpu().numpy().reshape(hi - lo, t, -1)
            sent[lo:hi] = s.cpu().numpy()
        return emb, sent

    def __call__(self, ids, max_len):
        return self.encode(ids, max_len)[0]


class TextEncoder:
    """``get_bert_for_captions`` of the reference: captions -> ``(embedding, sentence_embedding, max_len)``.

    ``vocab_file``: the WordPiece vocabulary (``vocab.txt`` of bert-base-uncased); ``checkpoint_path``: see ``bert_model``
    (``None`` = random weights, whose embeddings mean nothing); ``ops``: a ``HipOps`` (default: a new float32 one, bf16 for
    ``fast``); ``encoder``: any callable ``(ids, max_len) -> embedding (N, T, hidden)`` in place of the HIP network."""

    def __init__(self, vocab_file, checkpoint_path, *, ops=None, fast=False, encoder=None, chunk=1024):
        self.tokenizer = wordpiece.FullTokenizer(vocab_file, do_lower_case=True)
        if encoder is None:
            if checkpoint_path is None:
                warnings.warn("TextEncoder: random BERT weights (checkpoint_path=None): caption embeddings from them mean "
                              "nothing; convert the real weights and pass their path", stacklevel=2)
            if ops is None:
                from ..ops import HipOps
                ops = HipOps(dtype=torch.bfloat16 if fast else torch.float32)
            encoder = BertEncoder(ops, bert_model(checkpoint_path), fast=fast, chunk=chunk)
        self.encoder = encoder

    def get_bert_for_captions(self, captions, max_text_length=17):
        """-> (embedding (N, T, hidden) float32, sentence_embedding (N, hidden) float32, max_len (N,) int64), NumPy, in the
        reference's return order.  The reference's quirk is kept: ``sentence_embedding = embedding.sum(axis=1) / max_len``
        sums over all T positions, the padded ones included (preprocess_data.py:57)."""
        ids, max_len = self.tokenizer.encode(captions, max_text_length)
        if isinstance(self.encoder, BertEncoder):
            embedding, sentence = self.encoder.encode(ids, max_len)          # (xmc_bert_sentence: the same sum on the device)
        else:
            embedding = np.asarray(self.encoder(ids, max_len), np.float32)
            sentence = embedding.sum(axis=1) / max_len[:, None].astype(np.float32)
        return embedding, sentence.astype(np.float32), max_len

    def caption_features(self, captions, max_text_length=17):
        """the caption part of one dataset example, in the value types ``tfrecord.serialize_example`` takes
        (preprocess_data.py:88-93): flat float32 embedding of ALL captions, int64 lengths, the texts as bytes"""
        captions = list(captions)
        embedding, _, max_len = self.get_bert_for_captions(captions, max_text_length)
        return {"caption/embedding": embedding.reshape(-1).astype(np.float32),
                "caption/max_len": max_len.astype(np.int64),
                "caption/text": [c if isinstance(c, bytes) else c.encode("utf-8") for c in captions]}
