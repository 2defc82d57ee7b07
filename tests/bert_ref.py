"""Plain-torch restatement of the caption encoder (utils/bert_utils.BertEncoder), the oracle of the GPU tests.

float64 by default.  ``dtype=torch.float32`` runs the same statements in float32 on the CPU (the yardstick e32 of the
whole-encoder tests); ``round_bf16=True`` rounds both operands of every dense product to bf16 first, as
``xmc_gemm_f32_bf16mfma`` does (the yardstick e_bf).  tests/test_bert_text.py ties this file to ``transformers.BertModel`` in
float64 on the same random state dict (1e-10), so the oracle does not rest on this repository alone.

A helper module, imported by tests."""
import math

import numpy as np
import torch

LN_EPS = 1e-12
HEAD_DIM = 64


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def layer_norm(v, gamma, beta, eps=LN_EPS):
    """-> (y, xhat): biased variance, two-pass"""
    mean = v.mean(dim=-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    xhat = d / torch.sqrt(var + eps)
    return xhat * gamma + beta, xhat


def gelu(v):
    return 0.5 * v * torch.erfc(-v / math.sqrt(2.0))          # = 0.5 v (1 + erf(v / sqrt 2)) without the cancellation


def dense(x, w, round_bf16=False):
    """x (rows, in) @ w (out, in)^T, no bias"""
    if round_bf16:
        x, w = x.to(torch.bfloat16).to(x.dtype), w.to(torch.bfloat16).to(w.dtype)
    return x @ w.t()


def attention(qkv, bias_qkv, max_len, t):
    """qkv (n * t, 3h) without bias -> (ctx (n * t, h), sum_j |p_j v_j| of the same shape): softmax over keys j < max_len"""
    rows, h3 = qkv.shape
    h, n = h3 // 3, rows // t
    heads = h // HEAD_DIM
    z = (qkv + bias_qkv).view(n, t, 3, heads, HEAD_DIM)
    q, k, v = (z[:, :, i].permute(0, 2, 1, 3) for i in range(3))             # (n, heads, t, 64)
    s = q @ k.transpose(-1, -2) / 8.0
    live = torch.arange(t)[None, :] < torch.as_tensor(np.asarray(max_len)).view(n, 1)      # (n, t) keys
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    ctx = (p @ v).permute(0, 2, 1, 3).reshape(rows, h)
    mag = (p @ v.abs()).permute(0, 2, 1, 3).reshape(rows, h)
    return ctx, mag


def embed(params, ids, dtype=torch.float64):
    """-> (y, xhat, gamma) of the embedding LayerNorm, rows = n * t"""
    n, t = ids.shape
    word, pos, typ = (_t(params[k], dtype) for k in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                                                     "embeddings.token_type_embeddings.weight"))
    v = word[torch.as_tensor(np.asarray(ids), dtype=torch.long).reshape(-1)] + pos[:t].repeat(n, 1) + typ[0]
    g, b = _t(params["embeddings.LayerNorm.weight"], dtype), _t(params["embeddings.LayerNorm.bias"], dtype)
    y, xhat = layer_norm(v, g, b)
    return y, xhat, g


def num_layers(params):
    return 1 + max(int(k.split(".")[2]) for k in params if k.startswith("encoder.layer."))


def forward(params, ids, max_len, dtype=torch.float64, round_bf16=False):
    """-> embedding (n, t, hidden) in ``dtype``"""
    ids = np.asarray(ids)
    n, t = ids.shape
    h, _, _ = embed(params, ids, dtype)
    for i in range(num_layers(params)):
        pre = f"encoder.layer.{i}."
        P = lambda name: _t(params[pre + name], dtype)                        # noqa: E731
        w_qkv = torch.cat([P(f"attention.self.{m}.weight") for m in ("query", "key", "value")])
        b_qkv = torch.cat([P(f"attention.self.{m}.bias") for m in ("query", "key", "value")])
        ctx, _ = attention(dense(h, w_qkv, round_bf16), b_qkv, max_len, t)
        a = dense(ctx, P("attention.output.dense.weight"), round_bf16) + P("attention.output.dense.bias")
        h1, _ = layer_norm(a + h, P("attention.output.LayerNorm.weight"), P("attention.output.LayerNorm.bias"))
        f = gelu(dense(h1, P("intermediate.dense.weight"), round_bf16) + P("intermediate.dense.bias"))
        o = dense(f, P("output.dense.weight"), round_bf16) + P("output.dense.bias")
        h, _ = layer_norm(o + h1, P("output.LayerNorm.weight"), P("output.LayerNorm.bias"))
    return h.view(n, t, -1)


def sentence(embedding, max_len):
    """the reference's quirk: the sum over ALL t positions divided by the number of real tokens"""
    return embedding.sum(dim=1) / torch.as_tensor(np.asarray(max_len)).to(embedding.dtype)[:, None]
