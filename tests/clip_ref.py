"""Plain-torch restatement of the CLIP dual encoder (utils/clip_utils.ClipEncoder), the oracle of the GPU tests.

float64 by default.  ``dtype=torch.float32`` runs the same statements in float32 on the CPU (the yardstick e32 of the
whole-encoder tests); ``round_bf16=True`` rounds both operands of every dense product to bf16 first, as
``xmc_gemm_f32_bf16mfma`` does (the yardstick e_bf).  tests/test_clip_text.py ties this file to ``transformers.CLIPModel`` in
float64 on the same random state dict, so the oracle does not rest on this repository alone.  The preprocessing (resize,
normalise, patch rows) is ``alignment_metrics.preprocess``, itself tied to Pillow by tests/test_alignment_metrics.py.

A helper module, imported by tests."""
import numpy as np
import torch

from xmcgan_image_generation_amd.utils import alignment_metrics, clip_arch

LN_EPS = 1e-5
HEAD_DIM = 64
V, T = "vision_model.", "text_model."


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def layer_norm(v, gamma, beta, eps=LN_EPS):
    """-> (y, xhat): biased variance, two-pass"""
    mean = v.mean(dim=-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    xhat = d / torch.sqrt(var + eps)
    return xhat * gamma + beta, xhat


def quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def dense(x, w, round_bf16=False):
    """x (rows, in) @ w (out, in)^T, no bias"""
    if round_bf16:
        x, w = x.to(torch.bfloat16).to(x.dtype), w.to(torch.bfloat16).to(w.dtype)
    return x @ w.t()


def attention(qkv, bias_qkv, lens, t, causal=False):
    """qkv (n * t, 3h) without bias -> (ctx (n * t, h), sum_j |p_j v_j| of the same shape): softmax over the keys j < lens[i], and
    j <= query row when ``causal``"""
    rows, h3 = qkv.shape
    h, n = h3 // 3, rows // t
    heads = h // HEAD_DIM
    z = (qkv + bias_qkv).view(n, t, 3, heads, HEAD_DIM)
    q, k, v = (z[:, :, i].permute(0, 2, 1, 3) for i in range(3))             # (n, heads, t, 64)
    s = q @ k.transpose(-1, -2) / 8.0
    live = (torch.arange(t)[None, :] < torch.as_tensor(np.asarray(lens)).view(n, 1))[:, None, None, :]      # keys
    if causal:
        live = live & (torch.arange(t)[None, :] <= torch.arange(t)[:, None])[None, None]
    s = s.masked_fill(~live, float("-inf"))
    p = torch.softmax(s, dim=-1)
    ctx = (p @ v).permute(0, 2, 1, 3).reshape(rows, h)
    mag = (p @ v.abs()).permute(0, 2, 1, 3).reshape(rows, h)
    return ctx, mag


def num_layers(params, tower):
    return 1 + max(int(k[len(tower):].split(".")[2]) for k in params if k.startswith(tower + "encoder.layers."))


def blocks(params, tower, h, n, t, causal, dtype, round_bf16):
    """the residual stream (n * t, width) through every pre-LN block of ``tower``"""
    lens = np.full((n,), t)
    for i in range(num_layers(params, tower)):
        pre = f"{tower}encoder.layers.{i}."
        P = lambda name: _t(params[pre + name], dtype)                        # noqa: E731
        w_qkv = torch.cat([P(f"self_attn.{m}_proj.weight") for m in "qkv"])
        b_qkv = torch.cat([P(f"self_attn.{m}_proj.bias") for m in "qkv"])
        y, _ = layer_norm(h, P("layer_norm1.weight"), P("layer_norm1.bias"))
        ctx, _ = attention(dense(y, w_qkv, round_bf16), b_qkv, lens, t, causal)
        h = h + dense(ctx, P("self_attn.out_proj.weight"), round_bf16) + P("self_attn.out_proj.bias")
        y, _ = layer_norm(h, P("layer_norm2.weight"), P("layer_norm2.bias"))
        f = quick_gelu(dense(y, P("mlp.fc1.weight"), round_bf16) + P("mlp.fc1.bias"))
        h = h + dense(f, P("mlp.fc2.weight"), round_bf16) + P("mlp.fc2.bias")
    return h


def vision_embed(params, patches, n, dtype=torch.float64):
    """patch products (n * g * g, width) -> (y, xhat, gamma) of pre_layrnorm over the (n * t, width) token rows"""
    cls, pos = _t(params[V + "embeddings.class_embedding"], dtype), _t(params[V + "embeddings.position_embedding.weight"], dtype)
    x = torch.cat([cls.expand(n, 1, -1), patches.view(n, -1, cls.numel())], dim=1) + pos
    g, b = _t(params[V + "pre_layrnorm.weight"], dtype), _t(params[V + "pre_layrnorm.bias"], dtype)
    y, xhat = layer_norm(x.reshape(-1, cls.numel()), g, b)
    return y, xhat, g


def encode_image(params, images, dtype=torch.float64, round_bf16=False):
    """images (n, H, W, 3) in [0, 1] -> (n, proj) in ``dtype``"""
    w = _t(params[V + "embeddings.patch_embedding.weight"], dtype)
    patch = w.shape[-1]
    t = params[V + "embeddings.position_embedding.weight"].shape[0]
    size = int(round((t - 1) ** 0.5)) * patch
    rows = _t(alignment_metrics.preprocess(np.asarray(images, np.float64), size, patch), dtype)
    n = np.asarray(images).shape[0]
    h, _, _ = vision_embed(params, dense(rows, w.reshape(w.shape[0], -1), round_bf16), n, dtype)
    h = blocks(params, V, h, n, t, False, dtype, round_bf16)
    pooled, _ = layer_norm(h.view(n, t, -1)[:, 0], _t(params[V + "post_layernorm.weight"], dtype),
                           _t(params[V + "post_layernorm.bias"], dtype))
    return dense(pooled, _t(params["visual_projection.weight"], dtype), round_bf16)


def text_embed(params, ids, dtype=torch.float64):
    n, t = np.asarray(ids).shape
    tok, pos = _t(params[T + "embeddings.token_embedding.weight"], dtype), _t(params[T + "embeddings.position_embedding.weight"], dtype)
    return tok[torch.as_tensor(np.asarray(ids), dtype=torch.long).reshape(-1)] + pos[:t].repeat(n, 1)


def encode_text(params, ids, eot, dtype=torch.float64, round_bf16=False):
    """ids (n, t), eot (n,) -> (n, proj) in ``dtype``"""
    ids = np.asarray(ids)
    n, t = ids.shape
    h = blocks(params, T, text_embed(params, ids, dtype), n, t, True, dtype, round_bf16)
    rows = h.view(n, t, -1)[torch.arange(n), torch.as_tensor(np.asarray(eot), dtype=torch.long)]
    pooled, _ = layer_norm(rows, _t(params[T + "final_layer_norm.weight"], dtype), _t(params[T + "final_layer_norm.bias"], dtype))
    return dense(pooled, _t(params["text_projection.weight"], dtype), round_bf16)


SMALL = dict(vision_layers=2, vision_width=128, vision_ffn=256, image_size=64, patch=32, text_layers=2, text_width=128,
             text_ffn=256, vocab=600, context=77, proj=64)


def small_params(seed=5, **over):
    """the issue's test dimensions: width 128 (2 heads), 2 layers, ffn 256, projection 64; text vocab 600, t = 77; vision 64 px with
    patch 32 (5 tokens)"""
    return clip_arch.init_clip(seed, **{**SMALL, **over})
