"""Architecture of the CLIP dual encoder the alignment metrics run on (``config.eval_extra_metrics`` ``"clip"``): the network of
``transformers.CLIPModel`` -- a ViT image tower (bias-free patch embedding, class token, position table, ``pre_layrnorm``, pre-LN
blocks, ``post_layernorm`` on the class row, bias-free ``visual_projection``) and a causal text tower (token and position tables,
pre-LN blocks, ``final_layer_norm``, the row at the end-of-text token, bias-free ``text_projection``).  A block is LN, fused
q | k | v with bias, attention (scale 1 / 8), out-projection, residual, LN, fc1, QuickGELU, fc2, residual.

Parameters are a flat dict of NumPy arrays under the state-dict names of a Hugging Face ``CLIPModel`` (dense weights
``(out, in)``), the layout a user gets from one ``np.savez`` of ``model.state_dict()``.
"""
from __future__ import annotations

from typing import Dict, NamedTuple

import numpy as np

HEAD_DIM = 64
LN_EPS = 1e-5
MAX_TOKENS = 128               # xmc_mha_attention's domain
MAX_WIDTH = 1024               # the row kernels' domain
# the normalisation constants of OpenAI's CLIP preprocessing (RGB)
IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)

V, T = "vision_model.", "text_model."
VISION_KEYS = (V + "embeddings.class_embedding", V + "embeddings.patch_embedding.weight", V + "embeddings.position_embedding.weight",
               V + "pre_layrnorm.weight", V + "pre_layrnorm.bias", V + "post_layernorm.weight", V + "post_layernorm.bias",
               "visual_projection.weight")
TEXT_KEYS = (T + "embeddings.token_embedding.weight", T + "embeddings.position_embedding.weight", T + "final_layer_norm.weight",
             T + "final_layer_norm.bias", "text_projection.weight")
LAYER_DENSE = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")
LAYER_NORMS = ("layer_norm1", "layer_norm2")


class ClipDims(NamedTuple):
    vision_layers: int
    vision_width: int
    vision_ffn: int
    image_size: int
    patch: int
    text_layers: int
    text_width: int
    text_ffn: int
    vocab: int
    context: int
    proj: int

    @property
    def vision_tokens(self):
        return 1 + (self.image_size // self.patch) ** 2


def layer_prefix(tower: str, i: int) -> str:
    return f"{tower}encoder.layers.{i}."


def _tower_shapes(out, tower, layers, h, f):
    for i in range(layers):
        pre = layer_prefix(tower, i)
        for n in LAYER_DENSE:
            o, k = (f, h) if n == "mlp.fc1" else (h, f) if n == "mlp.fc2" else (h, h)
            out[pre + n + ".weight"], out[pre + n + ".bias"] = (o, k), (o,)
        for n in LAYER_NORMS:
            out[pre + n + ".weight"], out[pre + n + ".bias"] = (h,), (h,)


def expected_shapes(d: ClipDims) -> Dict[str, tuple]:
    hv, ht = d.vision_width, d.text_width
    out = {VISION_KEYS[0]: (hv,), VISION_KEYS[1]: (hv, 3, d.patch, d.patch), VISION_KEYS[2]: (d.vision_tokens, hv),
           VISION_KEYS[3]: (hv,), VISION_KEYS[4]: (hv,), VISION_KEYS[5]: (hv,), VISION_KEYS[6]: (hv,), VISION_KEYS[7]: (d.proj, hv),
           TEXT_KEYS[0]: (d.vocab, ht), TEXT_KEYS[1]: (d.context, ht), TEXT_KEYS[2]: (ht,), TEXT_KEYS[3]: (ht,),
           TEXT_KEYS[4]: (d.proj, ht)}
    _tower_shapes(out, V, d.vision_layers, hv, d.vision_ffn)
    _tower_shapes(out, T, d.text_layers, ht, d.text_ffn)
    return out


def check_dims(d: ClipDims):
    """``ValueError`` for a model outside what the kernels serve (head dimension 64, width <= 1024, <= 128 tokens)"""
    for name, w in (("vision", d.vision_width), ("text", d.text_width)):
        if w % HEAD_DIM or not HEAD_DIM <= w <= MAX_WIDTH:
            raise ValueError(f"CLIP: {name} width {w} is not a multiple of 64 in 64..{MAX_WIDTH} (head dimension 64 only)")
    if d.patch < 1 or d.image_size % d.patch:
        raise ValueError(f"CLIP: image size {d.image_size} is no multiple of the patch size {d.patch}")
    if d.vision_tokens > MAX_TOKENS or d.context > MAX_TOKENS:
        raise ValueError(f"CLIP: {d.vision_tokens} image tokens / {d.context} text tokens: at most {MAX_TOKENS} tokens per sequence "
                         f"are supported (ViT-B/32 at 224 px has 50; B/16 with 197 is not)")
    if d.vision_tokens < 2 or d.context < 2 or d.image_size > 448:
        raise ValueError(f"CLIP: image size {d.image_size} / context {d.context} outside the supported range")
    if (3 * d.patch * d.patch) % 4 or d.vision_ffn % 4 or d.text_ffn % 4 or d.proj % 4:
        raise ValueError("CLIP: patch row, ffn and projection widths must be multiples of 4")


def init_clip(seed: int, vision_layers: int = 12, vision_width: int = 768, vision_ffn: int = 3072, image_size: int = 224,
              patch: int = 32, text_layers: int = 12, text_width: int = 512, text_ffn: int = 2048, vocab: int = 49408,
              context: int = 77, proj: int = 512) -> Dict[str, np.ndarray]:
    """Random float32 weights at ViT-B/32's dimensions by default (tests and benchmarks; scores from them mean nothing).  Scales keep
    every activation O(1): dense weights N(0, 1 / in), biases and LayerNorm offsets N(0, 0.1^2), LayerNorm gains 1 + N(0, 0.1^2),
    tables and the class token N(0, 1); the out-projection and fc2 are scaled by 1 / sqrt(2 layers) so the residual stream of the
    pre-LN blocks stays O(1) through the depth."""
    d = ClipDims(vision_layers, vision_width, vision_ffn, image_size, patch, text_layers, text_width, text_ffn, vocab, context, proj)
    check_dims(d)
    rng = np.random.default_rng(seed)
    p = {}
    for key, shape in expected_shapes(d).items():
        layers = vision_layers if key.startswith(V) else text_layers
        if "norm" in key and key.endswith(".weight"):
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        elif key.endswith(".bias"):
            a = 0.1 * rng.standard_normal(shape)
        elif "embedding" in key and "patch" not in key:
            a = rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))
            if "out_proj" in key or "fc2" in key:
                a = a / np.sqrt(2.0 * layers)
        p[key] = a.astype(np.float32)
    return p
