"""CLIP image-text dual encoder on the HIP kernels (``csrc/clip.hip`` + ``ops.gemm``): captions and images in, projected
embeddings out -- what the alignment metrics of ``utils/alignment_metrics.py`` are computed from.

``clip_model`` reads the weights: an ``.npz`` whose keys are the state-dict names of a Hugging Face ``CLIPModel`` (one
``np.savez(path, **{k: v.numpy() for k, v in model.state_dict().items()})``).  Nothing is downloaded.
``ClipEncoder`` is the network; ``ClipScorer`` the public interface (tokenizer + network) of the metrics.  ``ClipGuidance`` is what
``train_g_d`` trains against with ``config.clip_guidance_weight``: the image tower with a tape (``image_device(images,
tape=True)``) and its data gradient (``image_backward``; ``csrc/clip_grad.hip``, specification ``utils/clip_grad.py``), and the
text side that ``train()`` runs outside the captured step.
"""
from __future__ import annotations

import os
import re
import warnings

import numpy as np
import torch

from . import clip_arch as arch
from ..libml import clip_bpe


def _shape(params, key, ndim):
    if key not in params:
        raise ValueError(f"CLIP checkpoint: missing key {key}")
    s = tuple(np.asarray(params[key]).shape)
    if len(s) != ndim:
        raise ValueError(f"CLIP checkpoint: {key} has shape {s}, expected {ndim} dimension(s)")
    return s


def infer_dims(params) -> arch.ClipDims:
    """layer counts from the keys, widths from the tables, image size from the position table and the patch size"""
    out = []
    for tower in (arch.V, arch.T):
        idx = [int(m.group(1)) for k in params for m in [re.match(re.escape(tower) + r"encoder\.layers\.(\d+)\.", k)] if m]
        if not idx:
            raise ValueError(f"CLIP checkpoint: missing key {arch.layer_prefix(tower, 0)}self_attn.q_proj.weight")
        out.append((max(idx) + 1, _shape(params, arch.layer_prefix(tower, 0) + "mlp.fc1.weight", 2)[0]))
    (lv, fv), (lt, ft) = out
    hv, c, p, p2 = _shape(params, arch.VISION_KEYS[1], 4)
    if c != 3 or p != p2:
        raise ValueError(f"CLIP checkpoint: {arch.VISION_KEYS[1]} has shape {(hv, c, p, p2)}; expected (width, 3, patch, patch)")
    tokens = _shape(params, arch.VISION_KEYS[2], 2)[0]
    g = int(round((tokens - 1) ** 0.5))
    if g < 1 or g * g != tokens - 1:
        raise ValueError(f"CLIP checkpoint: {tokens} image positions are not 1 + a square")
    vocab, ht = _shape(params, arch.TEXT_KEYS[0], 2)
    context = _shape(params, arch.TEXT_KEYS[1], 2)[0]
    proj = _shape(params, arch.TEXT_KEYS[4], 2)[0]
    return arch.ClipDims(lv, hv, fv, g * p, p, lt, ht, ft, vocab, context, proj)


def validate(params) -> arch.ClipDims:
    """every key present and of its shape (``ValueError`` naming the key), the model inside the kernels' domain"""
    dims = infer_dims(params)
    arch.check_dims(dims)
    for key, shape in arch.expected_shapes(dims).items():
        if key not in params:
            raise ValueError(f"CLIP checkpoint: missing key {key}")
        got = tuple(np.asarray(params[key]).shape)
        if got != shape:
            raise ValueError(f"CLIP checkpoint: {key} has shape {got}, expected {shape}")
    return dims


def clip_model(checkpoint_path, seed: int = 0, **init_kw):
    """-> dict of float32 NumPy arrays under the Hugging Face ``CLIPModel`` state-dict names (``logit_scale`` and buffers such as
    ``position_ids`` are ignored).  ``checkpoint_path``: an ``.npz`` (read with ``allow_pickle=False``); a path that does not exist
    raises ``FileNotFoundError``, a missing or mis-shaped key ``ValueError`` naming it.  ``None`` is the explicit opt-in to
    ``clip_arch.init_clip(seed, **init_kw)`` random weights (tests, benchmarks)."""
    if checkpoint_path is None:
        return arch.init_clip(seed, **init_kw)
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"{checkpoint_path}: CLIP checkpoint not found (np.savez the state_dict() of a Hugging Face "
                                f"CLIPModel of openai/clip-vit-base-patch32; None = random weights)")
    with np.load(checkpoint_path, allow_pickle=False) as z:
        raw = {k: z[k] for k in z.files if not k.endswith("position_ids") and k != "logit_scale"}
    dims = validate(raw)
    return {k: np.ascontiguousarray(raw[k], dtype=np.float32) for k in arch.expected_shapes(dims)}


def check_text(ids, eot, vocab, context):
    """host-side domain check of a batch of id rows; raises ``ValueError`` before anything is launched"""
    ids, eot = np.asarray(ids), np.asarray(eot)
    if ids.ndim != 2 or eot.shape != (ids.shape[0],):
        raise ValueError(f"ids must be (n, t) and eot (n,), got {ids.shape} and {eot.shape}")
    t = ids.shape[1]
    if not 1 <= t <= min(context, arch.MAX_TOKENS):
        raise ValueError(f"context {t} outside 1..{min(context, arch.MAX_TOKENS)}")
    if ids.size and (ids.min() < 0 or ids.max() >= vocab):
        bad = ids[(ids < 0) | (ids >= vocab)]
        raise ValueError(f"token id {int(bad[0])} outside the vocabulary 0..{vocab - 1}")
    if eot.size and (eot.min() < 0 or eot.max() >= t):
        raise ValueError(f"eot must lie in 0..{t - 1}")


class ClipEncoder:
    """``encode_text(ids (n, t) int, eot (n,) int) -> (n, proj)`` and ``encode_image(images (n, H, W, 3) in [0, 1], H = W) ->
    (n, proj)``: the un-normalised projected embeddings, float32 NumPy.  ``images``: a NumPy array or a torch tensor on the host or
    the device (float32 or bf16; anything else is converted to float32).

    Image tower: ``xmc_clip_preprocess`` (resize + normalise + patch rows), GEMM (the patch convolution), ``xmc_clip_vision_embed``,
    the blocks, ``xmc_gather_rows_ln`` on the class row, GEMM.  Text tower: ``xmc_clip_text_embed``, the blocks with a causal mask,
    ``xmc_gather_rows_ln`` on the end-of-text row, GEMM.  A block: ``xmc_bias_add_ln`` (the previous product's bias and residual
    and this LayerNorm in one pass), GEMM (q | k | v), ``xmc_mha_attention``, GEMM, ``xmc_bias_add_ln``, GEMM,
    ``xmc_bias_quick_gelu``, GEMM.  The GEMMs get no split-K workspace and every other kernel works row by row or sequence by
    sequence, so an embedding does not depend on what shares its chunk.  ``fast=True`` (opt-in) rounds the GEMM operands to bf16
    for the bf16 MFMA (the operator table must be the bf16 one); everything else stays float32."""

    def __init__(self, ops, params, fast=False, chunk=256):
        if fast and ops.dtype != torch.bfloat16:
            raise ValueError("fast=True needs HipOps(dtype=torch.bfloat16): ops.gemm(fast=True) is the float32 GEMM otherwise")
        self.ops, self.fast, self.chunk = ops, bool(fast), max(1, int(chunk))
        self.dims = d = validate(params)
        self.launches = 0
        dev = ops.device

        def up(a):
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def tower(prefix, layers):
            out = []
            for i in range(layers):
                pre = arch.layer_prefix(prefix, i)
                qkv = [pre + f"self_attn.{n}_proj" for n in ("q", "k", "v")]
                layer = {"w_qkv": up(np.concatenate([params[k + ".weight"] for k in qkv], axis=0)),
                         "b_qkv": up(np.concatenate([params[k + ".bias"] for k in qkv], axis=0))}
                for short, name in (("o", "self_attn.out_proj"), ("ln1", "layer_norm1"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"),
                                    ("ln2", "layer_norm2")):
                    layer["w_" + short], layer["b_" + short] = up(params[pre + name + ".weight"]), up(params[pre + name + ".bias"])
                out.append(layer)
            return out

        vk, tk = arch.VISION_KEYS, arch.TEXT_KEYS
        self.vision = {"cls": up(params[vk[0]]), "w_patch": up(np.asarray(params[vk[1]]).reshape(d.vision_width, -1)),
                       "pos": up(params[vk[2]]), "pre": (up(params[vk[3]]), up(params[vk[4]])),
                       "final": (up(params[vk[5]]), up(params[vk[6]])), "w_proj": up(params[vk[7]]),
                       "layers": tower(arch.V, d.vision_layers)}
        self.text = {"tok": up(params[tk[0]]), "pos": up(params[tk[1]]), "final": (up(params[tk[2]]), up(params[tk[3]])),
                     "w_proj": up(params[tk[4]]), "layers": tower(arch.T, d.text_layers)}
        self._bufs = {}

    def buffers(self, kind, n, t, h, f):
        key = (kind, n, t)
        b = self._bufs.get(key)
        if b is None:
            ops, rows, f32 = self.ops, n * t, torch.float32
            b = {"h": ops.empty((rows, h), f32), "y": ops.empty((rows, h), f32), "prod": ops.empty((rows, h), f32),
                 "ctx": ops.empty((rows, h), f32), "qkv": ops.empty((rows, 3 * h), f32), "ff": ops.empty((rows, f), f32),
                 "pooled": ops.empty((n, h), f32), "emb": ops.empty((n, self.dims.proj), f32),
                 "len": torch.full((n,), t, dtype=torch.int32).to(ops.device), "idx": ops.empty((n,), torch.int32),
                 "ids": ops.empty((rows,), torch.int32)}
            if kind == "vision":
                d = self.dims
                b["patches"] = ops.empty((n * (t - 1), 3 * d.patch * d.patch), f32)
                b["pe"] = ops.empty((n * (t - 1), h), f32)
            self._bufs[key] = b
        return b

    def _gemm(self, x, w, out):
        self.launches += 1
        return self.ops.gemm(x, w, tb=True, out=out, fast=self.fast, split_k=False)

    def _blocks(self, b, layers, t, causal, final, tape=None):
        """the residual stream b["h"] through ``layers``; returns it.  The last add also normalises with ``final`` (unused rows:
        the pooled row is normalised again from the stream by the caller's gather).  ``tape`` (``tape_buffers``): the same launches
        in the same order, but every state of the stream, every ``qkv`` and every pre-activation ``ff`` goes to a buffer of its own
        (the stream is then ``tape["hs"][0]`` on entry and ``tape["hs"][-1]`` on return)"""
        ops, y = self.ops, b["y"]
        h = b["h"] if tape is None else tape["hs"][0]
        n = b["len"].numel()
        lens_host = np.full((n,), t, np.int32)
        ops.bias_add_ln(h, None, None, layers[0]["w_ln1"], layers[0]["b_ln1"], out=y, eps=arch.LN_EPS)
        self.launches += 1
        for i, L in enumerate(layers):
            qkv, ff = (b["qkv"], b["ff"]) if tape is None else (tape["qkv"][i], tape["ff"][i])
            mid, nxt = (h, h) if tape is None else (tape["hs"][2 * i + 1], tape["hs"][2 * i + 2])
            self._gemm(y, L["w_qkv"], qkv)
            ops.mha_attention(qkv, L["b_qkv"], b["len"], lens_host, b["ctx"], t, causal=causal)
            self._gemm(b["ctx"], L["w_o"], b["prod"])
            ops.bias_add_ln(b["prod"], L["b_o"], h, L["w_ln2"], L["b_ln2"], s=mid, out=y, eps=arch.LN_EPS)
            self._gemm(y, L["w_fc1"], ff)
            ops.bias_quick_gelu(ff, L["b_fc1"], out=b["ff"])
            self._gemm(b["ff"], L["w_fc2"], b["prod"])
            g, be = (layers[i + 1]["w_ln1"], layers[i + 1]["b_ln1"]) if i + 1 < len(layers) else final
            ops.bias_add_ln(b["prod"], L["b_fc2"], mid, g, be, s=nxt, out=y, eps=arch.LN_EPS)
            h = nxt
            self.launches += 4
        return h

    def tape_buffers(self, n):
        """what ``image_backward`` reads, for a chunk of n images: the stream entering each LayerNorm (2 L + 1 states), each
        layer's ``qkv`` and pre-activation ``ff``, the patch products, and the pullback's own scratch.  One set per n, reused from call to call as the
        ResNet-50 tape's buffers are: a tape is valid until the next taped call of the same n (77 MB per layer at ViT-B/32 and
        n = 56, 0.9 GB in all)."""
        key = ("tape", n)
        tb = self._bufs.get(key)
        if tb is None:
            ops, d, f32 = self.ops, self.dims, torch.float32
            rows, h, f, L = n * d.vision_tokens, d.vision_width, d.vision_ffn, d.vision_layers
            prow = n * (d.vision_tokens - 1)
            tb = {"hs": [ops.empty((rows, h), f32) for _ in range(2 * L + 1)],
                  "qkv": [ops.empty((rows, 3 * h), f32) for _ in range(L)], "ff": [ops.empty((rows, f), f32) for _ in range(L)],
                  "dh": ops.empty((rows, h), f32), "dy": ops.empty((rows, h), f32), "dqkv": ops.empty((rows, 3 * h), f32),
                  "dff": ops.empty((rows, f), f32), "dpooled": ops.empty((n, h), f32), "dpe": ops.empty((prow, h), f32),
                  "pe": ops.empty((prow, h), f32),
                  "dpatches": ops.empty((prow, 3 * d.patch * d.patch), f32)}
            self._bufs[key] = tb
        return tb

    def image_device(self, images, tape=False):
        """one chunk -> (n, proj) float32 device tensor owned by this object, valid until the next call of the same shape.
        ``tape=True`` -> (emb, tape): the same kernels in the same order (``emb`` has the same bits), with what
        ``image_backward`` needs kept in ``tape_buffers(n)``"""
        d, ops = self.dims, self.ops
        if not isinstance(images, torch.Tensor):
            images = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32))
        if images.dim() != 4 or images.shape[1] != images.shape[2] or images.shape[3] != 3:
            raise ValueError(f"images are (n, H, W, 3) with H = W, got {tuple(images.shape)}")
        if not 32 <= images.shape[1] <= 512:
            raise ValueError(f"image side {images.shape[1]} outside 32..512")
        if images.dtype not in (torch.float32, torch.bfloat16):
            images = images.float()
        images = images.to(ops.device).contiguous()
        n, t, v = images.shape[0], d.vision_tokens, self.vision
        b = self.buffers("vision", n, t, d.vision_width, d.vision_ffn)
        rec = None
        if tape:
            rec = dict(self.tape_buffers(n), n=n, hw=images.shape[1], dtype=images.dtype, len=b["len"])
        ops.clip_preprocess(images, d.image_size, d.patch, arch.IMAGE_MEAN, arch.IMAGE_STD, out=b["patches"])
        pe = b["pe"] if rec is None else rec["pe"]
        self._gemm(b["patches"], v["w_patch"], pe)
        ops.clip_vision_embed(pe, v["cls"], v["pos"], *v["pre"], b["h"] if rec is None else rec["hs"][0], t, eps=arch.LN_EPS)
        self.launches += 2
        h = self._blocks(b, v["layers"], t, False, v["final"], rec)
        ops.gather_rows_ln(h, None, None, *v["final"], t, out=b["pooled"], eps=arch.LN_EPS)
        self.launches += 1
        emb = self._gemm(b["pooled"], v["w_proj"], b["emb"])
        return emb if rec is None else (emb, rec)

    def _dgemm(self, dy, w, out, alpha=1.0):
        """the dense adjoint dX = alpha dY W on the (out, in) weight: the forward's GEMM entry point, operands rounded as there"""
        self.launches += 1
        return self.ops.gemm(dy, w, alpha=alpha, out=out, fast=self.fast, split_k=False)

    def _grad_op(self, name):
        """a kernel of csrc/clip_grad.hip, or its float64 specification on an operator table without it"""
        fn = getattr(self.ops, name, None)
        if fn is not None:
            return fn
        from . import clip_grad
        spec = {"mha_attention_bwd": lambda qkv, bias, lens, lens_host, dctx, t, causal=False, out=None:
                clip_grad.attention_bwd(qkv.cpu(), bias.cpu(), lens_host, dctx.cpu(), t, causal),
                "ln_bwd_add": lambda x, gamma, dy, dres=None, out=None, eps=1e-5, mode="rows", t=1, pos=None:
                clip_grad.ln_bwd_add(x.cpu(), gamma.cpu(), dy.cpu(), None if dres is None else dres.cpu(), eps, mode, t,
                                     None if pos is None else pos.cpu()),
                "bias_quick_gelu_bwd": lambda x, bias, dy, out=None: clip_grad.bias_quick_gelu_bwd(x.cpu(), bias.cpu(), dy.cpu()),
                "clip_preprocess_bwd": lambda dp, hw, size, patch, std, dtype=torch.float32, out=None:
                clip_grad.preprocess_adjoint(dp.cpu(), hw, size, patch, std)}[name]

        def run(*args, out=None, **kw):
            res = torch.from_numpy(np.ascontiguousarray(spec(*args, **kw)))
            if out is None:
                return res.to(kw.get("dtype", torch.float32)).to(self.ops.device)
            return out.copy_(res.to(out.dtype))
        return run

    def image_backward(self, tape, demb, dtype=None, scale=1.0):
        """the pullback of ``image_device(images, tape=True)``: demb (n, proj) float32 -> d images (n, H, W, 3) in ``dtype``
        (default: the images' own).  The weights are frozen: data gradient only.  Per block, backwards: GEMM (fc2), QuickGELU',
        GEMM (fc1), LayerNorm' + residual, GEMM (out), attention', GEMM (q | k | v), LayerNorm' + residual; around them the
        pooled row's LayerNorm' (scattered to the class rows), pre_layrnorm's (class row dropped), the patch GEMM and the
        transpose of the preprocessing.  ``scale`` multiplies the result (a loss weight; folded into the first product).  The
        result is a new tensor; everything else lives in the tape's buffers."""
        d, ops, v = self.dims, self.ops, self.vision
        n, t = tape["n"], d.vision_tokens
        demb = demb.to(ops.device, torch.float32).contiguous()
        if tuple(demb.shape) != (n, d.proj):
            raise ValueError(f"demb must be ({n}, {d.proj}), got {tuple(demb.shape)}")
        ln, attn, gelu, pre = (self._grad_op(k) for k in ("ln_bwd_add", "mha_attention_bwd", "bias_quick_gelu_bwd",
                                                           "clip_preprocess_bwd"))
        dh, dy, hs = tape["dh"], tape["dy"], tape["hs"]
        lens_host = np.full((n,), t, np.int32)
        self._dgemm(demb, v["w_proj"], tape["dpooled"], alpha=float(scale))
        ln(hs[-1], v["final"][0], tape["dpooled"], out=dh, eps=arch.LN_EPS, mode="gather", t=t)
        self.launches += 1
        for i in reversed(range(d.vision_layers)):
            L = v["layers"][i]
            self._dgemm(dh, L["w_fc2"], tape["dff"])
            gelu(tape["ff"][i], L["b_fc1"], tape["dff"], out=tape["dff"])
            self._dgemm(tape["dff"], L["w_fc1"], dy)
            ln(hs[2 * i + 1], L["w_ln2"], dy, dres=dh, out=dh, eps=arch.LN_EPS)
            self._dgemm(dh, L["w_o"], dy)
            attn(tape["qkv"][i], L["b_qkv"], tape["len"], lens_host, dy, t, causal=False, out=tape["dqkv"])
            self._dgemm(tape["dqkv"], L["w_qkv"], dy)
            ln(hs[2 * i], L["w_ln1"], dy, dres=dh, out=dh, eps=arch.LN_EPS)
            self.launches += 4
        ln(tape["pe"], v["pre"][0], dh, out=tape["dpe"], eps=arch.LN_EPS, mode="vision", t=t, pos=v["pos"])
        self._dgemm(tape["dpe"], v["w_patch"], tape["dpatches"])
        self.launches += 2
        return pre(tape["dpatches"], tape["hw"], d.image_size, d.patch, arch.IMAGE_STD, dtype=dtype or tape["dtype"])

    def text_device(self, ids, eot):
        """one chunk -> (n, proj) float32 device tensor owned by this object"""
        d, ops, x = self.dims, self.ops, self.text
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        eot = np.ascontiguousarray(eot, dtype=np.int64)
        check_text(ids, eot, d.vocab, d.context)
        n, t = ids.shape
        b = self.buffers("text", n, t, d.text_width, d.text_ffn)
        eot32 = eot.astype(np.int32)
        b["ids"].copy_(torch.as_tensor(ids.astype(np.int32).reshape(-1)))
        b["idx"].copy_(torch.as_tensor(eot32))
        ops.clip_text_embed(b["ids"], x["tok"], x["pos"], b["h"], t)
        self.launches += 1
        h = self._blocks(b, x["layers"], t, True, x["final"])
        ops.gather_rows_ln(h, b["idx"], eot32, *x["final"], t, out=b["pooled"], eps=arch.LN_EPS)
        self.launches += 1
        return self._gemm(b["pooled"], x["w_proj"], b["emb"])

    def encode_image(self, images):
        n = images.shape[0]
        out = np.empty((n, self.dims.proj), np.float32)
        for lo in range(0, n, self.chunk):
            out[lo:lo + self.chunk] = self.image_device(images[lo:lo + self.chunk]).cpu().numpy()
        return out

    def encode_text(self, ids, eot):
        ids, eot = np.asarray(ids), np.asarray(eot)
        check_text(ids, eot, self.dims.vocab, self.dims.context)             # the WHOLE list first: nothing runs on a bad one
        n = ids.shape[0]
        out = np.empty((n, self.dims.proj), np.float32)
        for lo in range(0, n, self.chunk):
            out[lo:lo + self.chunk] = self.text_device(ids[lo:lo + self.chunk], eot[lo:lo + self.chunk]).cpu().numpy()
        return out


class ClipGuidance:
    """What ``xmc_gan.create_additional_data`` hands to ``train_g_d`` as ``clip_guidance`` (config.clip_guidance_weight > 0): the
    frozen CLIP's weights and tokenizer.  Like the ResNet-50's ``ImageModel`` it binds itself to the step's operator table on
    first use (``bind``).  ``embed_text(ops, captions)`` is the text side, run OUTSIDE the step: strings -> (rows, proj) float32
    device tensor, the batch's ``clip_text``.  ``keep`` (tests): the last half step's images, embeddings, text rows and image
    cotangent are retained in ``kept``."""

    def __init__(self, params, tokenizer, fast=False, chunk=256):
        self.params, self.tokenizer, self.fast, self.chunk = params, tokenizer, bool(fast), max(1, int(chunk))
        self.dims = validate(params)
        self.proj = self.dims.proj
        if tokenizer is not None and tokenizer.vocab_size > self.dims.vocab:
            raise ValueError(f"the BPE vocabulary has {tokenizer.vocab_size} entries, the token table {self.dims.vocab} rows")
        self.encoder, self.keep, self.kept = None, False, None

    @classmethod
    def from_config(cls, config):
        path = config.get("clip_ckpt_path", None)
        if path is None:
            warnings.warn("clip_guidance_weight > 0 with random CLIP weights (clip_ckpt_path=None): the term then pulls the "
                          "generator towards nothing meaningful; convert the real weights and pass their path", stacklevel=2)
        fast = config.get("clip_guidance_fast", None)
        fast = config.dtype == "bfloat16" if fast is None else bool(fast)
        return cls(clip_model(path), clip_bpe.ClipTokenizer(config.clip_vocab_path, config.clip_merges_path), fast=fast)

    def bind(self, ops):
        if self.encoder is None or self.encoder.ops is not ops:
            self.encoder = ClipEncoder(ops, self.params, fast=self.fast, chunk=self.chunk)
        return self.encoder

    def embed_text(self, ops, captions):
        """the frozen text tower on the current stream, chunked as ``encode_text``; the WHOLE list is checked before anything runs"""
        enc = self.bind(ops)
        ids, eot = self.tokenizer.encode([c.decode("utf-8") if isinstance(c, bytes) else str(c) for c in captions], self.dims.context)
        ids, eot = np.asarray(ids), np.asarray(eot)
        check_text(ids, eot, self.dims.vocab, self.dims.context)
        out = ops.empty((ids.shape[0], self.proj), torch.float32)
        for lo in range(0, ids.shape[0], self.chunk):
            out[lo:lo + self.chunk].copy_(enc.text_device(ids[lo:lo + self.chunk], eot[lo:lo + self.chunk]))
        return out


class ClipScorer:
    """strings and images -> embeddings.  ``vocab`` / ``merges``: the BPE files (``libml/clip_bpe.py``); ``checkpoint_path``: see
    ``clip_model`` (``None`` = random weights, whose scores mean nothing); ``ops``: a ``HipOps`` (default: a new float32 one, bf16
    for ``fast``); ``encoder``: a ready ``ClipEncoder`` (or any object with its two methods and ``dims.context``) in place of the HIP
    network."""

    def __init__(self, vocab, merges, checkpoint_path, *, ops=None, fast=False, encoder=None, chunk=256):
        self.tokenizer = clip_bpe.ClipTokenizer(vocab, merges)
        if encoder is None:
            if checkpoint_path is None:
                warnings.warn("ClipScorer: random CLIP weights (checkpoint_path=None): CLIPScore and R-precision from them mean "
                              "nothing; convert the real weights and pass their path", stacklevel=2)
            if ops is None:
                from ..ops import HipOps
                ops = HipOps(dtype=torch.bfloat16 if fast else torch.float32)
            encoder = ClipEncoder(ops, clip_model(checkpoint_path), fast=fast, chunk=chunk)
        self.encoder = encoder
        self.ops = ops if ops is not None else getattr(encoder, "ops", None)
        vocab_size = getattr(getattr(encoder, "dims", None), "vocab", None)
        if vocab_size is not None and self.tokenizer.vocab_size > vocab_size:
            raise ValueError(f"the BPE vocabulary has {self.tokenizer.vocab_size} entries, the token table {vocab_size} rows")

    def embed_text(self, captions):
        ids, eot = self.tokenizer.encode(list(captions), self.encoder.dims.context)
        return self.encoder.encode_text(ids, eot)

    def embed_image(self, images):
        return self.encoder.encode_image(images)
