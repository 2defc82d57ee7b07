#!/usr/bin/env python
"""Throughput of the CLIP dual encoder at ViT-B/32 size: images/s (128 px inputs resized to 224 on the device) and captions/s (77
tokens) for float32 and ``fast`` (bf16 MFMA GEMMs), and the time of every kernel of csrc/clip.hip at the shapes of one chunk.
Random weights and inputs (the arithmetic does not depend on them; the token table is cut to 1000 rows, its length is no kernel's
concern).  Device events around whole forward passes, after a warm-up, over a timed window of at least one second; the upload of the
ids is inside the window, the download of the embeddings is not.

usage (on the GPU box): python tools/bench_clip.py [--out profiles/rNN_clip.txt] [--chunk 256] [--modes float32 fast] [--image 128]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from xmcgan_image_generation_amd.ops import HipOps  # noqa: E402
from xmcgan_image_generation_amd.utils import clip_arch, clip_utils  # noqa: E402


def dense_flops(layers, tokens, h, f):
    return 2 * tokens * layers * (3 * h * h + h * h + 2 * h * f)


def timed(fn, window):
    """-> (passes, seconds) of ``fn`` repeated until at least ``window`` seconds of device time"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    passes = 4
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(passes):
            fn()
        t1.record()
        torch.cuda.synchronize()
        seconds = t0.elapsed_time(t1) / 1e3
        if seconds >= window:
            return passes, seconds
        passes = max(passes * 2, int(passes * 1.2 * window / max(seconds, 1e-3)) + 1)


def kernel_times(ops, d, chunk, hw, window):
    """microseconds per launch of every kernel of csrc/clip.hip at the image tower's (and the text attention's) shapes of one chunk"""
    dev, f32 = ops.device, torch.float32
    t, h, f = d.vision_tokens, d.vision_width, d.vision_ffn
    rows = chunk * t
    rnd = lambda *s: torch.randn(*s, dtype=f32, device=dev)                   # noqa: E731
    img = torch.rand(chunk, hw, hw, 3, dtype=f32, device=dev)
    patches = ops.empty((chunk * (t - 1), 3 * d.patch ** 2), f32)
    x, res, y, ff = rnd(rows, h), rnd(rows, h), ops.empty((rows, h), f32), rnd(rows, f)
    qkv, ctx = rnd(rows, 3 * h), ops.empty((rows, h), f32)
    g, b, b3, bf = torch.ones(h, device=dev), torch.zeros(h, device=dev), torch.zeros(3 * h, device=dev), torch.zeros(f, device=dev)
    lens = torch.full((chunk,), t, dtype=torch.int32, device=dev)
    lens_host = np.full((chunk,), t, np.int32)
    tt, ht = d.context, d.text_width
    qkv_t, ctx_t = rnd(chunk * tt, 3 * ht), ops.empty((chunk * tt, ht), f32)
    lens_t, lens_t_host = torch.full((chunk,), tt, dtype=torch.int32, device=dev), np.full((chunk,), tt, np.int32)
    tok, pos_t = rnd(1000, ht), rnd(tt, ht)
    ids = torch.randint(0, 1000, (chunk * tt,), dtype=torch.int32, device=dev)
    xt = ops.empty((chunk * tt, ht), f32)
    pe, cls, pos = rnd(chunk * (t - 1), h), rnd(h), rnd(t, h)
    pooled = ops.empty((chunk, h), f32)
    a, c = rnd(chunk, d.proj), rnd(chunk, d.proj)
    cos = torch.empty((chunk,), dtype=torch.float64, device=dev)
    truth = np.arange(chunk, dtype=np.int32)
    cand = np.stack([(i + 1 + np.arange(min(99, chunk - 1))) % chunk for i in range(chunk)]).astype(np.int32)
    hit = torch.empty((chunk,), dtype=torch.uint8, device=dev)
    cases = [
        (f"xmc_clip_preprocess {hw}->{d.image_size}", lambda: ops.clip_preprocess(img, d.image_size, d.patch, clip_arch.IMAGE_MEAN,
                                                                                 clip_arch.IMAGE_STD, out=patches)),
        ("xmc_clip_vision_embed", lambda: ops.clip_vision_embed(pe, cls, pos, g, b, y, t)),
        ("xmc_clip_text_embed", lambda: ops.clip_text_embed(ids, tok, pos_t, xt, tt)),
        ("xmc_bias_add_ln", lambda: ops.bias_add_ln(x, b, res, g, b, s=res, out=y)),
        ("xmc_bias_quick_gelu", lambda: ops.bias_quick_gelu(ff, bf, out=ff)),
        (f"xmc_mha_attention t={t}", lambda: ops.mha_attention(qkv, b3, lens, lens_host, ctx, t)),
        (f"xmc_mha_attention t={tt} causal", lambda: ops.mha_attention(qkv_t, torch.zeros(3 * ht, device=dev), lens_t, lens_t_host,
                                                                       ctx_t, tt, causal=True)),
        ("xmc_gather_rows_ln", lambda: ops.gather_rows_ln(x, None, None, g, b, t, out=pooled)),
        ("xmc_pair_cosine", lambda: ops.pair_cosine(a, c, out=cos)),
        (f"xmc_rprecision_hits c={cand.shape[1]}", lambda: ops.rprecision_hits(a, c, truth, cand, out=hit)),
    ]
    out = []
    for name, fn in cases:
        passes, seconds = timed(fn, window / 4)
        out.append(f"kernel {name} chunk={chunk} {seconds / passes * 1e6:.1f} us")
        print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--image", type=int, default=128, help="side of the input images")
    ap.add_argument("--modes", nargs="+", default=["float32", "fast"], choices=["float32", "fast"])
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per measurement (at least)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    params = clip_arch.init_clip(0, vocab=1000)
    rng = np.random.default_rng(0)
    lines = [f"# tools/bench_clip.py on {torch.cuda.get_device_name(0)}: CLIP ViT-B/32 (image 12 x 768, 50 tokens; text 12 x 512, 77 "
             f"tokens), random weights, {a.image} px inputs, chunk {a.chunk}", "# mode tower passes seconds items/s dense_TFLOP/s"]
    for mode in a.modes:
        fast = mode == "fast"
        ops = HipOps(dtype=torch.bfloat16 if fast else torch.float32)
        enc = clip_utils.ClipEncoder(ops, params, fast=fast, chunk=a.chunk)
        d = enc.dims
        images = torch.rand(a.chunk, a.image, a.image, 3, device=ops.device)
        ids = rng.integers(0, d.vocab - 1, (a.chunk, d.context))
        eot = rng.integers(1, d.context, a.chunk)
        flops = {"image": dense_flops(d.vision_layers, d.vision_tokens, d.vision_width, d.vision_ffn)
                 + 2 * (d.vision_tokens - 1) * 3 * d.patch ** 2 * d.vision_width,
                 "text": dense_flops(d.text_layers, d.context, d.text_width, d.text_ffn)}
        for tower, fn in (("image", lambda: enc.image_device(images)), ("text", lambda: enc.text_device(ids, eot))):
            passes, seconds = timed(fn, a.window)
            rate = passes * a.chunk / seconds
            lines.append(f"{mode} {tower} {passes} {seconds:.3f} {rate:.1f} {rate * flops[tower] / 1e12:.2f}")
            print(lines[-1], flush=True)
        if not fast:
            lines += kernel_times(ops, d, a.chunk, a.image, a.window)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
