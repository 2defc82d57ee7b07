#!/usr/bin/env python
"""Cost of the CLIP guidance term (config.clip_guidance_weight) at ViT-B/32 size:

* the image tower's forward WITH its tape and its data-gradient pass (ClipEncoder.image_device(tape=True) / image_backward) at
  B = 56 images of 128 px, float32 and ``fast`` (bf16 MFMA GEMMs), per call, and backward / forward;
* the backward's split: every kernel of csrc/clip_grad.hip and every dense adjoint at the shapes of that chunk, per launch and
  times the launches per pass (float32 and fast GEMMs);
* the C1 step (batch 56, bf16, ResNet-50 term on, hipGraph replay) with the switch off and on, ALTERNATED in one process: the
  switch-off time of the same run is the yardstick.

Random weights and inputs (the arithmetic does not depend on them).  Device events around whole passes, after a warm-up, over a
timed window of at least one second; medians over the alternated rounds for the step.

usage (on the GPU box): python tools/bench_clip_guidance.py [--out profiles/rNN_clip_guidance.txt] [--batch 56] [--image 128]
                                                            [--skip-step] [--rounds 5] [--steps 30]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_clip import dense_flops, timed  # noqa: E402
from xmcgan_image_generation_amd.ops import HipOps  # noqa: E402
from xmcgan_image_generation_amd.utils import clip_arch, clip_utils  # noqa: E402


def tower_times(params, batch, hw, window, lines):
    for mode in ("float32", "fast"):
        fast = mode == "fast"
        ops = HipOps(dtype=torch.bfloat16 if fast else torch.float32)
        enc = clip_utils.ClipEncoder(ops, params, fast=fast)
        d = enc.dims
        images = torch.rand(batch, hw, hw, 3, device=ops.device).to(ops.dtype)
        demb = torch.randn(batch, d.proj, device=ops.device)
        flops = batch * (dense_flops(d.vision_layers, d.vision_tokens, d.vision_width, d.vision_ffn)
                         + 2 * (d.vision_tokens - 1) * 3 * d.patch ** 2 * d.vision_width)
        _, tape = enc.image_device(images, tape=True)
        res = {}
        for name, fn in (("forward", lambda: enc.image_device(images)), ("forward+tape", lambda: enc.image_device(images, tape=True)),
                         ("backward", lambda: enc.image_backward(tape, demb))):
            passes, seconds = timed(fn, window)
            res[name] = seconds / passes
            lines.append(f"tower {mode} {name} B={batch} {hw}px: {res[name] * 1e3:.3f} ms/call, {batch / res[name]:.0f} images/s, "
                         f"{flops / res[name] / 1e12:.1f} dense TFLOP/s")
            print(lines[-1], flush=True)
        lines.append(f"tower {mode} backward / forward+tape = {res['backward'] / res['forward+tape']:.2f}")
        print(lines[-1], flush=True)
        if not fast:
            kernel_split(ops, d, batch, hw, window, lines)
        else:
            gemm_split(ops, d, batch, window, lines, True)


def gemm_split(ops, d, batch, window, lines, fast):
    dev, f32 = ops.device, torch.float32
    t, h, f = d.vision_tokens, d.vision_width, d.vision_ffn
    rows = batch * t
    rnd = lambda *s: torch.randn(*s, dtype=f32, device=dev)                   # noqa: E731
    total = 0.0
    for name, m, k, n, count in (("fc2' (rows,h)x(h,f)", rows, h, f, d.vision_layers), ("fc1' (rows,f)x(f,h)", rows, f, h, d.vision_layers),
                                 ("out' (rows,h)x(h,h)", rows, h, h, d.vision_layers), ("qkv' (rows,3h)x(3h,h)", rows, 3 * h, h, d.vision_layers),
                                 ("patch' (B g^2,h)x(h,3p^2)", batch * (t - 1), h, 3 * d.patch ** 2, 1)):
        dy, w, out = rnd(m, k), rnd(k, n), ops.empty((m, n), f32)
        passes, seconds = timed(lambda: ops.gemm(dy, w, out=out, fast=fast, split_k=False), window / 4)
        us = seconds / passes * 1e6
        total += us * count
        lines.append(f"backward {'fast' if fast else 'float32'} GEMM {name}: {us:.1f} us x {count} = {us * count / 1e3:.3f} ms, "
                     f"{2.0 * m * k * n / us / 1e6:.1f} TFLOP/s")
        print(lines[-1], flush=True)
    lines.append(f"backward {'fast' if fast else 'float32'} GEMMs in all: {total / 1e3:.3f} ms")
    print(lines[-1], flush=True)


def kernel_split(ops, d, batch, hw, window, lines):
    dev, f32 = ops.device, torch.float32
    t, h, f = d.vision_tokens, d.vision_width, d.vision_ffn
    rows, L = batch * t, d.vision_layers
    rnd = lambda *s: torch.randn(*s, dtype=f32, device=dev)                   # noqa: E731
    x, dy, dh, pe, pos, g = rnd(rows, h), rnd(rows, h), rnd(rows, h), rnd(batch * (t - 1), h), rnd(t, h), torch.ones(h, device=dev)
    dpool, dpe = rnd(batch, h), ops.empty((batch * (t - 1), h), f32)
    qkv, b3, dqkv = rnd(rows, 3 * h), torch.zeros(3 * h, device=dev), ops.empty((rows, 3 * h), f32)
    ff, bf, dff = rnd(rows, f), torch.zeros(f, device=dev), rnd(rows, f)
    lens, lens_host = torch.full((batch,), t, dtype=torch.int32, device=dev), np.full((batch,), t, np.int32)
    dpatch = rnd(batch * (t - 1), 3 * d.patch ** 2)
    dimg = ops.empty((batch, hw, hw, 3), torch.bfloat16)
    total = 0.0
    for name, count, fn in (
            (f"xmc_mha_attention_bwd t={t}", L, lambda: ops.mha_attention_bwd(qkv, b3, lens, lens_host, dy, t, out=dqkv)),
            ("xmc_ln_bwd_add rows", 2 * L, lambda: ops.ln_bwd_add(x, g, dy, dres=dh, out=dh)),
            ("xmc_ln_bwd_add gather", 1, lambda: ops.ln_bwd_add(x, g, dpool, out=dh, mode="gather", t=t)),
            ("xmc_ln_bwd_add vision", 1, lambda: ops.ln_bwd_add(pe, g, dy, out=dpe, mode="vision", t=t, pos=pos)),
            ("xmc_bias_quick_gelu_bwd", L, lambda: ops.bias_quick_gelu_bwd(ff, bf, dff, out=dff)),
            (f"xmc_clip_preprocess_bwd {d.image_size}->{hw} bf16", 1,
             lambda: ops.clip_preprocess_bwd(dpatch, hw, d.image_size, d.patch, clip_arch.IMAGE_STD, out=dimg))):
        passes, seconds = timed(fn, window / 4)
        us = seconds / passes * 1e6
        total += us * count
        lines.append(f"backward kernel {name} B={batch}: {us:.1f} us x {count} = {us * count / 1e3:.3f} ms")
        print(lines[-1], flush=True)
    lines.append(f"backward kernels of csrc/clip_grad.hip in all: {total / 1e3:.3f} ms")
    print(lines[-1], flush=True)
    gemm_split(ops, d, batch, window, lines, False)


def step_times(params, batch, rounds, steps, lines):
    """the C1 step, graph replay, switch off and on in alternating rounds of ``steps`` replays each -> median ms/step"""
    from xmcgan_image_generation_amd import synthetic as syn, train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1
    rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)
    rstate = {"params": rp, "batch_stats": rs}
    runs = {}
    for name, lam in (("off", 0.0), ("on", 1.0)):
        cfg = coco_xmc.get_c1_config()
        cfg.batch_size = batch
        golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
        cfg.update(clip_guidance_weight=lam, clip_vocab_path=os.path.join(golden, "clip_bpe_vocab.json"),       # (check_config asks
                   clip_merges_path=os.path.join(golden, "clip_bpe_merges.txt"))      # for them; the text rows here are random)
        extra = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=batch).items()}
        if lam > 0.0:
            extra["clip_guidance"] = clip_utils.ClipGuidance(params, None, fast=True)
            tb["clip_text"] = torch.randn(tb["image"].shape[0], extra["clip_guidance"].proj, device="cuda")
        state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, extra)
        torch.cuda.synchronize()
        graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, extra)
        for _ in range(3):
            graphed(graphed.state)
        torch.cuda.synchronize()
        runs[name] = graphed
    ms = {"off": [], "on": []}
    for _ in range(rounds):
        for name in ("off", "on"):
            gr = runs[name]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                _, metrics = gr(gr.state)
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / steps)
    for name in ("off", "on"):
        lines.append(f"step C1 B={batch} bf16 graph replay, switch {name}: median {statistics.median(ms[name]):.2f} ms/step over "
                     f"{rounds} rounds of {steps} (min {min(ms[name]):.2f}, max {max(ms[name]):.2f})")
        print(lines[-1], flush=True)
    lines.append(f"step on - off = {statistics.median(ms['on']) - statistics.median(ms['off']):.2f} ms "
                 f"({statistics.median(ms['on']) / statistics.median(ms['off']):.3f} x); finite: "
                 f"{all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in metrics.values())}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=56)
    ap.add_argument("--image", type=int, default=128, help="side of the generated images")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per measurement (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="replays per round (x ~40 ms: a window of over a second)")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-tower", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    params = clip_arch.init_clip(0, vocab=1000)
    lines = [f"# tools/bench_clip_guidance.py on {torch.cuda.get_device_name(0)}: CLIP ViT-B/32 image tower (12 x 768, 50 tokens), random "
             f"weights, B = {a.batch}, {a.image} px"]
    if not a.skip_tower:
        tower_times(params, a.batch, a.image, a.window, lines)
    if not a.skip_step:
        step_times(params, a.batch, a.rounds, a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
