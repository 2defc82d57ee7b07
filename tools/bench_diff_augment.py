#!/usr/bin/env python
"""What config.diff_augment costs.

  kernels  xmc_diffaug_fwd / xmc_diffaug_bwd alone at C1 (B = 56, 128 px, bf16) and C3 (B = 32, 256 px, bf16), colour off
           (one launch) and on (two): device events around --launches back-to-back calls, --warmup untimed rounds, then the
           median of --repeats timed ones, with the bytes each call moves.
  step     ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen ResNet-50 term on, hipGraph replay)
           with the switch off and on ("color,translation,cutout"), ALTERNATED in one process on one GPU -- off, on, off, on,
           ... -- so that clock and temperature drift hit both alike; every replay of the "on" step gets a new plan.

Prints one line per kernel measurement and one JSON line for the step.

    python tools/bench_diff_augment.py [--rounds 5] [--steps 20] [--repeats 5] [--warmup 2] [--launches 20] [--skip-step]"""
import argparse
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLICY = "color,translation,cutout"


def timed(fn, warmup, repeats, launches):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / launches)
    return st.median(us), us


def bench_kernels(args):
    import numpy as np
    import torch
    from xmcgan_image_generation_amd.libml import diff_augment as da
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    for name, b, hw in (("C1", 56, 128), ("C3", 32, 256)):
        gen = torch.Generator().manual_seed(b)
        real = (torch.rand((b, hw, hw, 3), generator=gen) * 2 - 1).to(torch.bfloat16).cuda()
        fake = (torch.rand((b, hw, hw, 3), generator=gen) * 2 - 1).to(torch.bfloat16).cuda()
        host = np.ascontiguousarray(da.draw_plan(1, 1, 0, b, hw, hw, POLICY).transpose(1, 0, 2).reshape(2 * b, 8))
        plan = torch.from_numpy(host).cuda()
        mb = b * hw * hw * 3 * 2 / 1e6                                   # one (B, H, W, 3) bf16 tensor
        for flags in (0, 7):
            passes = 2 if flags & 4 else 1
            for what, fn, moved in (("fwd", lambda: ops.diff_augment(real, fake, plan, host, flags), (2 * passes + 2) * mb),
                                    ("bwd", lambda: ops.diff_augment_bwd(fake, plan[b:], host[b:], flags), (passes + 1) * mb)):
                med, us = timed(fn, args.warmup, args.repeats, args.launches)
                print(f"kernel: xmc_diffaug_{what} {name} B={b} {hw}px bf16 flags={flags}: {med:.1f} us per call "
                      f"({passes} launch{'es' if passes > 1 else ''}; median of {args.repeats} x {args.launches} back-to-back calls: "
                      f"{', '.join(f'{v:.1f}' for v in us)}); {moved:.1f} MB moved, {moved / med:.2f} TB/s", flush=True)


def bench_step(args):
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.libml import diff_augment as da
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1

    def workload(policy):
        cfg = coco_xmc.get_c1_config()
        if args.batch:
            cfg.batch_size = args.batch
        cfg.diff_augment = policy
        rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)        # bench.py's random-initialised ResNet-50
        rstate = {"params": rp, "batch_stats": rs}
        additional = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size).items()}
        rows, hw = tb["image"].shape[0], cfg.image_size
        plans = [torch.from_numpy(da.draw_plan(0, s, 0, rows, hw, hw, policy)).pin_memory() for s in range(args.steps)] if policy else None
        if policy:
            tb["d_aug"] = plans[0]
        state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
        torch.cuda.synchronize()
        graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional)

        def run(n):                                                      # (``graphed`` keeps ``additional`` -- the ResNet-50's buffers -- alive)
            for i in range(n):
                if policy:                                               # a new plan per step, as train() draws one
                    graphed.static_batch["d_aug"].copy_(plans[i % len(plans)], non_blocking=True)
                graphed(graphed.state)
        run(args.step_warmup)
        torch.cuda.synchronize()
        return run

    def one_round(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    off, on = workload(""), workload(POLICY)
    rounds = {"off": [], "on": []}
    for _ in range(args.rounds):
        rounds["off"].append(one_round(off))
        rounds["on"].append(one_round(on))
    med = {k: st.median(v) for k, v in rounds.items()}
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained on graph replay", "policy": POLICY,
                      "steps_per_round": args.steps,
                      "ms_per_step_off": [round(v, 3) for v in rounds["off"]], "ms_per_step_on": [round(v, 3) for v in rounds["on"]],
                      "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
                      "cost_ms": round(med["on"] - med["off"], 3), "cost_percent": round(100 * (med["on"] / med["off"] - 1), 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if not args.skip_kernels:
        bench_kernels(args)
    if not args.skip_step:
        bench_step(args)


if __name__ == "__main__":
    main()
