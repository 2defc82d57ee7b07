#!/usr/bin/env python
"""What the split BatchNorm kernels of cross-replica groups cost in ONE process (no collective): replayed C1 steps with
batch_norm_group_size = the batch (one replica = one group: bn_batch_sums + bn_finalize_rows per site, rows_mean per site in
the backward pass) beside replayed default steps, alternated window by window inside the same call.  Informational: the cost at
N > 1 (the all-gathers) is NOT what this measures.
usage: python tools/bench_syncbn_split.py [--steps 50] [--window 10] [--batch 56]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from xmcgan_image_generation_amd import synthetic as syn  # noqa: E402
from xmcgan_image_generation_amd import train_utils, xmc_gan  # noqa: E402
from xmcgan_image_generation_amd.configs import coco_xmc  # noqa: E402


def workload(group, batch):
    cfg = coco_xmc.get_c1_config()
    cfg.batch_size = batch
    cfg.batch_norm_group_size = group
    cfg.pretrained_image_contrastive = False          # the G/D step alone: BatchNorm lives in the generator only
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=batch).items()}
    state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    torch.cuda.synchronize()
    graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, {})
    return graphed, tb, cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--batch", type=int, default=56)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    runs = {"default (batch_norm_group_size = -1)": workload(-1, args.batch),
            f"groups (batch_norm_group_size = {args.batch})": workload(args.batch, args.batch)}
    states = {k: g.state for k, (g, _, _) in runs.items()}
    for k, (g, tb, _) in runs.items():                       # warm-up: every shape of the timed window
        for _ in range(3):
            states[k], _ = g(states[k], tb)
    torch.cuda.synchronize()
    total = {k: 0.0 for k in runs}
    windows = {k: [] for k in runs}
    for _ in range(args.steps // args.window):
        for k, (g, tb, _) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.window):
                states[k], m = g(states[k], tb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            total[k] += dt
            windows[k].append(1e3 * dt / args.window)
            assert all(torch.isfinite(v).all() for v in m.values())
    n = (args.steps // args.window) * args.window
    print(f"C1 (128 px, bf16, per-GPU batch {args.batch}, G/D step without the ResNet term), hipGraph replay, {n} steps each, "
          f"alternating windows of {args.window}:")
    for k in runs:
        print(f"  {k}: {1e3 * total[k] / n:.3f} ms/step   windows: " + " ".join(f"{w:.3f}" for w in windows[k]))


if __name__ == "__main__":
    main()
