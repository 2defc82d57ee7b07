#!/usr/bin/env python
"""What config.ada_target costs on top of config.diff_augment.

  kernels  xmc_ada_gate / xmc_ada_update alone at the C1 batch (B = 56): device events around --launches back-to-back calls,
           --warmup untimed rounds, then the median of --repeats timed ones.
  step     ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen ResNet-50 term on, hipGraph replay)
           with diff_augment = "color,translation,cutout" -- the parent's step, the yardstick -- and the same step with
           ada_target = 0.6, ALTERNATED in one process on one GPU -- parent, ada, parent, ada, ... -- so that clock and temperature
           drift hit both alike; every replay gets a new plan (and the "ada" step new gate uniforms).

Prints one line per kernel measurement and one JSON line for the step.

    python tools/bench_ada.py [--rounds 5] [--steps 20] [--repeats 5] [--warmup 2] [--launches 20] [--breakdown] [--skip-step]"""
import argparse
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLICY = "color,translation,cutout"
TARGET = 0.6


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
    import torch
    from xmcgan_image_generation_amd.libml import ada, diff_augment as da
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    b = args.batch or 56
    plan = torch.from_numpy(da.draw_plan(1, 1, 0, b, 128, 128, POLICY)).cuda()
    u = torch.from_numpy(ada.draw_gates(1, 1, 0, b)).cuda()
    state = torch.zeros((8,), dtype=torch.float64, device="cuda")
    state[0] = 0.3
    logit = torch.randn((2 * b,), device="cuda")
    for what, fn in (("xmc_ada_gate", lambda: ops.ada_gate(plan, u, state)),
                     ("xmc_ada_update", lambda: ops.ada_update(logit, b, state, TARGET, 500000.0, 4, ada.P_MAX)),
                     ("torch transpose + copy (what the gate replaces)", lambda: plan.transpose(0, 1).reshape(2 * b, 8))):
        med, us = timed(fn, args.warmup, args.repeats, args.launches)
        print(f"kernel: {what} B={b}: {med:.1f} us per call (1 launch; median of {args.repeats} x {args.launches} back-to-back "
              f"calls: {', '.join(f'{v:.1f}' for v in us)})", flush=True)


def bench_step(args):
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.libml import ada, diff_augment as da
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1

    def workload(target, copy_gates=True):
        cfg = coco_xmc.get_c1_config()
        if args.batch:
            cfg.batch_size = args.batch
        cfg.diff_augment = POLICY
        if target:
            cfg.ada_target = target
        rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)        # bench.py's random-initialised ResNet-50
        rstate = {"params": rp, "batch_stats": rs}
        additional = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        if target:
            state.ada.state[0] = 0.3                                     # (a p at which some parts are gated and some are not)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size).items()}
        rows, hw = tb["image"].shape[0], cfg.image_size
        plans = [torch.from_numpy(da.draw_plan(0, s, 0, rows, hw, hw, POLICY)).pin_memory() for s in range(args.steps)]
        gates = [torch.from_numpy(ada.draw_gates(0, s, 0, rows)).pin_memory() for s in range(args.steps)] if target else None
        tb["d_aug"] = plans[0]
        if target:
            tb["d_aug_u"] = gates[0]
        state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
        torch.cuda.synchronize()
        graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional)

        def run(n):                                                      # (``graphed`` keeps ``additional`` -- the ResNet-50's buffers -- alive)
            for i in range(n):
                graphed.static_batch["d_aug"].copy_(plans[i % len(plans)], non_blocking=True)   # a new plan per step, as train() draws one
                if target and copy_gates:
                    graphed.static_batch["d_aug_u"].copy_(gates[i % len(gates)], non_blocking=True)
                graphed(graphed.state)
        run(args.step_warmup)
        torch.cuda.synchronize()
        return run, (state.ada if target else None)

    def one_round(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    (parent, _), (adaptive, ctl) = workload(0.0), workload(TARGET)
    rounds = {"parent": [], "ada": []}
    extra = None
    if args.breakdown:                                                   # where the difference goes: the same step, but the uniforms of
        extra, _ = workload(TARGET, copy_gates=False)                    # the capture stay in the static batch (no copy per replay)
        rounds["ada_without_the_gate_copy"] = []
    for _ in range(args.rounds):
        rounds["parent"].append(one_round(parent))
        rounds["ada"].append(one_round(adaptive))
        if extra is not None:
            rounds["ada_without_the_gate_copy"].append(one_round(extra))
    med = {k: st.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained on graph replay", "policy": POLICY, "ada_target": TARGET,
                      "steps_per_round": args.steps,
                      "ms_per_step_parent": [round(v, 3) for v in rounds["parent"]], "ms_per_step_ada": [round(v, 3) for v in rounds["ada"]],
                      "median_parent": round(med["parent"], 3), "median_ada": round(med["ada"], 3),
                      "spread_parent": round(spread["parent"], 3), "spread_ada": round(spread["ada"], 3),
                      **({"ms_per_step_ada_without_the_gate_copy": [round(v, 3) for v in rounds["ada_without_the_gate_copy"]],
                          "median_ada_without_the_gate_copy": round(med["ada_without_the_gate_copy"], 3)} if extra is not None else {}),
                      "paired_cost_ms": [round(a - b, 3) for a, b in zip(rounds["ada"], rounds["parent"])],
                      "cost_ms": round(med["ada"] - med["parent"], 3), "cost_percent": round(100 * (med["ada"] / med["parent"] - 1), 2),
                      "controller": ctl.read()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--breakdown", action="store_true", help="a third alternated step: ada without the per-replay copy of the uniforms")
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
