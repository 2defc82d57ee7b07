#!/usr/bin/env python
"""What config.lecam_weight costs.

  kernel   xmc_lecam alone at the C1 batch (B = 56), active phase (the form that reads and writes dld): device events around
           --launches back-to-back calls, --warmup untimed rounds, then the median of --repeats timed ones.
  step     ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen ResNet-50 term on, hipGraph replay)
           with the key absent -- the parent's step, the yardstick -- and the same step with lecam_weight = 0.3, ALTERNATED in one
           process on one GPU -- parent, lecam, parent, lecam, ... -- so that clock and temperature drift hit both alike.

Prints one line for the kernel measurement and one JSON line for the step.

    python tools/bench_lecam.py [--rounds 5] [--steps 20] [--repeats 5] [--warmup 2] [--launches 20] [--breakdown] [--skip-step]"""
import argparse
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT = 0.3


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


def bench_kernel(args):
    import torch
    from xmcgan_image_generation_amd.libml import lecam
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    b = args.batch or 56
    state = torch.zeros((lecam.STATE_WIDTH,), dtype=torch.float64, device="cuda")
    logit = torch.randn((2 * b,), device="cuda")
    dld = torch.zeros((2 * b,), device="cuda")
    ops.lecam(logit, dld, b, state, WEIGHT, lecam.DECAY, 0, False)       # the first update: every later call is active
    for what, one_sided in (("two-sided", False), ("one-sided", True)):
        med, us = timed(lambda: ops.lecam(logit, dld, b, state, WEIGHT, lecam.DECAY, 0, one_sided), args.warmup, args.repeats, args.launches)
        print(f"kernel: xmc_lecam {what} B={b}: {med:.1f} us per call (1 launch + the torch.zeros of its loss slot; median of "
              f"{args.repeats} x {args.launches} back-to-back calls: {', '.join(f'{v:.1f}' for v in us)})", flush=True)


def bench_step(args):
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1

    def workload(weight, start=0, zero_weight=False, nonzero_dld=False):
        from xmcgan_image_generation_amd.libml import losses
        cfg = coco_xmc.get_c1_config()
        if args.batch:
            cfg.batch_size = args.batch
        if weight:
            cfg.lecam_weight = weight
        if start:
            cfg.lecam_start = start
        rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)        # bench.py's random-initialised ResNet-50
        rstate = {"params": rp, "batch_stats": rs}
        additional = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        if zero_weight:                                                  # the ACTIVE launch with lambda = 0: dld is read, takes 0 * d and
            state.lecam.settings["weight"] = 0.0                         # is written back with the parent's values (the config reads 0 as off)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size).items()}
        plain = losses.hinge_loss
        if nonzero_dld:
            # the parent's step, no xmc_lecam, but dld takes a fixed nowhere-zero vector of the term's size (one torch add, captured
            # with the step): what D's gradient VALUES alone do to the step's time
            noise = (torch.randn((2 * cfg.batch_size,), device="cuda") * (2 * WEIGHT / cfg.batch_size)).contiguous()

            def perturbed(ops, logit, b, d_acc, g_acc):
                dld, dlg = plain(ops, logit, b, d_acc, g_acc)
                dld.add_(noise)
                return dld, dlg
            losses.hinge_loss = perturbed
        try:
            state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)   # (the first update: active from here on)
            torch.cuda.synchronize()
            graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional)
        finally:
            losses.hinge_loss = plain

        def zeros_in_dld():
            """one more EAGER step from the replayed state: the share of exactly-zero elements in what the hinge launch writes"""
            seen = []

            def recording(ops, logit, b, d_acc, g_acc):
                dld, dlg = plain(ops, logit, b, d_acc, g_acc)
                seen.append(round(float((dld == 0).float().mean()), 4))
                return dld, dlg
            losses.hinge_loss = recording
            try:
                train_utils.train_step(0, graphed.state, tb, xmc_gan, gen, disc, cfg, additional)
                torch.cuda.synchronize()
            finally:
                losses.hinge_loss = plain
            return seen

        def run(n):                                                      # (``graphed`` keeps ``additional`` -- the ResNet-50's buffers -- alive)
            for _ in range(n):
                graphed(graphed.state)
        run(args.step_warmup)
        torch.cuda.synchronize()
        return run, (state.lecam if weight else None), zeros_in_dld

    def one_round(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    (parent, _, parent_zeros), (with_term, ctl, _) = workload(0.0), workload(WEIGHT)
    rounds = {"parent": [], "lecam": []}
    extra = {}
    if args.breakdown:
        # where a difference comes from: a SECOND parent step built after the others (what the order of construction alone does);
        # the term held in its warm-up for the whole run (the launch is there and moves the anchors, but dld is not touched); and
        # the active launch with lambda = 0 (the whole kernel, dld rewritten, but D's gradient is the parent's); and the parent's step
        # with a nowhere-zero dld and no xmc_lecam at all
        extra = {"parent_again": workload(0.0)[0], "lecam_warm_up_only": workload(WEIGHT, start=1 << 30)[0],
                 "lecam_active_weight_zero": workload(WEIGHT, zero_weight=True)[0],
                 "parent_with_nonzero_dld": workload(0.0, nonzero_dld=True)[0]}
        rounds.update({k: [] for k in extra})
    for _ in range(args.rounds):
        rounds["parent"].append(one_round(parent))
        rounds["lecam"].append(one_round(with_term))
        for k, run in extra.items():
            rounds[k].append(one_round(run))
    med = {k: st.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained on graph replay", "lecam_weight": WEIGHT,
                      "steps_per_round": args.steps,
                      "ms_per_step_parent": [round(v, 3) for v in rounds["parent"]], "ms_per_step_lecam": [round(v, 3) for v in rounds["lecam"]],
                      "median_parent": round(med["parent"], 3), "median_lecam": round(med["lecam"], 3),
                      "spread_parent": round(spread["parent"], 3), "spread_lecam": round(spread["lecam"], 3),
                      **{f"ms_per_step_{k}": [round(v, 3) for v in rounds[k]] for k in extra},
                      **{f"median_{k}": round(med[k], 3) for k in extra},
                      "paired_cost_ms": [round(a - b, 3) for a, b in zip(rounds["lecam"], rounds["parent"])],
                      "cost_ms": round(med["lecam"] - med["parent"], 3), "cost_percent": round(100 * (med["lecam"] / med["parent"] - 1), 2),
                      **({"parent_share_of_zero_dld_elements_per_half_step_after_the_rounds": parent_zeros()} if args.breakdown else {}),
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
    ap.add_argument("--breakdown", action="store_true", help="four more alternated steps (parent again, warm-up only, active with lambda = 0, parent with a nonzero dld) and the parent's share of zeros in dld")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if not args.skip_kernel:
        bench_kernel(args)
    if not args.skip_step:
        bench_step(args)


if __name__ == "__main__":
    main()
