#!/usr/bin/env python
"""What config.ada_target + config.lecam_weight + config.skip_nonfinite_updates cost WITH the replicas' exchange around them
(DESIGN.md 9f.3), as far as one GPU can show it: world 1 on RCCL, dp.GradSync(schedule="exclusive").

  kernels  xmc_ada_update_rows, xmc_lecam_rows, xmc_verdict_merge with one row at the C1 batch (B = 56) and one
           GradSync.gather_rows of the (2B,) logit vector at world 1: device events around --launches back-to-back calls,
           --warmup untimed rounds, then the median of --repeats timed ones.
  step     ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen ResNet-50 term on, hipGraph replay)
           with config.diff_augment on and the exclusive exchange at world 1 -- switches OFF (a step the parent commit runs too)
           against the same step with the three switches ON, ALTERNATED in one process: off, on, off, on, ...  With the switches
           on every half step captures two more all-gathers (logits, verdicts) and the three one-row kernels.

A world of one exchanges nothing: the all-gathers' cost here is their launch, not a transfer.  The cost at N > 1 ranks is NOT
measured by this tool (RCCL with more than one rank has never run on this project's hardware).

Prints one line per kernel and one JSON line for the step.

    python tools/bench_replica_controllers.py [--rounds 5] [--steps 20] [--repeats 5] [--warmup 2] [--launches 20]"""
import argparse
import json
import os
import statistics as st
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLICY = "color,translation,cutout"
SWITCHES = dict(ada_target=0.6, lecam_weight=0.3, skip_nonfinite_updates=True)


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


def bench_kernels(args, sync):
    import torch
    from xmcgan_image_generation_amd.libml import ada, lecam
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    b = args.batch or 56
    logit = torch.randn((2 * b,), device="cuda")
    rows = logit.view(1, -1)
    dld = torch.zeros((2 * b,), device="cuda")
    a_state = torch.zeros((ada.STATE_WIDTH,), dtype=torch.float64, device="cuda")
    l_state = torch.zeros((lecam.STATE_WIDTH,), dtype=torch.float64, device="cuda")
    ops.lecam_rows(rows, 0, dld, b, l_state, 0.3, lecam.DECAY, 0, False)  # the first update: every later call is active
    local = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    verdict, counters = torch.zeros((4,), dtype=torch.int32, device="cuda"), torch.zeros((4,), dtype=torch.int32, device="cuda")
    calls = {"xmc_ada_update_rows (1 launch)": lambda: ops.ada_update_rows(rows, b, a_state, 0.6, 500000.0, 4, ada.P_MAX),
             "xmc_lecam_rows (1 launch + the torch.zeros of its loss slot)": lambda: ops.lecam_rows(rows, 0, dld, b, l_state, 0.3, lecam.DECAY, 0, False),
             "xmc_verdict_merge (1 launch)": lambda: ops.verdict_merge(local, verdict, counters),
             f"GradSync.gather_rows of ({2 * b},) float32 (torch.empty + one RCCL all-gather, eager)": lambda: sync.gather_rows(logit),
             "GradSync.gather_rows of (4,) int32 (eager)": lambda: sync.gather_rows(local[0])}
    for what, fn in calls.items():
        med, us = timed(fn, args.warmup, args.repeats, args.launches)
        print(f"kernel: {what}, world 1, B={b}: {med:.1f} us per call (median of {args.repeats} x {args.launches} back-to-back "
              f"calls: {', '.join(f'{v:.1f}' for v in us)})", flush=True)


def bench_step(args, sync):
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.libml import ada, diff_augment
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1

    def workload(on):
        cfg = coco_xmc.get_c1_config()
        if args.batch:
            cfg.batch_size = args.batch
        cfg.diff_augment = POLICY
        if on:
            cfg.update(SWITCHES)
        rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)        # bench.py's random-initialised ResNet-50
        rstate = {"params": rp, "batch_stats": rs}
        additional = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size).items()}
        rows = cfg.batch_size * cfg.d_step_per_g_step
        tb["d_aug"] = torch.from_numpy(diff_augment.draw_plan(3, 0, 0, rows, cfg.image_size, cfg.image_size, POLICY))
        if on:
            tb["d_aug_u"] = torch.from_numpy(ada.draw_gates(3, 0, 0, rows))
        state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional, grad_sync=sync)
        torch.cuda.synchronize()
        graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional, grad_sync=sync)

        def run(n):                                                      # (``graphed`` keeps ``additional`` -- the ResNet-50's buffers -- alive)
            for _ in range(n):
                graphed(graphed.state)
        run(args.step_warmup)
        torch.cuda.synchronize()
        return run, graphed.state

    def one_round(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    (off, _), (on, state) = workload(False), workload(True)
    rounds = {"off": [], "on": []}
    for _ in range(args.rounds):
        rounds["off"].append(one_round(off))
        rounds["on"].append(one_round(on))
    med = {k: st.median(v) for k, v in rounds.items()}
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained, diff_augment {POLICY}, graph replay, world 1 on RCCL, "
                                  "GradSync(schedule='exclusive')", "switches": SWITCHES, "steps_per_round": args.steps,
                      "ms_per_step_off": [round(v, 3) for v in rounds["off"]], "ms_per_step_on": [round(v, 3) for v in rounds["on"]],
                      "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
                      "spread_off": round(max(rounds["off"]) - min(rounds["off"]), 3),
                      "spread_on": round(max(rounds["on"]) - min(rounds["on"]), 3),
                      "paired_cost_ms": [round(a - b, 3) for a, b in zip(rounds["on"], rounds["off"])],
                      "cost_ms": round(med["on"] - med["off"], 3), "cost_percent": round(100 * (med["on"] / med["off"] - 1), 2),
                      "cost_at_more_than_one_rank": "not measured",
                      "ada": state.ada.read(), "lecam": state.lecam.read(), "guard": state.guard.read()}))


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
    if args.rounds < 5:
        ap.error("--rounds must be at least 5: the medians are of alternated rounds")
    import torch
    import torch.distributed as dist
    from xmcgan_image_generation_amd import dp
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("nccl", init_method=f"file://{tmp}/store", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        try:
            sync = dp.GradSync(schedule="exclusive")
            if not args.skip_kernels:
                bench_kernels(args, sync)
            if not args.skip_step:
                bench_step(args, sync)
        finally:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
