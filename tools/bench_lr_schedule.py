#!/usr/bin/env python
"""What the schedules of libml/opt_schedule.py (config.lr_schedule, config.ema_ramp, ...) cost.

  advance  the scheduled advance kernel.  The ABI has no advance-only entry point, so it is measured where the Adam kernel behind
           it is one workgroup: xmc_adam_ema_dev against xmc_adam_ema_dev_sched on a 64-float arena, the two forms ALTERNATED.
  entries  each Adam entry point on the C1 arenas (gf = df = 96) in both forms, alternated: the flat form and the zeroing form on
           G's arena, the sigma form on D's arena, and the sigma form with the batched-preparation weights skipped + the tile
           form behind it.  Device events around --launches back-to-back calls, --warmup untimed rounds, the median of --repeats.
  step     ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen ResNet-50 term on, hipGraph replay)
           with every key absent -- the parent's step, the yardstick -- and the same step with a cosine schedule, a warm-up and
           an EMA ramp, ALTERNATED in one process on one GPU -- parent, scheduled, parent, scheduled, ... -- so that clock and
           temperature drift hit both alike.

Prints one line per kernel measurement and one JSON line for the step.

    python tools/bench_lr_schedule.py [--rounds 5] [--steps 20] [--repeats 5] [--warmup 2] [--launches 20] [--breakdown] [--skip-step]"""
import argparse
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = dict(lr_schedule="cosine", lr_warmup_steps=1000, lr_decay_start_step=1000, lr_decay_end_step=100000, lr_final_ratio=0.1,
            ema_ramp=10.0, ema_start_step=100)
BETAS = dict(beta1=0.5, beta2=0.999)


def one(fn, launches):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def alternated(name, parent, sched, args):
    """parent, scheduled, parent, scheduled, ...: us per call, median and every round"""
    import torch
    for _ in range(args.warmup):
        parent()
        sched()
    torch.cuda.synchronize()
    us = {"parent": [], "scheduled": []}
    for _ in range(args.repeats):
        us["parent"].append(one(parent, args.launches))
        us["scheduled"].append(one(sched, args.launches))
    mp, ms = st.median(us["parent"]), st.median(us["scheduled"])
    spread = max(max(v) - min(v) for v in us.values())
    print(f"{name}: parent {mp:.2f} us, scheduled {ms:.2f} us per call, difference {ms - mp:+.2f} us (spread between rounds "
          f"{spread:.2f} us; parent {', '.join(f'{v:.2f}' for v in us['parent'])}; scheduled "
          f"{', '.join(f'{v:.2f}' for v in us['scheduled'])})", flush=True)


def bench_kernels(args):
    import torch
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.libml import opt_schedule
    cfg = coco_xmc.get_c1_config()
    cfg.update(KEYS)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    d = disc(train=True)
    ops = d.ops
    sg = opt_schedule.for_optimizer(cfg, "g", cfg.g_lr, cfg.polyak_decay)
    sd = opt_schedule.for_optimizer(cfg, "d", cfg.d_lr, 0.0)
    host = dict(lr=cfg.g_lr, ema_decay=cfg.polyak_decay)

    def state8():
        return torch.zeros((8,), dtype=torch.float32, device="cuda")

    # the advance kernel: a 64-float arena, where the Adam kernel is one workgroup
    t = {k: torch.zeros((64,), device="cuda") for k in ("p", "g", "m", "v", "ema")}
    s0, s1 = state8(), state8()
    alternated("advance (64-float arena: advance + a one-workgroup Adam kernel)",
               lambda: ops.adam_ema_dev(t["p"], t["g"], t["m"], t["v"], t["ema"], s0, **host, **BETAS),
               lambda: ops.adam_ema_dev_sched(t["p"], t["g"], t["m"], t["v"], t["ema"], s1, sg, **BETAS), args)

    ga, da = state.g_optimizer.arena, state.d_optimizer.arena
    g_grads, d_grads = torch.randn_like(ga.params) * 1e-3, torch.randn_like(da.params) * 1e-3
    ema = ga.params.clone()
    s0, s1 = state8(), state8()
    n_g = f"G's arena, {ga.size * 4 / 2 ** 20:.0f} MiB per buffer, with EMA"
    alternated(f"xmc_adam_ema_dev ({n_g})",
               lambda: ops.adam_ema_dev(ga.params, g_grads, ga.m, ga.v, ema, s0, **host, **BETAS),
               lambda: ops.adam_ema_dev_sched(ga.params, g_grads, ga.m, ga.v, ema, s1, sg, **BETAS), args)
    alternated(f"xmc_adam_ema_dev_sn, no table ({n_g})",
               lambda: ops.adam_ema_dev_sn(ga.params, g_grads, ga.m, ga.v, ema, s0, zero_grads=False, **host, **BETAS),
               lambda: ops.adam_ema_dev_sn_sched(ga.params, g_grads, ga.m, ga.v, ema, s1, sg, zero_grads=False, **BETAS), args)
    # D: u, v, sigma of one forward's power iteration; kvec once (xmc_sn_batched_dot is not part of either form)
    params, sn = state.d_optimizer.target, state.discriminator_state["spectral_norm_stats"]
    d._bind(params)
    d.prepare(params, sn)
    _, u, v, scal = d._sn_ctx[:4]
    kvec = ops.sn_bank_dot(d.bank, da.params, d_grads, scal)
    host_d = dict(lr=cfg.d_lr, ema_decay=0.0)
    n_d = f"D's arena, {da.size * 4 / 2 ** 20:.0f} MiB per buffer, no EMA"
    fix = (d.sn_map, d.bank, kvec, scal, u, v)
    alternated(f"xmc_adam_ema_dev_sn, sigma table ({n_d})",
               lambda: ops.adam_ema_dev_sn(da.params, d_grads, da.m, da.v, None, s0, zero_grads=False, fix=fix, **host_d, **BETAS),
               lambda: ops.adam_ema_dev_sn_sched(da.params, d_grads, da.m, da.v, None, s1, sd, zero_grads=False, fix=fix, **BETAS), args)
    skip = ops.wprep_skip_map(d.wp, da.size, base=d.sn_map)
    out = ops.wprep_alloc(d.wp)
    fix, tfix = (skip, d.bank, kvec, scal, u, v), (kvec, scal, u, v)

    def tiles_parent():
        ops.adam_ema_dev_sn(da.params, d_grads, da.m, da.v, None, s0, zero_grads=False, fix=fix, **host_d, **BETAS)
        ops.adam_wprep(d.wp, out, da.params, d_grads, da.m, da.v, None, s0, zero_grads=False, fix=tfix, **host_d, **BETAS)

    def tiles_sched():
        ops.adam_ema_dev_sn_sched(da.params, d_grads, da.m, da.v, None, s1, sd, zero_grads=False, fix=fix, **BETAS)
        ops.adam_wprep_sched(d.wp, out, da.params, d_grads, da.m, da.v, None, s1, zero_grads=False, fix=tfix, **BETAS)
    alternated(f"xmc_adam_ema_dev_sn with the prepared weights skipped + xmc_adam_wprep_tiles ({n_d})", tiles_parent, tiles_sched, args)


def bench_step(args):
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.libml import opt_schedule
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1

    def workload(keys):
        cfg = coco_xmc.get_c1_config()
        if args.batch:
            cfg.batch_size = args.batch
        cfg.update(keys)
        rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)        # bench.py's random-initialised ResNet-50
        rstate = {"params": rp, "batch_stats": rs}
        additional = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size).items()}
        state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
        torch.cuda.synchronize()
        graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional)

        def run(n):                                                      # (``graphed`` keeps ``additional`` -- the ResNet-50's buffers -- alive)
            for _ in range(n):
                graphed(graphed.state)
        run(args.step_warmup)
        torch.cuda.synchronize()
        return run, graphed, cfg

    def one_round(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    (parent, _, _), (sched, graphed, cfg) = workload({}), workload(KEYS)
    rounds = {"parent": [], "scheduled": []}
    extra = {}
    if args.breakdown:
        # where a difference comes from: a SECOND parent step built after the others (what the order of construction alone does), and
        # the scheduled step with a CONSTANT descriptor -- the scheduled launches and kernels, but the parent's rates, so the parent's
        # values bit for bit: what is left between it and the full schedule is what the VALUES of a step at another rate cost
        extra = {"parent_again": workload({})[0], "scheduled_constant": workload(dict(lr_schedule="constant"))[0]}
        rounds.update({k: [] for k in extra})
    for _ in range(args.rounds):
        rounds["parent"].append(one_round(parent))
        rounds["scheduled"].append(one_round(sched))
        for k, run in extra.items():
            rounds[k].append(one_round(run))
    med = {k: st.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained on graph replay", "schedule": KEYS,
                      "steps_per_round": args.steps,
                      "ms_per_step_parent": [round(v, 3) for v in rounds["parent"]],
                      "ms_per_step_scheduled": [round(v, 3) for v in rounds["scheduled"]],
                      "median_parent": round(med["parent"], 3), "median_scheduled": round(med["scheduled"], 3),
                      "spread_parent": round(spread["parent"], 3), "spread_scheduled": round(spread["scheduled"], 3),
                      **{f"ms_per_step_{k}": [round(v, 3) for v in rounds[k]] for k in extra},
                      **{f"median_{k}": round(med[k], 3) for k in extra},
                      "paired_cost_ms": [round(a - b, 3) for a, b in zip(rounds["scheduled"], rounds["parent"])],
                      "cost_ms": round(med["scheduled"] - med["parent"], 3),
                      "cost_percent": round(100 * (med["scheduled"] / med["parent"] - 1), 2),
                      "rates_after_the_rounds": train_utils.optimizer_rates(graphed.state, cfg),
                      "updates_g_d": [graphed.state.g_optimizer.arena.sync_opt_step(), graphed.state.d_optimizer.arena.sync_opt_step()],
                      "specification_at_those_updates": [
                          float(opt_schedule.evaluate(opt_schedule.for_optimizer(cfg, "g", cfg.g_lr, 0.0), graphed.state.g_optimizer.arena.opt_step)[0]),
                          float(opt_schedule.evaluate(opt_schedule.for_optimizer(cfg, "d", cfg.d_lr, 0.0), graphed.state.d_optimizer.arena.opt_step)[0])]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--breakdown", action="store_true", help="two more alternated steps: the parent again, and the scheduled step with a constant descriptor")
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
