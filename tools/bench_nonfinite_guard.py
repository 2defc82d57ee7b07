#!/usr/bin/env python
"""What config.skip_nonfinite_updates costs: (1) ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen
ResNet-50 term on, hipGraph replay) with the switch off and on, ALTERNATED in one process on one GPU -- off, on, off, on, ... -- so
that clock and temperature drift hit both alike; (2) xmc_nonfinite_verdict alone on C1's arenas (the train_d table, the train_g_d
table), HIP events around batches of launches, against the floor (bytes scanned) / (HBM rate of profiles/r02_hbm_bw_probe.txt).
Prints one JSON line.

    python tools/bench_nonfinite_guard.py [--rounds 5] [--steps 20] [--batch 56] [--pretrained on|off] [--kernel-iters 2000]"""
import argparse
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# profiles/r02_hbm_bw_probe.txt has no read-only line; its "copy" line (bytes read + bytes written per second) is the rate used
HBM_TBPS = 5.218


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--pretrained", default="on", choices=["on", "off"])
    ap.add_argument("--kernel-iters", type=int, default=2000)
    args = ap.parse_args()
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    torch.cuda.set_device(0)

    def workload(on):
        cfg = coco_xmc.get_c1_config()
        if args.batch:
            cfg.batch_size = args.batch
        cfg.pretrained_image_contrastive = False         # (create_additional_data would look for the checkpoint file)
        cfg.skip_nonfinite_updates = on
        additional = xmc_gan.create_additional_data(cfg)
        cfg.pretrained_image_contrastive = args.pretrained == "on"
        if cfg.pretrained_image_contrastive:             # bench.py's random-initialised ResNet-50
            from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1
            rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)
            state = {"params": rp, "batch_stats": rs}
            additional.update({"image_model": pretrained_model_utils.ImageModel(state), "image_model_state": state})
        gen, disc, state = train_utils.create_train_state(cfg, 0)
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size).items()}
        state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
        torch.cuda.synchronize()
        graphed = train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional)
        for _ in range(args.warmup):
            graphed(graphed.state)
        torch.cuda.synchronize()
        return graphed, gen(train=True).ops

    def timed(graphed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            graphed(graphed.state)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    off, _ = workload(False)
    on, ops = workload(True)
    rounds = {"off": [], "on": []}
    for _ in range(args.rounds):
        rounds["off"].append(timed(off))
        rounds["on"].append(timed(on))
    med = {k: st.median(v) for k, v in rounds.items()}
    state = on.state
    skipped = state.guard.read()

    # ---- the verdict kernel alone, on the arenas the guarded step scans
    da, ga = state.d_optimizer.arena, state.g_optimizer.arena
    u0 = state.discriminator_state["spectral_norm_stats"].flat
    bn = state.generator_state["batch_stats"].flat
    da.grads.zero_()                                     # (finite contents: a first-write arena may hold anything between steps)
    ga.grads.zero_()
    verdict = torch.zeros((4,), dtype=torch.int32, device="cuda")
    counters = torch.zeros((4,), dtype=torch.int32, device="cuda")
    kernel = {}
    for name, segs in (("train_d", [da.grads, u0, bn]), ("train_g_d", [da.grads, ga.grads, u0, bn])):
        ws = torch.empty((ops.nonfinite_verdict_ws_bytes([t.numel() for t in segs]),), dtype=torch.uint8, device="cuda")
        for _ in range(5):
            ops.nonfinite_verdict(segs, verdict, counters, ws)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_iters):
            ops.nonfinite_verdict(segs, verdict, counters, ws)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / args.kernel_iters * 1e3
        nbytes = 4 * sum(t.numel() for t in segs)
        kernel[name] = {"mb": round(nbytes / 1e6, 1), "us": round(us, 1), "tb_per_s": round(nbytes / us / 1e6, 3),
                        "floor_us": round(nbytes / HBM_TBPS / 1e6, 1)}
    assert verdict.cpu().tolist() == [0, 0, -1, 0]
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained {args.pretrained} graph replay", "steps_per_round": args.steps,
                      "ms_per_step_off": [round(v, 3) for v in rounds["off"]], "ms_per_step_on": [round(v, 3) for v in rounds["on"]],
                      "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
                      "cost_ms": round(med["on"] - med["off"], 3), "cost_percent": round(100 * (med["on"] / med["off"] - 1), 2),
                      "half_steps_skipped": skipped["skipped"], "verdict_kernel": kernel, "floor_rate_tb_per_s": HBM_TBPS}))


if __name__ == "__main__":
    main()
