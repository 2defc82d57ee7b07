#!/usr/bin/env python
"""What config.train_statistics costs: ms/step of the C1 training step (bench.py's workload: batch 56, bf16, the frozen ResNet-50
term on, hipGraph replay) with the switch off and on, ALTERNATED in one process on one GPU -- off, on, off, on, ... -- so that
clock and temperature drift hit both alike.  Prints one JSON line: per-round figures, the two medians and their difference.

    python tools/bench_train_statistics.py [--rounds 5] [--steps 20] [--batch 56] [--pretrained on|off]"""
import argparse
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--pretrained", default="on", choices=["on", "off"])
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
        cfg.train_statistics = on
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
        return graphed, additional

    def timed(graphed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            graphed(graphed.state)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    off, _ = workload(False)
    on, additional = workload(True)
    rounds = {"off": [], "on": []}
    for _ in range(args.rounds):
        rounds["off"].append(timed(off))
        rounds["on"].append(timed(on))
    window = additional["statistics"].read()
    med = {k: st.median(v) for k, v in rounds.items()}
    print(json.dumps({"workload": f"C1 batch {args.batch or 56} bf16 pretrained {args.pretrained} graph replay", "steps_per_round": args.steps,
                      "ms_per_step_off": [round(v, 3) for v in rounds["off"]], "ms_per_step_on": [round(v, 3) for v in rounds["on"]],
                      "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
                      "cost_ms": round(med["on"] - med["off"], 3), "cost_percent": round(100 * (med["on"] / med["off"] - 1), 2),
                      "statistic_steps": window["count"],
                      "d_grad_norm_mean": window["sums"]["d_grad_norm"] / max(window["count"], 1)}))


if __name__ == "__main__":
    main()
