#!/usr/bin/env python
"""The device-resident dataset cache (config.device_dataset_cache, libml/device_cache.py) against the host input pipeline, on the
GPU box: one process, the two modes alternated.

  fill    seconds and records/s of the cache fill over generated 640 x 480 PNG records (the shard generator of
          tools/bench_input_pipeline.py, its records repeated to --examples x --repeat), next to the host pipeline's examples/s
          in the same decode layout (--procs x --threads)
  stream  examples/s of the cached training iterator (one planning thread, batches gathered on the device)
  kernel  time per xmc_cache_gather launch at N = 112, 128 px (device events over --launches launches) and the bytes it moves;
          `--only kernel` runs nothing else, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python ...)
  loop    ms/step of a C1 training loop (graph replay, ResNet-50 term on, random initialisation) fed by the cache and by the
          host pipeline, alternated

usage: python tools/bench_device_cache.py [--only fill,stream,kernel,loop] [--examples 256] [--repeat 32] [--procs 16] [--threads 1]"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_input_pipeline import write_shards  # noqa: E402
from xmcgan_image_generation_amd.configs import coco_xmc  # noqa: E402
from xmcgan_image_generation_amd.libml import coco_dataset, device_cache, input_pipeline  # noqa: E402


def make_shards(d, examples, repeat, nshard):
    """``examples`` distinct generated records in ``nshard`` training shards, each shard present ``repeat`` times (links to one
    file under further shard names): decoding a record twice costs what decoding two records costs, generating one costs far
    more than decoding it, and the set stays small on disk"""
    os.makedirs(os.path.join(d, "once"))
    write_shards(os.path.join(d, "once"), examples, nshard, np.random.default_rng(0))
    for name in sorted(os.listdir(os.path.join(d, "once"))):
        stem, k = name.split(".tfrecord-")
        for r in range(repeat if "train" in name else 1):
            os.symlink(os.path.join(d, "once", name), os.path.join(d, f"{stem}.tfrecord-r{r:03d}-{k}"))
    return examples // nshard * nshard * repeat


def host_rate(cfg, procs, threads, batches):
    """examples/s of create_datasets' training iterator; with processes: warm-up and timing over whole rounds of the workers"""
    it, _, _ = input_pipeline.create_datasets(cfg, data_rng=1, workers=threads, procs=procs, prefetch=4)
    per = cfg.batch_size * cfg.d_step_per_g_step
    rounds = max(1, procs)
    for _ in range(2 * rounds + 2):
        next(it)
    nb = rounds * max(5, -(-batches // rounds))
    t0 = time.perf_counter()
    for _ in range(nb):
        next(it)
    return nb * per / (time.perf_counter() - t0), it


def bench_kernel(launches):
    from xmcgan_image_generation_amd import ops
    n, hw, s, t, e, slots = 112, 128, 5, 17, 768, 512
    g = torch.Generator(device="cuda").manual_seed(0)
    dev = (torch.rand((slots, hw, hw, 3), device="cuda", generator=g), torch.randn((slots, s, t, e), device="cuda", generator=g),
           torch.randn((slots, s, e), device="cuda", generator=g), torch.ones((slots, s), device="cuda"))
    rng = np.random.default_rng(0)
    plans = []
    for _ in range(8):
        p = np.zeros((n, device_cache.PLAN_STRIDE), np.int32)
        p[:, 0], p[:, 1], p[:, 2] = rng.permutation(slots)[:n], rng.integers(0, s, n), rng.integers(0, 2, n)
        p[:, 3], p[:, 4], p[:, 5] = rng.integers(0, 9, n), rng.integers(0, 9, n), rng.integers(0, 2, n)
        plans.append((torch.from_numpy(p).cuda(), p))
    for pd, ph in plans:
        ops.cache_gather(*dev, pd, ph)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        ops.cache_gather(*dev, *plans[i % len(plans)])
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / launches
    img, cap = n * hw * hw * 3 * 4, n * (t * e + e + 1) * 4
    print(f"kernel: xmc_cache_gather N={n} {hw}px S,T,E={s},{t},{e}: {us:.1f} us per launch over {launches} back-to-back launches "
          f"(device events; includes the launch gaps).  Bytes by shape: writes {2 * img + cap} (image + image_aug {2 * img}, caption "
          f"rows {cap}), reads {2 * img + cap} of which {img} re-read the rows `image` just read -> {(4 * img + 2 * cap) / us / 1e6:.2f} "
          f"TB/s counting every read, {(3 * img + 2 * cap) / us / 1e6:.2f} TB/s counting the image rows once", flush=True)


def bench_loop(cfg, iters, steps, rounds):
    """iters: {name: training iterator of device tensors}; one graphed C1 step, fed by each iterator in turn"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = cfg.copy()
    cfg.pretrained_model_path = None                 # explicit random initialisation of the frozen ResNet-50
    additional = xmc_gan.create_additional_data(cfg)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    first = next(iter(iters.values()))
    batch = train_utils._array_fields(next(first))
    state, _ = train_utils.train_step(0, state, batch, xmc_gan, gen, disc, cfg, additional)
    graphed = train_utils.GraphedTrainStep(state, batch, xmc_gan, gen, disc, cfg, additional)
    state = graphed.state
    for it in iters.values():                        # warm both feeds through the graph
        for _ in range(3):
            state, _ = graphed(state, train_utils._array_fields(next(it)))
    torch.cuda.synchronize()
    res = {k: [] for k in iters}
    for _ in range(rounds):
        for name, it in iters.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                state, metrics = graphed(state, train_utils._array_fields(next(it)))
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    assert all(np.isfinite(float(v)) for v in metrics.values())
    for name, v in res.items():
        print(f"loop: C1 training loop fed by {name}: ms/step per round of {steps} steps {' '.join(f'{x:.2f}' for x in v)} "
              f"(median {np.median(v):.2f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="fill,stream,kernel,loop")
    ap.add_argument("--examples", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=32)
    ap.add_argument("--shards", type=int, default=16)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=32, help="records per staging upload of the fill")
    ap.add_argument("--batches", type=int, default=200, help="batches of the stream-rate window")
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    only = set(args.only.split(","))
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_cache.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    if "kernel" in only:
        bench_kernel(args.launches)
    if not only & {"fill", "stream", "loop"}:
        return
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        n = make_shards(d, args.examples, args.repeat, args.shards)
        print(f"wrote {n} training records ({args.examples} distinct x {args.repeat}) in {args.shards * args.repeat} shards in "
              f"{time.perf_counter() - t0:.1f} s; CPU budget {input_pipeline.cpu_budget():.0f} cores", flush=True)
        cfg = coco_xmc.get_c1_config()
        cfg.update(data_dir=d + "/", coco_version="2014", shuffle_buffer_size=1000, train_shuffle=True, eval_batch_size=2,
                   dataset="mscoco", num_decode_procs=args.procs, num_decode_workers=args.threads)
        per = cfg.batch_size * cfg.d_step_per_g_step
        ds = coco_dataset.COCODataset(image_size=cfg.image_size, z_dim=cfg.z_dim, data_dir=cfg.data_dir)
        cache = None
        if "fill" in only:
            for rnd in range(2):                     # host pipeline, fill, host pipeline, fill
                rate, it = host_rate(cfg, args.procs, args.threads, 40)
                del it
                print(f"fill: round {rnd}: host pipeline {args.procs} processes x {args.threads} thread(s): {rate:.0f} examples/s", flush=True)
                cache = None
                torch.cuda.empty_cache()
                cache = device_cache.DeviceDatasetCache(ds, ds.files("train"), "cuda", args.threads, args.procs, args.chunk)
                print(f"fill: round {rnd}: cache fill of {cache.slots} records ({cache.nbytes / 2 ** 30:.2f} GiB) in the same layout, chunks of {args.chunk}: "
                      f"{cache.fill_seconds:.2f} s = {cache.slots / cache.fill_seconds:.0f} records/s including the start of the worker "
                      f"processes; {cache.fill_first_seconds:.2f} s until the first chunk arrived, then "
                      f"{(cache.slots - cache.first_chunk) / max(cache.fill_seconds - cache.fill_first_seconds, 1e-9):.0f} records/s", flush=True)
        if cache is None:
            cache = device_cache.DeviceDatasetCache(ds, ds.files("train"), "cuda", args.threads, args.procs, args.chunk)
        if "stream" in only:
            for rnd in range(3):
                it = cache.batches([1, 0, 0], True, 1000, True, per, 2)
                for _ in range(5):
                    next(it)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.batches):
                    b = next(it)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"stream: round {rnd}: cached iterator, one planning thread: {args.batches * per / dt:.0f} examples/s "
                      f"({args.batches} batches of {per}, consumer only waits)", flush=True)
                del it, b
        if "loop" in only:
            cached = cache.batches([1, 0, 0], True, 1000, True, per, 2)
            host, _, _ = input_pipeline.create_datasets(cfg, data_rng=1, device="cuda", prefetch=2)
            bench_loop(cfg, {"the device cache": cached, f"the host pipeline ({args.procs} x {args.threads})": host}, args.steps, args.rounds)


if __name__ == "__main__":
    main()
