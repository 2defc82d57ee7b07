#!/usr/bin/env python
"""Benchmark of the XMC-GAN G+D training step on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]     (N > 1: launched by torch.distributed.run)

A "step" is one ``train_step`` (train_d on 56 images + train_g_d on 56 images per GPU) of the C1
workload -- 128 px coco_xmc, gf = df = 96, per-GPU batch 56, bf16, EMA off, the frozen ResNet-50 image-contrastive
term ON as in the reference's default config (``--pretrained off`` times the G/D step alone), synthetic COCO-shaped
batch and random-init weights resident in HBM.  ``value`` = config.batch_size * N images per step
divided by the step time (max over ranks), the reference's accounting (input_pipeline.py:46-47).

The timed steps are replays of ONE captured hipGraph of the whole train_step (train_utils.GraphedTrainStep;
``--graph off`` times the eager Python + ctypes enqueue path instead; for N > 1 the RCCL all-reduces are captured
inside the graph).
``python bench.py --gpus N`` with N > 1 and no torchrun environment re-launches itself under
``torch.distributed.run`` (one rank per GPU, 127.0.0.1 rendezvous).

A plain run sets up, warms up, times exactly K steps and prints the JSON line (``ms_per_step`` = milliseconds of one timed
step).  ``--dump-outputs DIR`` writes what the last timed step returned to its caller as DIR/<name>.npy (see
``step_outputs``); the inputs are seeded, so two builds run with the same arguments can be compared output for output.

Extra objects on the JSON line, measured only with ``--full`` (after the timed steps; ``--no-*`` drop single ones):
  host_enqueue_ms_per_step -- host time of issuing one more step into an empty queue.
  roofline     -- the dominant kernel family, ``conv_stream_kernel`` / ``conv_phase_kernel`` (bf16 3x3 implicit-GEMM fwd +
                  dgrad; two wave tilings; the launches next to a 2x resampling as four 2x2 convolutions):
                  algorithmic FLOPs (2*M*K*N per launch with M = the conv's own output pixels, before any
                  fused pooling; SURVEY.md 8(d) accounting) / HIP-event duration of those launches,
                  measured live in an instrumented eager extra step.  ``executed_*`` = the MFMA FLOPs the launches
                  really issue (the phase-decomposed launches do 4/9 of the 3x3 formulation's).  ``family`` = all conv fwd/dgrad
                  launches (1x1, RGB, split-K finish included), ``wgrad`` = the weight-gradient launches.
                  ``traffic`` is NOT measured in this run: it is the per-launch HBM byte count of the same
                  kernel from the committed rocprofv3 PMC passes (``traffic_source``).
  gd_only      -- (N = 1, C1) the same step with the ResNet-50 term off, timed by the same harness in the same run:
                  the workload BASELINE.json's 40 % MFMA target is defined on (24.93 TFLOP algorithmic).
  cpu_baseline -- the oracle (oracle/torch_ref.py, a port of the reference math) timed on the host
                  cores at the same network, per-device batch 8 (rank 0, N = 1 only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

STEP_TFLOP_C1 = 24.93          # algorithmic FLOPs of one C1 train_step, G + D only; the frozen
                               # ResNet-50 term adds 3 * B * 8.18 GFLOP (fwd on 2B images, data gradient on B)
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3


class _ConvTimer:
    """Wraps ops.conv / ops.conv_wgrad with HIP events on the launch stream (instrumented step)."""

    def __init__(self, ops):
        self.ops, self.recs = ops, []
        self._conv, self._wgrad = ops.conv, ops.conv_wgrad

    def __enter__(self):
        def conv(x, w, bias=None, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = self._conv(x, w, bias, **kw)
            e.record()
            n, hi, wi, _ = x.shape
            m = n * hi * wi * (4 if kw.get("ups") else 1)        # the conv's own output pixels (y may be 2x2-pooled)
            packed = hasattr(w, "taps")
            taps_cin = w.taps * w.cin if packed else w.shape[1] * w.shape[2]
            cout = w.cout if packed else w.shape[0]
            fl = getattr(self.ops, "acct_flops", None)           # canvas / stride hint of the frozen ResNet-50's layers
            self.ops.acct_flops = None
            # conv_stream = the weight-streaming 3x3 kernel (dominant); packed 1x1 = the pointwise kernel of the same file
            name = "conv_stream" if packed and w.taps == 9 else "conv_other"
            alg = fl if fl is not None else 2.0 * m * taps_cin * cout
            # a launch next to a 2x resampling runs as four 2x2 convolutions (conv_phase_kernel): 4/9 of the MFMAs
            self.recs.append((name, alg, s, e, alg * (4.0 / 9.0 if getattr(self.ops, "last_conv_phase", False) else 1.0)))
            return y

        def wgrad(x, dy, dw, db=None, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            self._wgrad(x, dy, dw, db, **dict(kw, sync=True))      # on the launch stream (not the async wgrad stream): timed alone
            e.record()
            n, h, w_, _ = x.shape
            m = n * h * w_ * (4 if kw.get("x_ups") else 1)
            ph = self.ops.wgrad_is_phase(x, dy, **{k: v for k, v in kw.items() if k in ("ks", "x_ups", "x_relu", "dy_ups")})
            self.recs.append(("conv_wgrad", 2.0 * m * dw.numel(), s, e, 2.0 * m * dw.numel() * (4.0 / 9.0 if ph else 1.0)))
        self.ops.conv, self.ops.conv_wgrad = conv, wgrad
        return self

    def __exit__(self, *a):
        self.ops.conv, self.ops.conv_wgrad = self._conv, self._wgrad

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, fl, s, e, ex in self.recs:
            d = out.setdefault(name, dict(flops=0.0, ms=0.0, launches=0, executed=0.0))
            d["flops"] += fl
            d["executed"] += ex
            d["ms"] += s.elapsed_time(e)
            d["launches"] += 1
        return out


def _usable_cores():
    """Cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(cfg, per_device_batch=8, timed=3):
    """Oracle train_step on the host cores (kind "port": the reference itself cannot be imported in this image -- SURVEY.md
    F1/F2).  SURVEY.md 8(d)'s protocol: 1 warm-up + ``timed`` timed steps of the same network at per-device batch 8 (the
    reference's own per-GPU batch, README.md:76) -> images/sec, plus the tiny parity config C0 (1 + 3 steps) as steps/sec.
    Bounded: ~35 s on 16 cores."""
    from oracle import torch_ref as R
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd.configs import coco_xmc
    cores = min(_usable_cores(), 64)         # torch-CPU conv scaling flattens well before 64 threads
    torch.set_num_threads(cores)

    def run(c, pdb, n):
        c = c.copy()
        c.dtype = "float32"
        gp, gs = syn.init_generator(c, seed=42)
        dp_, ds = syn.init_discriminator(c, seed=43)
        batch = R.batch_to_torch(syn.make_batch(c, per_device_batch=pdb))
        resnet = None
        if c.get("pretrained_image_contrastive", False):
            from xmcgan_image_generation_amd.utils import resnet_v1
            resnet = resnet_v1.init_resnet50(seed=7, head_scale=0.05)
        state = R.make_state(gp, gs, dp_, ds, resnet=resnet)
        state, _ = R.train_step(state, batch, c)                  # warm-up: thread pool, oneDNN primitive caches, allocator
        t0 = time.perf_counter()
        for _ in range(n):
            state, _ = R.train_step(state, batch, c)
        return (time.perf_counter() - t0) / n

    dt = run(cfg, per_device_batch, timed)
    c0 = coco_xmc.get_test_config()
    dt0 = run(c0, c0.batch_size, 3)
    return {"value": per_device_batch / dt, "unit": "images/sec", "cores": cores, "kind": "port",
            "c0_steps_per_sec": round(1.0 / dt0, 3),
            "sample": f"oracle train_step (torch-CPU fp32 restatement of the reference math), same network, per-device batch "
                      f"{per_device_batch} ({2 * per_device_batch} images through D): 1 warm-up + {timed} timed steps, {dt:.2f} s per step; "
                      f"c0_steps_per_sec: the tiny parity config C0 (128 px, gf = df = 16, per-device batch {c0.batch_size}), 1 + 3 steps"}


def _self_launch(args):
    """``python bench.py --gpus N`` (N > 1) outside torchrun: run under torch.distributed.run as a child, one rank per GPU."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


DUMP_SAMPLE = 1 << 21          # values kept of each flat parameter / Adam-moment arena (tens of millions each at C1)
DUMP_LIMIT_BYTES = 64 << 20


def step_outputs(state, metrics, ema=False):
    """What a caller of the timed step received from its last call, as host float32 / float64 arrays by name: the losses
    (float64 scalars), G's BatchNorm running statistics and D's spectral-norm vectors in full, and a fixed, seeded sample
    of ``DUMP_SAMPLE`` positions of each flat arena -- parameters, both Adam moments, the EMA parameters when EMA is on."""
    import numpy as np
    from xmcgan_image_generation_amd import synthetic as syn
    out = {k: np.float64(float(v)) for k, v in metrics.items()}

    def tree(t):
        return torch.cat([v.detach().reshape(-1).float() for _, v in sorted(syn.tree_leaves(t), key=lambda kv: kv[0])]).cpu().numpy()

    out["g_batch_stats"] = tree(state.generator_state["batch_stats"])
    out["d_spectral_norm_stats"] = tree(state.discriminator_state["spectral_norm_stats"])
    for net, opt in (("g", state.g_optimizer), ("d", state.d_optimizer)):
        arena = opt.arena
        n = arena.params.numel()
        pos = np.sort(np.random.default_rng(0).choice(n, size=min(n, DUMP_SAMPLE), replace=False))
        idx = torch.from_numpy(pos).to(arena.params.device)
        bufs = {"params": arena.params, "adam_m": arena.m, "adam_v": arena.v}
        if ema and net == "g":
            bufs["ema_params"] = state.ema_buffer
        for name, buf in bufs.items():
            out[f"{net}_{name}"] = buf.index_select(0, idx).float().cpu().numpy()
    total = sum(np.asarray(v).nbytes for v in out.values())
    assert total <= DUMP_LIMIT_BYTES, f"step outputs take {total} bytes, more than {DUMP_LIMIT_BYTES}"
    return out


def _pmc_traffic(kernel_prefixes):
    """Per-launch HBM bytes (FETCH_SIZE + WRITE_SIZE, corrected per the MI355X guide), launch-weighted over EVERY kernel
    ``roofline.kernel`` names, from the newest committed rocprofv3 PMC summary under profiles/ -- NOT measured in this run."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic_per_launch.json")), reverse=True):
        rec = [v for k, v in json.load(open(path)).items() if k.startswith(tuple(kernel_prefixes))]
        n = sum(r["launches"] for r in rec)
        if n:
            return round(sum(r["launches"] * (r["fetch_MB"] + r["write_MB"]) for r in rec) / n * 1e6), os.path.relpath(path, ROOT)
    return None, None


def _in_graph_families():
    """Per-family kernel time inside the REPLAYED graph of the default schedule (tools/graph_family_time.py on a committed
    rocprofv3 kernel trace) -- NOT measured in this run; sits next to the serial-eager figures of ``roofline``."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_time_in_replayed_graph.json")), reverse=True):
        d = json.load(open(path))
        d["source"] = os.path.relpath(path, ROOT)
        return d
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c1", choices=["c1", "c3", "c4", "tiny"],
                    help="c1 = BASELINE config #2 (the headline), c3 = 256 px per-GPU batch 32 (#4), c4 = c3 with MX-fp8 convolutions (#5)")
    ap.add_argument("--fp8", action="store_true", help="config.conv_fp8 on top of --config (MX-fp8 3x3 convolutions)")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch override (debug only)")
    ap.add_argument("--dtype", default=None, choices=[None, "bfloat16", "float32"])
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="replay the step as one captured hipGraph (auto = on, with an eager fallback if the capture fails)")
    ap.add_argument("--pretrained", default="on", choices=["on", "off"],
                    help="the frozen ResNet-50 image-contrastive term of the reference's default config "
                         "(coco_xmc.py:65: on); off = the G/D step alone")
    ap.add_argument("--grad-transport", default="float32", choices=["float32", "bf16"],
                    help="N > 1: dtype of the gradient all-reduce (float32 = the reference's pmean; bf16 halves the xGMI bytes)")
    ap.add_argument("--grad-schedule", default="auto", choices=["auto", "overlapped", "exclusive"],
                    help="N > 1: when the gradient exchanges are issued (dp.GradSync.schedule).  auto = time 3 steps of each schedule "
                         "during warm-up and keep the faster (the choice is printed in the JSON line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="also measure host_enqueue_ms_per_step, roofline, gd_only and cpu_baseline (off: the headline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without cpu_baseline")
    ap.add_argument("--no-instrument", action="store_true", help="--full without the instrumented extra step (roofline)")
    ap.add_argument("--no-gd-only", action="store_true", help="--full without the second timed workload (the G/D step alone)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "RANK" not in os.environ:
        _self_launch(args)

    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # test hook (tests/test_gpu_dp.py): XMC_BENCH_BACKEND=gloo puts every rank on GPU 0 and exchanges through gloo, so the
    # N > 1 control flow of this file (per-rank data, barriers, max over ranks, rank-0 printing) runs on a 1-GPU box;
    # RCCL refuses two ranks per device.  Eager only: gloo collectives cannot be captured into a hipGraph.
    backend = os.environ.get("XMC_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    grad_sync = None
    if world > 1 or "RANK" in os.environ:          # under torch.distributed.run: always take the RCCL path
        import torch.distributed as dist
        from xmcgan_image_generation_amd.dp import GradSync
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
        grad_sync = GradSync(transport=args.grad_transport,
                             schedule="overlapped" if args.grad_schedule == "auto" else args.grad_schedule)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    cfg = {"c1": coco_xmc.get_c1_config, "c3": coco_xmc.get_c3_config, "c4": coco_xmc.get_c4_config,
           "tiny": coco_xmc.get_test_config}[args.config]()
    if args.fp8:
        cfg.conv_fp8 = True
    if args.dtype:
        cfg.dtype = args.dtype
    if args.batch:
        cfg.batch_size = args.batch
    cfg.pretrained_image_contrastive = args.pretrained == "on"
    b = cfg.batch_size
    additional_data = {}
    step_tflop = STEP_TFLOP_C1 * (b / 56.0)
    if cfg.pretrained_image_contrastive:
        # random-init ResNet-50 (no network for the checkpoint) with a non-zero head so that the gradient path carries data
        from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1
        rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)
        st = {"params": rp, "batch_stats": rs}
        additional_data = {"image_model": pretrained_model_utils.ImageModel(st), "image_model_state": st}
        # forward on the 2B real + generated images, data gradient on the B generated ones (true 224^2 geometry)
        step_tflop += 3 * b * resnet_v1.forward_flops_per_image() / 1e12

    def time_workload(cfg, additional_data, dump=False):
        """state -> one eager step -> capture -> warm-up -> EXACTLY args.steps timed steps between barrier + synchronize
        (``dump``: what the last of them returned, copied to the host before anything else runs)"""
        gen, disc, state = train_utils.create_train_state(cfg, 0)          # identical init on every rank
        batch = syn.make_batch(cfg, per_device_batch=b, rank=rank)         # independent per-rank data
        tb = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}

        def eager_step(st):
            return train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, additional_data, grad_sync=grad_sync)

        # ---- first step eager (lazy library / RCCL setup), then capture the step once
        state, metrics = eager_step(state)
        fence()
        # N > 1: the captured graph holds the RCCL all-reduces too (tests/test_gpu_dp.py replays it on the RCCL backend);
        # a capture problem falls back to the eager loop below, never loses the measurement
        use_graph = args.graph in ("on", "auto")
        graphed, graph_note = None, None

        def capture(st):
            """-> (GraphedTrainStep or None, state, note)"""
            if not use_graph:
                return None, st, None
            try:
                gr = train_utils.GraphedTrainStep(st, tb, xmc_gan, gen, disc, cfg, additional_data, grad_sync=grad_sync)
                return gr, gr.state, None
            except Exception as e:                     # never lose the measurement to a capture problem: fall back to eager
                if args.graph == "on":
                    raise
                torch.cuda.synchronize()
                return None, st, f"capture failed ({type(e).__name__}: {e}); eager"

        # test hook (tests/test_gpu_dp.py): XMC_BENCH_FORCE_SCHEDULE_TRIAL=1 runs the trial at world size 1 too, so that the capture /
        # re-capture path below executes with RCCL inside the graphs on a 1-GPU box
        force_trial = os.environ.get("XMC_BENCH_FORCE_SCHEDULE_TRIAL", "0") != "0"
        if grad_sync is not None and (world > 1 or force_trial) and args.grad_schedule == "auto":
            try:
                # both exchange schedules are bit-equal on the parameters (tests/test_dist_gloo.py): pick by the clock, on THIS node's
                # links -- 1 + 3 steps of each (part of the warm-up), max over ranks so that every rank takes the same decision
                trial = {}
                for sched in ("overlapped", "exclusive"):
                    grad_sync.schedule = sched
                    gr, state, note = capture(state)
                    run = (lambda st: gr(st)) if gr is not None else eager_step
                    state, metrics = run(state)
                    fence()
                    t0 = time.perf_counter()
                    for _ in range(3):
                        state, metrics = run(state)
                    fence()
                    t = torch.tensor([time.perf_counter() - t0], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
                    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
                    trial[sched] = (float(t) / 3 * 1e3, gr, note)
                best = os.environ.get("XMC_BENCH_TRIAL_PICK") or min(trial, key=lambda k: trial[k][0])     # (PICK: test hook, both branches below)
                grad_sync.schedule = best
                sched_info.update(chosen=best, how="auto: 3 timed steps of each during warm-up",
                                  trial_ms_per_step={k: round(v[0], 3) for k, v in trial.items()})
                if best == sched:                          # the schedule trialled last owns the current state: keep its graph
                    _, graphed, graph_note = trial[best]
                else:                                      # the other one's graph owns an older copy of the per-step state: capture afresh
                    trial.clear()
                    gr = None
                    graphed, state, graph_note = capture(state)
                trial.clear()
            except Exception as e:                     # never lose the measurement to the trial: the overlapped schedule, plain capture
                if os.environ.get("XMC_BENCH_TRIAL_STRICT", "0") != "0":
                    raise
                torch.cuda.synchronize()
                grad_sync.schedule = "overlapped"
                sched_info.clear()
                sched_info.update(chosen="overlapped", how=f"auto: the trial failed ({type(e).__name__}: {e}); default schedule")
                graphed, state, graph_note = capture(state)
        else:
            graphed, state, graph_note = capture(state)
            if grad_sync is not None:
                sched_info.update(chosen=grad_sync.schedule, how="--grad-schedule" if args.grad_schedule != "auto" else "world 1: nothing to choose")

        def step(st):
            return graphed(st) if graphed is not None else eager_step(st)

        for _ in range(max(args.warmup - 1, 0)):
            state, metrics = step(state)
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            state, metrics = step(state)
        t_host = time.perf_counter() - t0            # host time spent issuing the steps (includes queue back-pressure)
        fence()
        dt = time.perf_counter() - t0
        if grad_sync is not None:
            t = torch.tensor([dt], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t)
        losses = {k: round(float(v), 4) for k, v in metrics.items()}
        outputs = None
        if dump:
            state = xmc_gan._flush(state)              # N > 1 eager: apply the D update the last step left in flight
            if rank == 0:
                outputs = step_outputs(state, metrics, ema=cfg.get("ema", True))
        host_one = None
        if args.full:
            # host cost of issuing ONE step into an empty queue (no back-pressure): what the host needs per step
            fence()
            t1 = time.perf_counter()
            state, metrics = step(state)
            host_one = round((time.perf_counter() - t1) * 1e3, 3)
            fence()
        return dict(dt=dt, t_host=t_host, host_one=host_one, losses=losses, graphed=graphed, graph_note=graph_note,
                    state=state, gen=gen, eager_step=eager_step, outputs=outputs)

    def fence():
        if grad_sync is not None:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    sched_info = {}
    r = time_workload(cfg, additional_data, dump=args.dump_outputs is not None)
    dt, t_host, host_one, losses, graphed, graph_note = (r[k] for k in ("dt", "t_host", "host_one", "losses", "graphed", "graph_note"))
    state, gen, eager_step = r["state"], r["gen"], r["eager_step"]
    ms = dt / args.steps * 1e3
    value = b * world * args.steps / dt
    if r["outputs"] is not None:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in r["outputs"].items():
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), arr)
        r["outputs"] = None

    # ---- instrumented eager extra step (outside the timed region): per-kernel HIP-event durations
    peak = PEAK_BF16_TFLOPS if cfg.dtype == "bfloat16" else PEAK_F32_TFLOPS
    roofline = None
    if args.full and not args.no_instrument:
        # the instrumented step runs SERIALLY (one stream: no overlapped pullbacks, no prefetched generator forward, no
        # async weight gradients), so every event pair brackets exactly one kernel running alone on the GPU -- the
        # same conditions as the committed rocprofv3 kernel trace (tools/profile_round.sh)
        ops = gen(train=True).ops
        saved = (xmc_gan._OVERLAP_BWD, xmc_gan._PREFETCH_G, ops.wgrad_async)
        xmc_gan._OVERLAP_BWD, xmc_gan._PREFETCH_G, ops.wgrad_async = False, False, False
        try:
            state, _ = eager_step(state)          # untimed: the caching allocator re-learns the serial stream assignment
            torch.cuda.synchronize()              # (a fresh hipMalloc between a start event and its kernel would be timed)
            # the host must run AHEAD of the GPU: with an empty queue a start event executes the moment it is enqueued and
            # the Python + ctypes launch latency that follows lands inside the measured interval (on boxes with a slow host
            # the 3x3 launches "took" 18.8 instead of 15.3 ms).  A sleeping wave holds the stream while the step is enqueued.
            from xmcgan_image_generation_amd import _lib as _xl
            _xl.check(_xl.load_probe().xmc_delay(60000, torch.cuda.current_stream().cuda_stream), "xmc_delay")
            with _ConvTimer(ops) as ct:
                state, _ = eager_step(state)
        finally:
            xmc_gan._OVERLAP_BWD, xmc_gan._PREFETCH_G, ops.wgrad_async = saved
        ks = ct.summary()
        tf = lambda d: d["flops"] / (d["ms"] * 1e-3) / 1e12 if d and d["ms"] > 0 else None
        dom = ks.get("conv_stream") or ks.get("conv_other")
        fam = dict(flops=sum(ks[k]["flops"] for k in ("conv_stream", "conv_other") if k in ks),
                   ms=sum(ks[k]["ms"] for k in ("conv_stream", "conv_other") if k in ks),
                   launches=sum(ks[k]["launches"] for k in ("conv_stream", "conv_other") if k in ks))
        wg = ks.get("conv_wgrad")
        traffic, traffic_src = (None, None)
        if cfg.dtype == "bfloat16" and args.config == "c1" and "conv_stream" in ks:
            traffic, traffic_src = _pmc_traffic(("conv_stream_kernel", "conv_phase4_kernel", "conv_phase_kernel"))
        achieved = tf(dom)
        roofline = {"bound": "mfma",
                    "kernel": ("conv_stream_mx8_kernel (MX-fp8, peak 5000) + the bf16 conv_stream_kernel launches of the 96-channel layers: "
                               "3x3 fwd + dgrad, quantisation passes and split-K finish included; frac is quoted against the bf16 peak"
                               if cfg.get("conv_fp8") else
                               "conv_stream_kernel<3,2,4,2> + <3,3,2,1> + <3,1,4,2> and conv_phase4_kernel / conv_phase_kernel<1,...> (bf16 3x3 implicit-GEMM fwd + dgrad "
                               "launches: 128-, 96- and 64-cout tilings; the launches next to a 2x resampling run as four 2x2 convolutions = 4/9 "
                               "of the MFMAs, see executed_*; achieved counts the ALGORITHMIC 2MKN of the 3x3 formulation; split-K finish included)")
                    if "conv_stream" in ks else "conv_igemm / conv_patch kernels (fwd + dgrad launches)",
                    "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                    "traffic": traffic, "traffic_source": traffic_src,
                    "launches": dom["launches"], "avg_launch_ms": round(dom["ms"] / max(dom["launches"], 1), 4),
                    "flop_per_launch_avg": dom["flops"] / max(dom["launches"], 1),
                    "tflop_per_step": round(dom["flops"] / 1e12, 3), "ms_per_step": round(dom["ms"], 3),
                    "executed_tflop_per_step": round(dom["executed"] / 1e12, 3),
                    "executed_achieved": round(dom["executed"] / (dom["ms"] * 1e-3) / 1e12, 2),
                    # MFMA-pipe utilisation of these launches: the FLOPs the matrix cores really execute / peak (``frac`` is the
                    # model-FLOPs utilisation: the phase-decomposed launches deliver the 3x3 result with 4/9 of the MFMAs)
                    "executed_frac": round(dom["executed"] / (dom["ms"] * 1e-3) / 1e12 / peak, 4),
                    "family": {"what": "all conv fwd + dgrad launches (3x3, pointwise 1x1, RGB, split-K finish; the frozen ResNet-50's included)",
                               "achieved": round(tf(fam), 2), "frac": round(tf(fam) / peak, 4), "launches": fam["launches"],
                               "tflop_per_step": round(fam["flops"] / 1e12, 3), "ms_per_step": round(fam["ms"], 3)},
                    "wgrad": {"achieved": round(tf(wg), 2), "frac": round(tf(wg) / peak, 4), "launches": wg["launches"],
                              "tflop_per_step": round(wg["flops"] / 1e12, 3), "ms_per_step": round(wg["ms"], 3),
                              "executed_tflop_per_step": round(wg["executed"] / 1e12, 3),
                              "executed_achieved": round(wg["executed"] / (wg["ms"] * 1e-3) / 1e12, 2),
                              "executed_frac": round(wg["executed"] / (wg["ms"] * 1e-3) / 1e12 / peak, 4)} if wg else None,
                    "measured_in": "one serial eager step after the timed region (single stream; HIP events per launch)",
                    "in_replayed_graph": _in_graph_families() if args.config == "c1" and cfg.dtype == "bfloat16" else None,
                    "step_tflop": round(step_tflop, 3) if args.config == "c1" else None,
                    "step_mfma_frac": round(step_tflop / (ms * 1e-3) / peak, 4) if args.config == "c1" else None}

    launch_mode = "hipGraph replay (1 graph launch per step)" if graphed is not None else \
        "eager (Python + ctypes, ~700 kernel launches per step)" + (f"; {graph_note}" if graph_note else "")
    # ---- the G/D step alone (BASELINE.json's 40 % target is defined on its 24.93 TFLOP): same harness, same run,
    #      ResNet-50 term off -- a driver-timed number for that workload next to the reference-default headline
    gd_only = None
    if args.full and cfg.pretrained_image_contrastive and args.config == "c1" and world == 1 and not args.no_gd_only:
        del r, graphed, eager_step, state
        torch.cuda.empty_cache()
        cfg_gd = cfg.copy()
        cfg_gd.pretrained_image_contrastive = False
        r2 = time_workload(cfg_gd, {})
        ms_gd = r2["dt"] / args.steps * 1e3
        gd_tflop = STEP_TFLOP_C1 * (b / 56.0)
        gd_only = {"what": "the same step with pretrained_image_contrastive off (generator + discriminator only)",
                   "ms_per_step": round(ms_gd, 3), "value": round(b * world * args.steps / r2["dt"], 2), "unit": "images/sec",
                   "steps": args.steps, "step_tflop": round(gd_tflop, 3),
                   "step_mfma_frac": round(gd_tflop / (ms_gd * 1e-3) / peak, 4), "losses": r2["losses"],
                   "launch_mode": "hipGraph replay" if r2["graphed"] is not None else "eager"}
        del r2

    metric = "images/sec (G+D step, 128px COCO bs=56)" if args.config == "c1" and b == 56 else \
        f"images/sec (G+D step, {cfg.image_size}px COCO bs={b})"
    out = {"metric": metric, "value": round(value, 2), "unit": "images/sec",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": ("mx-fp8 conv fwd/dgrad (f32 accumulate) + bf16" if cfg.get("conv_fp8") else "bf16") if cfg.dtype == "bfloat16" else "f32",
           "data": "synthetic",
           "config": {"workload": f"{cfg.image_size}x{cfg.image_size} coco_xmc gf=df={cfg.gf_dim} z={cfg.z_dim} "
                                  f"train_step (train_d + train_g_d), per-GPU batch {b}, EMA "
                                  f"{'on' if cfg.get('ema', True) else 'off'}, pretrained_image_contrastive "
                                  f"{'on' if cfg.get('pretrained_image_contrastive') else 'off'}",
                      "global_batch": b * world, "parallelism": f"dp{world}"},
           "launch_mode": launch_mode,
           "grad_schedule": dict(sched_info) if sched_info else None,
           "host_enqueue_ms_per_step": host_one,
           "host_ms_per_step_in_timed_loop": round(t_host / args.steps * 1e3, 3),
           "losses": losses,
           "roofline": roofline}
    if gd_only is not None:
        out["gd_only"] = gd_only
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg)
        print(json.dumps(out), flush=True)
    if grad_sync is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
