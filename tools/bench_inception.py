"""Throughput of the Inception-v3 forward of the FID / IS evaluation (utils/inception_utils.InceptionV3Features).

Reports, per dtype (float32 on v_mfma_f32_32x32x2_f32, bf16 on v_mfma_f32_32x32x16_bf16) and chunk size: images/s of the
device forward (resize to 299, 94 conv launches, 13 pools, mean, head GEMM; 128 px inputs already on the device; random
weights), the algorithmic TF/s from the layer table (inception_arch.flops_per_image: 11.43 GFLOP per image) and its share
of the matching MFMA peak (157.3 TF f32, 2,500 TF bf16 dense).  With --rocprof it then runs itself once more under
``rocprofv3 --kernel-trace --stats`` (one dtype and chunk, separate process) and prints the per-launch kernel time.

    python tools/bench_inception.py [--chunks 64 256 512] [--iters 5] [--rocprof]
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = {"f32": 157.3, "bf16": 2500.0}


def run(dtypes, chunks, iters, warmup):
    import numpy as np
    import torch
    from xmcgan_image_generation_amd.ops import HipOps
    from xmcgan_image_generation_amd.utils import inception_arch as A, inception_utils as U
    torch.cuda.set_device(0)
    p, s = A.init_inception(0)
    flops = A.flops_per_image()
    rows = []
    for dn in dtypes:
        dt = torch.float32 if dn == "f32" else torch.bfloat16
        ops = HipOps(dtype=dt)
        f = U.InceptionV3Features(ops, p, s)
        for n in chunks:
            x = torch.as_tensor(np.random.default_rng(n).random((n, 128, 128, 3), dtype=np.float32)).to(dt).cuda()
            for _ in range(warmup):
                f.forward_device(x)
            torch.cuda.synchronize()
            times = []
            for _ in range(iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f.forward_device(x)
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b) * 1e-3)
            t = float(np.median(times))
            tf = flops * n / t / 1e12
            rows.append((dn, n, t * 1e3, n / t, tf, 100.0 * tf / PEAK_TF[dn], min(times) * 1e3, max(times) * 1e3))
            print(f"{dn:5s} chunk {n:4d}: {t * 1e3:9.2f} ms (min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}) "
                  f"{n / t:9.1f} img/s  {tf:7.2f} TF/s  {100.0 * tf / PEAK_TF[dn]:5.1f} % of {PEAK_TF[dn]:g} TF", flush=True)
            f._bufs.clear()
            torch.cuda.empty_cache()
    return rows


def rocprof(dtype, chunk, iters):
    out = tempfile.mkdtemp(prefix="incep_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--dtypes", dtype, "--chunks", str(chunk), "--iters", str(iters),
           "--warmup", "1"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        print("no kernel_stats.csv from rocprofv3", out)
        return
    with open(stats[0]) as fh:
        rows = list(csv.DictReader(fh))
    calls_per_fwd = iters + 1
    print(f"\nrocprofv3 --kernel-trace --stats, {dtype} chunk {chunk}, {calls_per_fwd} forwards "
          f"(per-launch time; 'per fwd' = total / forwards):")
    print(f"{'kernel':70s} {'calls':>6s} {'avg us':>9s} {'per fwd ms':>10s} {'%':>6s}")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"][:70]
        print(f"{name:70s} {int(r['Calls']):6d} {float(r['AverageNs']) / 1e3:9.1f} "
              f"{float(r['TotalDurationNs']) / 1e6 / calls_per_fwd:10.3f} {float(r['Percentage']):6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--chunks", nargs="+", type=int, default=[64, 256, 512])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rocprof", action="store_true", help="then one rocprofv3 kernel-trace run per dtype at chunk 256")
    a = ap.parse_args()
    run(a.dtypes, a.chunks, a.iters, a.warmup)
    if a.rocprof:
        for dt in a.dtypes:
            rocprof(dt, 256, 2)


if __name__ == "__main__":
    main()
