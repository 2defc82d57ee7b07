#!/usr/bin/env python
"""The pairwise passes of KID and improved precision / recall (csrc/sample_metrics.hip) at the evaluation's size, against their
NumPy specification (utils/sample_metrics.py) on the host.

Pools: non-negative random float32 (|N(0, 1)|, the sign pattern of Inception pools), n = m = 30000 rows of d = 2048.
  device  xmc_knn_radii (k = 3), xmc_ball_hits (radii of the second pool; about a quarter of the random rows are hit, never all 128 of a
          block, so no block finishes early and every tile is walked) and xmc_poly3_sums (100 subsets of 1000 rows): device events around each call
          on device-resident pools, --warmup untimed calls, then the median of --repeats timed ones.  Each is also given as a share
          of its floor: the pass's 2 n m d FLOP at the exact-fp32 MFMA's measured 155 TFLOP/s (the passes are compute-bound: a
          128 x 128 tile multiplies 2048-long rows).
  host    the specification, once, float64 in row blocks of 1024, on the threads this process may use: knn_radii_spec and
          ball_hits_spec at --host-n rows (the time of a pass grows with n^2: the 30000-row figure printed is that extrapolation
          unless --host-n is 30000) and poly3_sums_spec at --host-subsets subsets of 1000 (linear in the subsets).
  check   the device results of the first --host-n rows' worth of work against the host's, so the timed code is the tested code.

usage: python tools/bench_sample_metrics.py [--n 30000] [--d 2048] [--host-n 30000] [--host-subsets 100] [--repeats 5] [--warmup 2]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from xmcgan_image_generation_amd.utils import sample_metrics as S  # noqa: E402

PEAK_F32_MFMA = 155e12         # measured, v_mfma_f32_32x32x2_f32 back to back on every SIMD


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--host-n", type=int, default=30000)
    ap.add_argument("--host-subsets", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_metrics.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.float32)
    n, d, k = args.n, args.d, args.k
    g = torch.Generator(device="cuda").manual_seed(0)
    real = torch.randn((n, d), device="cuda", generator=g).abs_()
    fake = torch.randn((n, d), device="cuda", generator=g).abs_()
    gi, ri = S.kid_subsets(n, n, args.subsets, args.subset_size, 0)
    msub = gi.shape[1]
    print(f"pools: n = m = {n}, d = {d}, |N(0, 1)| float32 on the device; k = {k}; KID {args.subsets} subsets of {msub}; "
          f"{args.warmup} warm-up calls, median of {args.repeats}; host threads: {torch.get_num_threads()}", flush=True)

    radii = torch.empty((n,), dtype=torch.float64, device="cuda")
    hit = torch.empty((n,), dtype=torch.uint8, device="cuda")
    sums = torch.empty((args.subsets, 3), dtype=torch.float64, device="cuda")
    ops.knn_radii(fake, k, out=radii)
    passes = (
        ("xmc_knn_radii", lambda: ops.knn_radii(fake, k, out=radii), 2.0 * n * n * d),
        ("xmc_ball_hits", lambda: ops.ball_hits(real, fake, radii, out=hit), 2.0 * n * n * d),
        # three sums per subset: x.x, y.y and x.y, msub^2 dot products each (the p == q pairs of the first two are computed too)
        ("xmc_poly3_sums", lambda: ops.poly3_sums(fake, gi, real, ri, out=sums), 3 * 2.0 * args.subsets * msub * msub * d),
    )
    dev_ms = {}
    for name, fn, flop in passes:
        med, ms = timed(fn, args.warmup, args.repeats)
        dev_ms[name] = med
        floor = flop / PEAK_F32_MFMA * 1e3
        print(f"device: {name}: {med:.2f} ms (runs {' '.join(f'{x:.2f}' for x in ms)}), {flop / 1e12:.2f} TFLOP -> "
              f"{flop / med / 1e9:.1f} TFLOP/s; floor at 155 TFLOP/s {floor:.2f} ms = {100 * floor / med:.0f} % of the time "
              f"(includes the pass's norm / finish kernels and, for poly3, the upload of the index arrays)", flush=True)
    print(f"device: rows of the first pool inside a ball of the second: {int(hit.sum())} of {n}", flush=True)

    # ---- host specification, once
    hn = min(args.host_n, n)
    hreal, hfake = real[:hn].cpu().numpy(), fake[:hn].cpu().numpy()
    scale = (n / hn) ** 2
    t0 = time.perf_counter()
    href = S.knn_radii_spec(hfake, k)
    t_knn = time.perf_counter() - t0
    t0 = time.perf_counter()
    hhit = S.ball_hits_spec(hreal, hfake, href)
    t_hit = time.perf_counter() - t0
    hs = min(args.host_subsets, args.subsets)
    hx, hy = fake.cpu().numpy(), real.cpu().numpy()
    t0 = time.perf_counter()
    hsums = S.poly3_sums_spec(hx, gi[:hs], hy, ri[:hs])
    t_poly = time.perf_counter() - t0
    note = "measured at that size" if hn == n else f"n^2 extrapolation to n = {n}: x {scale:.1f}"
    print(f"host: knn_radii_spec at n = {hn}: {t_knn:.2f} s ({note} -> {t_knn * scale:.1f} s); device pass {dev_ms['xmc_knn_radii']:.1f} ms",
          flush=True)
    print(f"host: ball_hits_spec at n = m = {hn}: {t_hit:.2f} s ({note} -> {t_hit * scale:.1f} s); device pass {dev_ms['xmc_ball_hits']:.1f} ms",
          flush=True)
    print(f"host: poly3_sums_spec, {hs} subsets of {msub}: {t_poly:.2f} s (linear in the subsets -> {t_poly * args.subsets / hs:.1f} s for "
          f"{args.subsets}); device pass {dev_ms['xmc_poly3_sums']:.1f} ms", flush=True)

    # ---- the timed code computes what the specification computes (bounds: tests/test_gpu_sample_metrics.py)
    big = float(torch.linalg.vector_norm(torch.cat([real[:hn], fake[:hn]]).double(), dim=1).max())
    bound = 2 * (d + 2) * 2.0 ** -24 * big ** 2
    dref = ops.knn_radii(fake[:hn].contiguous(), k)
    dhit = ops.ball_hits(real[:hn].contiguous(), fake[:hn].contiguous(), href)
    rel = np.abs(sums[:hs].cpu().numpy() - hsums) / hsums
    print(f"check: radii max |device - host| {np.abs(dref - href).max():.3e} (bound {bound:.3e}); hits differ on "
          f"{int((dhit != hhit).sum())} of {hn} rows; cubic sums max relative difference {rel.max():.2e}", flush=True)
    assert np.abs(dref - href).max() <= bound


if __name__ == "__main__":
    main()
