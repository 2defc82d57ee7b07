#!/usr/bin/env python
"""Localized Narratives' caption length (T = 64) at the benchmarked C1 shapes (128 px, per-GPU batch 56, bf16, ResNet term on,
hipGraph replay) on synthetic batches:

  steps      ms/step at T = 64 with the long MFMA attention_for_g (attn_mfma.hip) ON and OFF (the VALU kernels the step ran
             before) and at T = 17, the three captured graphs replayed in alternating windows inside one process
  launches   per-launch times (HIP events) of attention_for_g forward / backward on both kernels, and of every word-loss launch,
             at T = 17 and T = 64

usage: python tools/bench_ln.py [--steps 60] [--window 10] [--batch 56] [--iters 30] [--timeout 420]
Without --child this is the driver: each part runs in a child process of its own under ``timeout``, and nothing more is started
after a part that did not end cleanly."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(t, attn_mfma, batch):
    """-> (GraphedTrainStep, batch tensors) of the C1 step at caption length t"""
    import torch
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1
    cfg = coco_xmc.get_c1_config()
    cfg.batch_size = batch
    cfg.pretrained_image_contrastive = True
    rp, rs = resnet_v1.init_resnet50(seed=7, head_scale=0.05)
    st = {"params": rp, "batch_stats": rs}
    additional = {"image_model": pretrained_model_utils.ImageModel(st), "image_model_state": st}
    os.environ["XMC_ATTN_MFMA"] = "1" if attn_mfma else "0"          # read when the networks build their operator tables
    try:
        gen, disc, state = train_utils.create_train_state(cfg, 0)
    finally:
        os.environ.pop("XMC_ATTN_MFMA", None)
    ops = gen(train=True).ops
    assert ops.attn_mfma == attn_mfma
    probe = torch.empty((batch, 256, syn.EMB_DIM), dtype=torch.bfloat16, device=ops.device)
    assert bool(ops.attn_g_sliced(probe, t)) == attn_mfma, "the attention route is not the one this row names"
    tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=batch, max_words=t).items()}
    state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
    torch.cuda.synchronize()
    return train_utils.GraphedTrainStep(state, tb, xmc_gan, gen, disc, cfg, additional), tb


def child_steps(args):
    import torch
    torch.cuda.set_device(0)
    runs = {"T = 64, long MFMA attention on ": workload(64, True, args.batch),
            "T = 64, long MFMA attention off": workload(64, False, args.batch),
            "T = 17                         ": workload(17, True, args.batch)}
    states = {k: g.state for k, (g, _) in runs.items()}
    for k, (g, tb) in runs.items():
        for _ in range(3):
            states[k], _ = g(states[k], tb)
    torch.cuda.synchronize()
    total = {k: 0.0 for k in runs}
    windows = {k: [] for k in runs}
    for _ in range(args.steps // args.window):
        for k, (g, tb) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.window):
                states[k], m = g(states[k], tb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            total[k] += dt
            windows[k].append(1e3 * dt / args.window)
            assert all(torch.isfinite(v).all() for v in m.values())
    n = (args.steps // args.window) * args.window
    print(f"C1 (128 px, bf16, per-GPU batch {args.batch}, ResNet term on), hipGraph replay, {n} steps each, alternating windows "
          f"of {args.window}:")
    for k in runs:
        print(f"  {k}: {1e3 * total[k] / n:.3f} ms/step   windows: " + " ".join(f"{w:.3f}" for w in windows[k]), flush=True)


def timed(fn, iters, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / iters          # us


def child_launches(args):
    import torch
    from xmcgan_image_generation_amd.libml import attention_lib as A
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    ops = HipOps(dtype=torch.bfloat16, stream_conv=False)
    b, r, e = args.batch, 256, 768
    print(f"per launch, B = {b}, R = {r}, E = {e}, bf16, {args.iters} launches each (us):")
    for rep in range(3):                                      # the two kernels alternated, three pairs
        for t in (17, 64):
            g = torch.Generator().manual_seed(t)
            region = torch.randn((b, r, e), generator=g).to(torch.bfloat16).cuda()
            dctx = torch.randn((b, r, e), generator=g).to(torch.bfloat16).cuda()
            words = torch.randn((b, t, e), generator=g).cuda()
            ml = torch.randint(4, t + 1, (b,), generator=g).float().cuda()
            wn = A.normalize_words(ops, words)
            row = {}
            for mfma in (True, False):
                ops.attn_mfma = mfma
                assert bool(ops.attn_g_sliced(region, t)) == mfma
                _, attn, rinv = ops.attn_g_fwd(region, wn, ml, 15.0)
                row[mfma] = (timed(lambda: ops.attn_g_fwd(region, wn, ml, 15.0), args.iters),
                             timed(lambda: ops.attn_g_bwd(dctx, region, wn, attn, rinv, 15.0), args.iters))
            ops.attn_mfma = True
            print(f"  attention_for_g T = {t:2d} (pair {rep + 1}): MFMA forward {row[True][0]:7.1f} backward {row[True][1]:7.1f}   "
                  f"VALU forward {row[False][0]:7.1f} backward {row[False][1]:7.1f}", flush=True)
    for t in (17, 64):
        g = torch.Generator().manual_seed(100 + t)
        feat = torch.randn((b, r, e), generator=g).to(torch.bfloat16).cuda()
        words = torch.randn((b, t, e), generator=g).cuda()
        ml = torch.randint(4, t + 1, (b, 1), generator=g).float().cuda()
        wn = A.normalize_words(ops, words)
        loss = torch.zeros(1, device="cuda")
        ops.wl_fused = True
        tape = A.word_loss_fwd(ops, feat, wn, ml, loss)
        assert tape.get("fused")
        f = timed(lambda: A.word_loss_fwd(ops, feat, wn, ml, loss), args.iters)
        bw = timed(lambda: A.word_loss_bwd(ops, tape), args.iters)
        print(f"  word_loss (fused) T = {t:2d}: forward {f:7.1f}   backward {bw:7.1f}", flush=True)
        w, wt = ops.wl_prep_words(wn)
        rn, rnt, rinv = ops.wl_prep_regions(feat)
        gm = ops.wl_tn_gemm(rn, rn, e, r, r, b, torch.bfloat16)
        nn, q = ops.wl_cols_fwd(rn, w, gm, ml.view(-1), t, 5.0)
        sim_t, pi = ops.wl_rows(nn, q, ml.view(-1), b, t, 5.0, 50.0)
        dsim = ops.xent_sym(sim_t, 1.0, loss, True, None)
        ds, a_s, al = ops.wl_cols_bwd(rn, w, gm, ml.view(-1), dsim, pi, t, 5.0, 50.0)
        ldp = w.shape[0]
        dg2 = ops.wl_tn_gemm(a_s, al, ldp, r, r, b, torch.bfloat16, alpha=2.0)
        drn = ops.wl_tn_gemm(ds, wt, ldp, r, e, b, torch.float32, x1=dg2, y1=rnt, k1=r, y0_shared=True)
        rows = [
            ("wl_prep_words", lambda: ops.wl_prep_words(wn)),
            ("wl_prep_regions", lambda: ops.wl_prep_regions(feat)),
            ("wl_tn_gemm  G = R^ R^^T", lambda: ops.wl_tn_gemm(rn, rn, e, r, r, b, torch.bfloat16)),
            ("wl_cols_fwd", lambda: ops.wl_cols_fwd(rn, w, gm, ml.view(-1), t, 5.0)),
            ("wl_rows", lambda: ops.wl_rows(nn, q, ml.view(-1), b, t, 5.0, 50.0)),
            ("xent_sym", lambda: ops.xent_sym(sim_t, 1.0, loss, True, None)),
            ("wl_cols_bwd", lambda: ops.wl_cols_bwd(rn, w, gm, ml.view(-1), dsim, pi, t, 5.0, 50.0)),
            ("wl_tn_gemm  dG = 2 (alpha dq) alpha^T", lambda: ops.wl_tn_gemm(a_s, al, ldp, r, r, b, torch.bfloat16, alpha=2.0)),
            ("wl_tn_gemm  dR^ = [dS | dG] [W^T | R^T]^T", lambda: ops.wl_tn_gemm(ds, wt, ldp, r, e, b, torch.float32, x1=dg2,
                                                                                  y1=rnt, k1=r, y0_shared=True)),
            ("l2norm_bwd_bf16y", lambda: ops.l2norm_bwd_bf16y(drn.view(b * r, e), rn.view(b * r, e), rinv, torch.bfloat16)),
        ]
        for name, fn in rows:
            print(f"    T = {t:2d}  {name:44s} {timed(fn, args.iters):7.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--batch", type=int, default=56)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=420, help="seconds each child process may take")
    ap.add_argument("--child", choices=["steps", "launches"])
    ap.add_argument("--only", choices=["steps", "launches"], help="driver: run this part alone")
    args = ap.parse_args()
    if args.steps // args.window < 3:
        ap.error("at least three alternating windows: --steps >= 3 * --window")
    if args.child == "steps":
        return child_steps(args)
    if args.child == "launches":
        return child_launches(args)
    for part in ("launches", "steps"):
        if args.only and part != args.only:
            continue
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", part,
               "--steps", str(args.steps), "--window", str(args.window), "--batch", str(args.batch), "--iters", str(args.iters)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            raise SystemExit(f"bench_ln: part '{part}' ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
