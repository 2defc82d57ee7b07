"""conv3x3 next to a 2x resampling: the 3x3 kernel (ups gather / pooled epilogue) vs four 2x2 convolutions on the low-resolution
grid (conv_phase_kernel), C1 shapes (B = 56; D at 2B = 112), forward and data gradient, interleaved rounds.
TF/s are ALGORITHMIC (the 3x3 formulation's 2 M K N); the phase launches execute 4/9 of them.
--fp8: the "out"-form rows (G's ups forwards, D's ups data gradients with a 64-multiple reduction) in the MX-fp8 mode instead:
the MX 3x3 kernel on the upsampled gather, the bf16 phase kernel and the MX phase kernel (ops.fp8_phase_mx), the two MX kernels
once with the quantisation pass in the launch ("+q") and once on packets that are already there ("pk").  Then the "in"-form rows
(D's pooled forwards, G's pooled data gradients with a 64-multiple reduction): the bf16 3x3 kernel with the pooled epilogue, the
MX 3x3 kernel with it, the bf16 "in" phase kernel and the MX "in" phase kernel (ops.fp8_phase_in_mx), "+q" and "pk" as above,
with the spread of the bf16 "in" phase row over the rounds (a row is a gain only beyond that spread).
usage (GPU box): PYTHONPATH=. python tools/bench_phase.py [--iters 5] [--fp8]"""
import argparse
import math
import torch
from xmcgan_image_generation_amd.ops import HipOps

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--batch", type=int, default=56)
ap.add_argument("--only-phase", action="store_true", help="time only the phase-decomposed forward / data-gradient launches (ablation builds)")
ap.add_argument("--fp8", action="store_true", help="MX 3x3 vs bf16 phase vs MX phase on the out-form rows")
args = ap.parse_args()
ops = HipOps(torch.bfloat16)
g = torch.Generator().manual_seed(0)
B = args.batch
# (name, kind, n, low-res side, cin, cout): "ups": x at low res; "pool": x at 2 * low res
LAYERS = [("G 4>8   1536>1536", "ups", B, 4, 1536, 1536), ("G 8>16  1536>768", "ups", B, 8, 1536, 768),
          ("G 16>32 768>384", "ups", B, 16, 768, 384), ("G 32>64 384>192", "ups", B, 32, 384, 192),
          ("G 64>128 192>96", "ups", B, 64, 192, 96),
          ("D 128>64 96>96", "pool", 2 * B, 64, 96, 96), ("D 64>32 192>192", "pool", 2 * B, 32, 192, 192),
          ("D 32>16 384>384", "pool", 2 * B, 16, 384, 384), ("D 16>8  768>768", "pool", 2 * B, 8, 768, 768),
          ("D 8>4   1536>1536", "pool", 2 * B, 4, 1536, 1536)]


def timed(fn):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 10


def fp8_rows():
    """one line per out-form launch: ms of bf16 3x3 | MX 3x3 +q, pk | bf16 phase | MX phase +q, pk | MX phase pk / bf16 phase"""
    print(f"{'launch':28s} {'GF':>6s} | bf16 3x3 | MX 3x3 +q     pk | bf16 phase | MX phase +q     pk | bf16 phase / MX phase: +q    pk")
    tot = [0.0] * 6
    for name, kind, n, lo, cin, cout in LAYERS:
        w = (torch.randn((cout, 9, cin), generator=g) / math.sqrt(9 * cin)).cuda()
        k = cin if kind == "ups" else cout               # reduction length of the out-form launch
        rows = cout if kind == "ups" else cin
        if k % 64:
            continue
        pick = (lambda pair: pair[0]) if kind == "ups" else (lambda pair: pair[1])
        ops.fp8, ops.fp8_phase, ops.fp8_phase_mx = False, True, False
        w3 = pick(ops.prep_conv_weight(w, None, True))
        ops.fp8, ops.fp8_phase = True, False
        w3x = pick(ops.prep_conv_weight(w, None, True))
        ops.fp8_phase, ops.fp8_phase_mx = True, True
        wph = pick(ops.prep_conv_weight(w, None, True, phase=kind))
        assert w3x.mx8 is not None and wph.phase_mx8 is not None
        t = torch.randn((n, lo, lo, k), generator=g).cuda().bfloat16()
        tq = t.clone()
        tq.mx8 = (ops.quantize_mx8(t), False)
        if kind == "ups":
            kw = dict(bias=torch.zeros(rows, device="cuda"))
        else:
            kw = dict(bias=None, alpha=0.25, alpha_dev=torch.ones(1, device="cuda"),
                      mask=torch.randn((n, 2 * lo, 2 * lo, rows), generator=g).cuda().bfloat16())

        def launch(mode, wt, src):
            ops.fp8, ops.fp8_phase, ops.fp8_phase_mx = mode
            y = ops.conv(src, wt, kw["bias"], ks=3, ups=True, **{a: b for a, b in kw.items() if a != "bias"})
            return y
        variants = [((False, True, False), w3, t, False, False), ((True, False, False), w3x, t, False, False), ((True, False, False), w3x, tq, False, False),
                    ((True, True, False), wph, t, True, False), ((True, True, True), wph, t, True, True), ((True, True, True), wph, tq, True, True)]
        for mode, wt, src, ph, mxph in variants:           # every column runs the kernel it is named after
            launch(mode, wt, src)
            assert ops.last_conv_phase == ph and ops.last_conv_mx8_phase == mxph, (name, mode)
        best = [1e9] * 6
        for r in range(args.iters):
            for i, (mode, wt, src, _, _) in enumerate(variants):
                best[i] = min(best[i], timed(lambda: launch(mode, wt, src)))
        for i in range(6):
            tot[i] += best[i]
        fl = 2.0 * n * 4 * lo * lo * k * rows * 9
        print(f"{name + (' fwd' if kind == 'ups' else ' dgrad'):28s} {fl / 1e9:6.1f} | {best[0]:8.3f} | {best[1]:9.3f} {best[2]:6.3f} | {best[3]:10.3f} |"
              f" {best[4]:11.3f} {best[5]:6.3f} | {best[3] / best[4]:25.2f} {best[3] / best[5]:5.2f}")
    print(f"{'TOTAL':28s}        | {tot[0]:8.3f} | {tot[1]:9.3f} {tot[2]:6.3f} | {tot[3]:10.3f} | {tot[4]:11.3f} {tot[5]:6.3f} |"
          f" {tot[3] / tot[4]:25.2f} {tot[3] / tot[5]:5.2f}")


def fp8_in_rows():
    """one line per in-form launch: ms of bf16 3x3 pooled | MX 3x3 pooled +q, pk | bf16 in-phase | MX in-phase +q, pk | ratios"""
    print(f"{'launch':28s} {'GF':>6s} | bf16 3x3 | MX 3x3 +q     pk | bf16 phase (spread) | MX phase +q     pk | bf16 phase / MX phase: +q    pk")
    tot = [0.0] * 6
    tot_hi = 0.0                                       # the bf16 "in" phase rows' slowest rounds: the spread of the yardstick
    for name, kind, n, lo, cin, cout in LAYERS:
        w = (torch.randn((cout, 9, cin), generator=g) / math.sqrt(9 * cin)).cuda()
        k = cin if kind == "pool" else cout              # reduction length of the in-form launch
        rows = cout if kind == "pool" else cin
        if k % 64:
            continue
        pick = (lambda pair: pair[0]) if kind == "pool" else (lambda pair: pair[1])
        ops.fp8, ops.fp8_phase, ops.fp8_phase_mx, ops.fp8_phase_in_mx = False, True, False, False
        w3 = pick(ops.prep_conv_weight(w, None, True))
        ops.fp8, ops.fp8_phase = True, False
        w3x = pick(ops.prep_conv_weight(w, None, True))
        ops.fp8_phase, ops.fp8_phase_in_mx = True, True
        wph = pick(ops.prep_conv_weight(w, None, True, phase="pool" if kind == "pool" else "ups"))
        assert w3x.mx8 is not None and wph.phase[0] == "in" and wph.phase_mx8 is not None
        relu = kind == "pool"
        t = torch.randn((n, 2 * lo, 2 * lo, k), generator=g).cuda().bfloat16()
        tq = t.clone()
        tq.mx8 = (ops.quantize_mx8(t, relu=relu), relu)
        if kind == "pool":
            bias = torch.zeros(rows, device="cuda")
            kw = dict(relu_in=True, res=torch.randn((n, lo, lo, rows), generator=g).cuda().bfloat16(), alpha_dev=torch.ones(1, device="cuda"))
        else:
            bias, kw = None, dict(alpha=4.0)

        def launch(mode, wt, src):
            ops.fp8, ops.fp8_phase, ops.fp8_phase_in_mx = mode
            if ops.can_pool_out(src, wt):
                return ops.conv(src, wt, bias, ks=3, pool_out=True, **kw)
            kw2 = {a: b for a, b in kw.items() if a != "res"}              # (grids under 32 pixels a row on the 3x3 kernels)
            return ops.pool2(ops.conv(src, wt, bias, ks=3, **{**kw2, "alpha": 1.0}), 0.25 * kw.get("alpha", 1.0), res=kw.get("res"))
        variants = [((False, True, False), w3, t, False, False), ((True, False, False), w3x, t, False, False), ((True, False, False), w3x, tq, False, False),
                    ((True, True, False), wph, t, True, False), ((True, True, True), wph, t, True, True), ((True, True, True), wph, tq, True, True)]
        for mode, wt, src, ph, mxph in variants:           # every column runs the kernel it is named after
            launch(mode, wt, src)
            assert ops.last_conv_phase == ph and ops.last_conv_mx8_phase_in == mxph and not ops.last_conv_mx8_phase, (name, mode)
        best = [1e9] * 6
        worst3 = 0.0
        for r in range(args.iters):
            for i, (mode, wt, src, _, _) in enumerate(variants):
                ms = timed(lambda: launch(mode, wt, src))
                best[i] = min(best[i], ms)
                if i == 3:
                    worst3 = max(worst3, ms)
        for i in range(6):
            tot[i] += best[i]
        tot_hi += worst3
        spread = worst3 / best[3] - 1.0
        fl = 2.0 * n * 4 * lo * lo * k * rows * 9
        verdict = "gain" if best[3] / best[5] > 1.0 + spread else ("level" if best[5] / best[3] <= 1.0 + spread else "slower")
        print(f"{name + (' fwd' if kind == 'pool' else ' dgrad'):28s} {fl / 1e9:6.1f} | {best[0]:8.3f} | {best[1]:9.3f} {best[2]:6.3f} | {best[3]:10.3f} ({spread * 100:4.1f} %) |"
              f" {best[4]:11.3f} {best[5]:6.3f} | {best[3] / best[4]:25.2f} {best[3] / best[5]:5.2f}  {verdict}")
    print(f"{'TOTAL':28s}        | {tot[0]:8.3f} | {tot[1]:9.3f} {tot[2]:6.3f} | {tot[3]:10.3f} ({(tot_hi / tot[3] - 1) * 100:4.1f} %) | {tot[4]:11.3f} {tot[5]:6.3f} |"
          f" {tot[3] / tot[4]:25.2f} {tot[3] / tot[5]:5.2f}")


if args.fp8:
    fp8_rows()
    print()
    fp8_in_rows()
    raise SystemExit(0)
print(f"{'layer':22s} {'GF':>6s} | fwd 3x3 ms TF/s | fwd phase ms TF/s    x | dgrad 3x3 ms TF/s | dgrad phase ms TF/s    x | wgrad 3x3 ms TF/s | wgrad phase ms TF/s    x")
tot = [0.0] * 6
for name, kind, n, lo, cin, cout in LAYERS:
    hi = 2 * lo
    w = torch.randn((cout, 9, cin), generator=g) / math.sqrt(9 * cin)
    ops.phase_conv = True
    wfp, wdp = ops.prep_conv_weight(w.cuda(), None, True, phase=kind)
    wf3, wd3 = ops.prep_conv_weight(w.cuda(), None, True)
    wsel = lambda: (wfp, wdp) if ops.phase_conv else (wf3, wd3)
    bias = torch.zeros(cout, device="cuda")
    if kind == "ups":
        x = torch.randn((n, lo, lo, cin), generator=g).cuda().bfloat16()
        dy = torch.randn((n, hi, hi, cout), generator=g).cuda().bfloat16()
        fwd = lambda: ops.conv(x, wsel()[0], bias, ks=3, ups=True)
        bwd = lambda: ops.conv(dy, wsel()[1], None, ks=3, pool_out=True, alpha=4.0) if ops.can_pool_out(dy, wsel()[1]) else ops.pool2(ops.conv(dy, wsel()[1], None, ks=3), 1.0)
    else:
        x = torch.randn((n, hi, hi, cin), generator=g).cuda().bfloat16()
        dy = torch.randn((n, lo, lo, cout), generator=g).cuda().bfloat16()
        res = torch.randn((n, lo, lo, cout), generator=g).cuda().bfloat16()
        fwd = lambda: ops.conv(x, wsel()[0], bias, ks=3, pool_out=True, relu_in=True, res=res) if ops.can_pool_out(x, wsel()[0]) else ops.pool2(ops.conv(x, wsel()[0], bias, ks=3, relu_in=True), 0.25, res=res)
        bwd = lambda: ops.conv(dy, wsel()[1], None, ks=3, ups=True, alpha=0.25, mask=x)
    fl = 2.0 * n * hi * hi * cin * cout * 9
    dw = torch.zeros((cout, 9, cin), device="cuda")
    db = torch.zeros((cout,), device="cuda")
    if kind == "ups":
        wg = lambda: ops.conv_wgrad(x, dy, dw, db, ks=3, x_ups=True, sync=True)
    else:
        wg = lambda: ops.conv_wgrad(x, dy, dw, db, ks=3, x_relu=True, dy_ups=True, alpha=0.25, sync=True)
    best = [1e9] * 6
    for r in range(args.iters):
        for k, (ph, fn) in enumerate(((False, fwd), (True, fwd), (False, bwd), (True, bwd), (False, wg), (True, wg))):
            if args.only_phase and k not in (1, 3):
                best[k] = 1.0
                continue
            ops.phase_conv = ph
            best[k] = min(best[k], timed(fn))
    for k in range(6):
        tot[k] += best[k]
    print(f"{name:22s} {fl / 1e9:6.1f} | {best[0]:7.3f} {fl / best[0] / 1e9:6.0f} | {best[1]:9.3f} {fl / best[1] / 1e9:6.0f} {best[0] / best[1]:5.2f} |"
          f" {best[2]:9.3f} {fl / best[2] / 1e9:6.0f} | {best[3]:11.3f} {fl / best[3] / 1e9:6.0f} {best[2] / best[3]:5.2f} |"
          f" {best[4]:9.3f} {fl / best[4] / 1e9:6.0f} | {best[5]:11.3f} {fl / best[5] / 1e9:6.0f} {best[4] / best[5]:5.2f}")
print(f"{'TOTAL':22s}        | {tot[0]:7.3f}        | {tot[1]:9.3f}        {tot[0] / tot[1]:5.2f} | {tot[2]:9.3f}        | {tot[3]:11.3f}        {tot[2] / tot[3]:5.2f} |"
      f" {tot[4]:9.3f}        | {tot[5]:11.3f}        {tot[4] / tot[5]:5.2f}")
