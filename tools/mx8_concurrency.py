"""Kernel-level hunt for the fp8 mode's race: each MX kernel (quantiser, weight packer, convolution with and without
split-K / upsampling / packet emission) is run repeatedly on one stream while a bf16 convolution keeps a second stream busy, and
its output bytes are compared with those of a run alone on the GPU.  A kernel whose result depends on who shares its CUs shows up.
    PYTHONPATH=. python tools/mx8_concurrency.py [--reps 30]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    from xmcgan_image_generation_amd._lib import XMC_BF16, XMC_CONV_PACKED, ConvDesc
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    dt = torch.bfloat16
    p_ = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    side = torch.cuda.Stream()
    # the neighbour: a long bf16 3x3 convolution
    nx = torch.randn((32, 64, 64, 192), generator=g).to(dt).cuda()
    nw = (torch.randn((192, 9, 192), generator=g) / 42).cuda()
    nwf, _ = ops.prep_conv_weight(nw)

    def noise(k=6):
        with torch.cuda.stream(side):
            for _ in range(k):
                ops.conv(nx, nwf, None, ks=3)

    cases = [  # tag, n, h, cin, cout, ups, relu_in, emit
        ("D 128 96>192-ish 64ch", 32, 128, 64, 128, False, True, True),
        ("G 64 192>192", 32, 64, 192, 192, False, False, None),
        ("G 32>64 384>192 ups", 32, 32, 384, 192, True, False, None),
        ("D 16 768>768", 32, 16, 768, 768, False, True, True),
        ("D 8 1536>1536 (split-K)", 32, 8, 1536, 1536, False, True, None),
        ("G 8>16 1536>768 ups (split-K)", 32, 8, 1536, 768, True, False, None),
    ]
    bad = 0
    for tag, n, h, cin, cout, ups, relu_in, emit in cases:
        x = torch.randn((n, h, h, cin), generator=g).to(dt).cuda()
        w = (torch.randn((cout, 9, cin), generator=g) / (9 * cin) ** 0.5).cuda()
        wf, _ = ops.prep_conv_weight(w)
        ho = 2 * h if ups else h
        d = ConvDesc(n, h, h, cin, cout, 3, int(ups), 0, 0, 0, XMC_BF16, 1.0, 1.0, XMC_CONV_PACKED, 0, 0, 0, 0, 0)
        wsb = ops.lib.xmc_conv2d_mx8_workspace_bytes(C.byref(d))

        def run_all():
            w8, wsc = ops.pack_mx8(wf)
            x8 = ops.quantize_mx8(x, relu=relu_in)
            y = torch.zeros((n, ho, ho, cout), dtype=dt, device="cuda")
            ws = torch.zeros((max(wsb, 4) // 4,), dtype=torch.float32, device="cuda")
            y8 = None
            if emit is not None and not wsb and cout % 64 == 0:
                y8 = torch.zeros((n * ho * ho, cout // 64, 80), dtype=torch.uint8, device="cuda")
            rc = ops.lib.xmc_conv2d_mx8(C.byref(d), p_(x8), p_(w8), p_(wsc), None, None, None, p_(y), p_(y8), int(bool(emit)),
                                        p_(ws) if wsb else None, ops._stream())
            assert rc == 0, rc
            return dict(w8=w8, wsc=wsc, x8=x8, y=y, y8=y8)
        torch.cuda.synchronize()
        ref = run_all()
        torch.cuda.synchronize()
        diffs = {}
        for r in range(a.reps):
            noise()
            got = run_all()
            torch.cuda.synchronize()
            for k, v in got.items():
                if v is None:
                    continue
                rv = ref[k]
                if k in ("x8", "y8"):                      # packets: 66 payload bytes of 80, the pad is never written
                    v, rv = v[..., :66], rv[..., :66]
                if not torch.equal(v.view(torch.uint8), rv.view(torch.uint8)):
                    diffs[k] = diffs.get(k, 0) + 1
        print(f"{tag:34s} split-K workspace {wsb >> 20:4d} MiB   differing runs of {a.reps}: {diffs if diffs else 'none'}", flush=True)
        bad += bool(diffs)
    print("RACE FOUND in the kernels above" if bad else "every MX kernel is bit-stable beside a busy neighbour")


if __name__ == "__main__":
    main()
