#!/usr/bin/env python
"""Throughput of the caption encoder at BERT-base size: captions/s for float32 and ``fast`` (bf16 MFMA GEMMs) at chunks 256 and 1024.
Random weights and ids (the arithmetic does not depend on them), T = 17.  Device events around whole forward passes, after a
warm-up, over a timed window of at least one second; the upload of the ids is inside the window, the download of the result is not.

usage (on the GPU box): python tools/bench_bert.py [--out profiles/r09_bench_bert.txt] [--chunks 256 1024] [--modes float32 fast]
       --passes N: run N forward passes of one mode / chunk and exit (for a kernel trace of the encoder alone)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from xmcgan_image_generation_amd.ops import HipOps  # noqa: E402
from xmcgan_image_generation_amd.utils import bert_arch, bert_utils  # noqa: E402

T = 17


def flops_per_caption(d):
    dense = 2 * T * d.layers * (3 * d.hidden * d.hidden + d.hidden * d.hidden + 2 * d.hidden * d.ffn)
    return dense, 4 * T * T * d.hidden * d.layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--chunks", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--modes", nargs="+", default=["float32", "fast"], choices=["float32", "fast"])
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per measurement (at least)")
    ap.add_argument("--passes", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    params = bert_arch.init_bert(0)
    rng = np.random.default_rng(0)
    lines = [f"# tools/bench_bert.py on {torch.cuda.get_device_name(0)}: BERT-base (12 x 768, 3072), T = {T}, random weights",
             "# mode chunk passes seconds captions/s dense_TFLOP/s"]
    for mode in a.modes:
        fast = mode == "fast"
        enc = bert_utils.BertEncoder(HipOps(dtype=torch.bfloat16 if fast else torch.float32), params, fast=fast)
        dense, _ = flops_per_caption(enc.dims)
        for chunk in a.chunks:
            max_len = rng.integers(4, T + 1, size=chunk)
            ids = np.zeros((chunk, T), np.int64)
            for i, m in enumerate(max_len):
                ids[i, :m] = rng.integers(1, enc.dims.vocab, size=m)
            if a.passes:
                for _ in range(a.passes):
                    enc.forward_device(ids, max_len)
                torch.cuda.synchronize()
                continue
            for _ in range(3):
                enc.forward_device(ids, max_len)
            torch.cuda.synchronize()
            passes, seconds = 4, 0.0
            while True:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(passes):
                    enc.forward_device(ids, max_len)
                t1.record()
                torch.cuda.synchronize()
                seconds = t0.elapsed_time(t1) / 1e3
                if seconds >= a.window:
                    break
                passes = max(passes * 2, int(passes * 1.2 * a.window / max(seconds, 1e-3)) + 1)
            rate = passes * chunk / seconds
            lines.append(f"{mode} {chunk} {passes} {seconds:.3f} {rate:.1f} {rate * dense / 1e12:.2f}")
            print(lines[-1], flush=True)
    if a.out and not a.passes:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
