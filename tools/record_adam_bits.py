#!/usr/bin/env python
"""Record the bits every Adam / EMA optimiser entry point produces (tests/golden/adam_parent_bits.npz, replayed by
tests/test_gpu_adam_bits.py): the flat kernel behind adam_ema, adam_ema_dev and adam_ema_dev_sn, its sigma term on the synthetic
spectral bank of tests/test_gpu_optimizer.py, the tile kernel behind adam_wprep on that file's tile arenas, and every guarded form
with a clean and with a bad verdict.  Needs the GPU; uses only HipOps methods.

Record on a tree built from the PARENT of the change under test, never from the code under test:
    python tools/record_adam_bits.py [--out tests/golden/adam_parent_bits.npz]

What is stored.  The raw bits of all these arrays are several megabytes (the smallest tile arena with a 3 x 3 tensor is 10 K
elements x 5 arrays a case), so the file holds one 64-bit BLAKE2b digest per 2048 bytes of every array's raw bits (512 float32,
1024 bfloat16), in order, under "<case>/<array>".  Equal digests for every chunk of every array = the same bits; a differing
digest names the 512 elements that moved.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import adam_reference as AR  # noqa: E402
from tests import test_gpu_optimizer as TO  # noqa: E402

CHUNK_BYTES = 2048
FLAT_N = 2051                                # 512 float4 (three workgroups) + a 3-element tail
VERDICTS = ("none", "clean", "bad")          # unguarded; guarded with verdict[0] == 0; guarded with verdict[0] != 0


def digests(t):
    """one uint64 per CHUNK_BYTES of the raw bits of a tensor / array (the last chunk may be short)"""
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous().cpu().view(torch.uint8).numpy()
    raw = np.ascontiguousarray(t).view(np.uint8).reshape(-1).tobytes()
    return np.array([int.from_bytes(hashlib.blake2b(raw[o:o + CHUNK_BYTES], digest_size=8).digest(), "little")
                     for o in range(0, len(raw), CHUNK_BYTES)], dtype=np.uint64)


def _verdict(kind):
    return {"none": None, "clean": torch.zeros((4,), dtype=torch.int32).cuda(),
            "bad": torch.tensor([1, 3, 0, 0], dtype=torch.int32).cuda()}[kind]


def _kw(hp):
    return dict(lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], grad_scale=hp["grad_scale"], ema_decay=hp["ema_decay"])


def _guard(verdict):
    return {} if verdict is None else {"verdict": verdict}


def flat_cases(ops):
    """the four steps of AR.STEPS on FLAT_N elements with non-zero moments; no spectral table"""
    hp = AR.PARAM_SETS["moments"]
    p, m, v, ema = AR.make_state(FLAT_N, "moments", 5)
    grads = AR.make_grads(FLAT_N, 6, AR.STEPS)
    runs = [("adam_ema", e, False, False, "none") for e in (True, False)]
    runs += [("adam_ema_dev", e, False, False, vd) for e in (True, False) for vd in VERDICTS]
    runs += [("adam_ema_dev_sn", e, z, k, vd) for e in (True, False) for z in (True, False) for k in (True, False) for vd in VERDICTS]
    for entry, with_ema, zero, keep, vd in runs:
        d = dict(p=TO._dev(p), m=TO._dev(m), v=TO._dev(v), ema=TO._dev(ema) if with_ema else None)
        state, verdict = TO._state_bits(0), _verdict(vd)
        ops.keep_grads = keep
        for s, g in enumerate(grads):
            gd = TO._dev(g)
            if entry == "adam_ema":
                ops.adam_ema(d["p"], gd, d["m"], d["v"], d["ema"], step=s + 1, **_kw(hp))
            elif entry == "adam_ema_dev":
                ops.adam_ema_dev(d["p"], gd, d["m"], d["v"], d["ema"], state, **_kw(hp), **_guard(verdict))
            else:
                ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=zero, **_kw(hp), **_guard(verdict))
        out = {k: a for k, a in d.items() if a is not None}
        out.update(g=gd, state=state)
        yield f"flat/{entry}/ema{int(with_ema)}_zero{int(zero)}_keep{int(keep)}_{vd}", out


def sigma_cases(ops):
    """adam_ema_dev_sn with the spectral table on the synthetic bank: both u_axis values, a cols % 4 != 0 tensor, 64-element
    padding, a -2 stretch; two updates"""
    A = TO._sn_arena(ops)
    hp = AR.PARAM_SETS["product"]
    ud, vd_, sd = TO._dev(A["u"]), TO._dev(A["v"]), TO._dev(A["scal"])
    for mode in ("keep", "zero", "untouched"):
        for vd in VERDICTS:
            ops.keep_grads = mode == "keep"
            d = {k: TO._dev(a) for k, a in A["state"].items()}
            state, verdict = TO._state_bits(0), _verdict(vd)
            for g_in in A["grads"]:
                gd = TO._dev(g_in)
                kd = ops.sn_bank_dot(A["bank"], d["p"], gd, sd)
                ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=(mode == "zero"),
                                    fix=(A["map"], A["bank"], kd, sd, ud, vd_), **_kw(hp), **_guard(verdict))
            yield f"sigma/{mode}_{vd}", dict(d, g=gd, kvec=kd, state=state)


def tile_cases(ops):
    """adam_wprep behind the flat call that advances the step and skips the table's tensors, as the product runs them; two
    updates into the same (zero-initialised) prepared buffers and partial rows"""
    hp = dict(AR.PARAM_SETS["product"], ema_decay=0.99)
    for with_spectral in (True, False):
        A = TO._wprep_arena(ops, with_spectral)
        wp, bank, size = A["wp"], A["bank"], A["size"]
        if with_spectral:
            ud, vd_, sd = TO._dev(A["u"]), TO._dev(A["v"]), TO._dev(A["scal"])
            skip = ops.wprep_skip_map(wp, size, base=ops.sn_bank_map(bank, size))
        else:
            skip = ops.wprep_skip_map(wp, size)
        for mode in ("keep", "zero"):
            for vd in VERDICTS:
                ops.keep_grads = mode == "keep"
                d = {k: TO._dev(a) for k, a in A["state"].items()}
                state, verdict = TO._state_bits(0), _verdict(vd)
                bufs, part = ops.wprep_alloc(wp)
                for b in bufs + [part]:
                    b.zero_()
                kd = None
                for g_in in A["grads"]:
                    gd = TO._dev(g_in)
                    if with_spectral:
                        kd = ops.sn_bank_dot(bank, d["p"], gd, sd)
                        ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=(mode == "zero"),
                                            fix=(skip, bank, kd, sd, ud, vd_), **_kw(hp), **_guard(verdict))
                    else:
                        ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=(mode == "zero"), skip_map=skip,
                                            **_kw(hp), **_guard(verdict))
                    ops.adam_wprep(wp, (bufs, part), d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=(mode == "zero"),
                                   fix=(kd, sd, ud, vd_) if with_spectral else None, **_kw(hp), **_guard(verdict))
                out = dict(d, g=gd, state=state, part=part[:max(wp["part"], 1)])
                out.update({k: b[:max(wp[k], 1)] for k, b in zip(("wf", "wd", "pf", "pd"), bufs)})
                yield f"tile/{'fix' if with_spectral else 'plain'}/{mode}_{vd}", out


def record(ops):
    """{"<case>/<array>": digests} of every case, on the code that ``ops`` runs"""
    keep = ops.keep_grads
    out = {}
    try:
        for gen in (flat_cases, sigma_cases, tile_cases):
            for case, arrays in gen(ops):
                torch.cuda.synchronize()
                for name, t in arrays.items():
                    out[f"{case}/{name}"] = digests(t)
    finally:
        ops.keep_grads = keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "adam_parent_bits.npz"))
    args = ap.parse_args()
    from xmcgan_image_generation_amd.ops import HipOps
    rec = record(HipOps(dtype=torch.bfloat16))
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} arrays, {sum(a.size for a in rec.values())} digests, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
