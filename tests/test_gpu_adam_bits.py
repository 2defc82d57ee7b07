"""Every Adam / EMA optimiser entry point reproduces, bit for bit, what tests/golden/adam_parent_bits.npz recorded from the
parent of the change that wrote the update's rounding down in source (csrc/adam_update.h): tools/record_adam_bits.py defines
the cases and runs them again here on the code under test.

The file holds one digest per 512 float32 of every array (see the recorder), so "equal" means every digest of every array.  The
ONE exception: the flat cases' last ``ema`` chunk, which is exactly the 3-element scalar tail of the 2051-element arena.  The
parent's tail mixed the EMA as round(d * ema) + round((1 - d) * p) while its float4 loop -- every element the product ever
runs, arenas being padded to 64 -- used fma(d, ema, round((1 - d) * p)); the tail now takes the loop's rounding.  Its p, m and
v rounded like the loop already and are compared."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_adam_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_optimiser_entry_point_reproduces_the_parents_bits():
    from xmcgan_image_generation_amd.ops import HipOps
    want = np.load(os.path.join(ROOT, "tests", "golden", "adam_parent_bits.npz"))
    got = rec.record(HipOps(dtype=torch.bfloat16))
    assert sorted(got) == sorted(want.files) and len(got) == 371
    assert rec.FLAT_N == 2051 and rec.FLAT_N * 4 // rec.CHUNK_BYTES * rec.CHUNK_BYTES == (rec.FLAT_N & ~3) * 4      # last chunk == tail
    moved, skipped = {}, 0
    for key in sorted(got):
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.size > 0, key
        if key.startswith("flat/") and key.endswith("/ema") and "_bad/" not in key:      # (a bad verdict: no arithmetic at all)
            g, w = g[:-1], w[:-1]
            skipped += 1
        if not np.array_equal(g, w):
            moved[key] = np.flatnonzero(g != w).tolist()
    assert skipped == 11                             # the flat cases that update an EMA
    assert not moved, ("arrays whose bits differ from the parent's -> their 512-element chunks", moved)
    # the recording is not vacuous: a bad verdict leaves another state behind than a clean one, a clean one the unguarded one
    for case in ("flat/adam_ema_dev/ema1_zero0_keep0", "sigma/keep", "tile/fix/zero", "tile/plain/zero"):
        assert np.array_equal(want[f"{case}_clean/p"], want[f"{case}_none/p"])
        assert not np.array_equal(want[f"{case}_bad/p"], want[f"{case}_none/p"])
