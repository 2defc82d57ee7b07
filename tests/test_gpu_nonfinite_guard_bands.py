"""The entry points of config.skip_nonfinite_updates inside the guard-band allocator (tests/guard.py): the case-running bodies of
tests/test_gpu_nonfinite_guard.py with torch's allocation functions routed through ``Guard.alloc``, at ``skew`` 0 and 16.  A body
passes only if its own bit-equality assertions still hold with NaN bytes around every operand (a scan that reads one element past a
segment counts a bad value the reference does not; a guarded launch that writes past its arena changes a band byte), no band byte
changed, and nothing was allocated behind the guard's back."""
import pytest

from tests import test_gpu_nonfinite_guard as NG
from tests.test_gpu_guard import _run, skews

pytestmark = pytest.mark.gpu


@skews
@pytest.mark.parametrize("kind", [None, "nan", "-inf"], ids=["benign", "nan", "-inf"])
def test_verdict_kernel(kind, skew):
    _run(skew, NG.body_verdict, kind)


@skews
def test_verdict_kernel_more_chunks_than_workgroups(skew):
    _run(skew, NG.body_verdict_many_chunks)


@skews
@pytest.mark.parametrize("n", [4099, 3, 1023 * 5 + 2])
def test_guarded_flat_adam(n, skew):
    _run(skew, NG.body_adam_dev, n)


@skews
@pytest.mark.parametrize("zero_grads", [True, False], ids=["zeroing", "first-write"])
def test_guarded_sigma_adam_and_tiles(zero_grads, skew):
    _run(skew, NG.body_adam_sn_and_tiles, zero_grads)


@skews
def test_commit_if_and_metrics_accum_if(skew):
    _run(skew, NG.body_commit_and_metrics)
