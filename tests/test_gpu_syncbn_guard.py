"""The split BatchNorm entry points of cross-replica groups (xmc_bn_batch_sums, xmc_bn_finalize_rows, xmc_rows_mean, and
ops.cbn_act_bwd with ``reduce_s``) inside the guard-band allocator (tests/guard.py): the case-running bodies of
tests/test_gpu_syncbn.py at ``skew`` 0 and 16.  A body passes only if its own float64 assertions still hold with NaN bytes around
every operand -- the [G][2C] row tables and the partial-row workspace included --, no byte of any guard band changed, and nothing
was allocated behind the guard's back."""
import pytest

from tests import test_gpu_syncbn as B
from tests.guard import Guard, guarded

pytestmark = pytest.mark.gpu

skews = pytest.mark.parametrize("skew", [0, 16])


def _run(skew, body, *args, **kw):
    g = Guard("cuda", skew=skew)
    try:
        with guarded(g):
            out = body(*args, **kw)
    except Exception as e:                                  # a faulted device answers every later call with the same error:
        if "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e):       # nothing more is started on it
            pytest.exit(f"GPU fault in {getattr(body, '__name__', body)}{args} at skew {skew}: {e}", returncode=3)
        raise
    assert g.served > 0, "the body allocated nothing through the guard"
    g.check()
    assert g.fallthrough == [], g.fallthrough
    return out


@skews
@pytest.mark.parametrize("dtype", B.DT)
@pytest.mark.parametrize("geo,groups", B.FWD_CASES)
def test_forward_statistics_over_shards(geo, groups, dtype, skew):
    _run(skew, B.run_fwd_shards, geo, groups, dtype)


@skews
@pytest.mark.parametrize("dtype", B.DT)
@pytest.mark.parametrize("geo", B.BWD_GEOS)
def test_backward_over_shards(geo, dtype, skew):
    _run(skew, B.run_bwd_shards, geo, dtype)
