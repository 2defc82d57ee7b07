"""Every entry point of the caption encoder inside the guard-band allocator (tests/guard.py): the case-running bodies of
tests/test_gpu_bert.py with N = 3 (51 rows: the last workgroup of the row kernels holds three live rows and an idle wave, the
GEMM tiles overhang), at ``skew`` 0 and 16.  A body passes only if its own float64 assertions still hold with NaN bytes around
every operand, no byte of any guard band changed, and nothing was allocated behind the guard's back."""
import pytest

from tests import test_gpu_bert as B
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
@pytest.mark.parametrize("h", [128, 768])
def test_embed_ln(h, skew):
    _run(skew, B.run_embed_ln, 3, h)


@skews
@pytest.mark.parametrize("h", [128, 768])
def test_bias_residual_ln(h, skew):
    _run(skew, B.run_bias_residual_ln, 3, h)


@skews
def test_bias_gelu(skew):
    _run(skew, B.run_bias_gelu, 51, 512)


@skews
@pytest.mark.parametrize("h", [128, 768])
def test_attention(h, skew):
    _run(skew, B.run_attention, 3, h)


@skews
def test_sentence(skew):
    _run(skew, B.run_sentence, 3, 128)


@skews
@pytest.mark.parametrize("fast", [False, True], ids=["float32", "fast"])
def test_encoder(fast, skew):
    """the whole chain, its GEMMs (no split-K workspace) included: weights, activations and outputs all inside bands"""
    B.reference("small", 3)                                  # (the CPU reference is computed outside the patched allocator)
    _run(skew, B.run_encoder, "small", 3, fast)
