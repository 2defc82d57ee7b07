"""Every entry point of csrc/clip.hip inside the guard-band allocator (tests/guard.py): the case-running bodies of
tests/test_gpu_clip.py at shapes whose last workgroup is partly idle (row counts that are no multiple of the four rows per
workgroup, t = 77 and 128 in the attention, GEMM tiles that overhang), at ``skew`` 0 and 16.  A body passes only if its own float64
assertions still hold with NaN bytes around every operand, no byte of any guard band changed, and nothing was allocated behind the
guard's back."""
import pytest
import torch

from tests import test_gpu_clip as B
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
@pytest.mark.parametrize("t,causal", [(1, 0), (77, 1), (128, 0), (128, 1)])
def test_mha_attention(t, causal, skew):
    _run(skew, B.run_attention, t, causal)


@skews
@pytest.mark.parametrize("rows,h,alias", [(7, 4, False), (9, 1024, True)])
def test_bias_add_ln(rows, h, alias, skew):
    _run(skew, B.run_bias_add_ln, rows, h, True, True, alias)


@skews
def test_plain_layer_norm(skew):
    _run(skew, B.run_bias_add_ln, 51, 128, False, False, False)


@skews
def test_bias_quick_gelu(skew):
    _run(skew, B.run_bias_quick_gelu, 51, 256)


@skews
def test_vision_embed(skew):
    _run(skew, B.run_vision_embed, 3, 128, 5)


@skews
def test_text_embed(skew):
    _run(skew, B.run_text_embed, 3, 128, 77)


@skews
def test_gather_rows_ln(skew):
    _run(skew, B.run_gather_rows_ln, 5, 128, 77)


@skews
@pytest.mark.parametrize("hw,size,dtype", [(32, 64, torch.float32), (256, 224, torch.float32), (128, 224, torch.bfloat16)])
def test_clip_preprocess(hw, size, dtype, skew):
    _run(skew, B.run_preprocess, hw, size, 32, dtype)


@skews
def test_pair_cosine(skew):
    _run(skew, B.run_pair_cosine, 7, 64)


@skews
def test_rprecision_hits(skew):
    _run(skew, B.run_rprecision, 7, 3, 64)


@skews
@pytest.mark.parametrize("tower", ["image", "text"])
def test_encoder(tower, skew):
    """the whole chain, its GEMMs (no split-K workspace) included: weights, activations and outputs all inside bands"""
    B.reference("small5", 5)                                 # (the CPU reference is computed outside the patched allocator)
    _run(skew, B.run_encoder, "small5", tower, 5)
