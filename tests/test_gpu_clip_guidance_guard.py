"""The four entry points of csrc/clip_grad.hip inside the guard-band allocator (tests/guard.py): the case-running bodies of
tests/test_gpu_clip_guidance.py at their smallest shape and at one odd shape each (row counts that are no multiple of the four rows
per workgroup, t = 1 and t = 65 in the attention -- the second pass of 32 query rows has one row --, an image side whose rows
overhang the 256 threads), at ``skew`` 0 and 16; and the whole pullback.  A body passes only if its own float64 assertions still
hold with NaN bytes around every operand, no byte of any guard band changed, and nothing was allocated behind the guard's back."""
import pytest
import torch

from tests import test_gpu_clip_guidance as B
from tests.test_gpu_clip_guard import _run

pytestmark = pytest.mark.gpu

skews = pytest.mark.parametrize("skew", [0, 16])


@skews
@pytest.mark.parametrize("t,causal", [(1, 0), (65, 1), (128, 0)])
def test_mha_attention_bwd(t, causal, skew):
    _run(skew, B.run_attention_bwd, t, causal)


@skews
@pytest.mark.parametrize("rows,h,alias", [(7, 4, False), (9, 1024, True)])
def test_ln_bwd_add(rows, h, alias, skew):
    _run(skew, B.run_ln_bwd, rows, h, True, alias)


@skews
@pytest.mark.parametrize("n,h,t", [(3, 128, 5), (2, 768, 50)])
def test_ln_bwd_add_row_maps(n, h, t, skew):
    _run(skew, B.run_ln_bwd_row_maps, n, h, t)


@skews
@pytest.mark.parametrize("rows,f", [(1, 8), (51, 256)])
def test_bias_quick_gelu_bwd(rows, f, skew):
    _run(skew, B.run_bias_quick_gelu_bwd, rows, f)


@skews
@pytest.mark.parametrize("hw,size,dtype", [(32, 64, torch.float32), (256, 224, torch.bfloat16)])
def test_clip_preprocess_bwd(hw, size, dtype, skew):
    _run(skew, B.run_preprocess_bwd, hw, size, 32, dtype)


@skews
def test_tower_gradient(skew):
    """the whole chain, its GEMMs included: weights, tape, scratch and the image cotangent all inside bands"""
    B.grad_reference("small5", 5)                            # (the CPU reference is computed outside the patched allocator)
    _run(skew, B.run_tower, "small5", False, 5)
