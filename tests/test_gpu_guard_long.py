"""The 64-token kernels inside the guard-band allocator (tests/guard.py), as tests/test_gpu_guard.py runs the others: the long
MFMA attention_for_g (dense and row-pitch forms) and ``xmc_bert_attention_long`` at their smallest cases, at skew 0 and 16.  A body
passes only if its own assertions hold with NaN bytes around every operand and in every fresh output, no guard byte changed and
nothing was allocated behind the guard's back."""
import pytest

from tests import test_gpu_attn_long as AL
from tests import test_gpu_bert_long as BL
from tests.test_gpu_guard import _run, skews

pytestmark = pytest.mark.gpu


@skews
@pytest.mark.parametrize("case", [(2, 128, 33, 768), (2, 128, 64, 128)], ids=["2-128-33-768", "2-128-64-128"])
def test_attention_for_g_long_on_mfma(case, skew):
    _run(skew, AL.run_case, *case)


@skews
def test_sliced_context_forms(skew):
    _run(skew, AL.run_sliced, 2, 128, 33, 768)


@skews
@pytest.mark.parametrize("t", [33, 64])
def test_bert_attention_long(t, skew):
    _run(skew, BL.run_attention_long, 3, 128, t)
