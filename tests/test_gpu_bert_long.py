"""The caption encoder at Localized Narratives' length (33 <= T <= 64): ``xmc_bert_attention_long`` against float64
(tests/bert_ref.py), its domain, the row kernels at T = 64, and the whole encoder at T = 64 with the yardsticks of
tests/test_gpu_bert.py (computed from the reference alone).

Kernel bound: a score is the same 64-term fmaf chain as at T = 17 and the context a chain of <= 64 fmaf instead of <= 17
(64 u sum|p v| = 3.8e-6 sum|p v|), still inside the existing 1e-5 sum_j |p_j v_j| + 1e-6.  max_len covers T, 2, the 32 / 33 boundary
of the short kernel's domain and a length between.  The sentence bound is T + 1 roundings (T serial adds, one division) in place of
18.  The last test needs no device: the argument checks run on the host before any HIP call."""
import functools

import numpy as np
import pytest
import torch

from tests import bert_ref as R
from xmcgan_image_generation_amd import _lib
from xmcgan_image_generation_amd.utils import bert_arch, bert_utils

gpu = pytest.mark.gpu

MAX_LENS = [64, 2, 33, 32, 47]
SMALL = dict(layers=2, hidden=128, ffn=512, vocab=64, max_pos=80)
T_ENC = 64


def get_ops(fast=False):
    from tests.test_gpu_bert import get_ops as g
    return g(fast)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _max_lens(n, t):
    return np.minimum(np.array(MAX_LENS[:n]), t)


def run_attention_long(n, h, t):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n * 1000 + h + t)
    rows = n * t
    qkv, bias = torch.randn(rows, 3 * h, generator=gen), 0.1 * torch.randn(3 * h, generator=gen)
    ml = _max_lens(n, t).astype(np.int32)
    want, mag = R.attention(qkv.double(), bias.double(), ml, t)
    ctx = _nan((rows, h), dev)                                               # an unwritten element stays NaN
    ops.bert_attention_long(qkv.to(dev), bias.to(dev), torch.as_tensor(ml).to(dev), ml, ctx, t)
    err = (ctx.cpu().double() - want).abs()
    bound = 1e-5 * mag + 1e-6
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))      # (NaN fails the comparison)
    return float((err / bound).max())


@gpu
@pytest.mark.parametrize("h", [128, 768])
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("t", [33, 64])
def test_attention_long(t, n, h):
    run_attention_long(n, h, t)


@gpu
def test_long_kernel_equals_the_short_one_inside_its_domain():
    """the two kernels add the same products in the same order: at T = 17 and T = 32 the results are bit-equal"""
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(7)
    for t in (17, 32):
        n, h = 3, 128
        qkv, bias = torch.randn(n * t, 3 * h, generator=gen).to(dev), (0.1 * torch.randn(3 * h, generator=gen)).to(dev)
        ml = _max_lens(n, t).astype(np.int32)
        a, b = _nan((n * t, h), dev), _nan((n * t, h), dev)
        ops.bert_attention(qkv, bias, torch.as_tensor(ml).to(dev), ml, a, t)
        ops.bert_attention_long(qkv, bias, torch.as_tensor(ml).to(dev), ml, b, t)
        assert torch.equal(a, b), t


@gpu
def test_long_attention_outside_its_domain():
    ops = get_ops()
    dev = ops.device

    def attempt(t, h, ml):
        n = len(ml)
        qkv, bias = torch.zeros(n * t, 3 * h).to(dev), torch.zeros(3 * h).to(dev)
        ctx = torch.full((n * t, h), 7.0).to(dev)
        ml = np.array(ml, np.int32)
        with pytest.raises(_lib.XmcError):
            ops.bert_attention_long(qkv, bias, torch.as_tensor(ml).to(dev), ml, ctx, t)
        torch.cuda.synchronize()
        assert bool((ctx == 7.0).all())                                      # nothing ran

    attempt(65, 128, [5, 65])            # T beyond 64
    attempt(64, 128, [9, 1])             # max_len below 2
    attempt(64, 128, [65, 9])            # max_len beyond T
    attempt(64, 96, [9, 9])              # H no multiple of 64


@gpu
@pytest.mark.parametrize("n,h", [(3, 128), (5, 768)])
def test_row_kernels_at_64_tokens(n, h):
    """xmc_bert_embed_ln and xmc_bert_sentence take any T up to the position table: T = 64"""
    from tests.test_gpu_bert import _ln_check
    ops, t = get_ops(), 64
    dev = ops.device
    params = bert_arch.init_bert(11, layers=1, hidden=h, ffn=4 * h, vocab=64, max_pos=64)
    gen = torch.Generator().manual_seed(n * 1000 + h)
    ids = torch.randint(0, 64, (n, t), generator=gen, dtype=torch.int32)
    want, xhat, gamma = R.embed(params, ids.numpy())
    tabs = [torch.as_tensor(params[k]).to(dev) for k in bert_arch.EMBEDDING_KEYS]
    out = _nan((n * t, h), dev)
    ops.bert_embed_ln(ids.reshape(-1).contiguous().to(dev), *tabs, out, t)
    _ln_check(out.cpu(), want, xhat, gamma)
    emb = torch.randn(n * t, h, generator=gen)
    ml = _max_lens(n, t).astype(np.int32)
    want = R.sentence(emb.double().view(n, t, h), ml)
    sent = _nan((n, h), dev)
    ops.bert_sentence(emb.to(dev), torch.as_tensor(ml).to(dev), t, out=sent)
    bound = (t + 1) * 2.0 ** -24 * R.sentence(emb.double().abs().view(n, t, h), ml) + 1e-30      # T adds and one division
    err = (sent.cpu().double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


@functools.lru_cache(maxsize=None)
def reference():
    """(params, ids, max_len, ref64, e32, e_bf) of the small encoder at T = 64: computed once, shared, never modified"""
    params = bert_arch.init_bert(5, **SMALL)
    rng = np.random.default_rng(0)
    max_len = np.array(MAX_LENS, np.int64)
    ids = np.zeros((len(max_len), T_ENC), np.int64)
    for i, m in enumerate(max_len):
        ids[i, :m] = rng.integers(1, SMALL["vocab"], size=m)
    ref = R.forward(params, ids, max_len)
    e32 = float((R.forward(params, ids, max_len, torch.float32).double() - ref).abs().max())
    e_bf = float((R.forward(params, ids, max_len, round_bf16=True) - ref).abs().max())
    return params, ids, max_len, ref, e32, e_bf


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["float32", "fast"])
def test_encoder_at_64_tokens(fast):
    params, ids, max_len, ref, e32, e_bf = reference()
    enc = bert_utils.BertEncoder(get_ops(fast), params, fast=fast)
    emb, sent = enc.encode(ids, max_len)
    assert emb.shape == ref.shape == (5, 64, 128) and emb.dtype == np.float32 and enc.launches == 2 + 8 * enc.dims.layers
    err = float((torch.as_tensor(emb).double() - ref).abs().max())
    yard, factor = (e_bf, 2.0) if fast else (e32, 16.0)
    print(f"bert small T=64 {'fast' if fast else 'float32'}: err {err:.3e}, yardstick {yard:.3e}, ratio {err / yard:.3f} "
          f"(limit {factor:g})")
    assert err <= factor * yard, (err, yard)
    want = emb.astype(np.float64).sum(axis=1) / max_len[:, None]
    assert np.abs(sent - want).max() <= (T_ENC + 1) * 2.0 ** -24 * (np.abs(emb).astype(np.float64).sum(axis=1) / max_len[:, None]).max()


@gpu
def test_a_64_token_caption_does_not_depend_on_its_batch():
    params, ids, max_len, *_ = reference()
    ops = get_ops()
    whole, _ = bert_utils.BertEncoder(ops, params).encode(ids, max_len)
    split, _ = bert_utils.BertEncoder(ops, params, chunk=2).encode(ids, max_len)      # chunks 2 + 2 + 1
    assert np.array_equal(whole, split)
    alone = bert_utils.BertEncoder(ops, params)
    for i in (0, 1, 2):                                                      # max_len 64, 2, 33
        one, _ = alone.encode(ids[i:i + 1], max_len[i:i + 1])
        assert np.array_equal(one[0], whole[i]), i


def test_long_entry_checks_its_domain_before_any_launch():
    """no device needed: with pointers that are never dereferenced (only ``max_len_host`` is read) every call outside the
    domain returns XMC_EINVAL"""
    import ctypes as C
    lib = _lib.load()
    p, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)

    def attention(t, h, max_len, ctx=p):
        ml = np.array(max_len, np.int32)
        return lib.xmc_bert_attention_long(p, p, p, C.c_void_p(ml.ctypes.data), ctx, len(max_len), t, h, None)

    einval = lib.xmc_bert_attention_long(None, p, p, p, p, 1, 64, 128, None)
    assert einval < 0 and einval > -1000                                     # XMC_EINVAL, not a HIP error
    assert attention(65, 128, [5, 65]) == einval and attention(64, 128, [9, 1]) == einval
    assert attention(64, 128, [65, 9]) == einval and attention(64, 96, [9, 9]) == einval and attention(1, 128, [1]) == einval
    assert attention(64, 128, [9, 9], ctx=odd) == einval
