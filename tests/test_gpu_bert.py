"""BERT caption encoder on the MI355X (csrc/bert.hip, utils/bert_utils.py): each kernel against float64 (tests/bert_ref.py, itself
tied to transformers.BertModel by tests/test_bert_text.py), the attention's domain, the whole encoder in float32 and in the bf16
"fast" mode, batch independence, and text -> images end to end.

Shapes: T = 17, N in {3, 5} (51 and 85 rows: neither a multiple of the four rows per workgroup of the row kernels nor of a GEMM
tile), max_len including 2, 9 and 17, H in {128, 768} (half a wave of 16-byte lanes, and three vectors per lane).

Per-kernel bounds, from operation counts (u = 2^-24, the float32 unit roundoff):

* LayerNorm kernels (embed + LN, bias + residual + LN): the input sum is two float32 adds (2u |v|); the mean is a 64-lane tree over
  H / 64 serial adds per lane (<= (H / 64 + 6) u mean|v|); the variance the same over fmaf squares of the held differences;
  1 / sqrt and the division are correctly rounded; the output is one multiply and one fmaf.  Relative to |xhat| that is
  <= ~(2 + 18 + 18 / 2 + 3) u ~ 2e-6 for H = 768 on ordinary rows (|v - mean| comparable to |v|), plus u |beta|.  Bound (the issue's):
  1e-5 (|gamma| |xhat| + 1).
* near-constant row v = 3 + 1e-4 noise: the float32 INPUT is the reference's input too, so the only amplified term is the mean's
  error, <= ~4 u * 3 = 7e-7 against a deviation of 1e-4: 7e-3 of xhat at worst, a two-pass float32 variance measured 6e-4 on the
  CPU; the one-pass E[v^2] - mean^2 gives variance 0 and |xhat| ~ 1e2.  Bound: 1e-2.
* GELU: evaluated in float64 and rounded once (<= 0.5 ulp of the result + the float64 erfc's error, negligible).  x + bias is
  chosen exactly representable so the comparison is of the function, not of the rounding of its argument (whose effect on the
  far negative tail, condition number v^2, no implementation can avoid).  Bound: 4 ulp of float32 at the result, |v| <= 10.
* attention: a score is a 64-term fmaf chain (error ~ sqrt(64) u |q||k| / 8 typically, 64 u sum|q k| / 8 at worst: 5e-7 .. 4e-6 for
  N(0, 1) operands), exp and the division are ~1 ulp each, so a probability carries a relative error of ~1e-6, and the context is
  a chain of <= 17 fmaf (17 u sum|p v|).  Bound (the issue's): 1e-5 sum_j |p_j v_j| + 1e-6.

Whole encoder: the tolerances are yardsticks computed from the reference alone.  float32: e32 = max|ref_float32 - ref_float64|
(the restatement in torch float32 on the CPU); required max|hip - ref_float64| <= 16 e32 -- the margin because the f32 MFMA sums up
to 3,072 products as ONE serial fmaf chain (~3.5e-7 sum|ab| at K = 4096) where the CPU GEMM sums in blocks.  fast: e_bf =
max|ref_operands_rounded_to_bf16 - ref_float64|; required max|hip_fast - ref_float64| <= 2 e_bf (the kernel makes the same roundings;
float32 accumulation and flipped roundings are second order).  ``run_encoder`` prints both ratios (pytest -s).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import bert_ref as R
from xmcgan_image_generation_amd import _lib
from xmcgan_image_generation_amd.utils import bert_arch, bert_utils

pytestmark = pytest.mark.gpu

T = 17
F64 = torch.float64
SMALL = dict(layers=2, hidden=128, ffn=512, vocab=64, max_pos=40)
MAX_LENS = [2, 9, 17, 5, 12]
VOCAB_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_vocab_small.txt")


@functools.lru_cache(maxsize=None)
def _ops(fast):
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.bfloat16 if fast else torch.float32)


def get_ops(fast=False):
    """the float32 operator table, or the bf16 one the "fast" GEMMs need (one of each per session)"""
    return _ops(bool(fast))


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _ln_check(got, want, xhat, gamma):
    err = (got.double() - want).abs()
    bound = 1e-5 * (gamma.abs() * xhat.abs() + 1.0)
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))
    return float((err / bound).max())


# --------------------------------------------------------------------------------------------------------- kernel bodies
def run_embed_ln(n, h):
    ops = get_ops()
    dev = ops.device
    params = bert_arch.init_bert(11, layers=1, hidden=h, ffn=4 * h, vocab=64, max_pos=40)
    gen = torch.Generator().manual_seed(n * 1000 + h)
    ids = torch.randint(0, 64, (n, T), generator=gen, dtype=torch.int32)
    ids[0, :2] = torch.tensor([0, 63], dtype=torch.int32)                    # both ends of the table
    want, xhat, gamma = R.embed(params, ids.numpy())
    tabs = [torch.as_tensor(params[k]).to(dev) for k in bert_arch.EMBEDDING_KEYS]
    out = _nan((n * T, h), dev)
    ops.bert_embed_ln(ids.reshape(-1).contiguous().to(dev), *tabs, out, T)
    return _ln_check(out.cpu(), want, xhat, gamma)


def run_bias_residual_ln(n, h):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n * 1000 + h + 1)
    rows = n * T
    x, res = torch.randn(rows, h, generator=gen) * 2.0, torch.randn(rows, h, generator=gen)
    bias, beta = torch.randn(h, generator=gen) * 0.5, torch.randn(h, generator=gen) * 0.1
    gamma = 1.0 + 0.1 * torch.randn(h, generator=gen)
    want, xhat = R.layer_norm(x.double() + bias.double() + res.double(), gamma.double(), beta.double())
    out = _nan((rows, h), dev)
    ops.bias_residual_ln(x.to(dev), bias.to(dev), res.to(dev), gamma.to(dev), beta.to(dev), out=out)
    return _ln_check(out.cpu(), want, xhat, gamma.double())


def run_near_constant_row(h):
    """v = 3 + 1e-4 noise with eps = 1e-12: the one-pass variance is 0 here"""
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(h)
    rows = 5
    x = 3.0 + 1e-4 * torch.randn(rows, h, generator=gen)
    zero, one = torch.zeros(h), torch.ones(h)
    _, xhat = R.layer_norm(x.double(), one.double(), zero.double())
    out = _nan((rows, h), dev)
    ops.bias_residual_ln(x.to(dev), zero.to(dev), torch.zeros(rows, h).to(dev), one.to(dev), zero.to(dev), out=out)
    err = float((out.cpu().double() - xhat).abs().max())
    assert float(xhat.abs().max()) > 2.0                                     # the rows are spread over +-3 sigma, not collapsed
    assert err <= 1e-2, err
    return err


def run_bias_gelu(rows, f):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(rows + f)
    # multiples of 2^-10: x + bias is exact in float32, |x + bias| <= 10
    x = torch.randint(-9728, 9729, (rows, f), generator=gen).float() / 1024.0
    bias = torch.randint(-256, 257, (f,), generator=gen).float() / 1024.0
    x[0, :8] = torch.tensor([9.75, -9.75, 0.0, -0.0, 1.0 / 1024, -1.0 / 1024, -5.0, 5.0]) - bias[:8]
    x[0, 8:10] = torch.tensor([10.0, -10.0]) - bias[8:10]
    v = x.double() + bias.double()
    assert bool((v.float().double() == v).all()) and float(v.abs().max()) == 10.0
    want = R.gelu(v)
    out = _nan((rows, f), dev)
    xd = x.to(dev)
    ops.bias_gelu(xd, bias.to(dev), out=out)
    got = out.cpu()
    ulp = torch.as_tensor(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
    err = (got.double() - want).abs()
    assert bool((err <= 4.0 * ulp).all()), float((err / ulp).max())
    ops.bias_gelu(xd, bias.to(dev), out=xd)                                  # in place, as the encoder calls it
    assert torch.equal(xd.cpu(), got)
    return float((err / ulp).max())


def run_attention(n, h):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n * 1000 + h + 2)
    rows = n * T
    qkv, bias = torch.randn(rows, 3 * h, generator=gen), 0.1 * torch.randn(3 * h, generator=gen)
    ml = np.array(MAX_LENS[:n], np.int32)
    want, mag = R.attention(qkv.double(), bias.double(), ml, T)
    ctx = _nan((rows, h), dev)                                               # an unwritten element stays NaN
    ops.bert_attention(qkv.to(dev), bias.to(dev), torch.as_tensor(ml).to(dev), ml, ctx, T)
    err = (ctx.cpu().double() - want).abs()
    bound = 1e-5 * mag + 1e-6
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))      # (NaN fails the comparison)
    return float((err / bound).max())


def run_sentence(n, h):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n + h)
    emb = torch.randn(n * T, h, generator=gen)
    ml = np.array(MAX_LENS[:n], np.int32)
    want = R.sentence(emb.double().view(n, T, h), ml)
    out = _nan((n, h), dev)
    ops.bert_sentence(emb.to(dev), torch.as_tensor(ml).to(dev), T, out=out)
    # 17 serial float32 adds and one division: <= 18 u sum|emb| / max_len
    bound = 18 * 2.0 ** -24 * R.sentence(emb.double().abs().view(n, T, h), ml) + 1e-30
    err = (out.cpu().double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def _batch(vocab, n, seed=0):
    rng = np.random.default_rng(seed)
    max_len = np.array(MAX_LENS[:n], np.int64)
    ids = np.zeros((n, T), np.int64)
    for i, m in enumerate(max_len):
        ids[i, :m] = rng.integers(1, vocab, size=m)
    return ids, max_len


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """(params, ids, max_len, ref64, e32, e_bf): computed once per configuration, shared by the tests, never modified"""
    params = bert_arch.init_bert(5, **SMALL) if name == "small" else bert_arch.init_bert(5)
    ids, max_len = _batch(bert_utils.infer_dims(params).vocab, n)
    ref = R.forward(params, ids, max_len)
    e32 = float((R.forward(params, ids, max_len, torch.float32).double() - ref).abs().max())
    e_bf = float((R.forward(params, ids, max_len, round_bf16=True) - ref).abs().max()) if name == "small" else None
    return params, ids, max_len, ref, e32, e_bf


def run_encoder(name, n, fast=False):
    params, ids, max_len, ref, e32, e_bf = reference(name, n)
    enc = bert_utils.BertEncoder(get_ops(fast), params, fast=fast)
    emb, sent = enc.encode(ids, max_len)
    assert emb.shape == ref.shape and emb.dtype == np.float32 and enc.launches == 2 + 8 * enc.dims.layers
    err = float((torch.as_tensor(emb).double() - ref).abs().max())
    yard, factor = (e_bf, 2.0) if fast else (e32, 16.0)
    print(f"bert {name} n={n} {'fast' if fast else 'float32'}: err {err:.3e}, yardstick {yard:.3e}, ratio {err / yard:.3f} "
          f"(limit {factor:g}), max|ref| {float(ref.abs().max()):.2f}")
    assert err <= factor * yard, (err, yard)
    # the device sentence embedding: the sum of the device rows in order, divided by max_len
    want = emb.astype(np.float64).sum(axis=1) / max_len[:, None]
    assert np.abs(sent - want).max() <= 18 * 2.0 ** -24 * (np.abs(emb).astype(np.float64).sum(axis=1) / max_len[:, None]).max()
    return err / yard


# ----------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("h", [128, 768])
@pytest.mark.parametrize("n", [3, 5])
def test_embed_ln(n, h):
    run_embed_ln(n, h)


@pytest.mark.parametrize("h", [128, 768])
@pytest.mark.parametrize("n", [3, 5])
def test_bias_residual_ln(n, h):
    run_bias_residual_ln(n, h)


@pytest.mark.parametrize("h", [128, 768])
def test_layer_norm_of_a_near_constant_row(h):
    run_near_constant_row(h)


@pytest.mark.parametrize("rows,f", [(51, 512), (85, 3072)])
def test_bias_gelu(rows, f):
    run_bias_gelu(rows, f)


@pytest.mark.parametrize("h", [128, 768])
@pytest.mark.parametrize("n", [3, 5])
def test_attention(n, h):
    run_attention(n, h)


@pytest.mark.parametrize("n,h", [(3, 128), (5, 768)])
def test_sentence(n, h):
    run_sentence(n, h)


def test_attention_outside_its_domain():
    ops = get_ops()
    dev = ops.device

    def attempt(t, h, ml):
        n = len(ml)
        qkv, bias = torch.zeros(n * t, 3 * h).to(dev), torch.zeros(3 * h).to(dev)
        ctx = torch.full((n * t, h), 7.0).to(dev)
        ml = np.array(ml, np.int32)
        with pytest.raises(_lib.XmcError):
            ops.bert_attention(qkv, bias, torch.as_tensor(ml).to(dev), ml, ctx, t)
        torch.cuda.synchronize()
        assert bool((ctx == 7.0).all())                                      # nothing ran

    attempt(33, 128, [5, 33])            # T beyond 32
    attempt(17, 128, [9, 1])             # max_len below 2
    attempt(17, 128, [18, 9])            # max_len beyond T
    attempt(17, 96, [9, 9])              # H no multiple of 64


@pytest.mark.parametrize("fast", [False, True], ids=["float32", "fast"])
def test_encoder_small(fast):
    run_encoder("small", 5, fast)


def test_encoder_base_size():
    run_encoder("base", 3)


def test_fast_needs_the_bf16_operator_table():
    params = reference("small", 5)[0]
    with pytest.raises(ValueError, match="fast"):
        bert_utils.BertEncoder(get_ops(False), params, fast=True)


@pytest.mark.parametrize("fast", [False, True], ids=["float32", "fast"])
def test_a_caption_does_not_depend_on_its_batch(fast):
    params, ids, max_len, *_ = reference("small", 5)
    ops = get_ops(fast)
    whole, _ = bert_utils.BertEncoder(ops, params, fast=fast).encode(ids, max_len)
    split, _ = bert_utils.BertEncoder(ops, params, fast=fast, chunk=2).encode(ids, max_len)      # chunks 2 + 2 + 1
    assert np.array_equal(whole, split)
    alone = bert_utils.BertEncoder(ops, params, fast=fast)
    for i in (0, 2, 3):                                                      # max_len 2, 17, 5
        one, _ = alone.encode(ids[i:i + 1], max_len[i:i + 1])
        assert np.array_equal(one[0], whole[i]), i


def test_out_of_range_token_id_launches_nothing(monkeypatch):
    params, ids, max_len, *_ = reference("small", 5)
    ops = get_ops()
    enc = bert_utils.BertEncoder(ops, params, chunk=2)
    calls = []
    for name in ("gemm", "bert_embed_ln", "bert_attention", "bias_residual_ln", "bias_gelu", "bert_sentence"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    bad = ids.copy()
    bad[4, 1] = 64                                                           # in the LAST chunk: the whole list is checked first
    with pytest.raises(ValueError, match="token id 64"):
        enc.encode(bad, max_len)
    bad[4, 1] = -1
    with pytest.raises(ValueError, match="token id -1"):
        enc.encode(bad, max_len)
    assert calls == [] and enc.launches == 0


def test_text_to_embeddings_end_to_end():
    from xmcgan_image_generation_amd.libml import wordpiece
    params = bert_arch.init_bert(8, layers=2, hidden=128, ffn=512, vocab=80, max_pos=40)
    te = bert_utils.TextEncoder(VOCAB_FILE, None, encoder=bert_utils.BertEncoder(get_ops(), params))
    caps = ["A man riding a horse on the beach.", "", "two dogs sitting on a red table with pizza and a cat on the street riding"]
    emb, sent, max_len = te.get_bert_for_captions(caps)
    ids, ml = wordpiece.FullTokenizer(VOCAB_FILE).encode(caps)
    assert np.array_equal(ml, max_len) and max_len.tolist() == [11, 2, 17] and max_len.dtype == np.int64
    ref = R.forward(params, ids, ml)
    e32 = float((R.forward(params, ids, ml, torch.float32).double() - ref).abs().max())
    assert emb.shape == (3, 17, 128) and emb.dtype == sent.dtype == np.float32
    assert float((torch.as_tensor(emb).double() - ref).abs().max()) <= 16 * e32
    # sentence embedding: 17 rows each within 16 e32, summed in float32 (18 u sum|emb|), divided by max_len
    want = R.sentence(ref, ml).numpy()
    tol = (17 * 16 * e32 + 18 * 2.0 ** -24 * ref.abs().sum(dim=1).numpy()) / ml[:, None]
    assert bool((np.abs(sent - want) <= tol).all())


def test_text_to_images_end_to_end():
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds_ = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, _, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, gp, gs, dp, ds_)
    params = bert_arch.init_bert(9, layers=1, hidden=768, ffn=3072, vocab=80, max_pos=32)
    te = bert_utils.TextEncoder(VOCAB_FILE, None, encoder=bert_utils.BertEncoder(get_ops(), params))
    caps = ["a man riding a horse", "two dogs on the beach!", "a red bus", "Café table with pizza"]
    image, ema_image = train_utils.generate_from_captions(7, state, caps, gen, cfg, te)
    emb, sent, max_len = te.get_bert_for_captions(caps)
    batch = {"embedding": torch.as_tensor(emb), "sentence_embedding": torch.as_tensor(sent),
             "max_len": torch.as_tensor(max_len.astype(np.float32))[:, None]}
    image2, ema2 = train_utils.eval_step(7, state, batch, gen, cfg)
    assert tuple(image.shape) == tuple(ema_image.shape) == (4, 128, 128, 3)
    assert bool(torch.isfinite(image.float()).all()) and bool(torch.isfinite(ema_image.float()).all())
    assert torch.equal(image, image2) and torch.equal(ema_image, ema2)
