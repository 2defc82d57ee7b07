"""CLIP dual encoder and the alignment scores on the MI355X (csrc/clip.hip, utils/clip_utils.py, utils/alignment_metrics.py): each
kernel against float64 (tests/clip_ref.py, itself tied to transformers.CLIPModel by tests/test_clip_text.py; the preprocessing and
the scores against utils/alignment_metrics.py, tied to Pillow by tests/test_alignment_metrics.py), the attention's domain, the whole
encoders in float32 and in the bf16 "fast" mode, and EvalMetric end to end.

Per-kernel bounds, from operation counts (u = 2^-24, the float32 unit roundoff):

* LayerNorm kernels (vision embed, bias + residual + LN, gather + LN): as tests/test_gpu_bert.py derives for the same row
  arithmetic: 1e-5 (|gamma| |xhat| + 1); the written sum s = x + bias + res is two float32 adds: <= 2 u (|x| + |bias| + |res|).
  Near-constant row v = 3 + 1e-4 noise at eps = 1e-12: 1e-2 (the same derivation; the one-pass variance gives 0 there).
* text embed: ONE float32 add: bit-equal to NumPy's float32 sum.
* QuickGELU: evaluated in float64 and rounded once; x + bias is chosen exactly representable, |v| <= 40.  Bound: 4 ulp of float32
  at the result (0.5 ulp of the rounding + float64 exp, negligible).
* attention: the bound of tests/test_gpu_bert.py's attention test, 1e-5 sum_j |p_j v_j| + 1e-6 (a score is a 64-term fmaf chain, a
  context row a chain of <= t <= 128 fmaf: 128 u = 7.6e-6 of sum |p v| at worst).
* preprocess: weights are float64 values rounded to float32 (u each), the two passes are fmaf chains of ky and kx taps, then one
  subtraction and one product: |err| <= (kx + ky + 8) u (|wy|_1 |wx|_1 + |mean_c|) / std_c for inputs in [0, 1].
* cosines: float64 sums of d exact products in another order than NumPy's: <= (d + 8) 2^-53 relative to |a| |b|: 1e-13.
  Hits: exact equality, on inputs whose smallest margin exceeds 1e-6 (asserted on the CPU side).

Whole encoders: yardsticks computed from the reference alone.  float32: e32 = max|ref_float32 - ref_float64|; required
max|hip - ref_float64| <= 16 e32.  fast: e_bf = max|ref_operands_rounded_to_bf16 - ref_float64|; required <= 2 e_bf.  Every run
prints err, yardstick and ratio (pytest -s).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import clip_ref as R
from xmcgan_image_generation_amd import _lib
from xmcgan_image_generation_amd.utils import alignment_metrics as A, clip_arch, clip_utils

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = clip_arch.LN_EPS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB, MERGES = os.path.join(GOLDEN, "clip_bpe_vocab.json"), os.path.join(GOLDEN, "clip_bpe_merges.txt")


@functools.lru_cache(maxsize=None)
def _ops(fast):
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.bfloat16 if fast else torch.float32)


def get_ops(fast=False):
    return _ops(bool(fast))


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _ln_check(got, want, xhat, gamma):
    err = (got.double() - want).abs()
    bound = 1e-5 * (gamma.abs() * xhat.abs() + 1.0)
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))
    return float((err / bound).max())


def _lens(t, n):
    """ragged lengths that include 1 and t"""
    return np.array([t, 1, max(1, (2 * t) // 3), max(1, t // 2), min(t, 2)][:n], np.int32)


# --------------------------------------------------------------------------------------------------------- kernel bodies
def run_attention(t, causal, h=128, n=3):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(t * 10 + causal)
    rows = n * t
    qkv, bias = torch.randn(rows, 3 * h, generator=gen), 0.1 * torch.randn(3 * h, generator=gen)
    lens = _lens(t, n)
    want, mag = R.attention(qkv.double(), bias.double(), lens, t, causal=bool(causal))
    ctx = _nan((rows, h), dev)                                               # an unwritten element stays NaN
    dq, db, dl = qkv.to(dev), bias.to(dev), torch.as_tensor(lens).to(dev)
    ops.mha_attention(dq, db, dl, lens, ctx, t, causal=causal)
    err = (ctx.cpu().double() - want).abs()
    bound = 1e-5 * mag + 1e-6
    ratio = float((err / bound).max())
    print(f"mha_attention t={t} causal={causal} h={h}: max err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (float(err.max()), ratio)              # (NaN fails the comparison)
    again = _nan((rows, h), dev)
    ops.mha_attention(dq, db, dl, lens, again, t, causal=causal)
    assert torch.equal(again, ctx)                                           # two launches, the same bits
    return ratio


def run_bias_add_ln(rows, h, with_bias=True, with_res=True, alias=False):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(rows * 1000 + h + 2 * with_bias + with_res)
    x, res = torch.randn(rows, h, generator=gen) * 2.0, torch.randn(rows, h, generator=gen)
    bias, beta = torch.randn(h, generator=gen) * 0.5, torch.randn(h, generator=gen) * 0.1
    gamma = 1.0 + 0.1 * torch.randn(h, generator=gen)
    total = x.double() + (bias.double() if with_bias else 0.0) + (res.double() if with_res else 0.0)
    want, xhat = R.layer_norm(total, gamma.double(), beta.double())
    out = _nan((rows, h), dev)
    dres = res.to(dev) if with_res else None
    s = dres if alias else _nan((rows, h), dev)
    ops.bias_add_ln(x.to(dev), bias.to(dev) if with_bias else None, dres, gamma.to(dev), beta.to(dev), s=s, out=out, eps=EPS)
    mag = x.abs().double() + (bias.abs().double() if with_bias else 0.0) + (res.abs().double() if with_res else 0.0)
    assert bool(((s.cpu().double() - total).abs() <= 2 * U32 * mag).all())
    return _ln_check(out.cpu(), want, xhat, gamma.double())


def run_near_constant_row(h):
    """v = 3 + 1e-4 noise with eps = 1e-12: the one-pass variance is 0 here"""
    ops = get_ops()
    dev = ops.device
    x = 3.0 + 1e-4 * torch.randn(5, h, generator=torch.Generator().manual_seed(h))
    zero, one = torch.zeros(h), torch.ones(h)
    _, xhat = R.layer_norm(x.double(), one.double(), zero.double(), eps=1e-12)
    out = _nan((5, h), dev)
    ops.bias_add_ln(x.to(dev), None, None, one.to(dev), zero.to(dev), out=out, eps=1e-12)
    err = float((out.cpu().double() - xhat).abs().max())
    assert float(xhat.abs().max()) > 2.0 and err <= 1e-2, err
    return err


def run_bias_quick_gelu(rows, f):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(rows + f)
    # multiples of 2^-10: x + bias is exact in float32, |x + bias| <= 40
    x = torch.randint(-40448, 40449, (rows, f), generator=gen).float() / 1024.0
    bias = torch.randint(-512, 513, (f,), generator=gen).float() / 1024.0
    x[0, :8] = torch.tensor([39.5, -39.5, 0.0, -0.0, 1.0 / 1024, -1.0 / 1024, -5.0, 5.0]) - bias[:8]
    x[0, 8:10] = torch.tensor([40.0, -40.0]) - bias[8:10]
    v = (x.double() + bias.double()).numpy()
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and np.abs(v).max() == 40.0
    want = v / (1.0 + np.exp(-1.702 * v))
    out = _nan((rows, f), dev)
    xd = x.to(dev)
    ops.bias_quick_gelu(xd, bias.to(dev), out=out)
    got = out.cpu()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.double().numpy() - want)
    assert bool((err <= 4.0 * ulp).all()), float((err / ulp).max())
    ops.bias_quick_gelu(xd, bias.to(dev), out=xd)                            # in place, as the encoder calls it
    assert torch.equal(xd.cpu(), got)
    return float((err / ulp).max())


def run_vision_embed(n, h, t):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n * 100 + h + t)
    patch, cls, pos = torch.randn(n * (t - 1), h, generator=gen), torch.randn(h, generator=gen), torch.randn(t, h, generator=gen)
    gamma, beta = 1.0 + 0.1 * torch.randn(h, generator=gen), 0.1 * torch.randn(h, generator=gen)
    x = torch.cat([cls.double().expand(n, 1, h), patch.double().view(n, t - 1, h)], 1) + pos.double()
    want, xhat = R.layer_norm(x.reshape(n * t, h), gamma.double(), beta.double())
    out = _nan((n * t, h), dev)
    ops.clip_vision_embed(patch.to(dev), cls.to(dev), pos.to(dev), gamma.to(dev), beta.to(dev), out, t, eps=EPS)
    return _ln_check(out.cpu(), want, xhat, gamma.double())


def run_text_embed(n, h, t, vocab=64):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n * 100 + h + t + 1)
    tok, pos = torch.randn(vocab, h, generator=gen), torch.randn(t + 3, h, generator=gen)
    ids = torch.randint(0, vocab, (n, t), generator=gen, dtype=torch.int32)
    ids[0, :2] = torch.tensor([0, vocab - 1], dtype=torch.int32)              # both ends of the table
    want = tok.numpy()[ids.numpy().reshape(-1)] + np.tile(pos.numpy()[:t], (n, 1))        # float32: one rounding, as the kernel
    out = _nan((n * t, h), dev)
    ops.clip_text_embed(ids.reshape(-1).contiguous().to(dev), tok.to(dev), pos.to(dev), out, t)
    assert np.array_equal(out.cpu().numpy(), want)


def run_gather_rows_ln(n, h, t):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n + h + t)
    x = torch.randn(n * t, h, generator=gen)
    gamma, beta = 1.0 + 0.1 * torch.randn(h, generator=gen), 0.1 * torch.randn(h, generator=gen)
    idx = np.array([0, t - 1, t // 2, 1 % t, t - 1][:n], np.int32)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    worst = 0.0
    for index in (idx, None):
        rows = x.view(n, t, h)[torch.arange(n), torch.as_tensor(idx if index is not None else np.zeros(n), dtype=torch.long)]
        want, xhat = R.layer_norm(rows.double(), gamma.double(), beta.double())
        out = _nan((n, h), dev)
        ops.gather_rows_ln(xd, torch.as_tensor(index).to(dev) if index is not None else None, index, gd, bd, t, out=out, eps=EPS)
        worst = max(worst, _ln_check(out.cpu(), want, xhat, gamma.double()))
    return worst


def run_preprocess(hw, size, patch, dtype=torch.float32, n=2):
    ops = get_ops()
    dev = ops.device
    img = torch.rand(n, hw, hw, 3, generator=torch.Generator().manual_seed(hw + size)).to(dtype)
    exact = img.double().numpy()                                             # (the bf16 values themselves are the input)
    want = A.preprocess(exact, size, patch)
    resized = (A.resize(exact, size) - np.asarray(clip_arch.IMAGE_MEAN)) / np.asarray(clip_arch.IMAGE_STD)
    g = size // patch                                                        # the patch order, spelled out once more
    assert np.array_equal(want, resized.reshape(n, g, patch, g, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n * g * g, -1))
    _, cnt, w = A.cubic_coeffs(hw, size)
    l1 = float(np.abs(w).sum(1).max())
    bound = np.array([(2 * int(cnt.max()) + 8) * U32 * (l1 * l1 + m) / s for m, s in zip(clip_arch.IMAGE_MEAN, clip_arch.IMAGE_STD)])
    out = _nan((n * g * g, 3 * patch * patch), dev)
    ops.clip_preprocess(img.to(dev), size, patch, clip_arch.IMAGE_MEAN, clip_arch.IMAGE_STD, out=out)
    err = np.abs(out.cpu().double().numpy() - want).reshape(n * g * g, 3, patch * patch).max(axis=(0, 2))
    print(f"clip_preprocess {hw} -> {size} {dtype}: max err per channel {err}, bound {bound}")
    assert bool((err <= bound).all()), (err, bound)                          # (NaN fails the comparison)
    return float((err / bound).max())


def _embeddings(n, m, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)


def run_pair_cosine(n, d):
    ops = get_ops()
    a, b = _embeddings(n, n, d, n + d)
    a[0], b[1] = 0.0, 0.0                                                    # zero rows: cosine 0
    got = ops.pair_cosine(a, b)
    want = A.cosine_spec(a, b)
    assert got.dtype == np.float64 and got[0] == 0.0 and got[1] == 0.0
    assert float(np.abs(got - want).max()) <= 1e-13
    assert np.array_equal(got, ops.pair_cosine(a, b))                        # two launches, the same bits
    assert abs(A.clip_score(a, b, ops) - A.clip_score(a, b)) <= 2.5e-13


def run_rprecision(n, c, d):
    ops = get_ops()
    m = n + 1
    img, txt = _embeddings(n, m, d, 7 * n + d)
    truth = np.arange(n, dtype=np.int32)
    cand = A.draw_candidates([n, c, d], n, c)
    txt[:n] += 0.3 * img                                                     # own captions tend to win: both outcomes occur
    txt[0] = 2.0 * img[0]                                                    # row 0: its caption wins against every other (cosine 1) ...
    txt[m - 1] = txt[truth[0]]                                               # ... but one candidate duplicates it: a tie, a miss
    cand[0, 0] = m - 1
    margins = A.rprecision_margins(img, txt, truth, cand)
    assert margins[0] == 0.0 and float(np.abs(margins[1:]).min()) > 1e-6      # no tie decides any other row
    want = A.rprecision_hits(img, txt, truth, cand)
    got = A.rprecision_hits(img, txt, truth, cand, ops)
    assert got.dtype == bool and not got[0] and np.array_equal(got, want)
    assert 0 < want.sum() < n
    assert np.array_equal(got, ops.rprecision_hits(img, txt, truth, cand))


@functools.lru_cache(maxsize=None)
def reference(name, n=5):
    """(params, images, ids, eot, refs): computed once per configuration, shared by the tests, never modified.  refs[tower] =
    (ref64, e32, e_bf)"""
    if name == "small5":                         # 64 px at patch 32: 5 image tokens; the images are shrunk from 128 px
        params, hw = R.small_params(), 128
    elif name == "small50":                      # 224 px at patch 32: ViT-B/32's 50 tokens at width 128; enlarged from 128 px
        params, hw = R.small_params(image_size=224), 128
    else:                                        # ViT-B/32 itself (a short token table: its length is no kernel's concern)
        params, hw = clip_arch.init_clip(5, vocab=1000), 128
    dims = clip_utils.infer_dims(params)
    rng = np.random.default_rng(11)
    images = rng.random((n, hw, hw, 3)).astype(np.float32)
    ids = rng.integers(0, dims.vocab - 2, (n, dims.context))
    eot = np.array([5, dims.context - 1, 1, 40, 17][:n])
    for i, e in enumerate(eot):
        ids[i, e:] = dims.vocab - 1
    refs = {}
    for tower, f, args in (("image", R.encode_image, (images,)), ("text", R.encode_text, (ids, eot))):
        ref = f(params, *args)
        e32 = float((f(params, *args, dtype=torch.float32).double() - ref).abs().max())
        e_bf = float((f(params, *args, round_bf16=True) - ref).abs().max()) if name != "b32" else None
        refs[tower] = (ref, e32, e_bf)
    return params, images, ids, eot, refs


def run_encoder(name, tower, n=5, fast=False, chunk=2):
    params, images, ids, eot, refs = reference(name, n)
    ref, e32, e_bf = refs[tower]
    enc = clip_utils.ClipEncoder(get_ops(fast), params, fast=fast, chunk=chunk)
    d = enc.dims
    if tower == "image":
        emb = enc.encode_image(images)
        per_chunk = 6 + 8 * d.vision_layers
    else:
        emb = enc.encode_text(ids, eot)
        per_chunk = 4 + 8 * d.text_layers
    assert emb.shape == tuple(ref.shape) == (n, d.proj) and emb.dtype == np.float32 and bool(np.isfinite(emb).all())
    assert enc.launches == per_chunk * -(-n // chunk)
    err = float((torch.as_tensor(emb).double() - ref).abs().max())
    yard, factor = (e_bf, 2.0) if fast else (e32, 16.0)
    print(f"clip {name} {tower} n={n} {'fast' if fast else 'float32'}: err {err:.3e}, yardstick {yard:.3e}, ratio {err / yard:.3f} "
          f"(limit {factor:g}), max|ref| {float(ref.abs().max()):.2f}")
    assert err <= factor * yard, (err, yard)
    return emb


# ----------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("t", [1, 2, 5, 50, 64, 65, 77, 128])
def test_mha_attention(t, causal):
    run_attention(t, causal)


def test_mha_attention_twelve_heads():
    run_attention(50, 0, h=768)


def test_mha_attention_outside_its_domain():
    ops = get_ops()
    dev = ops.device

    def attempt(t, h, lens):
        n = len(lens)
        qkv, bias = torch.zeros(n * t, 3 * h).to(dev), torch.zeros(3 * h).to(dev)
        ctx = torch.full((n * t, h), 7.0).to(dev)
        lens = np.array(lens, np.int32)
        with pytest.raises(_lib.XmcError):
            ops.mha_attention(qkv, bias, torch.as_tensor(lens).to(dev), lens, ctx, t)
        torch.cuda.synchronize()
        assert bool((ctx == 7.0).all())                                      # nothing ran

    attempt(129, 128, [5, 129])          # t beyond 128
    attempt(17, 96, [9, 9])              # h no multiple of 64
    attempt(17, 128, [9, 0])             # len = 0 in the host copy
    attempt(17, 128, [18, 9])            # len beyond t


@pytest.mark.parametrize("with_bias,with_res,alias", [(True, True, False), (True, True, True), (False, False, False),
                                                      (True, False, False), (False, True, True)])
@pytest.mark.parametrize("rows,h", [(7, 4), (51, 128), (9, 1024)])
def test_bias_add_ln(rows, h, with_bias, with_res, alias):
    run_bias_add_ln(rows, h, with_bias, with_res, alias)


@pytest.mark.parametrize("h", [128, 768])
def test_layer_norm_of_a_near_constant_row(h):
    run_near_constant_row(h)


def test_bias_add_ln_rejects_an_output_that_is_the_sum():
    ops = get_ops()
    x = torch.zeros(4, 64).to(ops.device)
    g = torch.ones(64).to(ops.device)
    with pytest.raises(_lib.XmcError):
        ops.bias_add_ln(x, None, None, g, g, s=x, out=x)
    wide = torch.ones(1028).to(ops.device)
    with pytest.raises(_lib.XmcError):
        ops.bias_add_ln(torch.zeros(4, 1028).to(ops.device), None, None, wide, wide)    # h beyond 1024


@pytest.mark.parametrize("rows,f", [(51, 256), (85, 3072)])
def test_bias_quick_gelu(rows, f):
    run_bias_quick_gelu(rows, f)


@pytest.mark.parametrize("n,h,t", [(3, 128, 5), (2, 768, 50)])
def test_vision_embed(n, h, t):
    run_vision_embed(n, h, t)


@pytest.mark.parametrize("n,h,t", [(3, 128, 77), (2, 512, 9)])
def test_text_embed(n, h, t):
    run_text_embed(n, h, t)


@pytest.mark.parametrize("n,h,t", [(5, 128, 77), (3, 768, 50), (2, 64, 1)])
def test_gather_rows_ln(n, h, t):
    run_gather_rows_ln(n, h, t)


def test_gather_rows_ln_rejects_an_index_outside_the_sequence():
    ops = get_ops()
    dev = ops.device
    x, g = torch.zeros(2 * 5, 64).to(dev), torch.ones(64).to(dev)
    out = torch.full((2, 64), 7.0).to(dev)
    for bad in ([0, 5], [-1, 0]):
        idx = np.array(bad, np.int32)
        with pytest.raises(_lib.XmcError):
            ops.gather_rows_ln(x, torch.as_tensor(idx).to(dev), idx, g, g, 5, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("hw,size,patch,dtype", [(32, 64, 32, torch.float32), (128, 224, 32, torch.float32),
                                                 (256, 224, 32, torch.float32), (128, 224, 32, torch.bfloat16),
                                                 (96, 64, 16, torch.float32)])
def test_clip_preprocess(hw, size, patch, dtype):
    run_preprocess(hw, size, patch, dtype)


def test_clip_preprocess_outside_its_domain():
    ops = get_ops()
    dev = ops.device
    outs = []
    for hw, size, patch, std in ((16, 64, 32, None), (544, 64, 32, None), (64, 64, 24, None), (64, 480, 32, None),
                                 (64, 64, 32, (0.2, 0.0, 0.2))):
        g = size // patch
        outs.append(torch.full((g * g, 3 * patch * patch), 7.0).to(dev))
        with pytest.raises(_lib.XmcError):
            ops.clip_preprocess(torch.zeros(1, hw, hw, 3).to(dev), size, patch, clip_arch.IMAGE_MEAN, std or clip_arch.IMAGE_STD,
                                out=outs[-1])
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)                         # nothing ran


@pytest.mark.parametrize("n,d", [(7, 64), (257, 512)])
def test_pair_cosine(n, d):
    run_pair_cosine(n, d)


@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("n,c", [(7, 3), (257, 99)])
def test_rprecision_hits(n, c, d):
    run_rprecision(n, c, d)


def test_rprecision_hits_rejects_an_index_outside_the_captions():
    ops = get_ops()
    img, txt = _embeddings(4, 6, 64, 0)
    hit = torch.full((4,), 0x5A, dtype=torch.uint8).to(ops.device)
    cand = np.array([[1, 2], [0, 2], [0, 1], [0, 5]], np.int32)
    for truth, cd in ((np.array([0, 1, 2, 6], np.int32), cand), (np.arange(4, dtype=np.int32), np.where(cand == 5, 6, cand)),
                      (np.arange(4, dtype=np.int32), np.where(cand == 5, -1, cand))):
        with pytest.raises(_lib.XmcError):
            ops.rprecision_hits(img, txt, truth, cd, out=hit)
    torch.cuda.synchronize()
    assert bool((hit == 0x5A).all())                                         # nothing ran
    assert ops.rprecision_hits(img, txt, np.arange(4, dtype=np.int32), cand).shape == (4,)


@pytest.mark.parametrize("fast", [False, True], ids=["float32", "fast"])
@pytest.mark.parametrize("name,tower", [("small5", "image"), ("small50", "image"), ("small5", "text")])
def test_encoder_small(name, tower, fast):
    run_encoder(name, tower, 5, fast)


def test_an_embedding_does_not_depend_on_its_chunk():
    params, images, ids, eot, _ = reference("small5", 5)
    ops = get_ops()
    whole = clip_utils.ClipEncoder(ops, params, chunk=8)
    split = clip_utils.ClipEncoder(ops, params, chunk=2)
    assert np.array_equal(whole.encode_image(images), split.encode_image(images))
    assert np.array_equal(whole.encode_text(ids, eot), split.encode_text(ids, eot))
    dev_images = torch.as_tensor(images).to(ops.device)                      # device and host images: the same embeddings
    assert np.array_equal(whole.encode_image(dev_images), split.encode_image(images))


def test_encoder_b32_size():
    for tower in ("image", "text"):
        run_encoder("b32", tower, 2, chunk=2)


def test_fast_needs_the_bf16_operator_table():
    params = reference("small5", 5)[0]
    with pytest.raises(ValueError, match="fast"):
        clip_utils.ClipEncoder(get_ops(False), params, fast=True)


def test_out_of_range_token_id_launches_nothing():
    params, _, ids, eot, _ = reference("small5", 5)
    enc = clip_utils.ClipEncoder(get_ops(), params, chunk=2)
    bad = ids.copy()
    bad[4, 1] = 600                                                          # in the LAST chunk: the whole list is checked first
    with pytest.raises(ValueError, match="token id 600"):
        enc.encode_text(bad, eot)
    with pytest.raises(ValueError, match="eot"):
        enc.encode_text(ids, np.array([5, 77, 1, 40, 17]))
    assert enc.launches == 0


# ------------------------------------------------------------------------------------------------- end to end
class _Recording:
    """a ClipScorer that keeps what it returned"""

    def __init__(self, scorer):
        self.scorer, self.images, self.texts = scorer, [], []

    def embed_image(self, images):
        self.images.append(self.scorer.embed_image(images))
        return self.images[-1]

    def embed_text(self, captions):
        self.texts.append(self.scorer.embed_text(captions))
        return self.texts[-1]


def _stub_inception(images):
    from xmcgan_image_generation_amd.utils import inception_utils
    x = torch.as_tensor(images).detach().cpu().double().reshape(images.shape[0], -1, 3)
    m, sd = x.mean(1), x.std(1)
    pool = torch.cat([m, sd, m * sd, m ** 2], 1).numpy().astype(np.float32)
    return pool, inception_utils.softmax(8 * torch.cat([m, sd], 1).numpy()).astype(np.float32)


def test_eval_metric_clip_scores_end_to_end():
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.utils import eval_metrics
    words = ["a cat", "the dog sitting on a horse", "cat's dog", "a horse on the cat", "dog", "the cat on the dog", "horse 42",
             "sitting cat", "a dog's horse", "the"]
    cfg = coco_xmc.get_test_config()
    cfg.update(eval_num=8, eval_batch_size=3, eval_avg_num=1, r_precision_candidates=5)
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds_ = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, _, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, gp, gs, dp, ds_)
    ops = get_ops()

    def batches():
        data = []
        for s in range(3):
            b = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=3, seed=100 + s).items()}
            b["text"] = [words[(3 * s + i) % len(words)].encode() for i in range(3)]
            data.append(b)
        while True:
            yield from data

    plain = eval_metrics.EvalMetric(batches(), cfg, inception=_stub_inception, metric_ops=ops, chunk=4)
    want = plain.calculate_inception_fid(gen, state, 1234)
    cfg_clip = cfg.copy()
    cfg_clip.eval_extra_metrics = ("clip",)
    scorer = _Recording(clip_utils.ClipScorer(VOCAB, MERGES, None, encoder=clip_utils.ClipEncoder(ops, R.small_params())))
    em = eval_metrics.EvalMetric(batches(), cfg_clip, inception=_stub_inception, metric_ops=ops, chunk=4, clip=scorer)
    assert np.array_equal(em._pool, plain._pool)
    real_img, real_txt = np.concatenate(scorer.images)[:8], np.concatenate(scorer.texts)[:8]
    scorer.images, scorer.texts = [], []
    got = em.calculate_metrics(gen, state, 1234)
    assert tuple(got[k] for k in train_utils.EVAL_KEYS) == want              # FID / IS: bit-equal to the run without "clip"
    assert set(got) == set(train_utils.EVAL_KEYS) | set(eval_metrics.EXTRA_METRIC_KEYS["clip"])
    assert all(np.isfinite(v) for v in got.values())
    # the device scores against the NumPy fallback on the same embeddings: float64 sums in another order (1e-13 per cosine),
    # hits exactly equal when no margin is within 1e-6 of a tie
    txt = np.concatenate(scorer.texts)[:8]
    for prefix, img in (("", np.concatenate(scorer.images[0::2])[:8]), ("ema_", np.concatenate(scorer.images[1::2])[:8])):
        cand = A.draw_candidates(np.random.SeedSequence([1234, 0, A.CLIP_SALT]), 8, 5)
        assert abs(got[prefix + "clip_score"] - A.clip_score(img, txt)) <= 2.5e-13
        assert float(np.abs(A.rprecision_margins(img, txt, np.arange(8), cand)).min()) > 1e-6
        assert got[prefix + "r_precision"] == A.r_precision(img, txt, cand)
        assert got[prefix + "clip_score_std"] == got[prefix + "r_precision_std"] == 0.0
    seed = np.random.SeedSequence([int(cfg.seed), A.CLIP_SALT])
    assert abs(got["real_clip_score"] - A.clip_score(real_img, real_txt)) <= 2.5e-13
    real_cand = A.draw_candidates(seed, 8, 5)
    assert float(np.abs(A.rprecision_margins(real_img, real_txt, np.arange(8), real_cand)).min()) > 1e-6
    assert got["real_r_precision"] == A.r_precision(real_img, real_txt, real_cand)
