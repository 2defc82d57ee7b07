"""The data gradient of the CLIP image tower on the MI355X (csrc/clip_grad.hip, ClipEncoder.image_device(tape=True) /
image_backward) and the CLIP guidance term of train_g_d (config.clip_guidance_weight).  Each kernel against its float64
specification (utils/clip_grad.py, tied to autograd of tests/clip_ref.py by tests/test_clip_guidance.py), the whole pullback
against autograd of tests/clip_grad_ref.py, the step against the switch-off step and against the same oracle.

Per-kernel bounds, from operation counts (u = 2^-24, the float32 unit roundoff):

* attention backward.  The kernel recomputes the probabilities as the forward kernel does: a score is a 64-term fmaf chain scaled
  by 1/8, |ds| <= 65 u |q|.|k| / 8; the exponent's argument s - max is one subtraction, expf a few ulp, the row sum a 2-term add
  and a 6-level tree, one division.  A probability is therefore relatively off by at most
      e_P = 2 max_ij(65 u |q_i|.|k_j| / 8) + (16 + max(max - s)) u.
  dP is a 64-term chain: |d dP_ij| <= 64 u |dctx_i|.|v_j| =: 64 u A_ij (A >= |dP|).  delta = sum_j p_j dP_j (a 2-term fma and a
  tree) and dS = p (dP - delta) / 8 (three operations) then carry, each term bounded by its magnitude,
      |d dS_ij| <= (2 e_P + 80 u) M_ij,     M_ij = p_ij (A_ij + sum_j p_ij A_ij) / 8.
  With e = 2 e_P + 80 u + t u (the t-term chains of the three products, t <= 128):
      |d dQ| <= e (M |k|),   |d dK| <= e (M^T |q|),   |d dV| <= (e_P + t u) (P^T |dctx|) <= e (P^T |dctx|),
  plus 1e-7 for the terms of second order.  Masked keys: exactly 0.
* LayerNorm backward: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma.  xhat and rstd come from the forward kernels'
  row arithmetic, for which tests/test_gpu_clip.py (after tests/test_gpu_bert.py) takes 1e-5 on xhat (absolute, |xhat| = O(1))
  and, by the same derivation, relative on rstd; the two row means are <= 16-term chains and a 6-level tree (24 u of the mean of
  the magnitudes).  An absolute d on xhat and a relative d on rstd change dx by at most d M,
      M = rstd (|g| + (1 + |xhat|) (mean|g| + mean(|g| |xhat|))),
  each twice over (xhat enters twice): bound 2e-5 M + 2 u (|dx| + |dres|) for the final add.  Near-constant row (3 + 1e-4 noise,
  eps = 1e-12): the forward test's 1e-2 on xhat -> 2e-2 M.
* QuickGELU backward: evaluated in float64 and rounded once, x + bias exactly representable: 4 ulp of float32 at the result.
* preprocessing backward: taps are float64 values rounded to float32 (u each), the two gathers are fmaf chains over the at most
  my and mx outputs whose window holds the pixel, then one product with 1 / std (itself rounded):
      |err| <= (my + mx + 8) u (|R|^T |dY_c| |R|) / std_c;  bf16 output (8 significant bits) adds its rounding, 2^-8 |want|.
  Dot-product identity against the forward kernel: <F(x) - F(0), y> = <x, F'^T y>; the forward test's bound b_c per element of
  F gives sum_c b_c |y_c|_1.

Whole tower: yardsticks from the reference alone, as tests/test_gpu_clip.py: g32 = max|grad_float32_cpu - grad_float64|, float32
mode requires max|hip - grad_float64| <= 16 g32; g_bf the same with the rounding dense, fast mode requires <= 2 g_bf.  Every run
prints err, yardstick and ratio (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from tests import clip_grad_ref as GR
from tests import clip_ref as R
from tests import test_gpu_clip as F
from xmcgan_image_generation_amd import _lib
from xmcgan_image_generation_amd.libml import attention_lib
from xmcgan_image_generation_amd.utils import alignment_metrics as A, clip_arch, clip_grad, clip_utils

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = clip_arch.LN_EPS
get_ops, _nan, _lens = F.get_ops, F._nan, F._lens


# --------------------------------------------------------------------------------------------------------- kernel bodies
def run_attention_bwd(t, causal, h=128, n=3):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(t * 10 + causal + 1000)
    rows, heads = n * t, h // 64
    qkv, bias = torch.randn(rows, 3 * h, generator=gen), 0.1 * torch.randn(3 * h, generator=gen)
    dctx = torch.randn(rows, h, generator=gen)
    lens = _lens(t, n)
    want = clip_grad.attention_bwd(qkv.numpy(), bias.numpy(), lens, dctx.numpy(), t, bool(causal))
    # the bound of the header, per (sequence, head)
    z = (qkv.double() + bias.double()).numpy().reshape(n, t, 3, heads, 64)
    q, k, v = (np.abs(z[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))
    do = np.abs(dctx.double().numpy().reshape(n, t, heads, 64).transpose(0, 2, 1, 3))
    zs = z[:, :, 0].transpose(0, 2, 1, 3) @ z[:, :, 1].transpose(0, 2, 3, 1) / 8.0
    live = (np.arange(t)[None, :] < lens.reshape(n, 1))[:, None, None, :]
    if causal:
        live = live & (np.arange(t)[None, :] <= np.arange(t)[:, None])[None, None]
    zs = np.where(live, zs, -np.inf)
    p = np.where(live, np.exp(zs - zs.max(-1, keepdims=True)), 0.0)
    p /= p.sum(-1, keepdims=True)
    spread = float(np.where(live, zs.max(-1, keepdims=True) - zs, 0.0).max())
    e_p = 2 * 65 * U32 * float((q @ k.transpose(0, 1, 3, 2)).max()) / 8.0 + (16 + spread) * U32
    e = 2 * e_p + 80 * U32 + t * U32
    a = do @ v.transpose(0, 1, 3, 2)
    m = p * (a + (p * a).sum(-1, keepdims=True)) / 8.0
    bq, bk, bv = m @ k, m.transpose(0, 1, 3, 2) @ q, p.transpose(0, 1, 3, 2) @ do
    bound = e * np.stack([g.transpose(0, 2, 1, 3) for g in (bq, bk, bv)], axis=2).reshape(rows, 3 * h) + 1e-7
    out = _nan((rows, 3 * h), dev)                                           # an unwritten element stays NaN
    dq, db, dl, dd = qkv.to(dev), bias.to(dev), torch.as_tensor(lens).to(dev), dctx.to(dev)
    ops.mha_attention_bwd(dq, db, dl, lens, dd, t, causal=causal, out=out)
    got = out.cpu().double().numpy()
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print(f"mha_attention_bwd t={t} causal={causal} h={h}: max err {err.max():.3e}, max err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (float(err.max()), ratio)              # (NaN fails the comparison)
    assert not got[want == 0.0].any()                                        # masked keys: exactly 0
    again = _nan((rows, 3 * h), dev)
    ops.mha_attention_bwd(dq, db, dl, lens, dd, t, causal=causal, out=again)
    assert torch.equal(again, out)                                           # two launches, the same bits
    return ratio


def _ln_magnitude(x, gamma, dy, eps):
    x = np.asarray(x, np.float64)
    d = x - x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    xhat, g = np.abs(d * rstd), np.abs(np.asarray(dy, np.float64) * np.asarray(gamma, np.float64))
    return rstd * (g + (1.0 + xhat) * (g.mean(-1, keepdims=True) + (g * xhat).mean(-1, keepdims=True)))


def _ln_bwd_check(got, want, mag, dres, factor=2e-5):
    got, want = got.cpu().double().numpy(), np.asarray(want)
    bound = factor * mag + 2 * U32 * (np.abs(want) + (np.abs(dres) if dres is not None else 0.0))
    err = np.abs(got - want)
    ratio = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())      # (gather: rows of exact zeros)
    assert bool((err <= bound).all()), (float(err.max()), ratio)
    return ratio


def run_ln_bwd(rows, h, with_res=True, alias=False):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(rows * 1000 + h + with_res)
    x, dy, res = torch.randn(rows, h, generator=gen) * 2.0, torch.randn(rows, h, generator=gen), torch.randn(rows, h, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(h, generator=gen)
    dres = res.numpy() if with_res else None
    want = clip_grad.ln_bwd_add(x.numpy(), gamma.numpy(), dy.numpy(), dres, EPS)
    dr = res.to(dev) if with_res else None
    out = dr if (alias and with_res) else _nan((rows, h), dev)
    ops.ln_bwd_add(x.to(dev), gamma.to(dev), dy.to(dev), dres=dr, out=out, eps=EPS)
    return _ln_bwd_check(out, want, _ln_magnitude(x.numpy(), gamma.numpy(), dy.numpy(), EPS), dres)


def run_ln_bwd_row_maps(n, h, t):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(n * 100 + h + t + 5)
    rnd = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    gamma = 1.0 + 0.1 * rnd(h)
    worst = 0.0
    x, dy, res = rnd(n * t, h), rnd(n, h), rnd(n * t, h)                      # the pooled row -> the class rows of the stream
    for with_res in (False, True):
        dres = res.numpy() if with_res else None
        want = clip_grad.ln_bwd_add(x.numpy(), gamma.numpy(), dy.numpy(), dres, EPS, "gather", t)
        mag = np.zeros((n * t, h))
        mag[::t] = _ln_magnitude(x.numpy()[::t], gamma.numpy(), dy.numpy(), EPS)
        out = res.to(dev) if with_res else _nan((n * t, h), dev)             # (with dres: in place, as the encoder calls it)
        ops.ln_bwd_add(x.to(dev), gamma.to(dev), dy.to(dev), dres=out if with_res else None, out=out, eps=EPS, mode="gather", t=t)
        worst = max(worst, _ln_bwd_check(out, want, mag, dres))
        if not with_res:
            assert not out.cpu().view(n, t, h)[:, 1:].any()                   # every other row: exactly 0
    pe, pos, dyv = rnd(n * (t - 1), h), rnd(t, h), rnd(n * t, h)              # pre_layrnorm -> the patch products
    want = clip_grad.ln_bwd_add(pe.numpy(), gamma.numpy(), dyv.numpy(), None, EPS, "vision", t, pos.numpy())
    full = pe.double().numpy().reshape(n, t - 1, h) + pos.double().numpy()[1:]
    mag = _ln_magnitude(full, gamma.numpy(), dyv.numpy().reshape(n, t, h)[:, 1:], EPS).reshape(n * (t - 1), h)
    out = _nan((n * (t - 1), h), dev)
    ops.ln_bwd_add(pe.to(dev), gamma.to(dev), dyv.to(dev), out=out, eps=EPS, mode="vision", t=t, pos=pos.to(dev))
    return max(worst, _ln_bwd_check(out, want, mag, None))


def run_ln_bwd_near_constant_row(h):
    """x = 3 + 1e-4 noise with eps = 1e-12, as the forward test has"""
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(h)
    x, dy = 3.0 + 1e-4 * torch.randn(5, h, generator=gen), torch.randn(5, h, generator=gen)
    one = torch.ones(h)
    want = clip_grad.ln_bwd_add(x.numpy(), one.numpy(), dy.numpy(), None, 1e-12)
    out = _nan((5, h), dev)
    ops.ln_bwd_add(x.to(dev), one.to(dev), dy.to(dev), out=out, eps=1e-12)
    assert float(np.abs(want).max()) > 1e3                                   # rstd ~ 1e4: the case is what it claims to be
    return _ln_bwd_check(out, want, _ln_magnitude(x.numpy(), one.numpy(), dy.numpy(), 1e-12), None, factor=2e-2)


def run_bias_quick_gelu_bwd(rows, f):
    ops = get_ops()
    dev = ops.device
    gen = torch.Generator().manual_seed(rows + f + 1)
    x = torch.randint(-40448, 40449, (rows, f), generator=gen).float() / 1024.0       # multiples of 2^-10: x + bias is exact
    bias = torch.randint(-512, 513, (f,), generator=gen).float() / 1024.0
    x[0, :8] = torch.tensor([39.5, -39.5, 0.0, -0.0, 1.0 / 1024, -1.0 / 1024, -5.0, 5.0]) - bias[:8]
    dy = torch.randn(rows, f, generator=gen)
    v = (x.double() + bias.double()).numpy()
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    want = clip_grad.bias_quick_gelu_bwd(x.numpy(), bias.numpy(), dy.numpy())
    out = _nan((rows, f), dev)
    dyd = dy.to(dev)
    ops.bias_quick_gelu_bwd(x.to(dev), bias.to(dev), dyd, out=out)
    got = out.cpu()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.double().numpy() - want)
    assert bool((err <= 4.0 * ulp).all()), float((err / ulp).max())
    ops.bias_quick_gelu_bwd(x.to(dev), bias.to(dev), dyd, out=dyd)           # in place, as the encoder calls it
    assert torch.equal(dyd.cpu(), got)
    return float((err / ulp).max())


def run_preprocess_bwd(hw, size, patch, dtype=torch.float32, n=2):
    ops = get_ops()
    dev = ops.device
    g = size // patch
    gen = torch.Generator().manual_seed(hw + size + 3)
    dy = torch.randn(n * g * g, 3 * patch * patch, generator=gen)
    std = np.asarray(clip_arch.IMAGE_STD, np.float64)
    want = clip_grad.preprocess_adjoint(dy.numpy(), hw, size, patch)
    r = np.abs(A.resize_matrix(hw, size))
    mag = np.einsum("yh,nyxc,xw->nhwc", r, np.abs(clip_grad.patch_rows_adjoint(dy.numpy(), n, size, patch)) / std, r, optimize=True)
    m = int((r != 0).sum(0).max())
    bound = (2 * m + 8) * U32 * mag + (2.0 ** -8 * np.abs(want) if dtype == torch.bfloat16 else 0.0)
    out = torch.full((n, hw, hw, 3), float("nan"), dtype=dtype, device=dev)
    dyd = dy.to(dev)
    ops.clip_preprocess_bwd(dyd, hw, size, patch, clip_arch.IMAGE_STD, out=out)
    got = out.cpu().double().numpy()
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print(f"clip_preprocess_bwd {size} -> {hw} {dtype}: max err {err.max():.3e}, max err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (float(err.max()), ratio)              # (NaN fails the comparison)
    # <F(x) - F(0), y> = <x, F'^T y> with F the forward KERNEL (the identity wants the float32 transpose)
    x = torch.rand(n, hw, hw, 3, generator=gen)
    full = ops.clip_preprocess_bwd(dyd, hw, size, patch, clip_arch.IMAGE_STD, dtype=torch.float32)
    f1 = ops.clip_preprocess(x.to(dev), size, patch, clip_arch.IMAGE_MEAN, clip_arch.IMAGE_STD)
    f0 = ops.clip_preprocess(torch.zeros(n, hw, hw, 3).to(dev), size, patch, clip_arch.IMAGE_MEAN, clip_arch.IMAGE_STD)
    lhs = float(((f1.cpu().double() - f0.cpu().double()) * dy.double()).sum())
    rhs = float((x.double() * full.cpu().double()).sum())
    _, cnt, w = A.cubic_coeffs(hw, size)
    l1 = float(np.abs(w).sum(1).max())
    y1 = dy.double().abs().view(n * g * g, 3, patch * patch).sum((0, 2)).numpy()       # |y_c|_1
    fwd = np.array([(2 * int(cnt.max()) + 8) * U32 * (l1 * l1 + mu) / s for mu, s in zip(clip_arch.IMAGE_MEAN, clip_arch.IMAGE_STD)])
    print(f"  dot-product identity: |lhs - rhs| {abs(lhs - rhs):.3e}, bound {float((fwd * y1).sum()):.3e}")
    assert abs(lhs - rhs) <= float((fwd * y1).sum()), (lhs, rhs)
    return ratio


# ----------------------------------------------------------------------------------------------------------- whole tower
@functools.lru_cache(maxsize=None)
def grad_reference(name, n=5):
    """(params, images, text, grad64, g32, g_bf): computed once per configuration, shared by the tests, never modified"""
    params, images = F.reference(name, n)[:2]
    text = np.random.default_rng(23).standard_normal((n, clip_utils.infer_dims(params).proj)).astype(np.float32)
    _, loss, g64 = GR.loss_and_grad(params, images, text)
    _, _, g32 = GR.loss_and_grad(params, images, text, dtype=torch.float32)
    _, _, gbf = GR.loss_and_grad(params, images, text, round_bf16=True)
    return params, images, text, (loss, g64), float((g32 - g64).abs().max()), float((gbf - g64).abs().max())


def tower_grad(enc, images, text):
    """InfoNCE of the image embeddings against fixed text rows on the kernels -> (emb, loss, d images)"""
    ops = enc.ops
    emb, tape = enc.image_device(images, tape=True)
    acc = torch.zeros(1).to(ops.device)
    ctape = attention_lib.contrastive_loss_fwd(ops, emb, torch.as_tensor(text).to(ops.device), acc)
    demb, _ = attention_lib.contrastive_loss_bwd(ops, ctape, want_b=False)
    return emb, acc, enc.image_backward(tape, demb)


def run_tower(name, fast=False, n=5):
    params, images, text, (loss, g64), g32, g_bf = grad_reference(name, n)
    ops = get_ops(fast)
    enc = clip_utils.ClipEncoder(ops, params, fast=fast)
    dev_images = torch.as_tensor(images).to(ops.device)
    plain = enc.image_device(dev_images).clone()
    emb, acc, dimg = tower_grad(enc, dev_images, text)
    assert torch.equal(emb, plain)                                           # the tape changes no bit of the embedding
    assert dimg.shape == dev_images.shape and dimg.dtype == torch.float32
    err = float((dimg.cpu().double() - g64).abs().max())
    yard, factor = (g_bf, 2.0) if fast else (g32, 16.0)
    print(f"clip grad {name} n={n} {'fast' if fast else 'float32'}: err {err:.3e}, yardstick {yard:.3e}, ratio {err / yard:.3f} "
          f"(limit {factor:g}), max|grad| {float(g64.abs().max()):.3e}, loss {float(acc):.6f} (float64 {float(loss):.6f})")
    assert err <= factor * yard, (err, yard)
    _, _, again = tower_grad(enc, dev_images, text)
    assert torch.equal(again, dimg)                                          # two runs, the same bits
    return err / yard


# ----------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("t", [1, 2, 5, 50, 64, 65, 128])
def test_mha_attention_bwd(t, causal):
    run_attention_bwd(t, causal)


def test_mha_attention_bwd_twelve_heads():
    run_attention_bwd(50, 0, h=768)


def test_mha_attention_bwd_outside_its_domain():
    ops = get_ops()
    dev = ops.device
    for t, h in ((129, 128), (17, 96)):              # t beyond 128; h no multiple of 64
        lens = np.array([t, t], np.int32)
        qkv, bias, dctx = torch.zeros(2 * t, 3 * h).to(dev), torch.zeros(3 * h).to(dev), torch.zeros(2 * t, h).to(dev)
        out = torch.full((2 * t, 3 * h), 7.0).to(dev)
        with pytest.raises(_lib.XmcError):
            ops.mha_attention_bwd(qkv, bias, torch.as_tensor(lens).to(dev), lens, dctx, t, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                                      # nothing ran


@pytest.mark.parametrize("with_res,alias", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("rows,h", [(7, 4), (51, 128), (9, 1024)])
def test_ln_bwd_add(rows, h, with_res, alias):
    run_ln_bwd(rows, h, with_res, alias)


@pytest.mark.parametrize("n,h,t", [(3, 128, 5), (2, 768, 50)])
def test_ln_bwd_add_row_maps(n, h, t):
    run_ln_bwd_row_maps(n, h, t)


@pytest.mark.parametrize("h", [128, 768])
def test_ln_bwd_of_a_near_constant_row(h):
    run_ln_bwd_near_constant_row(h)


@pytest.mark.parametrize("rows,f", [(51, 256), (85, 3072)])
def test_bias_quick_gelu_bwd(rows, f):
    run_bias_quick_gelu_bwd(rows, f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bf16"])
@pytest.mark.parametrize("hw,size,patch", [(32, 64, 32), (128, 224, 32), (256, 224, 32)])
def test_clip_preprocess_bwd(hw, size, patch, dtype):
    run_preprocess_bwd(hw, size, patch, dtype)


def test_clip_preprocess_bwd_outside_its_domain():
    ops = get_ops()
    dev = ops.device
    outs = []
    for hw, size, patch in ((16, 64, 32), (64, 64, 24)):                     # hw below 32; a size that is no multiple of the patch
        g = size // patch
        outs.append(torch.full((1, hw, hw, 3), 7.0).to(dev))
        with pytest.raises(_lib.XmcError):
            ops.clip_preprocess_bwd(torch.zeros(g * g, 3 * patch * patch).to(dev), hw, size, patch, clip_arch.IMAGE_STD, out=outs[-1])
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)                         # nothing ran


@pytest.mark.parametrize("fast", [False, True], ids=["float32", "fast"])
@pytest.mark.parametrize("name", ["small5", "small50"])
def test_tower_gradient(name, fast):
    run_tower(name, fast)


def test_tower_gradient_b32_size():
    params, images = F.reference("b32", 2)[:2]
    ops = get_ops()
    enc = clip_utils.ClipEncoder(ops, params)
    text = np.random.default_rng(3).standard_normal((2, enc.dims.proj)).astype(np.float32)
    emb, _, dimg = tower_grad(enc, torch.as_tensor(images).to(ops.device), text)
    assert dimg.shape == (2, 128, 128, 3) and bool(torch.isfinite(dimg).all()) and float(dimg.double().norm()) > 0.0
    assert bool(torch.isfinite(emb).all())


# ------------------------------------------------------------------------------------------------------- through the step
# The C0 test configuration (128 px) with the CLIP of clip_ref.SMALL (image size 64: the generated images are shrunk, 5 tokens);
# float32, and once more in bf16 where clip_guidance_fast defaults to on.  Against the oracle, on the images the half step kept:
# the embeddings within the forward gates of tests/test_gpu_clip.py (16 e32 / 2 e_bf), the image cotangent within the gradient
# gates above (16 g32 / 2 g_bf, all yardsticks from the reference on those images), and the loss against float64 InfoNCE of the
# KEPT embeddings to 1e-5 relative -- the loss kernels' own float32 arithmetic (a normalisation, a 64-term product scaled by
# 10, a log-softmax over 2 rows); a scalar yardstick |loss32 - loss64| could be small by accident, so none is used.
B = 2
LAM = 0.5
DTYPES = ["float32", "bfloat16"]
WORDS = ["a cat", "the dog sitting on a horse", "cat's dog", "a horse on the cat", "dog", "the cat on the dog", "horse 42",
         "sitting cat"]
_STEPS = {}


def _cfg(dtype, lam="absent", **kw):
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.update(dtype=dtype, batch_size=B, pretrained_image_contrastive=False)
    if lam != "absent":
        cfg.update(clip_guidance_weight=lam, clip_vocab_path=F.VOCAB, clip_merges_path=F.MERGES)
    cfg.update(kw)
    return cfg


def _guidance(cfg):
    from xmcgan_image_generation_amd.libml import clip_bpe
    return clip_utils.ClipGuidance(R.small_params(), clip_bpe.ClipTokenizer(F.VOCAB, F.MERGES), fast=cfg.dtype == "bfloat16")


def _fresh(cfg):
    from xmcgan_image_generation_amd import synthetic as syn, train_utils
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp, ds)


def _batches(cfg, n, guidance=None, ops=None):
    from xmcgan_image_generation_amd import synthetic as syn
    out = []
    for r in range(n):
        tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=B, rank=r).items()}
        if guidance is not None:
            tb["clip_text"] = guidance.embed_text(ops, [WORDS[(r + i) % len(WORDS)] for i in range(tb["image"].shape[0])])
        out.append(tb)
    return out


def _one_step(dtype, which, **kw):
    """one train_step from the same state and batch: "absent", "zero", "on" -> tensors after the step"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    key = (dtype, which, tuple(sorted(kw.items())))
    if key in _STEPS:
        return _STEPS[key]
    cfg = _cfg(dtype, {"absent": "absent", "zero": 0.0, "on": LAM}[which], **kw)
    gen, disc, state = _fresh(cfg)
    extra, guidance = {}, None
    if kw.get("pretrained_image_contrastive"):       # a random frozen ResNet-50, as __graft_entry__.smoke builds it
        from xmcgan_image_generation_amd.utils import pretrained_model_utils, resnet_v1
        rp, rs = resnet_v1.init_resnet50(7, head_scale=0.2, randomize_bn=True)
        rstate = {"params": rp, "batch_stats": rs}
        extra = {"image_model": pretrained_model_utils.ImageModel(rstate), "image_model_state": rstate}
    if which == "on":
        guidance = extra["clip_guidance"] = _guidance(cfg)
        guidance.keep = True
    tb = _batches(cfg, 1, guidance, gen.ops)[0]
    if cfg.get("diff_augment", ""):
        from xmcgan_image_generation_amd.libml import diff_augment as DA
        tb["d_aug"] = torch.from_numpy(DA.draw_plan(3, 0, 0, tb["image"].shape[0], cfg.image_size, cfg.image_size, cfg.diff_augment))
    state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, extra)
    torch.cuda.synchronize()
    leaves = {k: v.clone() for k, v in (("g", state.g_optimizer.arena.params), ("d", state.d_optimizer.arena.params),
                                        ("g_grads", state.g_optimizer.arena.grads), ("d_grads", state.d_optimizer.arena.grads),
                                        ("ema", state.ema_buffer), ("g_m", state.g_optimizer.arena.m), ("d_v", state.d_optimizer.arena.v))}
    for name, tree in (("bn", state.generator_state["batch_stats"]), ("sn", state.discriminator_state["spectral_norm_stats"])):
        for path, t in xmc_gan._leaves(tree):
            leaves[name + path] = t.clone()
    _STEPS[key] = dict(leaves=leaves, metrics={k: float(v) for k, v in metrics.items()}, kept=guidance.kept if guidance else None,
                       text=tb.get("clip_text"))
    return _STEPS[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_zero_is_the_step_without_the_key(keep_grads, dtype):
    absent, zero = _one_step(dtype, "absent"), _one_step(dtype, "zero")
    assert zero["metrics"] == absent["metrics"] and set(absent["metrics"]) == set(xmc_gan_keys())
    assert set(zero["leaves"]) == set(absent["leaves"])
    for k, v in absent["leaves"].items():
        assert torch.equal(zero["leaves"][k], v), k


def xmc_gan_keys():
    from xmcgan_image_generation_amd import xmc_gan
    return xmc_gan.METRIC_KEYS


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_step_with_the_term(keep_grads, dtype):
    off, on = _one_step(dtype, "absent"), _one_step(dtype, "on")
    m_on, m_off = on["metrics"], off["metrics"]
    assert set(m_on) == set(xmc_gan_keys()) | {"c_loss_g_clip"} and all(np.isfinite(v) for v in m_on.values())
    # D never sees the term
    assert m_on["d_loss"] == m_off["d_loss"] and m_on["c_loss_d"] == m_off["c_loss_d"]
    assert torch.equal(on["leaves"]["d_grads"], off["leaves"]["d_grads"]) and torch.equal(on["leaves"]["d"], off["leaves"]["d"])
    # g_loss grows by lambda c, G's gradient changes
    c = m_on["c_loss_g_clip"]
    assert c > 0.0 and abs((m_on["g_loss"] - m_off["g_loss"]) - LAM * c) <= 4 * U32 * (abs(m_on["g_loss"]) + LAM * c)
    assert not torch.equal(on["leaves"]["g_grads"], off["leaves"]["g_grads"])
    # the half step's own images, embeddings and cotangent against the oracle
    kept, fast = on["kept"], dtype == "bfloat16"
    params = R.small_params()
    img, text = kept["img"].float().cpu().numpy(), kept["text"].cpu().numpy()
    assert img.shape == (B, 128, 128, 3) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    emb64, _, g64 = GR.loss_and_grad(params, img, text)
    if fast:
        emb_y, _, g_y = GR.loss_and_grad(params, img, text, round_bf16=True)
    else:
        emb_y, _, g_y = GR.loss_and_grad(params, img, text, dtype=torch.float32)
    factor = 2.0 if fast else 16.0
    e_yard, g_yard = float((emb_y - emb64).abs().max()), float((g_y - g64).abs().max())
    e_err = float((kept["emb"].cpu().double() - emb64).abs().max())
    g_err = float((kept["dimg"].float().cpu().double() - LAM * g64).abs().max())
    loss_kept = float(GR.info_nce(kept["emb"].cpu().double(), torch.as_tensor(text).double()))
    print(f"clip guidance step {dtype}: emb err {e_err:.3e} / yardstick {e_yard:.3e} = {e_err / e_yard:.3f}; cotangent err "
          f"{g_err:.3e} / (lambda yardstick {LAM * g_yard:.3e}) = {g_err / (LAM * g_yard):.3f} (limit {factor:g}); loss {c:.7f}, "
          f"float64 on the kept embeddings {loss_kept:.7f}")
    assert e_err <= factor * e_yard and g_err <= factor * LAM * g_yard
    assert abs(c - loss_kept) <= 1e-5 * abs(loss_kept)
    assert kept["dimg"].dtype == kept["img"].dtype and kept["dimg"].shape == kept["img"].shape


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager_steps_and_runs_repeat(dtype):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(dtype, LAM)

    def eager_run():
        gen, disc, st = _fresh(cfg)
        guidance = _guidance(cfg)
        bs = _batches(cfg, 4, guidance, gen.ops)
        out = []
        for tb in bs:
            st, m = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {"clip_guidance": guidance})
            out.append(({k: float(v) for k, v in m.items()}, st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone()))
        return bs, out
    bs, eager = eager_run()
    _, again = eager_run()
    for (m1, g1, d1), (m2, g2, d2) in zip(eager, again):                      # two runs from the same seed: the same bits
        assert m1 == m2 and torch.equal(g1, g2) and torch.equal(d1, d2)
    gen2, disc2, st2 = _fresh(cfg)
    extra = {"clip_guidance": _guidance(cfg)}
    st2, m = train_utils.train_step(0, st2, bs[0], xmc_gan, gen2, disc2, cfg, extra)
    assert {k: float(v) for k, v in m.items()} == eager[0][0]
    graphed = train_utils.GraphedTrainStep(st2, bs[1], xmc_gan, gen2, disc2, cfg, extra)
    st2 = graphed.state
    for i, tb in enumerate(bs[1:], start=1):                                 # three replays, each with its own clip_text
        st2, m = graphed(st2, tb)
        got = {k: float(v) for k, v in m.items()}
        print(dtype, "step", i, "eager", eager[i][0], "graph", got)
        assert got == eager[i][0], i
        assert torch.equal(st2.g_optimizer.arena.params, eager[i][1]) and torch.equal(st2.d_optimizer.arena.params, eager[i][2]), i


@pytest.mark.parametrize("dtype,kw", [("float32", dict(pretrained_image_contrastive=True)),
                                      ("float32", dict(diff_augment="color,translation,cutout")),
                                      ("bfloat16", dict(conv_fp8=True))], ids=["resnet", "diff_augment", "conv_fp8"])
def test_one_step_beside_the_other_switches(dtype, kw):
    """(pretrained_image_contrastive off and no augmentation: test_first_step_with_the_term)"""
    m = _one_step(dtype, "on", **kw)["metrics"]
    assert set(m) == set(xmc_gan_keys()) | {"c_loss_g_clip"} and all(np.isfinite(v) for v in m.values())
    assert (m["c_loss_g_pretrained"] != 0.0) == ("pretrained_image_contrastive" in kw)
