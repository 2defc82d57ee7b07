"""Inception-v3 feature path on the MI355X: xmc_inception_conv on every conv geometry of the network in both dtypes, the
channel-slice contract, the pools, the whole forward against the CPU restatement (tests/inception_ref.py), batch
independence of an image's features, and EvalMetric end to end.

Tolerances.  float32: v_mfma_f32_32x32x2_f32 is an fp32 fmaf chain, so an output is within ~1.5e-7 * sum|x w| of float64 at
the network's K <= 3,456 (MI355X_MICROARCH.md); the bound used is 1e-5 * sum|x w| per element.  bf16: the inputs are the same
bf16 values on both sides (the restatement reads them exactly), the products are exact in the fp32 accumulator, so the
error is that fp32 summation plus ONE round-to-nearest-even of the output to bf16 (relative 2^-9): bound 2^-8 |ref| +
1e-5 sum|x w| (the first layer also rounds clip(2x - 1) to bf16 as it loads: + 2^-8 sum|x w|).  The whole network: float32 pools and predictions within 1e-4 of their scale; bf16 rounds every one of the
~20 activations on an input-to-pool path, each to 2^-9 relative, so pools within 5e-2 of their scale and predictions within
5e-2 absolute.
"""
import numpy as np
import pytest
import torch

from tests import inception_ref as R
from xmcgan_image_generation_amd import _lib
from xmcgan_image_generation_amd.utils import inception_arch as A, inception_utils as U

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module", params=["f32", "bf16"])
def ops(request):
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=DT[request.param])


def _bound(ops, x, w, ref, kh, kw, stride, pad, first):
    absconv = R.conv_ref(x.abs() if not first else torch.ones_like(x), w.abs(), None, kh=kh, kw=kw, stride=stride, pad=pad,
                         relu=False)
    b = 1e-5 * absconv
    if ops.dtype == torch.bfloat16:
        b = b + 2.0 ** -8 * ref.abs()
        if first:                     # the first layer rounds clip(2x - 1) of its bf16 pixels to bf16 once more (2^-9)
            b = b + 2.0 ** -8 * absconv
    return b + 1e-30


def _run_conv(ops, spec, n, gen, x_pad=0, y_pad=0):
    dt, dev = ops.dtype, ops.device
    first = spec.cin == 3
    cin_row = spec.cin + 2 * x_pad
    x = torch.rand if first else torch.randn
    xw = (x(n, spec.hi, spec.wi, cin_row, generator=gen) if first else torch.randn(n, spec.hi, spec.wi, cin_row, generator=gen))
    xw = xw.to(dt)
    w = (torch.randn(spec.cout, spec.kh * spec.kw, spec.cin, generator=gen) / np.sqrt(spec.kh * spec.kw * spec.cin)).to(dt)
    bias = torch.randn(spec.cout, generator=gen) * 0.1
    ldy = spec.cout + 2 * y_pad
    sentinel = torch.full((n, spec.ho, spec.wo, ldy), 12345.0, dtype=dt)
    out = sentinel.to(dev)
    ops.inception_conv(xw.to(dev).contiguous(), w.to(dev).contiguous(), bias.to(dev), out, kh=spec.kh, kw=spec.kw,
                       stride=spec.stride, pad=spec.pad, x_off=x_pad, y_off=y_pad, first=first)
    torch.cuda.synchronize()
    xs = xw[..., x_pad:x_pad + spec.cin]
    ref = R.conv_ref(xs, w, bias, kh=spec.kh, kw=spec.kw, stride=spec.stride, pad=spec.pad, first=first)
    got = out.cpu()
    bound = _bound(ops, xs.double(), w.double(), ref, spec.kh, spec.kw, spec.stride, spec.pad, first)
    return got, sentinel, ref, bound


def test_conv_every_geometry(ops):
    gen = torch.Generator().manual_seed(0)
    seen = set()
    for spec in A.CONVS:
        if spec.geometry in seen:
            continue
        seen.add(spec.geometry)
        n = 1 if spec.ho >= 70 else 2
        got, _, ref, bound = _run_conv(ops, spec, n, gen)
        err = (got.double() - ref).abs()
        assert bool((err <= bound).all()), (spec.geometry, float(err.max()), float((err / bound).max()))
    assert len(seen) == 43


def test_conv_slices_leave_other_channels_untouched(ops):
    gen = torch.Generator().manual_seed(1)
    for idx in (12, 44, 85):                                      # 5x5 at 35, 7x1 at 17, 3x3 at 8
        spec = A.CONVS[idx]
        got, sentinel, ref, bound = _run_conv(ops, spec, 2, gen, x_pad=16, y_pad=24)
        inside = got[..., 24:24 + spec.cout]
        assert bool(((inside.double() - ref).abs() <= bound).all()), idx
        assert torch.equal(got[..., :24], sentinel[..., :24]) and torch.equal(got[..., 24 + spec.cout:], sentinel[..., 24 + spec.cout:])


def test_conv_rejects_bad_geometry(ops):
    dev, dt = ops.device, ops.dtype
    x = torch.zeros(1, 8, 8, 16, dtype=dt, device=dev)
    with pytest.raises(_lib.XmcError):                             # cout not a multiple of 8
        ops.inception_conv(x, torch.zeros(12, 1, 16, dtype=dt, device=dev), None, torch.zeros(1, 8, 8, 12, dtype=dt, device=dev),
                           kh=1, kw=1)
    with pytest.raises(_lib.XmcError):                             # y_off not a multiple of 8
        ops.inception_conv(x, torch.zeros(16, 1, 16, dtype=dt, device=dev), None, torch.zeros(1, 8, 8, 32, dtype=dt, device=dev),
                           kh=1, kw=1, y_off=4)
    with pytest.raises(_lib.XmcError):                             # slice past the end of the row
        ops.inception_conv(x, torch.zeros(16, 1, 16, dtype=dt, device=dev), None, torch.zeros(1, 8, 8, 16, dtype=dt, device=dev),
                           kh=1, kw=1, y_off=8)
    with pytest.raises(_lib.XmcError):                             # cin = 12 outside the first layer
        ops.inception_conv(torch.zeros(1, 8, 8, 12, dtype=dt, device=dev), torch.zeros(16, 1, 12, dtype=dt, device=dev), None,
                           torch.zeros(1, 8, 8, 16, dtype=dt, device=dev), kh=1, kw=1)
    with pytest.raises(_lib.XmcError):                             # 9x9 kernel
        ops.inception_conv(x, torch.zeros(16, 81, 16, dtype=dt, device=dev), None, torch.zeros(1, 8, 8, 16, dtype=dt, device=dev),
                           kh=9, kw=9, pad=(4, 4))


def test_pools(ops):
    dev, dt = ops.device, ops.dtype
    gen = torch.Generator().manual_seed(2)
    for h, c in ((147, 64), (35, 288), (17, 768)):
        x = torch.randn(2, h, h, c, generator=gen).to(dt)
        ho = (h - 3) // 2 + 1
        out = torch.full((2, ho, ho, c + 32), 777.0, dtype=dt)
        outd = out.to(dev)
        ops.maxpool3x3s2_valid(x.to(dev), outd, 16)
        got = outd.cpu()
        want = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).to(dt)
        assert torch.equal(got[..., 16:16 + c], want)
        assert torch.equal(got[..., :16], out[..., :16]) and torch.equal(got[..., 16 + c:], out[..., 16 + c:])
    for h, c in ((35, 192), (17, 768), (8, 1280)):
        x = torch.randn(2, h, h, c, generator=gen).to(dt)
        got = ops.avgpool3x3_same(x.to(dev)).cpu().double()
        want = torch.nn.functional.avg_pool2d(x.double().permute(0, 3, 1, 2), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
        tol = 2.0 ** -8 * want.abs() + 1e-6 if dt == torch.bfloat16 else 1e-6 * (1 + want.abs())
        assert bool(((got - want).abs() <= tol).all())
    x = torch.randn(3, 8, 8, 2048, generator=gen).to(dt)
    got = ops.mean_hw(x.to(dev)).cpu().double()
    assert torch.allclose(got, x.double().mean(dim=(1, 2)), rtol=0, atol=1e-5)


@pytest.fixture(scope="module")
def net_params():
    return A.init_inception(3)


_REF = {}


def _reference(p, s, size):
    """float64 restatement of 4 images of ``size`` px (cached across the two dtypes)"""
    if size not in _REF:
        img = np.random.default_rng(size).random((4, size, size, 3), dtype=np.float32)
        pool, logits = R.forward(p, s, img, torch.float64)
        _REF[size] = (img, pool.numpy(), U.softmax(logits.numpy()))
    return _REF[size]


@pytest.mark.parametrize("size", [128, 256])
def test_forward_matches_the_restatement(ops, net_params, size):
    p, s = net_params
    img, pool_ref, preds_ref = _reference(p, s, size)
    f = U.InceptionV3Features(ops, p, s)
    pool, preds = f(img)
    scale = np.abs(pool_ref).max()
    perr, qerr = np.abs(pool - pool_ref).max() / scale, np.abs(preds - preds_ref).max()
    print(f"{ops.dtype} {size}px: pool err {perr:.3e} of scale, preds err {qerr:.3e}")
    if ops.dtype == torch.float32:
        assert perr <= 1e-4 and qerr <= 1e-4 * max(preds_ref.max(), 1e-3) + 1e-6
    else:
        assert perr <= 5e-2 and qerr <= 5e-2


def test_features_do_not_depend_on_the_batch(ops, net_params):
    p, s = net_params
    f = U.InceptionV3Features(ops, p, s)
    rng = np.random.default_rng(9)
    one = rng.random((1, 128, 128, 3), dtype=np.float32)
    ref_pool, ref_preds = f(one)
    for n in (7, 64):
        batch = rng.random((n, 128, 128, 3), dtype=np.float32)
        batch[n // 2] = one[0]
        pool, preds = f(batch)
        assert np.array_equal(pool[n // 2], ref_pool[0]), n
        np.testing.assert_allclose(preds[n // 2], ref_preds[0], rtol=1e-5, atol=1e-7)


def test_eval_metric_end_to_end(ops):
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.utils import eval_metrics
    cfg = coco_xmc.get_test_config()
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds_ = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, _, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, gp, gs, dp, ds_)

    def batches():                    # a 2-batch cycle: every pass (eval_num // eval_batch_size + 1 = 2 batches) sees the same data
        data = [{k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.eval_batch_size, seed=s).items()}
                for s in (100, 101)]
        while True:
            yield from data

    with pytest.warns(UserWarning, match="random Inception"):
        em = eval_metrics.EvalMetric(batches(), cfg, ops=ops, chunk=256)
    out = em.calculate_inception_fid(gen, state, 1234)
    assert len(out) == 8 and np.all(np.isfinite(out))
    fid, _, is_, _, ema_fid, _, ema_is, _ = out
    assert fid >= -1e-6 and ema_fid >= -1e-6 and is_ >= 1 - 1e-6 and ema_is >= 1 - 1e-6
    assert em.calculate_inception_fid(gen, state, 1234) == out
