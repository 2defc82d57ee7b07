"""Bit-exact parity of the convolution, weight-gradient and stem kernels on small-integer operands (tests/exact_operands.py).

Ternary activations / weights / gradients, integer biases, residuals and masks, power-of-two scales: every product, partial sum
and epilogue step is exact in float32 and the result is exact in the output dtype (asserted on the float64 reference), so each
kernel must EQUAL the float64 reference whatever its summation order, split-K, tile shape or route.  Every comparison of a
kernel's output is ``torch.equal`` (exact_operands.assert_equal); a failure message locates the differing elements.

The cases are those of tests/test_gpu_kernels.py (its lists, and the parametrisations of its tests read from their marks)."""
import pytest
import torch

from tests import exact_operands as E
from tests import test_gpu_kernels as K
from tests.test_exact_operands import (C96_CASES, COMPACT_CASES, FIRST_WRITE_CASES, MX_CASES, PHASE_CASES, POOL_CASES, S2_CASES, _ids,
                                       wgrad_first_write_scenario_of, wgrad_phase_scenario_of, wgrad_scenario_of)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BF16_ROUTES = ("plain", "stream3", "pointwise", "pw_dual", "phase_out", "phase_in", "phase_s2")
ROUTES_SEEN = set()


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda().contiguous()


def _conv(ops, route, *args, **kw):
    """one launch; the route it took is the one the test means to check"""
    y = ops.conv(*args, **kw)
    assert ops.last_conv_route == route, (ops.last_conv_route, route)
    ROUTES_SEEN.add(route)
    return y


def _split_settings(ops, packed):
    """launches on fragment-packed weights run with split-K allowed (the launcher's choice) and forbidden (ops.no_split_k)"""
    return (False, True) if packed else (False,)


def _run_forward(dtype, case, packed):
    """the launch of test_gpu_kernels._run_conv_case, and for cout % 32 == 0 the dgrad-layout weight on a gradient at the
    output resolution: plain for a same-size layer; pool_out with alpha = 4 behind a fused upsample (ConvSite.dgrad_sumpool),
    where the weight-streaming kernel takes it"""
    n, h, cin, cout, ks, ups, relu_in, ex = case
    ops = K._ops(dtype)
    o, refs = E.conv_scenario(case, dtype)
    wf, wd = ops.prep_conv_weight(o["w"].float().cuda())
    route = ("stream3" if ks == 3 else "pointwise") if packed else "plain"
    if packed:
        wf = ops.pack_conv_weight(wf)
    x, bias, mask, res = _dev(o["x"], dtype), _dev(o["bias"], torch.float32), _dev(o["mask"], dtype), _dev(o["res"], dtype)
    for off in _split_settings(ops, packed):
        ops.no_split_k = off
        y = _conv(ops, route, x, wf, bias, ks=ks, ups=ups, relu_in=relu_in, mask=mask, res=res, res_ups=ex.get("res_ups", False),
                  res_scale=o["res_scale"], alpha=o["alpha"], out_f32=ex.get("out_f32", False), relu_out=ex.get("relu_out", False),
                  mask_after_res=ex.get("mask_after_res", False), valid=ex.get("valid", 0))
        assert y.dtype == refs["y"][1]
        E.assert_equal(y, refs["y"][0], f"conv {case} {route} no_split_k={off}")
    if "dx" not in refs:
        return
    if packed:
        wd = ops.pack_conv_weight(wd)
    dy = _dev(o["dy"], dtype)
    if ups and not (packed and ops.can_pool_out(dy, wd)):
        return
    for off in _split_settings(ops, packed):
        ops.no_split_k = off
        if ups:
            dx = _conv(ops, route, dy, wd, None, ks=ks, pool_out=True, alpha=4.0)
        else:
            dx = _conv(ops, route, dy, wd, None, ks=ks)
        E.assert_equal(dx, refs["dx"][0], f"dgrad {case} {route} no_split_k={off}")


@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", K.CONV_CASES, ids=_ids(K.CONV_CASES))
def test_conv_plain_exact(dtype, case):
    """the LDS-staged kernels (unpacked weights), float32 and bf16"""
    _run_forward(dtype, case, packed=False)


@pytest.mark.parametrize("case", K.STREAM_CASES, ids=_ids(K.STREAM_CASES))
def test_conv_stream_exact(case):
    """the weight-streaming 3x3 kernel, split-K through the workspace and without"""
    _run_forward(BF, case, packed=True)


@pytest.mark.parametrize("case", K.PW_CASES, ids=_ids(K.PW_CASES))
def test_conv_pointwise_exact(case):
    _run_forward(BF, case, packed=True)


@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_conv_stream_pool_out_exact(case):
    """2x2 average pooling (+ the pooled residual) in the weight-streaming kernel's epilogue: the launch of test_conv_stream_pool_out"""
    n, h, cin, cout, ups, relu_in = case
    ops = K._ops(BF)
    o, refs = E.conv_scenario(case, BF, pool=True)
    wf, _ = ops.prep_conv_weight(o["w"].float().cuda())
    pw = ops.pack_conv_weight(wf)
    x = _dev(o["x"], BF)
    assert ops.can_pool_out(x, pw, ups)
    for off in (False, True):
        ops.no_split_k = off
        y = _conv(ops, "stream3", x, pw, _dev(o["bias"], torch.float32), ks=3, ups=ups, relu_in=relu_in, res=_dev(o["res"], BF),
                  res_scale=0.5, alpha=0.5, pool_out=True)
        E.assert_equal(y, refs["y"][0], f"pool_out {case} no_split_k={off}")


@pytest.mark.parametrize("case", COMPACT_CASES, ids=_ids(COMPACT_CASES))
def test_conv_pointwise_compact_exact(case):
    """pointwise kernel on a canvas: the whole-canvas launch equals the reference (zero margin); the compact launch equals it on
    the valid corner and leaves the margin of the caller's buffer untouched (or, on the split-K route, zeroed)"""
    n, s, hv, cin, cout = case
    ops = K._ops(BF)
    ops.stream_conv = True
    o, refs = E.compact_scenario(case)
    wf, _ = ops.prep_conv_weight(o["w"].float().cuda(), None, True)
    x, bias, res, m = _dev(o["x"], BF), _dev(o["bias"], torch.float32), _dev(o["res"], BF), _dev(o["mask"], BF)
    ref = refs["y"][0]
    margin = torch.ones((n, s, s), dtype=torch.bool, device="cuda")
    margin[:, :hv, :hv] = False
    for off in (False, True):
        ops.no_split_k = off
        kw = dict(ks=1, res=res, mask=m, mask_after_res=True, relu_out=True, valid=hv, emit_bits=True)
        full = _conv(ops, "pointwise", x, wf, bias, **kw)
        E.assert_equal(full, ref, f"canvas {case} no_split_k={off}")
        out = torch.full((n, s, s, cout), 7.0, dtype=BF, device="cuda")
        y = _conv(ops, "pointwise", x, wf, bias, compact=True, out=out, **kw)
        assert y is out
        E.assert_equal(y[:, :hv, :hv], ref[:, :hv, :hv], f"compact {case} no_split_k={off}")
        assert bool((y[margin] == 7.0).all()) or bool((y[margin] == 0).all()), "the compact launch wrote into the margin"


def test_conv_pw_dual_exact():
    """the dual-source pointwise launch of test_conv_routes: [x | x2] W^T on the valid corner, the zeroed margin never written"""
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=BF)
    o, refs = E.pw_dual_scenario()
    w, _ = ops.prep_conv_weight(o["w"].float().cuda(), None, True)
    out = torch.zeros(tuple(refs["y"][0].shape), dtype=BF, device="cuda")
    y = _conv(ops, "pw_dual", _dev(o["x"], BF), w, None, ks=1, x2=_dev(o["x2"], BF), valid=14, compact=True, out=out)
    assert y is out
    E.assert_equal(y, refs["y"][0], "pw_dual")


@pytest.mark.parametrize("case", PHASE_CASES, ids=_ids(PHASE_CASES))
def test_conv_phase_exact(case):
    """conv3x3(upsample2(.)) / avg_pool2(conv3x3(.)) and their data gradients as four 2x2 convolutions on the low-resolution grid:
    the launches of test_conv_phase.  The phase copies hold SUMS of up to four taps rounded to bf16 (xmc_phase_conv_weight; the
    "in" kind times 1/4): with ternary taps these are integers in [-4, 4] (quarters of them), exact -- the one intermediate
    rounding of this route stays exact too."""
    kind, n, h, cin, cout = case
    ops = K._ops(BF)
    ops.stream_conv = True
    o, refs = E.phase_scenario(case)
    wf, wd = ops.prep_conv_weight(o["w"].float().cuda(), None, True, phase=kind)
    assert wf.phase is not None and wd.phase is not None
    x, bias, dy = _dev(o["x"], BF), _dev(o["bias"], torch.float32), _dev(o["dy"], BF)
    for off in (False, True):
        ops.no_split_k = off
        if kind == "ups":
            y = _conv(ops, "phase_out", x, wf, bias, ks=3, ups=True, mask=_dev(o["mask"], BF), alpha=0.5)
            dx = _conv(ops, "phase_in", dy, wd, None, ks=3, pool_out=True, alpha=4.0)
        else:
            y = _conv(ops, "phase_in", x, wf, bias, ks=3, relu_in=True, res=_dev(o["res"], BF), res_scale=0.5, pool_out=True)
            dx = _conv(ops, "phase_out", dy, wd, None, ks=3, ups=True, alpha=0.25, mask=x)
        E.assert_equal(y, refs["y"][0], f"phase {case} no_split_k={off}")
        E.assert_equal(dx, refs["dx"][0], f"phase dgrad {case} no_split_k={off}")


@pytest.mark.parametrize("case", S2_CASES, ids=_ids(S2_CASES))
def test_conv_stride2_phase_exact(case):
    """stride-2 SAME 3x3 convolution and its adjoint on the phase kernel: the launches of test_conv_stride2_phase"""
    n, h, cin, cout = case
    ops = K._ops(BF)
    ops.stream_conv = True
    o, refs = E.stride2_scenario(case)
    wf, wd = ops.prep_conv_weight(o["w"].float().cuda(), None, True, phase="s2")
    assert ops.can_stride2(wf, h, h) and ops.can_stride2(wd, h // 2, h // 2)
    x, bias, dy, m = _dev(o["x"], BF), _dev(o["bias"], torch.float32), _dev(o["dy"], BF), _dev(o["mask"], BF)
    for off in (False, True):
        ops.no_split_k = off
        y = _conv(ops, "phase_s2", x, wf, bias, ks=3, relu_out=True, stride2=True)
        E.assert_equal(y, refs["y"][0], f"stride-2 {case} no_split_k={off}")
        dx = _conv(ops, "phase_s2", dy, wd, None, ks=3, mask=m, stride2=True)
        E.assert_equal(dx, refs["dx"][0], f"stride-2 adjoint {case} no_split_k={off}")


# ------------------------------------------------------------------------------------------------- weight / bias gradients
def _wgrad_exact(ops, scenario, kw, alpha, what):
    """two accumulating launches into zeros == 2 alpha ref; one overwriting launch into NaNs == alpha ref (dw and db, float32)"""
    o, refs = scenario
    x, dy = _dev(o["x"], ops.dtype), _dev(o["dy"], ops.dtype)
    cout, cin, taps = dy.shape[-1], x.shape[-1], kw["ks"] ** 2
    dw = torch.zeros((cout, taps, cin), device="cuda")
    db = torch.zeros((cout,), device="cuda")
    ops.conv_wgrad(x, dy, dw, db, alpha=alpha, sync=True, **kw)
    ops.conv_wgrad(x, dy, dw, db, alpha=alpha, sync=True, **kw)
    E.assert_equal(dw, 2 * alpha * refs["dw"][0], f"wgrad x2 {what}", axes=E.W_AXES)
    E.assert_equal(db, 2 * alpha * refs["db"][0], f"bias grad x2 {what}", axes=E.W_AXES[:1])
    dw = torch.full((cout, taps, cin), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    ops.conv_wgrad(x, dy, dw, db, alpha=alpha, sync=True, overwrite=True, **kw)
    E.assert_equal(dw, alpha * refs["dw"][0], f"wgrad first write {what}", axes=E.W_AXES)
    E.assert_equal(db, alpha * refs["db"][0], f"bias grad first write {what}", axes=E.W_AXES[:1])


@pytest.mark.parametrize("dtype,variant", [(torch.float32, 0), (BF, 0), (BF, 1)], ids=["f32-v0", "bf16-v0", "bf16-v1"])
@pytest.mark.parametrize("case", K.WG_CASES, ids=_ids(K.WG_CASES))
def test_conv_wgrad_exact(dtype, variant, case):
    """the generic, patch and LDS-DMA weight-gradient kernels, selected through the variant bits as in test_conv_wgrad"""
    n, h, cin, cout, ks, x_ups, x_relu, dy_ups, alpha = case
    _wgrad_exact(K._ops(dtype, variant), wgrad_scenario_of(case), dict(ks=ks, x_ups=x_ups, x_relu=x_relu, dy_ups=dy_ups), alpha,
                 f"{case} v{variant}")


@pytest.mark.parametrize("phase", [True, False], ids=["phase", "3x3"])
@pytest.mark.parametrize("case", K.WGP_CASES, ids=_ids(K.WGP_CASES))
def test_conv_wgrad_phase_exact(case, phase):
    """the phase-decomposed weight gradient next to a 2x resampling, and the 3x3 kernel on the same launch (ops.phase_conv off)"""
    ops = K._ops(BF, 1)
    assert ops.deterministic and ops.phase_conv
    scenario, kw = wgrad_phase_scenario_of(case)
    x, dy = scenario[0]["x"], scenario[0]["dy"]
    assert ops.wgrad_is_phase(x, dy, **kw)
    ops.phase_conv = phase
    assert ops.wgrad_is_phase(x, dy, **kw) == phase
    _wgrad_exact(ops, scenario, kw, 1.0 if case[0] == "ups" else 0.25, f"{case} phase={phase}")


@pytest.mark.parametrize("no_c96", [False, True], ids=["c96", "c128"])
@pytest.mark.parametrize("case", C96_CASES, ids=_ids(C96_CASES))
def test_conv_wgrad_96_cout_tiles_exact(case, no_c96):
    """the LDS-DMA kernel's 96-cout wave mapping and the 128-cout one (XMC_WGRAD_NO_C96) on the 96 / 192 / 288-cout launches"""
    from xmcgan_image_generation_amd._lib import XMC_WGRAD_NO_C96
    n, h, cin, cout, x_relu = case
    ops = K._ops(BF, 1)
    ops.wgrad_variant = 1 | (XMC_WGRAD_NO_C96 if no_c96 else 0)
    scenario = E.wgrad_scenario(case, n, h, h, cin, cout, 3, x_relu=x_relu)
    _wgrad_exact(ops, scenario, dict(ks=3, x_relu=x_relu), 0.5, f"{case} no_c96={no_c96}")


@pytest.mark.parametrize("case", FIRST_WRITE_CASES, ids=_ids(FIRST_WRITE_CASES))
def test_conv_wgrad_every_kernel_path_exact(case):
    """the launches of test_conv_wgrad_first_write_every_kernel_path: phase-decomposed (one / several splits), pointwise, generic"""
    ops = K._ops(BF, 1)
    scenario, kw, alpha = wgrad_first_write_scenario_of(case)
    if case[0] in ("ups", "pool"):
        assert ops.wgrad_is_phase(scenario[0]["x"], scenario[0]["dy"], **kw)
    _wgrad_exact(ops, scenario, kw, alpha, f"{case}")


# ------------------------------------------------------------------------------------------------- stem
def test_stem_conv_and_dgrad_exact():
    """xmc_stem_conv7x7s2 and its data gradient on the canvas geometry of tests/test_gpu_resnet.py (256 canvas, 224 valid, 112
    out), n = 2, against the float64 7x7 stride-2 SAME convolution and its adjoint; margins untouched"""
    from xmcgan_image_generation_amd.ops import HipOps, _p, check
    ops = HipOps(dtype=BF)
    n = 2
    o, refs = E.stem_scenario(n, 224, 112)
    x0 = torch.zeros((n, 256, 256, 3), dtype=BF)
    x0[:, :224, :224] = o["img"].to(BF)
    out = torch.full((n, 128, 128, 64), 7.0, dtype=BF, device="cuda")
    y = ops.stem_conv(x0.cuda(), ops.pack_stem_weight(o["w"].float().numpy()), _dev(o["bias"], torch.float32), 224, 112, out)
    E.assert_equal(y[:, :112, :112], refs["y"][0], "stem")
    margin = y.clone()
    margin[:, :112, :112] = 7.0
    assert bool((margin == 7.0).all())                                          # nothing outside the valid corner is written
    ds = torch.full((n, 128, 128, 64), 3.0, dtype=BF)                           # the margin of ds must not be read
    ds[:, :112, :112] = o["ds"].to(BF)
    wfrag = ops.pack_stem_dgrad_weight(o["w"].float().numpy())
    dx = ops.stem_dgrad(ds.cuda(), wfrag, 112, 256)
    E.assert_equal(dx[:, :224, :224], refs["dx"][0], "stem dgrad")
    # the same launch into a buffer of our own (ops.stem_dgrad allocates its result): the margin of dx is untouched
    dsd = ds.cuda()
    dx2 = torch.full((n, 256, 256, 3), 7.0, dtype=BF, device="cuda")
    check(ops.lib.xmc_stem_conv7x7s2_dgrad(_p(dsd), _p(wfrag), _p(dx2), n, 128, 128, 112, 112, 256, 256, ops._stream()),
          "xmc_stem_conv7x7s2_dgrad")
    E.assert_equal(dx2[:, :224, :224], refs["dx"][0], "stem dgrad (own buffer)")
    dx2[:, :224, :224] = 7.0
    assert bool((dx2 == 7.0).all())


# ------------------------------------------------------------------------------------------------- MX-fp8 routes
@pytest.mark.parametrize("route,case,pool", MX_CASES, ids=[c[0] for c in MX_CASES])
def test_conv_mx8_routes_exact(route, case, pool):
    """one launch per MX-fp8 route, shaped as in test_conv_routes.  Ternary activations and weights -- and the phase copies' sums
    of up to four ternary taps (times 1/4 for the "in" kind) -- are e4m3 numbers under any power-of-two block scale, so the
    block-scaled products and their float32 sums are exact and the same bit-exact check applies."""
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=BF)
    ops.fp8 = True
    ops.fp8_phase_mx = ops.fp8_phase_in_mx = route != "mx8"
    o, refs = E.conv_scenario(case, BF, pool=pool)
    phase = {"mx8": None, "mx8_phase_out": "ups", "mx8_phase_in": "pool"}[route]
    wf, _ = ops.prep_conv_weight(o["w"].float().cuda(), None, True, phase=phase)
    x, bias = _dev(o["x"], BF), _dev(o["bias"], torch.float32)
    if pool:
        y = _conv(ops, route, x, wf, bias, ks=3, res=_dev(o["res"], BF), res_scale=0.5, alpha=0.5, pool_out=True)
    else:
        y = _conv(ops, route, x, wf, bias, ks=3, ups=case[5])
    assert (ops.last_conv_mx8_phase, ops.last_conv_mx8_phase_in) == (route == "mx8_phase_out", route == "mx8_phase_in")
    E.assert_equal(y, refs["y"][0], route)


# ------------------------------------------------------------------------------------------------- coverage
def test_routes_covered():
    """runs last: the launches of this module (run as a whole) went through every bf16 route of HipOps.conv"""
    assert set(BF16_ROUTES) <= ROUTES_SEEN, sorted(set(BF16_ROUTES) - ROUTES_SEEN)
