"""CPU tests of tests/exact_operands.py: the operands of every case of tests/test_gpu_exact.py meet the conditions the bit-exact
comparison rests on (so the GPU file never fails for a reason of its own); a one-term corruption that the old bf16 bar (_close)
accepts is rejected by the exact comparison; the helper's reference agrees with a plain loop over taps."""
import pytest
import torch

from tests import exact_operands as E
from tests import test_gpu_kernels as K


def cases_of(fn, arg="case"):
    """the case list of an existing parametrised test, read from its marks (kept in one place: the test itself)"""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == arg]
    return list(mark.args[1])


def _uniq(cases):
    seen, out = set(), []
    for c in cases:
        if repr(c) not in seen:
            seen.add(repr(c))
            out.append(c)
    return out


FWD_CASES = _uniq(K.CONV_CASES + K.STREAM_CASES + K.PW_CASES)
POOL_CASES = cases_of(K.test_conv_stream_pool_out)
PHASE_CASES = cases_of(K.test_conv_phase)
S2_CASES = cases_of(K.test_conv_stride2_phase)
# every case of test_conv_pointwise_compact but its 40-image one (the same kernel path as (3, 64, 56, 64, 256) on 42 M outputs)
COMPACT_CASES = [c for c in cases_of(K.test_conv_pointwise_compact) if c[0] < 40]
C96_CASES = cases_of(K.test_conv_wgrad_96_cout_tiles_equal_128_cout_tiles_and_first_write)
FIRST_WRITE_CASES = cases_of(K.test_conv_wgrad_first_write_every_kernel_path)
# the MX-fp8 routes, shaped as the launches of test_conv_routes: (route, conv_scenario case, pooled form?)
MX_CASES = [("mx8", (2, 16, 64, 64, 3, False, False, dict(bias=True)), False),
            ("mx8_phase_out", (2, 16, 64, 64, 3, True, False, dict(bias=True)), False),
            ("mx8_phase_in", (2, 8, 64, 64, False, False), True)]


def wgrad_scenario_of(case):
    """WG_CASES tuple -> scenario"""
    n, h, cin, cout, ks, x_ups, x_relu, dy_ups, _ = case
    ho = 2 * h if x_ups else h
    hd = ho // 2 if dy_ups else ho
    return E.wgrad_scenario(case, n, h, hd, cin, cout, ks, x_ups=x_ups, x_relu=x_relu, dy_ups=dy_ups)


def wgrad_phase_scenario_of(case):
    """WGP_CASES tuple (form, n, V side, cin, cout, x_relu) -> scenario, launch keywords"""
    form, n, v, cin, cout, x_relu = case
    ups = form == "ups"
    kw = dict(ks=3, x_ups=ups, x_relu=x_relu, dy_ups=not ups)
    return E.wgrad_scenario(case, n, v if ups else 2 * v, 2 * v if ups else v, cin, cout, 3, x_ups=ups, x_relu=x_relu, dy_ups=not ups), kw


def wgrad_first_write_scenario_of(case):
    """a case of test_conv_wgrad_first_write_every_kernel_path (kind, n, h, cin, cout) -> scenario, launch keywords, alpha"""
    kind, n, h, cin, cout = case
    ks = 1 if kind == "1x1" else 3
    hx, hd = (h, 2 * h) if kind == "ups" else (2 * h, h) if kind == "pool" else (h, h)
    kw = dict(ks=ks, x_ups=kind == "ups", x_relu=False, dy_ups=kind == "pool")
    return E.wgrad_scenario(case, n, hx, hd, cin, cout, ks, x_ups=kw["x_ups"], dy_ups=kw["dy_ups"]), kw, 0.25 if kind == "pool" else 1.0


def _ids(cases):
    return [repr(c).replace(" ", "") for c in cases]


# ---------------------------------------------------------------------------------------------- representability
# (each scenario builder asserts both conditions itself -- the non-zero shares and the round trip of every reference through its
# output dtype -- so building it IS the test; the float32 plain route shares the bf16 operands' integers, exact a fortiori)
@pytest.mark.parametrize("case", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_cases_are_representable(case):
    for dtype in (torch.bfloat16, torch.float32) if case in K.CONV_CASES else (torch.bfloat16,):      # float32: the plain route only
        o, refs = E.conv_scenario(case, dtype)
        assert E.share_of(o["x"]) >= 0.25 and E.share_of(o["w"]) >= 0.25
        for name, (ref, dt) in refs.items():
            assert torch.equal(ref.detach().to(dt).double(), ref.detach()), name
            assert float(ref.abs().max()) > 0, name


@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_pool_out_cases_are_representable(case):
    o, refs = E.conv_scenario(case, torch.bfloat16, pool=True)
    ref, dt = refs["y"]
    assert torch.equal(ref.to(dt).double(), ref) and E.share_of(o["x"]) >= 0.25 and E.share_of(o["w"]) >= 0.25


@pytest.mark.parametrize("build,cases", [(E.phase_scenario, PHASE_CASES), (E.stride2_scenario, S2_CASES), (E.compact_scenario, COMPACT_CASES)],
                         ids=["phase", "stride2", "compact"])
def test_phase_stride2_and_compact_cases_are_representable(build, cases):
    for case in cases:
        o, refs = build(case)
        assert E.share_of(o["x"]) >= 0.25 and E.share_of(o["w"]) >= 0.25, case
        for name, (ref, dt) in refs.items():
            assert torch.equal(ref.to(dt).double(), ref) and float(ref.abs().max()) > 0, (case, name)


def test_wgrad_cases_are_representable():
    scen = [wgrad_scenario_of(c) for c in K.WG_CASES] + [wgrad_phase_scenario_of(c)[0] for c in K.WGP_CASES]
    scen += [wgrad_first_write_scenario_of(c)[0] for c in FIRST_WRITE_CASES]
    scen += [E.wgrad_scenario(c, c[0], c[1], c[1], c[2], c[3], 3, x_relu=c[4]) for c in C96_CASES]
    for o, refs in scen:
        assert E.share_of(o["x"]) >= 0.25 and E.share_of(o["dy"]) >= 0.25
        for name, (ref, dt) in refs.items():
            # twice the accumulation at the largest alpha in use
            assert torch.equal((8 * ref).to(dt).double(), 8 * ref) and float(ref.abs().max()) > 0, name


def test_stem_pw_dual_and_mx_cases_are_representable():
    for o, refs in [E.stem_scenario(), E.pw_dual_scenario()] + [E.conv_scenario(c, torch.bfloat16, pool=p) for _, c, p in MX_CASES]:
        for name, (ref, dt) in refs.items():
            assert torch.equal(ref.to(dt).double(), ref) and float(ref.abs().max()) > 0, name


def test_generators():
    g = E.generator(("a", 1))
    t = E.ternary((3, 5, 7, 9), 0.25, g)
    assert int((t != 0).sum()) == -(-t.numel() // 4) and set(t.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert torch.equal(t, E.ternary((3, 5, 7, 9), 0.25, E.generator(("a", 1))))           # seeded from the case tuple
    assert not torch.equal(t, E.ternary((3, 5, 7, 9), 0.25, E.generator(("a", 2))))
    # relu_in cases: the negatives are there for the ReLU to zero
    o, _ = E.conv_scenario(K.CONV_CASES[1], torch.bfloat16)
    assert K.CONV_CASES[1][6] and bool((o["x"] < 0).any())
    with pytest.raises(AssertionError):
        E.assert_share(E.ternary((64, 64), 0.2, g))
    with pytest.raises(AssertionError):
        E.assert_representable(torch.tensor([257.0]), torch.bfloat16)
    E.assert_representable(torch.tensor([256.0, -0.25 * 255, 264.0]), torch.bfloat16)


def test_mismatch_report_locates_the_difference():
    want = torch.zeros((2, 4, 32, 64), dtype=torch.bfloat16)
    got = want.clone()
    got[1, 3, 17, 40] = 1.0
    got[1, 1, 1, 8] = float("nan")
    with pytest.raises(AssertionError) as e:
        E.assert_equal(got, want.double(), "demo")
    msg = str(e.value)
    assert "2 of 16384 elements differ" in msg and "row: 1..3 of 4, row mod 2 in [1]" in msg and "col mod 16 in [1]" in msg
    assert "channel mod 32 in [8]" in msg and "at (1, 3, 17, 40): got 1.0, want 0.0" in msg
    E.assert_equal(want, want.double())


# ---------------------------------------------------------------------------------------------- sensitivity
def test_one_missing_term_passes_the_old_bf16_bar_and_fails_the_exact_comparison_forward():
    """forward, cin >= 64: the output a kernel would give if it dropped ONE tap of ONE input channel at ONE corner pixel (a wrong
    halo element) -- inside tests/test_gpu_kernels.py's bf16 bar (_close), rejected by the exact comparison"""
    case = (16, 8, 512, 512, 3, False, False, dict(mask=True, res=True, mask_after_res=True, valid=7))
    assert case in K.STREAM_CASES
    o, refs = E.conv_scenario(case, torch.bfloat16)
    ref = refs["y"][0]
    x, w = o["x"], o["w"]
    # output pixel (0, 0) of image 0 reads input pixel (0, 0) through the centre tap (4); pick a channel / cout whose product is
    # non-zero and whose output the mask lets through
    ci = int((x[0, 0, 0] != 0).nonzero()[0])
    co = int(((w[:, 4, ci] != 0) & (o["mask"][0, 0, 0] > 0)).nonzero()[0])
    bad = ref.clone()
    bad[0, 0, 0, co] -= o["alpha"] * w[co, 4, ci] * x[0, 0, 0, ci]
    assert float((bad - ref).abs().max()) == 1.0
    K._close(bad.bfloat16(), ref, torch.bfloat16, "one missing term")                     # the old check accepts it
    with pytest.raises(AssertionError, match="1 of"):
        E.assert_equal(bad.bfloat16(), ref, "one missing term")
    E.assert_equal(ref.bfloat16(), ref)


def test_one_missing_pixel_passes_the_old_bf16_bar_and_fails_the_exact_comparison_wgrad():
    """weight gradient: one corner pixel's whole contribution left out (a ragged last tile) -- inside the bf16 bar the existing
    test applies to the float32 gradient, rejected by the exact comparison"""
    case = (1, 128, 32, 96, 3, False, False, False, 1.0)
    assert case in K.WG_CASES
    o, refs = wgrad_scenario_of(case)
    dw = refs["dw"][0]
    x, dy = o["x"].clone(), o["dy"]
    x[0, -1, -1] = 0                                                                       # the corner pixel never reaches the sum
    dw_bad, _ = E.wgrad_reference(x, dy, 3)
    assert not torch.equal(dw_bad, dw) and float((dw_bad - dw).abs().max()) == 1.0
    K._close((2 * dw_bad).float(), 2 * dw, torch.bfloat16, "one missing pixel", scale=float((2 * dw).abs().max()))
    with pytest.raises(AssertionError, match="elements differ"):
        E.assert_equal((2 * dw_bad).float(), 2 * dw, "one missing pixel", axes=E.W_AXES)


# ---------------------------------------------------------------------------------------------- independent formulation
def _loop_conv(x, w, ks, ups=False, relu_in=False):
    """a plain loop over taps on a zero-padded copy: no F.conv2d, no autograd"""
    if relu_in:
        x = x.clamp(min=0)
    if ups:
        n, h, _, c = x.shape
        big = torch.zeros((n, 2 * h, 2 * h, c), dtype=x.dtype)
        for dy in range(2):
            for dx in range(2):
                big[:, dy::2, dx::2] = x
        x = big
    n, h, wd, c = x.shape
    p = ks // 2
    pad = torch.zeros((n, h + 2 * p, wd + 2 * p, c), dtype=x.dtype)
    pad[:, p:p + h, p:p + wd] = x
    y = torch.zeros((n, h, wd, w.shape[0]), dtype=x.dtype)
    for ky in range(ks):
        for kx in range(ks):
            y += torch.einsum("nhwc,oc->nhwo", pad[:, ky:ky + h, kx:kx + wd], w[:, ky * ks + kx])
    return y


@pytest.mark.parametrize("form", ["3x3", "ups", "pool"])
def test_reference_against_a_plain_loop_over_taps(form):
    g = E.generator(("loop", form))
    x = E.ternary((2, 4, 4, 5), 0.5, g)
    w = E.ternary((6, 9, 5), 0.5, g)
    bias = E.integers((6,), -8, 8, g)
    if form == "3x3":
        mask, res = E.mask_values((2, 4, 4, 6), g), E.integers((2, 4, 4, 6), -8, 8, g)
        got = E.conv_reference(x, w, 3, relu_in=True, alpha=0.25, bias=bias, mask=mask, res=res, res_scale=0.5, relu_out=True, valid=3)
        want = (0.25 * _loop_conv(x, w, 3, relu_in=True) + bias) * (mask > 0) + 0.5 * res
        want = want.clamp(min=0)
        want[:, 3:] = 0
        want[:, :, 3:] = 0
    elif form == "ups":
        mask, res = E.mask_values((2, 8, 8, 6), g), E.integers((2, 4, 4, 6), -8, 8, g)
        got = E.conv_reference(x, w, 3, ups=True, bias=bias, mask=mask, res=res, res_ups=True, res_scale=0.25, mask_after_res=True)
        big = torch.zeros((2, 8, 8, 6), dtype=torch.float64)
        for dy in range(2):
            for dx in range(2):
                big[:, dy::2, dx::2] = res
        want = (_loop_conv(x, w, 3, ups=True) + bias + 0.25 * big) * (mask > 0)
    else:
        res = E.integers((2, 2, 2, 6), -8, 8, g)
        got = E.conv_reference(x, w, 3, alpha=0.5, bias=bias, res=res, res_scale=0.5, pool_out=True)
        full = 0.5 * _loop_conv(x, w, 3) + bias
        want = 0.25 * (full[:, 0::2, 0::2] + full[:, 0::2, 1::2] + full[:, 1::2, 0::2] + full[:, 1::2, 1::2]) + 0.5 * res
    assert torch.equal(got, want)
