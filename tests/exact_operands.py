"""Small-integer operands for bit-exact kernel tests (tests/test_gpu_exact.py, tests/test_exact_operands.py).

With ternary activations / weights / output gradients, small-integer biases, residuals and masks and power-of-two scales every
product, every partial sum in any order and every epilogue step of a convolution is exact in float32, and the final value is
exact in the output dtype as long as it has at most 8 significant bits (bf16) -- a CONDITION this module asserts on the float64
reference, over every element.  A correct kernel then equals the reference bit for bit whatever its summation order, split-K,
tile shape or route; one missing, extra or misplaced term changes some output by at least one grid step.

The module holds no tests.  Everything is float64 torch on the CPU; tensors are NHWC, weights (cout, taps, cin).
"""
import math
import zlib

import torch
import torch.nn.functional as F

MIN_SHARE = 0.25
# (activation share, weight share) of non-zero entries, densest first: ``fit`` takes the first at which every reference of a
# scenario is representable in its kernel's output dtype.  Never below MIN_SHARE on either side.
SHARES = ((0.5, 0.5), (0.5, 0.25), (0.25, 0.25))
_fitted = {}            # scenario key -> index into SHARES (so that a second build in the same process does not search again)


# ------------------------------------------------------------------------------------------------- generators
def seed_of(case, salt=0):
    """a seed from the case tuple, stable across processes (``hash`` of a tuple that holds a string is not)"""
    return (zlib.crc32(repr(case).encode()) + 7919 * salt) % (2 ** 31)


def generator(case, salt=0):
    return torch.Generator().manual_seed(seed_of(case, salt))


def ternary(shape, share, gen):
    """values in {-1, 0, 1}: EXACTLY ceil(share * numel) non-zero entries at random places, random signs"""
    n = int(math.prod(shape))
    k = min(n, int(math.ceil(share * n)))
    u = torch.rand((n,), generator=gen, dtype=torch.float64)
    nz = u <= torch.kthvalue(u, k).values
    sign = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int8).double() * 2 - 1
    return (nz.double() * sign).reshape(shape)


def integers(shape, lo, hi, gen):
    """integers in [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).double()


def mask_values(shape, gen):
    """integers of mixed sign in [-2, 2]: the kernels' rule is ``mask > 0``, so zeros and negatives must both be there"""
    m = integers(shape, -2, 2, gen)
    assert bool((m == 0).any()) and bool((m < 0).any()) and bool((m > 0).any())
    return m


def share_of(t):
    return float((t != 0).double().mean())


def assert_share(t, what=""):
    assert share_of(t) >= MIN_SHARE, (what, share_of(t))
    assert bool(((t == 0) | (t == 1) | (t == -1)).all()), what


# ------------------------------------------------------------------------------------------------- conditions
def representable(ref, dtype):
    """does every element of the float64 reference survive the round trip through ``dtype``?"""
    ref = ref.detach()
    return torch.equal(ref.to(dtype).double(), ref)


def assert_representable(ref, dtype, what=""):
    ref = ref.detach()
    back = ref.to(dtype).double()
    if not torch.equal(back, ref):
        bad = back != ref
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} reference values are not exact in {dtype} "
                             f"(max |ref| {float(ref.abs().max())}, first {ref[bad][:3].tolist()})")


# ------------------------------------------------------------------------------------------------- references
def conv_linear(x, w, ks, ups=False, relu_in=False, stride2=False):
    """the linear part: x NHWC, w (cout, ks*ks, cin) -> NHWC.  ``stride2``: stride-2 SAME of an even-sized map with flax's
    padding (0, 1): y[o] = sum_r w[r] x[2 o + r]"""
    cout, taps, cin = w.shape
    assert taps == ks * ks and x.shape[-1] == cin
    if relu_in:
        x = torch.relu(x)
    if ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    wk = w.reshape(cout, ks, ks, cin).permute(0, 3, 1, 2)
    xc = x.permute(0, 3, 1, 2)
    if stride2:
        assert ks == 3 and not ups
        y = F.conv2d(F.pad(xc, (0, 1, 0, 1)), wk, None, stride=2)
    else:
        y = F.conv2d(xc, wk, None, padding=ks // 2)
    return y.permute(0, 2, 3, 1)


def epilogue(lin, *, alpha=1.0, bias=None, mask=None, res=None, res_ups=False, res_scale=1.0, mask_after_res=False,
             relu_out=False, valid=0, pool_out=False):
    """the kernels' epilogue on the linear result, in their order: alpha, bias, mask, residual (2x repeat for ``res_ups``),
    mask_after_res, relu_out, the ``valid`` margin.  ``pool_out``: the 2x2 average comes after alpha and bias, the residual
    (which has the pooled resolution) and relu_out after it; a pooled launch takes no mask and no margin."""
    y = alpha * lin
    if bias is not None:
        y = y + bias
    if pool_out:
        assert mask is None and not valid and not res_ups
        y = F.avg_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    if mask is not None and not mask_after_res:
        y = torch.where(mask > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res_scale * (res.repeat_interleave(2, 1).repeat_interleave(2, 2) if res_ups else res)
    if mask is not None and mask_after_res:
        y = torch.where(mask > 0, y, torch.zeros_like(y))
    if relu_out:
        y = torch.relu(y)
    if valid:
        keep = torch.zeros(y.shape[1:3], dtype=torch.bool)
        keep[:valid, :valid] = True
        y = torch.where(keep[None, :, :, None], y, torch.zeros_like(y))
    return y


def conv_reference(x, w, ks, *, ups=False, relu_in=False, stride2=False, **ep):
    return epilogue(conv_linear(x, w, ks, ups, relu_in, stride2), **ep)


def data_gradient(x, w, ks, cot, *, ups=False, relu_in=False, stride2=False, pool=False):
    """d <cot, f(x)> / dx by autograd, f = conv_linear (then the 2x2 average for ``pool``)"""
    xr = x.clone().requires_grad_(True)
    y = conv_linear(xr, w, ks, ups, relu_in, stride2)
    if pool:
        y = F.avg_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    (g,) = torch.autograd.grad(y, xr, cot)
    return g


def wgrad_reference(x, dy, ks, *, x_ups=False, x_relu=False, dy_ups=False):
    """(dw, db) for alpha = 1 by autograd through conv_linear: dw (cout, ks*ks, cin), db (cout,)"""
    cout, cin = dy.shape[-1], x.shape[-1]
    wr = torch.zeros((cout, ks * ks, cin), dtype=torch.float64, requires_grad=True)
    y = conv_linear(x, wr, ks, x_ups, x_relu)
    cot = dy.repeat_interleave(2, 1).repeat_interleave(2, 2) if dy_ups else dy
    (dw,) = torch.autograd.grad(y, wr, cot)
    return dw, cot.sum((0, 1, 2))


def stem_linear(img, w):
    """7x7 stride-2 SAME (2 before, 3 after): img (n, h, h, 3), w (64, 49, 3) with tap = ky * 7 + kx"""
    wk = w.reshape(w.shape[0], 7, 7, 3).permute(0, 3, 1, 2)
    return F.conv2d(F.pad(img.permute(0, 3, 1, 2), (2, 3, 2, 3)), wk, None, stride=2).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------- comparison
ACT_AXES = (("image", None), ("row", 2), ("col", 16), ("channel", 32))
W_AXES = (("cout", 32), ("tap", None), ("cin", 32))


def mismatch_report(got, want, axes, what=""):
    """None if ``got`` equals ``want`` bit for bit (same dtype), else a message that locates the difference: how many
    elements, their range per axis, the residues they fall on, the first five (coordinate, got, want)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if torch.equal(got, want):
        return None
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    axes = axes[-got.dim():] if got.dim() <= len(axes) else (("axis", None),) * (got.dim() - len(axes)) + tuple(axes)
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} elements differ"]
    for a, (name, mod) in enumerate(axes):
        col = idx[:, a]
        s = f"  {name}: {int(col.min())}..{int(col.max())} of {got.shape[a]}"
        if mod:
            s += f", {name} mod {mod} in {sorted(set((col % mod).tolist()))}"
        lines.append(s)
    for row in idx[:5]:
        c = tuple(row.tolist())
        lines.append(f"  at {c}: got {float(got[c])}, want {float(want[c])}")
    return "\n".join(lines)


def assert_equal(got, ref, what="", axes=ACT_AXES):
    """the kernel's output (any device) against the float64 reference cast to the kernel's own dtype: torch.equal"""
    got = got.detach().cpu()
    ref = ref.detach()
    assert_representable(ref, got.dtype, what)
    msg = mismatch_report(got, ref.to(got.dtype), axes, what)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------- scenarios
def fit(key, build):
    """``build(x_share, w_share)`` -> (operands, {name: (float64 reference, output dtype)}).  Returns the build at the densest
    pair of SHARES at which every reference is representable; the last pair's failure is raised as it stands."""
    start = _fitted.get(key, 0)
    for i in range(start, len(SHARES)):
        ops_, refs = build(*SHARES[i])
        if i == len(SHARES) - 1 or all(representable(r, dt) for r, dt in refs.values()):
            for name, (r, dt) in refs.items():
                assert_representable(r, dt, f"{key} {name}")
            _fitted[key] = i
            return ops_, refs


def out_dtype(dtype, out_f32=False):
    return torch.float32 if out_f32 or dtype == torch.float32 else torch.bfloat16


def conv_scenario(case, dtype, pool=False):
    """a case tuple of CONV_CASES / STREAM_CASES / PW_CASES (n, h, cin, cout, ks, ups, relu_in, extras) -> operands and the
    references "y" (forward with the whole epilogue) and, for cout % 32 == 0, "dx": the data gradient of the linear part that
    the dgrad-layout weight computes -- of the plain convolution, or (``ups``) of conv(upsample2(.)), which the kernels run
    as pool_out with alpha = 4 on a gradient at the output resolution.
    ``pool``: the form of test_conv_stream_pool_out -- case (n, h, cin, cout, ups, relu_in), bias, alpha = 0.5, pooled residual
    with res_scale = 0.5."""
    if pool:
        n, h, cin, cout, ups, relu_in = case
        ks, ex = 3, dict(bias=True, res=True, res_scale=0.5, alpha=0.5, pool_out=True)
    else:
        n, h, cin, cout, ks, ups, relu_in, ex = case
    ho = 2 * h if ups else h
    hy = ho // 2 if pool else ho

    def build(xs, ws):
        g = generator(case[:7])
        o = dict(x=ternary((n, h, h, cin), xs, g), w=ternary((cout, ks * ks, cin), ws, g), bias=None, mask=None, res=None,
                 alpha=ex.get("alpha", 1.0), res_scale=ex.get("res_scale", 1.0))
        assert_share(o["x"], "x")
        assert_share(o["w"], "w")
        if ex.get("bias"):
            o["bias"] = integers((cout,), -8, 8, g)
        if ex.get("mask"):
            o["mask"] = mask_values((n, ho, ho, cout), g)
        if ex.get("res"):
            hr = hy // 2 if ex.get("res_ups") else hy
            o["res"] = integers((n, hr, hr, cout), -8, 8, g)
        y = conv_reference(o["x"], o["w"], ks, ups=ups, relu_in=relu_in, alpha=o["alpha"], bias=o["bias"], mask=o["mask"],
                           res=o["res"], res_ups=ex.get("res_ups", False), res_scale=o["res_scale"],
                           mask_after_res=ex.get("mask_after_res", False), relu_out=ex.get("relu_out", False),
                           valid=ex.get("valid", 0), pool_out=bool(pool))
        refs = {"y": (y, out_dtype(dtype, ex.get("out_f32", False)))}
        if cout % 32 == 0 and not pool:
            o["dy"] = ternary((n, ho, ho, cout), xs, g)
            refs["dx"] = (data_gradient(torch.zeros_like(o["x"]), o["w"], ks, o["dy"], ups=ups), out_dtype(dtype))
        return o, refs
    return fit(("conv", case[:7], bool(pool), dtype), build)


def phase_scenario(case):
    """a case of test_conv_phase (kind, n, h, cin, cout), bf16.  "ups": y = mask(0.5 conv(upsample2 x) + bias), dx = the data
    gradient (launched as pool_out, alpha = 4).  "pool": y = avg_pool2(conv(relu x)) + bias + 0.5 res, dh = the data gradient
    of the pooled convolution including the ReLU mask (launched as ups, alpha = 0.25, mask = x)."""
    kind, n, h, cin, cout = case
    bf = torch.bfloat16

    def build(xs, ws):
        g = generator(case)
        o = dict(x=ternary((n, h, h, cin), xs, g), w=ternary((cout, 9, cin), ws, g), bias=integers((cout,), -8, 8, g))
        assert_share(o["x"], "x")
        assert_share(o["w"], "w")
        if kind == "ups":
            o["mask"] = mask_values((n, 2 * h, 2 * h, cout), g)
            o["dy"] = ternary((n, 2 * h, 2 * h, cout), xs, g)
            y = conv_reference(o["x"], o["w"], 3, ups=True, alpha=0.5, bias=o["bias"], mask=o["mask"])
            dx = data_gradient(o["x"], o["w"], 3, o["dy"], ups=True)
        else:
            o["res"] = integers((n, h // 2, h // 2, cout), -8, 8, g)
            o["dy"] = ternary((n, h // 2, h // 2, cout), xs, g)
            y = conv_reference(o["x"], o["w"], 3, relu_in=True, bias=o["bias"], res=o["res"], res_scale=0.5, pool_out=True)
            dx = data_gradient(o["x"], o["w"], 3, o["dy"], relu_in=True, pool=True)
        return o, {"y": (y, bf), "dx": (dx, bf)}
    return fit(("phase", case), build)


def stride2_scenario(case):
    """a case of test_conv_stride2_phase (n, h, cin, cout), bf16: y = relu(conv_s2(x) + bias), dx = mask(adjoint(dy))"""
    n, h, cin, cout = case
    bf = torch.bfloat16

    def build(xs, ws):
        g = generator(case)
        o = dict(x=ternary((n, h, h, cin), xs, g), w=ternary((cout, 9, cin), ws, g), bias=integers((cout,), -8, 8, g),
                 dy=ternary((n, h // 2, h // 2, cout), xs, g), mask=mask_values((n, h, h, cin), g))
        assert_share(o["x"], "x")
        assert_share(o["w"], "w")
        y = conv_reference(o["x"], o["w"], 3, stride2=True, bias=o["bias"], relu_out=True)
        dx = data_gradient(o["x"], o["w"], 3, o["dy"], stride2=True)
        dx = torch.where(o["mask"] > 0, dx, torch.zeros_like(dx))
        return o, {"y": (y, bf), "dx": (dx, bf)}
    return fit(("s2", case), build)


def compact_scenario(case):
    """a case of test_conv_pointwise_compact (n, canvas side, valid side, cin, cout), bf16: y = the ``valid`` corner of
    relu(mask_after_res(conv1x1(x) + bias + res)), zero elsewhere"""
    n, s, hv, cin, cout = case

    def build(xs, ws):
        g = generator(case)
        o = dict(x=ternary((n, s, s, cin), xs, g), w=ternary((cout, 1, cin), ws, g), bias=integers((cout,), -8, 8, g),
                 res=integers((n, s, s, cout), -8, 8, g), mask=mask_values((n, s, s, cout), g))
        assert_share(o["x"], "x")
        assert_share(o["w"], "w")
        y = conv_reference(o["x"], o["w"], 1, bias=o["bias"], res=o["res"], mask=o["mask"], mask_after_res=True, relu_out=True, valid=hv)
        return o, {"y": (y, torch.bfloat16)}
    return fit(("compact", case), build)


def pw_dual_scenario(n=2, h=16, c1=64, c2=32, cout=64, valid=14):
    """the dual-source pointwise launch of test_conv_routes: y = [x | x2] W^T on the valid corner, the margin untouched"""
    key = ("pw_dual", n, h, c1, c2, cout, valid)

    def build(xs, ws):
        g = generator(key)
        o = dict(x=ternary((n, h, h, c1), xs, g), x2=ternary((n, h, h, c2), xs, g), w=ternary((cout, 1, c1 + c2), ws, g))
        assert_share(o["x"], "x")
        assert_share(o["x2"], "x2")
        assert_share(o["w"], "w")
        y = conv_reference(torch.cat([o["x"], o["x2"]], -1), o["w"], 1, valid=valid)
        return o, {"y": (y, torch.bfloat16)}
    return fit(key, build)


def wgrad_scenario(key, n, hx, hd, cin, cout, ks, *, x_ups=False, x_relu=False, dy_ups=False):
    """x (n, hx, hx, cin) and dy (n, hd, hd, cout) ternary -> references "dw", "db" for alpha = 1 (float32 outputs: integers far
    below 2^24, any power-of-two alpha keeps them exact)"""
    def build(xs, ws):
        g = generator(key)
        o = dict(x=ternary((n, hx, hx, cin), xs, g), dy=ternary((n, hd, hd, cout), ws, g))
        assert_share(o["x"], "x")
        assert_share(o["dy"], "dy")
        dw, db = wgrad_reference(o["x"], o["dy"], ks, x_ups=x_ups, x_relu=x_relu, dy_ups=dy_ups)
        assert float(dw.abs().max()) * 8 < 2 ** 24 and float(db.abs().max()) * 8 < 2 ** 24
        return o, {"dw": (dw, torch.float32), "db": (db, torch.float32)}
    return fit(("wgrad", key), build)


def stem_scenario(n=2, hv=224, hov=112):
    """ternary images and folded weights of the 7x7 stride-2 stem: "y" = conv + bias (n, hov, hov, 64), "dx" = its adjoint
    applied to a ternary ds (n, hv, hv, 3); bf16"""
    key = ("stem", n, hv, hov)
    bf = torch.bfloat16

    def build(xs, ws):
        g = generator(key)
        o = dict(img=ternary((n, hv, hv, 3), xs, g), w=ternary((64, 49, 3), ws, g), bias=integers((64,), -8, 8, g),
                 ds=ternary((n, hov, hov, 64), xs, g))
        assert_share(o["img"], "img")
        assert_share(o["w"], "w")
        y = stem_linear(o["img"], o["w"]) + o["bias"]
        xr = torch.zeros_like(o["img"]).requires_grad_(True)
        (dx,) = torch.autograd.grad(stem_linear(xr, o["w"]), xr, o["ds"])
        return o, {"y": (y, bf), "dx": (dx, bf)}
    return fit(key, build)
