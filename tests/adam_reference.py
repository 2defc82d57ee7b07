"""Float64 restatement of one Adam (+ EMA) update as the C ABI documents it (xmc_adam_ema, xmc_adam_ema_dev,
xmc_adam_ema_dev_sn, xmc_adam_wprep_tiles; the definition is oracle/torch_ref.py::adam_apply), of the gradient through sigma
that the spectral forms apply on the way in, and the per-element float32 rounding bounds the GPU tests hold the kernels to.

The comparison is TEACHER-FORCED: every step's reference starts from the state the code under test held before the call, so
each bound is a ONE-step bound (U = 2^-24, the unit round-off of float32):

    m    4U * (|beta1 * m_old| + |(1 - beta1) * gs * g|)       the two terms may cancel: the bound follows the terms, not m
    v    6U * v_ref                                             all terms are non-negative
    p    2U * max(|p_old|, |p_ref|) + 1e-5 * lr                 store + subtraction, and ~100 U of the update (~ lr)
    ema  3U * (|d * ema_old| + |(1 - d) * p_ref|) + (1 - d) * p_bound

They are derived, not measured.  tests/test_adam_reference.py runs a float32 emulation of the kernel's operation order
(``adam_step_emulated``, with and without contraction of a * b + c) against them on a machine without a GPU, and shows that the
listed corruptions of that emulation break them.
"""
import numpy as np

U = 2.0 ** -24

# the parameter sets of tests/test_gpu_optimizer.py and tests/test_adam_reference.py (4 steps each)
PARAM_SETS = {
    "product": dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, ema_decay=0.999),
    "decay0.9": dict(lr=1e-2, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, ema_decay=0.9),
    "decay0": dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, ema_decay=0.0),
    "no_ema": dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, ema_decay=0.999),
    "big_eps": dict(lr=2e-4, beta1=0.5, beta2=0.9, eps=1e-3, grad_scale=0.5, ema_decay=0.999),
    "moments": dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, ema_decay=0.999),
}
STEPS = 4


def _f32(x):
    return float(np.float32(x))


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def bias_corrections(beta1, beta2, t):
    """1 / (1 - beta^t) in float64 from the DOUBLE betas (adam_advance_kernel; xmc_adam_ema's host does the same)"""
    return 1.0 / (1.0 - float(beta1) ** int(t)), 1.0 / (1.0 - float(beta2) ** int(t))


def adam_step_ref(p, g, m, v, ema, *, lr, beta1, beta2, eps, grad_scale, ema_decay, t):
    """One update in float64.  lr, eps, grad_scale, ema_decay and the betas of the moment recurrences are rounded to float32
    first (the kernel receives them as ``float``; 1 - beta is then exact in float32); the bias corrections come from the double
    betas.  ``ema`` may be None.  Returns a dict: p, m, v, ema (float64) and p_bound, m_bound, v_bound, ema_bound."""
    p, g, m, v, ema = _f64(p), _f64(g), _f64(m), _f64(v), _f64(ema)
    ic1, ic2 = bias_corrections(beta1, beta2, t)
    lr, eps, gs, d, b1, b2 = _f32(lr), _f32(eps), _f32(grad_scale), _f32(ema_decay), _f32(beta1), _f32(beta2)
    gr = gs * g
    m_new = b1 * m + (1.0 - b1) * gr
    v_new = b2 * v + (1.0 - b2) * gr * gr
    p_new = p - lr * (m_new * ic1) / (np.sqrt(v_new * ic2) + eps)
    out = dict(p=p_new, m=m_new, v=v_new, ema=None, ema_bound=None)
    out["m_bound"] = 4 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * gr))
    out["v_bound"] = 6 * U * v_new
    out["p_bound"] = 2 * U * np.maximum(np.abs(p), np.abs(p_new)) + 1e-5 * lr
    if ema is not None:
        out["ema"] = d * ema + (1.0 - d) * p_new
        out["ema_bound"] = 3 * U * (np.abs(d * ema) + np.abs((1.0 - d) * p_new)) + (1.0 - d) * out["p_bound"]
    return out


def sigma_fix_ref(g, w, u, v, k, inv_sigma, rows, cols, u_axis):
    """The gradient through sigma of one spectrally-normalised (rows, cols) weight: g' = (g - k * u_r * v_c) * inv_sigma
    (u_axis == 0: u runs over the rows) or (g - k * u_c * v_r) * inv_sigma (u_axis == 1), with k = <G, W> * inv_sigma given.
    Returns (g', bound) as (rows, cols) float64; bound = 3 * 2^-24 * (|g| + |k u v|) * |inv_sigma|."""
    g = _f64(g).reshape(rows, cols)
    assert w is None or np.asarray(w).size == rows * cols
    u, v = _f64(u).reshape(-1), _f64(v).reshape(-1)
    if u_axis == 0:
        assert u.size == rows and v.size == cols
        uv = np.outer(u, v)
    else:
        assert u.size == cols and v.size == rows
        uv = np.outer(v, u)
    kuv = float(k) * uv
    inv_sigma = float(inv_sigma)
    return (g - kuv) * inv_sigma, 3 * U * (np.abs(g) + np.abs(kuv)) * abs(inv_sigma)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over all elements; a zero bound demands equality, a NaN anywhere gives inf"""
    got, ref, bound = _f64(got).reshape(-1), _f64(ref).reshape(-1), _f64(bound).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def check_step(got, ref, what=""):
    """``got``: dict p, m, v, ema (arrays as downloaded; ema may be None) -> dict of the worst error-to-bound ratios; asserts
    each is at most 1"""
    out = {}
    for k in ("m", "v", "p", "ema"):
        if ref[k] is None:
            assert got.get(k) is None
            continue
        out[k] = ratio(got[k], ref[k], ref[k + "_bound"])
    bad = {k: r for k, r in out.items() if not r <= 1.0}
    assert not bad, (what, "error / bound above 1", bad, out)
    return out


def merge_worst(worst, new):
    for k, r in new.items():
        worst[k] = max(worst.get(k, 0.0), r)
    return worst


# ---------------------------------------------------------------------------------------------------------------- test data
def make_grads(n, seed, steps=STEPS):
    """``steps`` fresh float32 gradients: magnitudes log-uniform over 1e-4 .. 1, random signs; on step 0 every 7th element is
    zero (with zero moments the element must not move at all), on step 2 every 7th from 3 (non-zero moments, zero gradient)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(steps):
        g = (10.0 ** rng.uniform(-4.0, 0.0, n)) * rng.choice([-1.0, 1.0], n)
        if s == 0:
            g[::7] = 0.0
        if s == 2:
            g[3::7] = 0.0
        out.append(g.astype(np.float32))
    return out


def make_state(n, name, seed):
    """float32 p, m, v, ema of parameter set ``name``: p ~ N(0, 1); the EMA is NOT the parameters (a run that has been going
    for a while: ema - p ~ 1e-2, so that every term of the blend is first order); moments zero except for "moments", where
    v spans 1e-7 .. 1e-1 and m / sqrt(v) is uniform over -1.4 .. 1.4"""
    rng = np.random.default_rng(seed + 1000)
    p = rng.standard_normal(n).astype(np.float32)
    ema = None if name == "no_ema" else (p + 1e-2 * rng.standard_normal(n)).astype(np.float32)
    if name == "moments":
        v = (10.0 ** rng.uniform(-7.0, -1.0, n)).astype(np.float32)
        m = (np.sqrt(v.astype(np.float64)) * rng.uniform(-1.4, 1.4, n)).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    return p, m, v, ema


# ------------------------------------------------------------------------------------------- float32 emulation of the kernel
def _mul(a, b):
    return (np.asarray(a, np.float32) * np.asarray(b, np.float32)).astype(np.float32)


def _add(a, b):
    return (np.asarray(a, np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def _fma(a, b, c):
    """a * b + c with one rounding: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam_step_emulated(p, g, m, v, ema, *, lr, beta1, beta2, eps, grad_scale, ema_decay, t, fma=False, corrupt=None):
    """adam_kernel's statements (csrc/pointwise.hip) in float32, operation by operation; ``fma``: a * b + c contracted where the
    compiler may.  ``corrupt`` names one deliberate error (tests/test_adam_reference.py): "ema_frozen", "ema_old_p",
    "eps_in_sqrt", "no_ic2", "v_unscaled_g", "v_beta1"."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    c1, c2 = bias_corrections(beta1, beta2, t)
    ic1, ic2 = f(c1), f(c2)
    lr, eps, gs, d, b1, b2 = f(lr), f(eps), f(grad_scale), f(ema_decay), f(beta1), f(beta2)
    one = f(1.0)
    gr = _mul(g, gs)
    gv = g if corrupt == "v_unscaled_g" else gr
    bv = b1 if corrupt == "v_beta1" else b2
    if fma:
        m_new = _fma(b1, m, _mul(one - b1, gr))
        v_new = _fma(bv, v, _mul(_mul(one - bv, gv), gv))
    else:
        m_new = _add(_mul(b1, m), _mul(one - b1, gr))
        v_new = _add(_mul(bv, v), _mul(_mul(one - bv, gv), gv))
    vh = v_new if corrupt == "no_ic2" else _mul(v_new, ic2)
    if corrupt == "eps_in_sqrt":
        den = np.sqrt(_add(vh, eps)).astype(f)
    else:
        den = _add(np.sqrt(vh).astype(f), eps)
    upd = (_mul(lr, _mul(m_new, ic1)) / den).astype(f)
    p_new = (p - upd).astype(f)
    ema_new = None
    if ema is not None:
        ema = np.asarray(ema, f)
        src = p if corrupt == "ema_old_p" else p_new
        if corrupt == "ema_frozen":
            ema_new = ema.copy()
        elif fma:
            ema_new = _fma(ema, d, _mul(one - d, src))
        else:
            ema_new = _add(_mul(ema, d), _mul(one - d, src))
    return dict(p=p_new, m=m_new, v=v_new, ema=ema_new)
