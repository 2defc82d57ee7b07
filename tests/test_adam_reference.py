"""The bounds of tests/adam_reference.py, checked without a GPU: a float32 emulation of adam_kernel's operation order must stay
inside them (with and without a * b + c contracted, at small and at large step counts), and each deliberate corruption of the
emulation must leave them -- so the bounds are neither too tight for a correct kernel nor too loose to notice a wrong one."""
import numpy as np
import pytest

from tests import adam_reference as AR

N = 4099
T0 = (0, 99990)
CORRUPTIONS = ("ema_frozen", "ema_old_p", "eps_in_sqrt", "no_ic2", "v_unscaled_g", "v_beta1")


def _run(name, t0, fma, corrupt=None, raise_on_miss=True):
    """4 teacher-forced steps of the emulation against adam_step_ref -> worst ratio per quantity"""
    hp = AR.PARAM_SETS[name]
    p, m, v, ema = AR.make_state(N, name, seed=5)
    worst = {}
    for s, g in enumerate(AR.make_grads(N, seed=6)):
        t = t0 + s + 1
        ref = AR.adam_step_ref(p, g, m, v, ema, t=t, **hp)
        got = AR.adam_step_emulated(p, g, m, v, ema, t=t, fma=fma, corrupt=corrupt, **hp)
        if raise_on_miss:
            AR.merge_worst(worst, AR.check_step(got, ref, (name, t, fma)))
        else:
            AR.merge_worst(worst, {k: AR.ratio(got[k], ref[k], ref[k + "_bound"]) for k in ("m", "v", "p", "ema") if ref[k] is not None})
        p, m, v, ema = got["p"], got["m"], got["v"], got["ema"]
    return worst


@pytest.mark.parametrize("fma", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("t0", T0)
@pytest.mark.parametrize("name", list(AR.PARAM_SETS))
def test_emulation_stays_inside_the_bounds(name, t0, fma):
    worst = _run(name, t0, fma)
    print(f"emulation {name} t0={t0} fma={fma}: worst error / bound", {k: round(r, 3) for k, r in worst.items()})
    assert set(worst) == ({"m", "v", "p"} if name == "no_ema" else {"m", "v", "p", "ema"})
    assert all(r <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("corrupt", CORRUPTIONS)
def test_corrupted_emulation_breaks_a_bound(corrupt):
    """over the parameter sets (t = 1 .. 4, where the bias corrections are far from 1), with and without contraction"""
    for fma in (False, True):
        broken = {}
        for name in AR.PARAM_SETS:
            worst = _run(name, 0, fma, corrupt=corrupt, raise_on_miss=False)
            over = {k: r for k, r in worst.items() if not r <= 1.0}
            if over:
                broken[name] = over
        print(f"corruption {corrupt} fma={fma}: bounds broken in", {n: sorted(o) for n, o in broken.items()})
        assert broken, (corrupt, fma, "no bound noticed")
        if corrupt.startswith("ema"):
            assert "decay0.9" in broken and "decay0" in broken and "no_ema" not in broken, broken
            assert all(set(o) == {"ema"} for o in broken.values()), broken
        else:
            assert "product" in broken, broken


def test_zero_gradient_and_moments_leave_the_parameter_alone():
    """reference and emulation: p is returned bit for bit where g, m and v are zero (and the bounds there demand it for m, v)"""
    hp = AR.PARAM_SETS["product"]
    p, m, v, ema = AR.make_state(N, "product", seed=5)
    g = AR.make_grads(N, seed=6)[0]
    ref = AR.adam_step_ref(p, g, m, v, ema, t=1, **hp)
    got = AR.adam_step_emulated(p, g, m, v, ema, t=1, **hp)
    z = g == 0
    assert z.sum() == (N + 6) // 7
    assert np.array_equal(ref["p"][z], p[z].astype(np.float64)) and np.array_equal(got["p"][z], p[z])
    assert float(ref["m_bound"][z].max()) == 0.0 and float(ref["v_bound"][z].max()) == 0.0


def test_sigma_fix_ref_axes_and_bound():
    rng = np.random.default_rng(0)
    for rows, cols, ax in ((5, 12, 0), (3, 7, 1), (40, 1, 1)):
        g = rng.standard_normal((rows, cols))
        u = rng.standard_normal(rows if ax == 0 else cols)
        v = rng.standard_normal(cols if ax == 0 else rows)
        out, bound = AR.sigma_fix_ref(g, None, u, v, 0.3, 0.5, rows, cols, ax)
        for r in range(rows):
            for c in range(cols):
                uv = u[r] * v[c] if ax == 0 else u[c] * v[r]
                assert abs(out[r, c] - (g[r, c] - 0.3 * uv) * 0.5) < 1e-15
                assert bound[r, c] == 3 * AR.U * (abs(g[r, c]) + abs(0.3 * uv)) * 0.5
        # a float32 evaluation in the kernel's order stays inside the bound
        f = np.float32
        g32, u32, v32 = g.astype(f), u.astype(f), v.astype(f)
        ref, bound = AR.sigma_fix_ref(g32, None, u32, v32, f(0.3), f(0.5), rows, cols, ax)
        uv32 = np.outer(u32, v32) if ax == 0 else np.outer(v32, u32)
        got = ((g32 - f(0.3) * uv32).astype(f) * f(0.5)).astype(f)
        assert AR.ratio(got, ref, bound) <= 1.0
