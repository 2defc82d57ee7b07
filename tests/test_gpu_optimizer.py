"""Every Adam / EMA optimiser kernel against float64, element by element: the flat adam_kernel behind xmc_adam_ema,
xmc_adam_ema_dev and xmc_adam_ema_dev_sn (with and without the gradient through sigma: FIX), adam_advance_kernel, the tile kernel
adam_wprep_kernel behind xmc_adam_wprep_tiles, and sn_dot_kernel / sn_dot_finish_kernel, which produce kvec.

The comparison is teacher-forced -- each step's reference starts from the device state downloaded before the call -- and the
bounds are the derived one-step float32 bounds of tests/adam_reference.py (checked on the CPU by tests/test_adam_reference.py).
Every test prints its worst error-to-bound ratio; a ratio above 1 is a finding about the kernel, not a bound to widen.
(The guarded forms are pinned bit for bit to these by tests/test_gpu_nonfinite_guard.py.)"""
import numpy as np
import pytest
import torch

from tests import adam_reference as AR

pytestmark = pytest.mark.gpu

SIZES = (3, 4, 4099, 1023 * 5 + 2, 4096)         # tail only; one vector, no tail; odd tails; whole vectors, several blocks
ENTRY_POINTS = ("adam_ema", "adam_ema_dev", "adam_ema_dev_sn")


@pytest.fixture(scope="module")
def ops():
    from xmcgan_image_generation_amd.ops import HipOps
    o = HipOps(dtype=torch.bfloat16)
    keep = o.keep_grads
    yield o
    o.keep_grads = keep


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _state_bits(t):
    """step_state[0] carries the int32 bits of t"""
    s = torch.zeros(4, dtype=torch.float32)
    s.view(torch.int32)[0] = t
    return s.cuda()


def _check_state(state, t, beta1, beta2):
    st = state.cpu()
    assert int(st.view(torch.int32)[0]) == t
    c1, c2 = AR.bias_corrections(beta1, beta2, t)
    for got, want in ((float(st[1]), c1), (float(st[2]), c2)):
        assert abs(got - want) <= 2.0 ** -23 * want, (t, got, want)


def _call(ops, entry, d, g, state, t, hp, zero_grads=False):
    kw = dict(lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], grad_scale=hp["grad_scale"], ema_decay=hp["ema_decay"])
    if entry == "adam_ema":
        ops.adam_ema(d["p"], g, d["m"], d["v"], d["ema"], step=t, **kw)
    elif entry == "adam_ema_dev":
        ops.adam_ema_dev(d["p"], g, d["m"], d["v"], d["ema"], state, **kw)
    else:
        ops.adam_ema_dev_sn(d["p"], g, d["m"], d["v"], d["ema"], state, zero_grads=zero_grads, **kw)


def _run_flat(ops, entry, name, n, t0=0, steps=AR.STEPS, seed=0):
    """``steps`` teacher-forced updates of ``n`` elements -> worst ratios (asserted <= 1 step by step)"""
    hp = AR.PARAM_SETS[name]
    p, m, v, ema = AR.make_state(n, name, seed)
    d = dict(p=_dev(p), m=_dev(m), v=_dev(v), ema=_dev(ema))
    state = _state_bits(t0)
    ops.keep_grads = False
    zero = entry == "adam_ema_dev_sn"                # the one unguarded flat entry point that rewrites the gradient
    worst, seen_still = {}, 0
    for s, g in enumerate(AR.make_grads(n, seed + 1, steps)):
        t = t0 + s + 1
        old = {k: _host(a) for k, a in d.items()}
        gd = _dev(g)
        _call(ops, entry, d, gd, state, t, hp, zero_grads=zero)
        got = {k: _host(a) for k, a in d.items()}
        ref = AR.adam_step_ref(old["p"], g, old["m"], old["v"], old["ema"], t=t, **hp)
        AR.merge_worst(worst, AR.check_step(got, ref, (entry, name, n, t)))
        if entry != "adam_ema":
            _check_state(state, t, hp["beta1"], hp["beta2"])
        if zero:
            assert not _host(gd).any(), "zero_grads leaves a zero gradient, tail included"
        else:
            assert _same_bits(_host(gd), g), "the gradient is an input"
        if hp["ema_decay"] == 0.0:                   # the blend degenerates to a copy: 0 * ema + 1 * p
            assert _same_bits(got["ema"], got["p"])
        still = (g == 0) & (old["m"] == 0) & (old["v"] == 0)
        seen_still += int(still.sum())
        for k in ("p", "m", "v"):
            assert _same_bits(got[k][still], old[k][still]), (k, "moved without gradient or moments")
    if name != "moments":
        assert seen_still >= (n + 6) // 7
    return worst


@pytest.mark.parametrize("name", list(AR.PARAM_SETS))
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_flat_adam_against_float64(ops, entry, name):
    worst = {}
    for n in SIZES:
        AR.merge_worst(worst, _run_flat(ops, entry, name, n, seed=n))
    print(f"flat {entry} {name}: worst error / bound", {k: round(r, 3) for k, r in worst.items()})
    assert set(worst) == ({"m", "v", "p"} if name == "no_ema" else {"m", "v", "p", "ema"})


def test_adam_ema_host_bias_corrections(ops):
    """xmc_adam_ema takes c1 = 1 - beta1^t, c2 = 1 - beta2^t from the host: steps 1, 2 and 1000"""
    hp = AR.PARAM_SETS["product"]
    n = 4099
    p, m, v, ema = AR.make_state(n, "moments", 3)
    d = dict(p=_dev(p), m=_dev(m), v=_dev(v), ema=_dev(ema))
    worst = {}
    for t, g in zip((1, 2, 1000), AR.make_grads(n, 4, 3)):
        old = {k: _host(a) for k, a in d.items()}
        _call(ops, "adam_ema", d, _dev(g), None, t, hp)
        ref = AR.adam_step_ref(old["p"], g, old["m"], old["v"], old["ema"], t=t, **hp)
        AR.merge_worst(worst, AR.check_step({k: _host(a) for k, a in d.items()}, ref, ("adam_ema", t)))
    print("flat adam_ema at steps 1, 2, 1000: worst error / bound", {k: round(r, 3) for k, r in worst.items()})


@pytest.mark.parametrize("t0", [30, 99990])
def test_device_step_counter_from_a_preset_step(ops, t0):
    """step_state preset to t0: after each of 4 updates state[0] holds t, state[1..2] the float64 corrections to one float32
    rounding, and the update is inside the bounds.  From 30 on, 0.5^t is below float32's resolution next to 1: ic1 == 1.0"""
    worst = _run_flat(ops, "adam_ema_dev", "product", 4099, t0=t0, seed=t0)
    print(f"device step counter from {t0}: worst error / bound", {k: round(r, 3) for k, r in worst.items()})
    hp = AR.PARAM_SETS["product"]
    state = _state_bits(t0)
    one = torch.ones(4, device="cuda")
    ops.adam_ema_dev(one.clone(), one, torch.zeros_like(one), torch.zeros_like(one), None, state, lr=hp["lr"], beta1=hp["beta1"],
                     beta2=hp["beta2"])
    _check_state(state, t0 + 1, hp["beta1"], hp["beta2"])
    assert float(state[1]) == 1.0, "1 / (1 - 0.5^t) rounds to exactly 1 in float32 for t > 24"
    if t0 == 99990:
        assert float(state[2]) == 1.0


def test_grid_stride_second_trip_and_tail(ops):
    """more elements than one trip of the capped grid covers (8192 workgroups x 256 lanes x 4), plus 300 vectors of a second
    trip, plus a 3-element tail: one step, every element checked, the worst ratio reported per range"""
    first = 8192 * 256 * 4
    n = first + 4 * 300 + 3
    hp = AR.PARAM_SETS["product"]
    rng = np.random.default_rng(11)
    p = rng.standard_normal(n).astype(np.float32)
    ema = (p + np.float32(1e-2) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    v = (10.0 ** rng.uniform(-7.0, -1.0, n)).astype(np.float32)
    m = (np.sqrt(v) * rng.uniform(-1.4, 1.4, n).astype(np.float32)).astype(np.float32)
    g = ((10.0 ** rng.uniform(-4.0, 0.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    d = dict(p=_dev(p), m=_dev(m), v=_dev(v), ema=_dev(ema))
    state = _state_bits(0)
    ops.adam_ema_dev(d["p"], _dev(g), d["m"], d["v"], d["ema"], state, lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"],
                     grad_scale=hp["grad_scale"], ema_decay=hp["ema_decay"])
    got = {k: _host(a) for k, a in d.items()}
    ref = AR.adam_step_ref(p, g, m, v, ema, t=1, **hp)
    report = {}
    for rname, sl in (("first trip", slice(0, first)), ("second trip", slice(first, n - 3)), ("tail", slice(n - 3, n))):
        report[rname] = {k: AR.ratio(got[k][sl], ref[k][sl], ref[k + "_bound"][sl]) for k in ("m", "v", "p", "ema")}
    print("grid-stride case, worst error / bound per range:", {r: {k: round(x, 3) for k, x in w.items()} for r, w in report.items()})
    for rname, w in report.items():
        assert all(x <= 1.0 for x in w.values()), (rname, w)


# ------------------------------------------------------------------------------------------- the sigma term (adam_kernel<FIX>)
SN_SHAPES = [(5, 12, 0),      # vector branch, 60 elements: the float4 at offset 60 is alignment padding
             (3, 7, 1),       # scalar branch, 21 elements: the last float4 is partial
             (8, 27, 0),      # the RGB convolutions' column count: a float4 straddles rows
             (64, 16, 1),     # vector branch, u over the columns, exactly 1024 elements
             (40, 1, 1),      # one column
             (32, 288, 0)]    # a real convolution shape
# the arena: spectral tensors at 64-aligned offsets between plain stretches; the stretch marked -2 belongs to "another kernel"
SN_LAYOUT = [("plain", 64, -1), ("sn", 0), ("plain", 128, -1), ("sn", 1), ("plain", 64, -2), ("sn", 2), ("plain", 64, -1), ("sn", 3),
             ("sn", 4), ("plain", 192, -1), ("sn", 5), ("plain", 128, -1)]


def _dot_chain(total):
    """L: the most float32 roundings between one product g * w and kvec (sn_dot_kernel, sn_dot_finish_kernel), each a factor of at
    most (1 + 2^-24) on a partial sum of |g w|:
      * the product itself (1; none where the compiler contracts it into the sum),
      * the lane's running sum over its share of the 64K-element chunk: (total & 3) == 0 reads float4s, 3 additions inside one
        4-term expression + one ``s +=`` per 1024-element trip; otherwise one ``s +=`` per 256-element trip,
      * wave_sum: 6 butterfly additions; the four waves: (r0 + r1) + (r2 + r3), 2 additions,
      * sn_dot_finish_kernel: ceil(chunks / 256) additions per lane, 8 levels of the LDS tree, the product with 1 / sigma (1)."""
    chunk = min(total, 65536)
    lane = 3 + -(-chunk // 1024) if total % 4 == 0 else -(-chunk // 256)
    return 1 + lane + 6 + 2 + -(-(-(-total // 65536)) // 256) + 8 + 1


def _fresh_values(rng, n, scale=1.0):
    return (scale * (10.0 ** rng.uniform(-4.0, 0.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _sn_arena(ops):
    rng = np.random.default_rng(21)
    entries, spans, off = [], [], 0
    for kind, a, mark in ((x + (None,))[:3] for x in SN_LAYOUT):
        if kind == "plain":
            spans.append(("plain", off, a, mark))
            off += a
        else:
            rows, cols, ax = SN_SHAPES[a]
            entries.append(dict(w_off=off, rows=rows, cols=cols, u_axis=ax, taps=1, is_conv=False))
            spans.append(("sn", off, rows * cols, a))
            off += (rows * cols + 63) // 64 * 64
    size = off
    bank = ops.sn_bank_create(entries)
    valid = np.zeros(size, bool)                     # everything but the spectral tensors' alignment padding
    for kind, o, n, _ in spans:
        valid[o:o + n] = True
    mp = ops.sn_bank_map(bank, size).cpu()
    frozen = np.zeros(size, bool)
    for kind, o, n, mark in spans:
        if kind == "plain" and mark == -2:
            mp[o // 64:(o + n) // 64] = -2
            frozen[o:o + n] = True
    nv = int(valid.sum())
    st = {k: np.zeros(size, np.float32) for k in ("p", "m", "v", "ema")}
    st["p"][valid] = rng.standard_normal(nv).astype(np.float32)
    st["ema"][valid] = (st["p"][valid] + 1e-2 * rng.standard_normal(nv)).astype(np.float32)
    st["v"][valid] = (10.0 ** rng.uniform(-7.0, -1.0, nv)).astype(np.float32)
    st["m"][valid] = (np.sqrt(st["v"][valid]) * rng.uniform(-1.4, 1.4, nv)).astype(np.float32)
    grads = []
    for _ in range(2):
        g = np.zeros(size, np.float32)
        g[valid] = _fresh_values(rng, nv)
        grads.append(g)
    # u, v: every float of slack (the 4-alignment slack behind each slice, 64 floats behind the last) is NaN
    u = np.full(bank["nu"] + 64, np.nan, np.float32)
    v = np.full(bank["nv"] + 64, np.nan, np.float32)
    scal = np.zeros(2 * bank["n"], np.float32)
    for i, e in enumerate(bank["entries"]):
        u[e["u_off"]:e["u_off"] + e["nu"]] = (rng.standard_normal(e["nu"]) / np.sqrt(e["nu"])).astype(np.float32)
        v[e["v_off"]:e["v_off"] + e["nv"]] = (rng.standard_normal(e["nv"]) / np.sqrt(e["nv"])).astype(np.float32)
        sigma = np.float32(rng.uniform(0.5, 3.0))
        scal[2 * i], scal[2 * i + 1] = sigma, np.float32(1.0) / sigma
    return dict(size=size, bank=bank, map=mp.cuda(), valid=valid, frozen=frozen, state=st, grads=grads, u=u, v=v, scal=scal)


def _check_kvec(bank, kvec, p, g, scal, what):
    worst = 0.0
    for i, e in enumerate(bank["entries"]):
        sl = slice(e["w_off"], e["w_off"] + e["rows"] * e["cols"])
        gw = g[sl].astype(np.float64) * p[sl].astype(np.float64)
        inv = float(scal[2 * i + 1])
        bound = _dot_chain(e["rows"] * e["cols"]) * AR.U * float(np.abs(gw).sum()) * inv
        r = abs(float(kvec[i]) - float(gw.sum()) * inv) / bound
        assert r <= 1.0, (what, "kvec", i, float(kvec[i]), float(gw.sum()) * inv, bound)
        worst = max(worst, r)
    return worst


def _sigma_grad_ref(bank, g_in, p, kvec, scal, u, v):
    """(g', bound) over the arena: sigma_fix_ref with the DEVICE's kvec inside the spectral tensors, g itself (bound 0) elsewhere"""
    ref, bound = g_in.astype(np.float64), np.zeros(g_in.size)
    for i, e in enumerate(bank["entries"]):
        sl = slice(e["w_off"], e["w_off"] + e["rows"] * e["cols"])
        r, b = AR.sigma_fix_ref(g_in[sl], p[sl], u[e["u_off"]:e["u_off"] + e["nu"]], v[e["v_off"]:e["v_off"] + e["nv"]], kvec[i],
                                scal[2 * i + 1], e["rows"], e["cols"], e["u_axis"])
        ref[sl], bound[sl] = r.reshape(-1), b.reshape(-1)
    return ref, bound


def test_sigma_term_against_float64_on_a_synthetic_bank(ops):
    A = _sn_arena(ops)
    bank, valid, frozen, size = A["bank"], A["valid"], A["frozen"], A["size"]
    live = ~frozen
    hp = AR.PARAM_SETS["product"]
    kw = dict(lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], grad_scale=hp["grad_scale"], ema_decay=hp["ema_decay"])
    ud, vd, sd = _dev(A["u"]), _dev(A["v"]), _dev(A["scal"])
    spectral = np.zeros(size, bool)
    for e in bank["entries"]:
        spectral[e["w_off"]:e["w_off"] + e["rows"] * e["cols"]] = True
    results, worst, worst_k, worst_g = {}, {}, 0.0, 0.0
    keep_before = ops.keep_grads
    try:
        for mode in ("keep", "zero", "untouched"):
            ops.keep_grads = mode == "keep"
            d = {k: _dev(a) for k, a in A["state"].items()}
            state = _state_bits(0)
            trace = []
            for it, g_in in enumerate(A["grads"]):
                t = it + 1
                old = {k: _host(a) for k, a in d.items()}
                gd = _dev(g_in)
                kd = ops.sn_bank_dot(bank, d["p"], gd, sd)
                ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=(mode == "zero"),
                                    fix=(A["map"], bank, kd, sd, ud, vd), **kw)
                got = {k: _host(a) for k, a in d.items()}
                g_out, kvec = _host(gd), _host(kd)
                trace.append(got)
                _check_state(state, t, hp["beta1"], hp["beta2"])
                if mode == "zero":
                    assert not g_out[live].any() and _same_bits(g_out[frozen], g_in[frozen])
                    continue
                if mode == "untouched":
                    assert _same_bits(g_out, g_in)
                    continue
                # (a) kvec = <G, W> / sigma
                worst_k = max(worst_k, _check_kvec(bank, kvec, old["p"], g_in, A["scal"], ("update", t)))
                # (b) the gradient written back: sigma_fix_ref inside the spectral tensors, the input bit for bit elsewhere
                g_ref, g_bound = _sigma_grad_ref(bank, g_in, old["p"], kvec, A["scal"], A["u"], A["v"])
                assert _same_bits(g_out[~spectral], g_in[~spectral])
                rg = AR.ratio(g_out[spectral], g_ref[spectral], g_bound[spectral])
                assert rg <= 1.0, ("written-back gradient", t, rg)
                worst_g = max(worst_g, rg)
                assert float(np.abs(g_out[spectral] - g_in[spectral]).max()) > 1e-3, "the sigma term must be first order here"
                # (c) p, m, v, ema with the written-back gradient as the step's g
                ref = AR.adam_step_ref(old["p"], g_out, old["m"], old["v"], old["ema"], t=t, **hp)
                AR.merge_worst(worst, AR.check_step({k: a[live] for k, a in got.items()},
                                                    {k: (a[live] if a is not None else None) for k, a in ref.items()}, ("sigma", t)))
                # (e) alignment padding: still exactly zero; nothing anywhere is NaN (a read past a u / v slice would be)
                for k, a in list(got.items()) + [("g", g_out)]:
                    assert not np.isnan(a).any(), (k, "NaN")
                    assert not a[~valid].any(), (k, "padding written")
                # (f) the stretch marked -2 belongs to another kernel
                for k in ("p", "m", "v", "ema"):
                    assert _same_bits(got[k][frozen], old[k][frozen]), (k, "-2 stretch")
                assert _same_bits(g_out[frozen], g_in[frozen])
            results[mode] = trace
    finally:
        ops.keep_grads = keep_before
    # (d) what happens to the gradient does not touch the update
    for mode in ("zero", "untouched"):
        for it in range(2):
            for k in ("p", "m", "v", "ema"):
                assert _same_bits(results[mode][it][k], results["keep"][it][k]), (mode, it, k)
    print("sigma term: worst error / bound", {k: round(r, 3) for k, r in worst.items()}, "kvec", round(worst_k, 3), "g", round(worst_g, 3))


# --------------------------------------------------------------------------------- the tile kernel (xmc_adam_wprep_tiles)
WP_SHAPES = [(32, 9, 32), (64, 1, 32), (32, 9, 64), (96, 9, 32)]     # (cout, taps, cin); taps == 1: the spare-slot path


def _wprep_arena(ops, with_spectral):
    """every shape once plain and (``with_spectral``) once spectral, 64 plain elements in front of each tensor and at the end"""
    rng = np.random.default_rng(31 + with_spectral)
    tensors, off = [], 64
    for spectral in ((False, True) if with_spectral else (False,)):
        for cout, taps, cin in WP_SHAPES:
            tensors.append(dict(w_off=off, cout=cout, taps=taps, cin=cin, spectral=spectral))
            off += cout * taps * cin + 64
    size = off
    out = dict(size=size, tensors=tensors, bank=None)
    if with_spectral:
        sn = [t for t in tensors if t["spectral"]]
        bank = ops.sn_bank_create([dict(w_off=t["w_off"], rows=t["cout"], cols=t["taps"] * t["cin"], u_axis=0, taps=t["taps"], is_conv=True)
                                   for t in sn])
        u = np.full(bank["nu"] + 64, np.nan, np.float32)
        v = np.full(bank["nv"] + 64, np.nan, np.float32)
        scal = np.zeros(2 * bank["n"], np.float32)
        for i, (t, e) in enumerate(zip(sn, bank["entries"])):
            t.update(site=i, u_off=e["u_off"], v_off=e["v_off"])
            u[e["u_off"]:e["u_off"] + e["nu"]] = (rng.standard_normal(e["nu"]) / np.sqrt(e["nu"])).astype(np.float32)
            v[e["v_off"]:e["v_off"] + e["nv"]] = (rng.standard_normal(e["nv"]) / np.sqrt(e["nv"])).astype(np.float32)
            sigma = np.float32(rng.uniform(0.5, 3.0))
            scal[2 * i], scal[2 * i + 1] = sigma, np.float32(1.0) / sigma
        out.update(bank=bank, u=u, v=v, scal=scal)
    out["wp"] = ops.wprep_create([dict(t, phase=None) for t in tensors])
    st = {}
    st["p"] = (0.05 * rng.standard_normal(size)).astype(np.float32)
    st["ema"] = (st["p"] + 1e-3 * rng.standard_normal(size)).astype(np.float32)
    st["v"] = (10.0 ** rng.uniform(-7.0, -1.0, size)).astype(np.float32)
    st["m"] = (np.sqrt(st["v"]) * rng.uniform(-1.4, 1.4, size)).astype(np.float32)
    out["state"] = st
    out["grads"] = [_fresh_values(rng, size) for _ in range(2)]
    inside = np.zeros(size, bool)
    for t in tensors:
        inside[t["w_off"]:t["w_off"] + t["cout"] * t["taps"] * t["cin"]] = True
    out["inside"] = inside
    return out


@pytest.mark.parametrize("with_spectral", [True, False], ids=["fix", "plain"])
def test_tile_kernel_against_float64(ops, with_spectral):
    """xmc_adam_wprep_tiles (adam_wprep_kernel<FIX> on a table of plain and spectral weights; <!FIX> on plain ones) after the flat
    call that advances step_state and skips the table's tensors (-2), as the product runs them; two consecutive updates"""
    A = _wprep_arena(ops, with_spectral)
    wp, bank, size, inside = A["wp"], A["bank"], A["size"], A["inside"]
    hp = dict(AR.PARAM_SETS["product"], ema_decay=0.99)
    kw = dict(lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], grad_scale=hp["grad_scale"], ema_decay=hp["ema_decay"])
    d = {k: _dev(a) for k, a in A["state"].items()}
    state = _state_bits(0)
    if with_spectral:
        ud, vd, sd = _dev(A["u"]), _dev(A["v"]), _dev(A["scal"])
        skip = ops.wprep_skip_map(wp, size, base=ops.sn_bank_map(bank, size))
    else:
        skip = ops.wprep_skip_map(wp, size)
    assert int((skip == -2).sum()) * 64 == int(inside.sum())
    worst, worst_flat, worst_g = {}, {}, 0.0
    keep_before = ops.keep_grads
    ops.keep_grads = True
    try:
        for it, g_in in enumerate(A["grads"]):
            t = it + 1
            gd = _dev(g_in)
            old = {k: _host(a) for k, a in d.items()}
            if with_spectral:
                kd = ops.sn_bank_dot(bank, d["p"], gd, sd)
                ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, fix=(skip, bank, kd, sd, ud, vd), **kw)
                kvec = _host(kd)
                _check_kvec(bank, kvec, old["p"], g_in, A["scal"], ("tiles", t))
            else:
                ops.adam_ema_dev_sn(d["p"], gd, d["m"], d["v"], d["ema"], state, skip_map=skip, **kw)
            _check_state(state, t, hp["beta1"], hp["beta2"])
            mid = {k: _host(a) for k, a in d.items()}
            # the flat call: the table's tensors untouched, the rest updated (no sigma term there)
            assert _same_bits(_host(gd), g_in)
            ref = AR.adam_step_ref(old["p"], g_in, old["m"], old["v"], old["ema"], t=t, **hp)
            for k in ("p", "m", "v", "ema"):
                assert _same_bits(mid[k][inside], old[k][inside]), (k, "the flat kernel wrote a tensor marked -2")
            AR.merge_worst(worst_flat, AR.check_step({k: a[~inside] for k, a in mid.items()}, {k: a[~inside] for k, a in ref.items()},
                                                     ("flat around the tiles", t)))
            # the tile call
            out = ops.wprep_alloc(wp)
            ops.adam_wprep(wp, out, d["p"], gd, d["m"], d["v"], d["ema"], state, zero_grads=False,
                           fix=(kd, sd, ud, vd) if with_spectral else None, **kw)
            got = {k: _host(a) for k, a in d.items()}
            g_out = _host(gd)
            for k in ("p", "m", "v", "ema"):
                assert _same_bits(got[k][~inside], mid[k][~inside]), (k, "the tile kernel wrote outside its tensors")
            assert _same_bits(g_out[~inside], g_in[~inside])
            if with_spectral:
                g_ref, g_bound = _sigma_grad_ref(bank, g_in, old["p"], kvec, A["scal"], A["u"], A["v"])
                spectral = g_bound > 0
                assert _same_bits(g_out[~spectral], g_in[~spectral])
                rg = AR.ratio(g_out[spectral], g_ref[spectral], g_bound[spectral])
                assert rg <= 1.0, ("kept gradient", t, rg)
                worst_g = max(worst_g, rg)
                assert float(np.abs(g_out[spectral] - g_in[spectral]).max()) > 1e-3
            else:
                assert _same_bits(g_out, g_in)
            ref = AR.adam_step_ref(old["p"], g_out, old["m"], old["v"], old["ema"], t=t, **hp)
            AR.merge_worst(worst, AR.check_step({k: a[inside] for k, a in got.items()}, {k: a[inside] for k, a in ref.items()},
                                                ("tiles", t)))
            assert not any(np.isnan(a).any() for a in got.values())
            # what the kernel emitted from the updated tile == the preparation pass run on the updated parameters, bit for bit
            rb, rpart = ops.wprep_run(wp, d["p"], ud if with_spectral else None)
            for name, a, b in zip(("wf", "wd", "pf", "pd"), out[0], rb):
                assert torch.equal(a[:wp[name]], b[:wp[name]]), ("prepared buffer", name, t)
            assert wp["wf"] > 0 and wp["wd"] > 0 and (wp["part"] > 0) == with_spectral
            assert torch.equal(out[1][:wp["part"]], rpart[:wp["part"]]), ("partial rows", t)
    finally:
        ops.keep_grads = keep_before
    print(f"tile kernel ({'fix' if with_spectral else 'plain'}): worst error / bound", {k: round(r, 3) for k, r in worst.items()},
          "kept g", round(worst_g, 3), "| flat kernel around it", {k: round(r, 3) for k, r in worst_flat.items()})
