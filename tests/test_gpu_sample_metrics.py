"""xmc_knn_radii / xmc_ball_hits / xmc_poly3_sums (csrc/sample_metrics.hip) against their NumPy specification
(utils/sample_metrics.py), under guard bands, twice for bit-identity, outside their domain, and through ``EvalMetric``.

Bounds.  The kernels differ from the float64 specification by the error of ONE length-d float32 dot product (a k-ordered fmaf
chain on v_mfma_f32_32x32x2_f32): |dot - ref| <= (d + 2) 2^-24 |u| |v| in the worst case; everything after it is float64.
* radii: d2 = |a|^2 + |b|^2 - 2 dot moves by at most E = 2 (d + 2) 2^-24 M^2 (M: the largest row norm), and an order statistic is
  1-Lipschitz in the distances: every row is held to E.
* hits: with T = 16 (d + 2) 2^-24 M^2 a row is CLEAR when some ball holds it with margin > T or every ball misses it by more than T;
  clear rows must match the specification exactly, the others (at most 8 % of a case's rows: a condition, not a measurement) are
  left out.
* cubic sums: d/ds (s / d + 1)^3 = 3 (s / d + 1)^2 / d, so a sum moves by at most the sum over its pairs of
  3 (1 + |s| / d)^2 (d + 2) 2^-24 |u| |v| / d (first order), evaluated here from the reference.
Shapes: no n or m is a multiple of the 128-row tile, A-C have more than one row block, d is 1, 3, 5 and 64 k-tiles of 32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from xmcgan_image_generation_amd.utils import sample_metrics as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = {"A": (384, 320, 96, 0.0, 1.0), "B": (257, 130, 2048, 0.02, 0.97), "C": (515, 389, 160, 0.1, 0.95), "D": (5, 4, 32, 0.0, 1.0)}


@functools.lru_cache(maxsize=None)
def _ops():
    from xmcgan_image_generation_amd.ops import HipOps
    return HipOps(dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _pools(shape):
    """(real, fake) float32 host arrays, their device copies, the largest row norm; shared, never written"""
    n, m, d, shift, scale = SHAPES[shape]
    r = np.random.default_rng(1)
    real = np.abs(r.standard_normal((n, d))).astype(np.float32)
    fake = np.abs(r.standard_normal((m, d)) * scale + shift).astype(np.float32)
    big = max(np.linalg.norm(real.astype(np.float64), axis=1).max(), np.linalg.norm(fake.astype(np.float64), axis=1).max())
    return real, fake, torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), float(big)


@functools.lru_cache(maxsize=None)
def _ref_radii(shape, which, k):
    return S.knn_radii_spec(_pools(shape)[which], k)


def _hit_k(shape, which):
    return 1 if (shape, which) == ("D", 1) else 3             # the 4-row fake set of shape D admits only k < 4


# ------------------------------------------------------------------------------------------------- radii
@pytest.mark.parametrize("shape,which,k", [(s, w, k) for s in "ABC" for w in (0, 1) for k in (1, 3, 8)] + [("D", 0, 1), ("D", 0, 3)])
def test_knn_radii_against_the_spec(shape, which, k):
    d, big = SHAPES[shape][2], _pools(shape)[4]
    got = _ops().knn_radii(_pools(shape)[2 + which], k)
    ref = _ref_radii(shape, which, k)
    bound = 2 * (d + 2) * U * big ** 2
    err = np.abs(got - ref).max()
    print(f"radii {shape}{which} k={k}: max err {err:.3e}, bound {bound:.3e}, smallest radius {ref.min():.3e}")
    assert got.dtype == np.float64 and got.shape == ref.shape and err <= bound
    assert np.array_equal(_ops().knn_radii(_pools(shape)[which], k), got)          # a host pool: the same launch after an upload


# ------------------------------------------------------------------------------------------------- hits
@functools.lru_cache(maxsize=None)
def _hit_case(shape, direction):
    """direction 0: generated rows against the real balls (precision), 1: real rows against the generated balls (recall)
    -> reference hits, mask of the clear rows"""
    real, fake, _, _, big = _pools(shape)
    d = SHAPES[shape][2]
    a, b, bw = (fake, real, 0) if direction == 0 else (real, fake, 1)
    radii = _ref_radii(shape, bw, _hit_k(shape, bw))
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    d2 = np.maximum(0.0, (a64 ** 2).sum(1)[:, None] + (b64 ** 2).sum(1)[None, :] - 2.0 * a64 @ b64.T)
    margin = radii[None, :] - d2
    t = 16 * (d + 2) * U * big ** 2
    clear = (margin > t).any(1) | (margin < -t).all(1)
    return S.ball_hits_spec(a, b, radii), clear, radii


@pytest.mark.parametrize("direction", [0, 1], ids=["precision", "recall"])
@pytest.mark.parametrize("shape", list("ABCD"))
def test_ball_hits_against_the_spec_on_clear_rows(shape, direction):
    ref, clear, radii = _hit_case(shape, direction)
    _, _, real, fake, _ = _pools(shape)
    a, b = (fake, real) if direction == 0 else (real, fake)
    got = _ops().ball_hits(a, b, radii)
    share = 1.0 - clear.mean()
    print(f"hits {shape} {('precision', 'recall')[direction]}: reference {ref.mean():.3f}, device {got.mean():.3f}, "
          f"ambiguous rows {int((~clear).sum())} of {len(clear)}")
    assert share <= 0.08                                      # the condition under which the comparison below says something
    if shape != "D":
        assert 0.05 <= ref.mean() <= 0.95                     # both outcomes occur
    assert got.dtype == bool and np.array_equal(got[clear], ref[clear])


@pytest.mark.parametrize("shape", list("ABC"))
def test_precision_recall_through_the_operator_table(shape):
    real, fake = _pools(shape)[:2]
    ref = S.precision_recall_spec(fake, real, 3)
    got = S.precision_recall(fake, real, 3, ops=_ops())
    again = S.precision_recall(fake, real, 3, ops=_ops(), real_radii=_ops().knn_radii(real, 3))
    print(f"precision / recall {shape}: reference {ref[0]:.3f} / {ref[1]:.3f}, device {got[0]:.3f} / {got[1]:.3f}")
    for direction in (0, 1):
        assert abs(got[direction] - ref[direction]) <= 1.0 - _hit_case(shape, direction)[1].mean()
    assert again == got


# ------------------------------------------------------------------------------------------------- cubic sums
def _poly3_bounds(x, xi, y, yi):
    """the first-order worst-case bound of each of the three sums of every subset, from the float64 reference"""
    d = x.shape[1]
    out = np.empty((len(xi), 3))
    for s in range(len(xi)):
        xs, ys = x[xi[s]].astype(np.float64), y[yi[s]].astype(np.float64)
        nx, ny = np.linalg.norm(xs, axis=1), np.linalg.norm(ys, axis=1)

        def bound(u, v, nu, nv, same):
            b = 3.0 * (1.0 + np.abs(u @ v.T) / d) ** 2 * (d + 2) * U * nu[:, None] * nv[None, :] / d
            if same:
                np.fill_diagonal(b, 0.0)
            return b.sum()
        out[s] = bound(xs, xs, nx, nx, True), bound(ys, ys, ny, ny, True), bound(xs, ys, nx, ny, False)
    return out


@pytest.mark.parametrize("shape,msub,same", [("B", 2, False), ("B", 130, False), ("B", 257, True), ("A", 320, False)])
def test_poly3_sums_against_the_spec(shape, msub, same):
    real, fake, dreal, dfake, _ = _pools(shape)
    x, y, dx, dy = (real, real, dreal, dreal) if same else (real, fake, dreal, dfake)        # same: x and y are ONE buffer
    r = np.random.default_rng(msub)
    xi = np.stack([r.permutation(len(x))[:msub] for _ in range(3)]).astype(np.int32)        # non-contiguous rows
    yi = np.stack([r.permutation(len(y))[:msub] for _ in range(3)]).astype(np.int32)
    ref = S.poly3_sums_spec(x, xi, y, yi)
    got = _ops().poly3_sums(dx, xi, dy, yi)
    bound = _poly3_bounds(x, xi, y, yi)
    print(f"poly3 {shape} msub={msub}: max err / bound {np.max(np.abs(got - ref) / bound):.3f}, rel err {np.max(np.abs(got - ref) / ref):.2e}")
    assert got.shape == (3, 3) and got.dtype == np.float64 and np.all(np.abs(got - ref) <= bound)
    with pytest.raises(ValueError):                            # validated on the host copy before anything is launched
        _ops().poly3_sums(dx, xi + len(x), dy, yi)


def test_kid_through_the_operator_table():
    real, fake = _pools("B")[:2]
    gi, ri = S.kid_subsets(len(fake), len(real), 3, 1000, 5)
    m = gi.shape[1]
    assert m == 130
    b = _poly3_bounds(fake, gi, real, ri)
    bound = float(np.mean(b[:, 0] / (m * (m - 1)) + b[:, 1] / (m * (m - 1)) + 2.0 * b[:, 2] / (m * m)))
    ref = S.kid(fake, real, 3, 1000, 5)
    got = S.kid(fake, real, 3, 1000, 5, ops=_ops())
    print(f"kid B: reference {ref[0]:.6e}, device {got[0]:.6e}, bound {bound:.3e}")
    assert abs(got[0] - ref[0]) <= bound


# ------------------------------------------------------------------------------------------------- determinism, bounds, domain
def _launch_all(real, fake, k=3):
    """every entry point once on device pools -> device outputs"""
    ops = _ops()
    n, m = real.shape[0], fake.shape[0]
    radii = ops.knn_radii(real, k, out=torch.empty((n,), dtype=torch.float64, device="cuda"))
    hit = ops.ball_hits(fake, real, radii, out=torch.empty((m,), dtype=torch.uint8, device="cuda"))
    r = np.random.default_rng(0)
    xi = np.stack([r.permutation(n)[:m] for _ in range(3)]).astype(np.int32)
    yi = np.stack([r.permutation(m) for _ in range(3)]).astype(np.int32)
    sums = ops.poly3_sums(real, xi, fake, yi, out=torch.empty((3, 3), dtype=torch.float64, device="cuda"))
    return radii, hit, sums


@pytest.mark.parametrize("shape", ["B", "C"])
def test_two_launches_are_bit_identical(shape):
    _, _, real, fake, _ = _pools(shape)
    first, second = _launch_all(real, fake), _launch_all(real, fake)
    for a, b in zip(first, second):
        assert torch.equal(a, b)                               # (no NaN in any of them: NaN != NaN would fail here)


def test_every_entry_point_stays_inside_its_buffers():
    """shape C between guard bands of 0xFF bytes at the weakest alignment the header admits: no band byte changes, and the results
    are those of the unguarded launches"""
    from tests.guard import Guard, guarded
    real, fake, dreal, dfake, _ = _pools("C")
    want = _launch_all(dreal, dfake)
    g = Guard("cuda", skew=16)
    with guarded(g):
        got = _launch_all(torch.from_numpy(real).to("cuda"), torch.from_numpy(fake).to("cuda"))
        assert not g.fallthrough, g.fallthrough
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert g.served >= 2 + 3 + 3 + 2                           # pools, outputs, workspaces, index arrays
    g.check()


def test_outside_the_domain_nothing_is_launched():
    from xmcgan_image_generation_amd import _lib
    lib, ops = _lib.load(), _ops()
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    n, m, d = 40, 36, 64
    x = torch.rand((n, d), device="cuda")
    y = torch.rand((m, d), device="cuda")
    x48 = torch.rand((n, 48), device="cuda")
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")
    radii = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    hit = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    sums = torch.full((2, 3), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.arange(0, 2 * 8, dtype=torch.int32, device="cuda") % 8
    st = ops._stream()
    bad = [
        lib.xmc_knn_radii(p(x48), n, 48, 3, p(radii), p(ws), st),
        lib.xmc_knn_radii(p(x), n, d, 0, p(radii), p(ws), st),
        lib.xmc_knn_radii(p(x), n, d, n, p(radii), p(ws), st),
        lib.xmc_knn_radii(p(x), n, d, 9, p(radii), p(ws), st),
        lib.xmc_knn_radii(p(x), n, d, 3, None, p(ws), st),
        lib.xmc_ball_hits(p(x48), n, p(x48), p(radii), n, 48, p(hit), p(ws), st),
        lib.xmc_ball_hits(p(x), n, p(y), p(radii), m, d, None, p(ws), st),
        lib.xmc_poly3_sums(p(x48), n, p(idx), p(x48), n, p(idx), 2, 8, 48, p(sums), p(ws), st),
        lib.xmc_poly3_sums(p(x), n, p(idx), p(y), m, p(idx), 2, 1, d, p(sums), p(ws), st),
        lib.xmc_poly3_sums(p(x), n, p(idx), p(y), m, p(idx), 2, 8, d, None, p(ws), st),
    ]
    torch.cuda.synchronize()
    assert bad == [-22] * len(bad)                              # XMC_EINVAL
    assert bool((radii == -7.0).all()) and bool((hit == 0x5A).all()) and bool((sums == -7.0).all())
    assert lib.xmc_sample_metrics_ws_bytes(n, m, 48, 0) == -22 and lib.xmc_sample_metrics_ws_bytes(n, m, d, 0) == 8 * (n + m)
    assert lib.xmc_sample_metrics_ws_bytes(300, 300, d, 50) == 8 * 600          # 450 partials of 3 row blocks: the norms are larger
    assert lib.xmc_sample_metrics_ws_bytes(300, 300, d, 100) == 3 * 100 * 3 * 8
    with pytest.raises(_lib.XmcError):
        ops.knn_radii(x, n)
    # inside the domain the same buffers are written
    assert lib.xmc_knn_radii(p(x), n, d, 3, p(radii), p(ws), st) == 0
    radii_y = torch.full((m,), 10.0, dtype=torch.float64, device="cuda")
    assert lib.xmc_ball_hits(p(x), n, p(y), p(radii_y), m, d, p(hit), p(ws), st) == 0
    assert lib.xmc_poly3_sums(p(x), n, p(idx), p(y), m, p(idx), 2, 8, d, p(sums), p(ws), st) == 0
    torch.cuda.synchronize()
    assert bool((radii >= 0).all()) and bool((hit <= 1).all()) and bool((sums > 0).all())


# ------------------------------------------------------------------------------------------------- end to end
def test_eval_metric_extras_on_the_device_match_the_spec_on_the_same_pools():
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.utils import eval_metrics
    cfg = coco_xmc.get_test_config()
    cfg.update(eval_num=24, eval_batch_size=7, eval_avg_num=1, eval_extra_metrics=("kid", "precision_recall"), kid_subsets=4,
               kid_subset_size=16, pr_k=3)
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds_ = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, _, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, gp, gs, dp, ds_)

    def batches():
        data = [{k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.eval_batch_size, seed=s).items()}
                for s in range(100, 104)]
        while True:
            yield from data

    with pytest.warns(UserWarning, match="random Inception"):
        em = eval_metrics.EvalMetric(batches(), cfg, ops=_ops(), chunk=16)
    assert em.metric_ops is _ops() and S.has_device_path(em.metric_ops)
    old = em.calculate_inception_fid(gen, state, 1234)
    got = em.calculate_metrics(gen, state, 1234)
    assert tuple(got[k] for k in train_utils.EVAL_KEYS) == old
    assert set(got) == set(train_utils.EVAL_KEYS) | set(eval_metrics.extra_metric_keys(cfg.eval_extra_metrics))

    pool, _, ema_pool, _ = em._get_generated_pool_for_evaluation(gen, state, (0, 1234))
    real = em._pool
    assert pool.shape == real.shape == (24, 2048)
    d = 2048
    big = max(np.linalg.norm(a.astype(np.float64), axis=1).max() for a in (pool, ema_pool, real))
    t = 16 * (d + 2) * U * big ** 2
    gi, ri = S.kid_subsets(24, 24, 4, 16, np.random.SeedSequence([1234, 0, 0x4B4944]))
    for prefix, p in (("", pool), ("ema_", ema_pool)):
        b = _poly3_bounds(p, gi, real, ri)
        kid_bound = float(np.mean(b[:, 0] / (16 * 15) + b[:, 1] / (16 * 15) + 2.0 * b[:, 2] / 256))
        kid_ref = S.kid_from_sums(S.poly3_sums_spec(p, gi, real, ri), 16)[0]
        print(f"{prefix}kid: reference {kid_ref:.6e}, device {got[prefix + 'kid']:.6e}, bound {kid_bound:.3e}")
        assert abs(got[prefix + "kid"] - kid_ref) <= kid_bound and got[prefix + "kid_std"] == 0.0
        ref_p, ref_r = S.precision_recall_spec(p, real, 3)
        for name, ref, a, bb in (("precision", ref_p, p, real), ("recall", ref_r, real, p)):
            a64, b64 = a.astype(np.float64), bb.astype(np.float64)
            margin = S.knn_radii_spec(bb, 3)[None, :] - np.maximum(0.0, (a64 ** 2).sum(1)[:, None] + (b64 ** 2).sum(1)[None, :] - 2.0 * a64 @ b64.T)
            unclear = 1.0 - ((margin > t).any(1) | (margin < -t).all(1)).mean()
            print(f"{prefix}{name}: reference {ref:.3f}, device {got[prefix + name]:.3f}, ambiguous share {unclear:.3f}")
            assert abs(got[prefix + name] - ref) <= unclear + 1e-12 and got[prefix + name + "_std"] == 0.0
