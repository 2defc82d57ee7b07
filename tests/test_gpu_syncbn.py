"""Cross-replica BatchNorm groups at the kernel level (ops.bn_batch_sums / bn_finalize_rows / rows_mean and the ``reduce_s`` hook
of ops.cbn_act_bwd): a tensor is cut along its batch axis into G shards -- the replicas of one group, run one after the other
on the one GPU -- and statistics, running statistics and gradients are compared with float64 BatchNorm over the WHOLE tensor.

Geometries (n, h, c, hc) are those of tests/test_gpu_kernels.py::test_cbn (they select the different partial-row and cell
kernels) plus (3, 5, 24, 1): 25 pixels per sample -- fewer than 64 per shard -- and c no multiple of 16.  Gates and scales are
test_cbn's: 2e-4 of the scale for float32 outputs, ``_tol(dtype)`` for dx.

The bodies are ``run_*`` functions: tests/test_gpu_syncbn_guard.py runs them again inside the guard-band allocator."""
import pytest
import torch

from tests.test_gpu_kernels import DT, _close, _ops, _tol

pytestmark = pytest.mark.gpu

GEOS = [(3, 8, 16, 1), (2, 16, 24, 4), (2, 16, 40, 16), (4, 4, 1536, 1), (2, 32, 64, 4), (3, 5, 24, 1)]
FWD_CASES = [(geo, g) for geo in GEOS for g in (1, 2, 3) if geo[0] % g == 0]          # 3: no power-of-two assumption survives
# The backward cases: the conditional-affine kernels (xmc_cbn_act_bwd_cells / _dx) take power-of-two maps only (make_geo: h = 5 is
# XMC_EINVAL; every generator map is a power of two), so (3, 4, 24, 1) -- 16 pixels per sample -- stands where the forward list has
# (3, 5, 24, 1); and a batch of 3 has no two equal shards, so the n = 3 geometries run with G = 3 (bwd_groups), the others with G = 2.
BWD_GEOS = GEOS[:5] + [(3, 4, 24, 1)]
# the geometry on which the backward pass WITHOUT the exchange misses the dx gate (run_bwd_shards(exchange=False)): 32 pixels
# per shard, so the shards' own channel means s / P differ from the group's by ~ 1 / sqrt(32) of the cotangent's spread
POWER_GEO = (4, 4, 1536, 1)


def _ratio(got, ref, scale=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    s = float(ref.abs().max()) if scale is None else scale
    return float((got - ref).abs().max()) / max(s, 1e-6)


def _inputs(geo, dtype):
    n, h, c, hc = geo
    g = torch.Generator().manual_seed(9)
    x = (torch.randn((n, h, h, c), generator=g) * 2.0).to(dtype)
    gamma = torch.randn((n, hc, hc, c), generator=g) * 0.3
    beta = torch.randn((n, hc, hc, c), generator=g) * 0.3
    dy = torch.randn((n, h, h, c), generator=g).to(dtype)
    return x, gamma, beta, dy


def _group_stats(ops, shards, pixels_per_shard, c):
    rows = torch.empty((len(shards), 2 * c), dtype=torch.float32, device="cuda")
    for r, xs in enumerate(shards):
        rows[r].copy_(ops.bn_batch_sums(xs))
    rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
    mean, rstd = ops.bn_finalize_rows(rows, pixels_per_shard, rm, rv, True)
    return mean, rstd, rm, rv


def run_fwd_shards(geo, groups, dtype):
    """-> {output: worst error / scale}; asserts test_cbn's gates, bit-equality with bn_batch_stats for one shard, and
    bit-identical repeats."""
    n, h, c, hc = geo
    ops = _ops(dtype)
    x, _, _, _ = _inputs(geo, dtype)
    xr = x.double()
    m = n // groups
    shards = [x[r * m:(r + 1) * m].contiguous().cuda() for r in range(groups)]
    mean, rstd, rm, rv = _group_stats(ops, shards, m * h * h, c)
    m_ref = xr.mean((0, 1, 2))
    v_ref = (xr * xr).mean((0, 1, 2)) - m_ref ** 2
    checks = (("mean", mean, m_ref, float(xr.abs().max())), ("rstd", rstd, torch.rsqrt(v_ref + 1e-5), None),
              ("running mean", rm, 0.1 * m_ref, 1.0), ("running var", rv, 0.9 + 0.1 * v_ref, 4.0))
    out = {what: _ratio(got, ref, scale) for what, got, ref, scale in checks}
    print(f"syncbn fwd {geo} G={groups} {dtype}: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items()) + "  (gate 2e-4)")
    for what, got, ref, scale in checks:
        _close(got, ref, torch.float32, f"group {what} {geo} G={groups}", scale=scale)
    again = _group_stats(ops, shards, m * h * h, c)
    for a, b in zip((mean, rstd, rm, rv), again):
        assert torch.equal(a, b), "two runs differ"
    if groups == 1:
        rm1, rv1 = torch.zeros(c).cuda(), torch.ones(c).cuda()
        mean1, rstd1 = ops.bn_batch_stats(shards[0], rm1, rv1, True)
        for what, a, b in (("mean", mean, mean1), ("rstd", rstd, rstd1), ("running mean", rm, rm1), ("running var", rv, rv1)):
            assert torch.equal(a, b), f"one row: {what} differs from bn_batch_stats"
    return out


def bwd_groups(geo):
    """2 shards where the batch divides, else 3 (the n = 3 geometries): equal pixel counts per replica, as in a real group"""
    return 2 if geo[0] % 2 == 0 else 3


def run_bwd_shards(geo, dtype, exchange=True):
    """cbn_act_bwd per shard with the GROUP mean / rstd and reduce_s = rows_mean over the shards' channel sums, against float64
    autograd of relu(x_hat (gamma + 1) + beta) over the whole tensor.  ``exchange=False``: the same calls without reduce_s,
    nothing asserted.  -> {output: worst error / scale over the shards}."""
    n, h, c, hc = geo
    ops = _ops(dtype)
    groups = bwd_groups(geo)
    m = n // groups
    x, gamma, beta, dy = _inputs(geo, dtype)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m_ref = xr.mean((0, 1, 2))
    v_ref = (xr * xr).mean((0, 1, 2)) - m_ref ** 2
    f = h // hc
    up = lambda t: t.repeat_interleave(f, 1).repeat_interleave(f, 2)
    y_ref = torch.relu((xr - m_ref) * torch.rsqrt(v_ref + 1e-5) * (up(gr) + 1) + up(br))
    rx, rg, rb = torch.autograd.grad(y_ref, (xr, gr, br), dy.double())
    sl = [slice(r * m, (r + 1) * m) for r in range(groups)]
    xs = [x[s].contiguous().cuda() for s in sl]
    dys = [dy[s].contiguous().cuda() for s in sl]
    gbs = [torch.cat([gamma[s], beta[s]], dim=-1).contiguous().cuda() for s in sl]
    mean, rstd, _, _ = _group_stats(ops, xs, m * h * h, c)
    reduce_s = None
    if exchange:
        # the replicas run in lock-step: every shard's sums exist before any shard's dx.  First pass: collect them.
        rows = torch.empty((groups, 2 * c), dtype=torch.float32, device="cuda")
        for r in range(groups):
            ops.cbn_act_bwd(dys[r], xs[r], mean, rstd, gbs[r], hc, reduce_s=lambda s, r=r: (rows[r].copy_(s), s)[1])
        reduce_s = lambda s: ops.rows_mean(rows)
        one = ops.rows_mean(rows[:1])
        assert torch.equal(one, rows[0]), "rows_mean of one row is not the row"
    out = {"dx": 0.0, "dgamma": 0.0, "dbeta": 0.0}
    got = []
    for r in range(groups):
        kw = {"reduce_s": reduce_s} if exchange else {}
        dx, dgb = ops.cbn_act_bwd(dys[r], xs[r], mean, rstd, gbs[r], hc, **kw)
        got.append((dx, dgb))
        out["dx"] = max(out["dx"], _ratio(dx, rx[sl[r]]))
        out["dgamma"] = max(out["dgamma"], _ratio(dgb[..., :c], rg[sl[r]], float(rg.abs().max())))
        out["dbeta"] = max(out["dbeta"], _ratio(dgb[..., c:], rb[sl[r]], float(rb.abs().max())))
    print(f"syncbn bwd {geo} G={groups} {dtype} exchange={exchange}: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items())
          + f"  (gates: dx {_tol(dtype):.1e}, dgamma / dbeta 2e-4 x {1 if dtype == torch.float32 else 40})")
    if exchange:
        wide = 1 if dtype == torch.float32 else 40
        for r, (dx, dgb) in enumerate(got):
            _close(dx, rx[sl[r]], dtype, f"group dx {geo} shard {r}")
            _close(dgb[..., :c], rg[sl[r]], torch.float32, f"dgamma {geo} shard {r}", scale=float(rg.abs().max()) * wide)
            _close(dgb[..., c:], rb[sl[r]], torch.float32, f"dbeta {geo} shard {r}", scale=float(rb.abs().max()) * wide)
    return out


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geo,groups", FWD_CASES)
def test_forward_statistics_over_shards(geo, groups, dtype):
    run_fwd_shards(geo, groups, dtype)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geo", BWD_GEOS)
def test_backward_over_shards(geo, dtype):
    run_bwd_shards(geo, dtype)


@pytest.mark.parametrize("dtype", DT)
def test_backward_without_the_exchange_misses(dtype):
    """Power of test_backward_over_shards: with per-shard sums (no reduce_s) dx must MISS its gate on POWER_GEO -- an exchange
    that did nothing would leave exactly this."""
    out = run_bwd_shards(POWER_GEO, dtype, exchange=False)
    assert out["dx"] > _tol(dtype), (out, _tol(dtype))
