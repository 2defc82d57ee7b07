"""config.train_statistics on the MI355X: ``xmc_segment_sumsq`` against float64 torch inside guard bands, and the statistics of a
whole step -- values against the oracle (tests/stats_reference.py), norms against the arenas the step left, the switch changing
nothing else, a captured graph accumulating what eager steps accumulate, and the bf16 mode at the C1 shapes."""
import ctypes as C

import pytest
import torch

from tests.guard import Guard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.float32)


# -------------------------------------------------------------------------------------------------------------- the kernel
LENGTHS = (0, 1, 63, 64, 65, 4097, 70001)        # none, one element, around a wave, a piece's half, 8.5 pieces (8192 each)


def _table():
    """segments in table order with ODD offsets (so no segment starts on a 16-byte boundary) and odd gaps between them"""
    segs, off = [], 3
    for n in LENGTHS:
        segs.append((off, n))
        off += n + (5 if (off + n) % 2 == 0 else 6)              # keeps the next offset odd
    assert all(o % 2 == 1 for o, _ in segs)
    return segs, off + 7


def _want(x, segs):
    xd = x.double()
    sums = [float((xd[o:o + n] * xd[o:o + n]).sum()) for o, n in segs]
    bad = [int((~torch.isfinite(x[o:o + n])).sum()) for o, n in segs]
    return sums, bad


def _run(ops, g, x_host, segs):
    flat = [v for s in segs for v in s]
    host = (C.c_int64 * len(flat))(*flat)
    nbytes = ops.segment_sumsq_ws_bytes(host, len(segs))
    x = g.place(x_host)
    table = g.place(torch.tensor(flat, dtype=torch.int64).view(-1, 2))
    sumsq, bad, ws = g.alloc((len(segs),), torch.float64), g.alloc((len(segs),), torch.int32), g.alloc((nbytes,), torch.uint8)
    ops.segment_sumsq(x, table, host, sumsq, bad, ws)
    first = (sumsq.cpu().clone(), bad.cpu().clone())
    sumsq.fill_(-1.0), bad.fill_(-1), ws.fill_(0x5A)              # a second run owes nothing to what the first left
    ops.segment_sumsq(x, table, host, sumsq, bad, ws)
    return first, (sumsq.cpu(), bad.cpu())


@pytest.mark.parametrize("skew", [0, 16])
def test_segment_sumsq_against_float64_inside_guard_bands(ops, skew):
    """counts exact; sums within 2 n 2^-53 relative per segment (the products are exact in float64, only the order of the n adds
    differs between the kernel and torch); a second run bit-identical; nothing outside the outputs and the workspace written,
    nothing outside the buffer read (the bands are NaN)"""
    segs, total = _table()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(total, generator=gen) * torch.logspace(-3, 3, total)
    nan_at, inf_at = segs[4][0] + 64, segs[6][0] + 8192 * 3 + 1          # the 65-element segment's last element; piece 3 of the longest
    x[nan_at], x[inf_at] = float("nan"), float("-inf")
    g = Guard("cuda", skew=skew)
    try:
        (sums, bad), (sums2, bad2) = _run(ops, g, x, segs)
    except Exception as e:
        if "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e):
            pytest.exit(f"GPU fault in xmc_segment_sumsq (skew {skew}): {e}", returncode=3)
        raise
    g.check()
    want_sums, want_bad = _want(x, segs)
    assert bad.tolist() == want_bad == [0, 0, 0, 0, 1, 0, 1]
    for i, (_, n) in enumerate(segs):
        got, want = float(sums[i]), want_sums[i]
        print(f"segment {i}: n = {n}, got {got!r}, want {want!r}")
        if want_bad[i]:
            assert got != got or got == float("inf")                    # NaN (inf * 0 never arises: -inf squared is +inf)
            assert (got != got) == (want != want)
        else:
            assert abs(got - want) <= 2 * n * 2.0 ** -53 * want
    assert float(sums[0]) == 0.0 and float(sums[1]) == float(x[segs[1][0]].double() ** 2)
    assert sums.numpy().tobytes() == sums2.numpy().tobytes() and torch.equal(bad, bad2)


def test_segment_sumsq_rejects_bad_arguments(ops):
    dev = ops.device
    x = torch.zeros(100, device=dev)
    out, bad, ws = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    table = torch.tensor([[0, 10], [90, 11]], dtype=torch.int64, device=dev)
    s = ops._stream()
    call = lambda host, n=100, wsb=64: ops.lib.xmc_segment_sumsq(x.data_ptr(), n, table.data_ptr(), host, 2, out.data_ptr(), bad.data_ptr(),
                                                                  ws.data_ptr(), wsb, s)
    assert call((C.c_int64 * 4)(0, 10, 90, 11)) == -22               # a segment ends behind the buffer
    assert call((C.c_int64 * 4)(-1, 10, 90, 10)) == -22
    assert call((C.c_int64 * 4)(0, 10, 90, 10), wsb=16) == -22       # two pieces need 32 bytes
    assert ops.lib.xmc_segment_sumsq_ws_bytes((C.c_int64 * 4)(0, 10, 90, -1), 2) == -22
    assert ops.lib.xmc_segment_sumsq_ws_bytes((C.c_int64 * 4)(0, 8193, 90, 0), 2) == 32
    torch.cuda.synchronize()
    assert not out.any() and not bad.any()


# ---------------------------------------------------------------------------------------------------------------- the step
def _fresh(ref, on, dtype="float32"):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = ref["cfg"].copy()
    cfg.dtype, cfg.train_statistics = dtype, on
    additional = xmc_gan.create_additional_data(cfg)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, ref["gp"], ref["gs"], ref["dp"], ref["ds"])
    return cfg, additional, gen, disc, state


def _one_step(ref, on):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg, additional, gen, disc, state = _fresh(ref, on)
    tb = {k: torch.as_tensor(v).cuda() for k, v in ref["batch"].items()}
    state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
    torch.cuda.synchronize()
    return additional, state, metrics


_STEP = {}


@pytest.fixture
def stepped(keep_grads):
    """ONE float32 step at C0, B = 4, statistics on, the gradient arenas kept (shared by the tests below)"""
    if not _STEP:
        from tests import stats_reference as SR
        ref = SR.reference(4)
        _STEP["v"] = (ref, *_one_step(ref, True))
    return _STEP["v"]


def test_step_values_match_the_oracle_fp32(stepped):
    """the CPU test's value checks at the float32 parity bar of tests/test_gpu_step.py: losses 1e-3, gradients 2.5e-3 (its bar for
    the generator's gradients; the discriminator's is 2e-3), post-step parameters 1e-3"""
    from tests import stats_reference as SR
    ref, additional, state, _ = stepped
    stats = additional["statistics"]
    got = dict(zip(stats.NAMES, stats.vec.double().cpu().tolist()))
    SR.check_values(got, ref, loss_tol=1e-3, grad_tol=2.5e-3, param_tol=1e-3)
    assert abs(got["d_grad_norm"] - ref["expect"]["d_grad_norm"]) <= 2e-3 * ref["expect"]["d_grad_norm"]
    assert 0 < got["d_sigma_min"] <= got["d_sigma_max"]
    window = stats.read()
    assert window["count"] == 1 and window["first_bad"] is None and all(v[2] == 0 for v in window["leaves"].values())


def test_step_accuracies_match_the_oracle_exactly_fp32(stepped):
    """equal to ``get_statistics`` of the oracle's ten matrices in float64, exactly, no row excluded, on the best of the scanned
    seeds (no seed separates every row's two largest entries by 1e-3 at C0: tests/stats_reference.py has the figures)"""
    from tests import stats_reference as SR
    ref, additional, _, _ = stepped
    stats = additional["statistics"]
    SR.check_accuracies(dict(zip(stats.NAMES, stats.vec.double().cpu().tolist())), ref)


def test_step_norms_match_the_arenas_the_step_left(stepped):
    """float32 mode, gradients kept: the gradient arenas after the step are what the updates consumed; per tensor and globally the
    kernel's sums equal float64 torch sums to 2 n 2^-53"""
    from xmcgan_image_generation_amd.train_statistics import arena_leaves
    _, additional, state, _ = stepped
    stats = additional["statistics"]
    window = stats.read()
    got = dict(zip(stats.NAMES, stats.vec.double().cpu().tolist()))
    for which, arena in (("d", state.d_optimizer.arena), ("g", state.g_optimizer.arena)):
        total, count = 0.0, 0
        grads = arena.grads.double().cpu()
        for p, off, n in arena_leaves(arena):
            want = float((grads[off:off + n] ** 2).sum())
            have = window["leaves"][f"{which}/{p}"][0]
            assert abs(have - want) <= 2 * n * 2.0 ** -53 * want, (which, p, have, want)
            total, count = total + want, count + n
        norm = total ** 0.5
        print(which, "grad norm", got[f"{which}_grad_norm"], "float64 over the arena", norm)
        assert abs(got[f"{which}_grad_norm"] - norm) <= (2.0 ** -24 + 2 * count * 2.0 ** -53) * norm       # stored as float32
        assert abs(float(grads.pow(2).sum()) - total) <= 1e-12 * total                                      # the arena's padding holds zeros


def test_on_and_off_are_bit_equal(stepped):
    from tests import stats_reference as SR
    from xmcgan_image_generation_amd import xmc_gan
    ref, _, state_on, metrics_on = stepped
    additional_off, state_off, metrics_off = _one_step(ref, False)
    assert "statistics" not in additional_off and set(metrics_on) == set(metrics_off) == set(xmc_gan.METRIC_KEYS)
    a, b = SR.snapshot(state_on, metrics_on), SR.snapshot(state_off, metrics_off)
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _window(stats):
    torch.cuda.synchronize()
    return {k: getattr(stats, k).cpu().clone() for k in ("sums", "info", "win_gsq", "win_psq", "win_bad", "vec")}


def _eager_then(ref, dtype, graph, n=3):
    """one eager step (lazy setup), the window zeroed, then n steps on n batches -- eager, or replays of one captured graph"""
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg, additional, gen, disc, state = _fresh(ref, True, dtype)
    b = cfg.batch_size
    bs = [{k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=b, rank=r).items()} for r in range(n + 1)]
    state, _ = train_utils.train_step(0, state, bs[0], xmc_gan, gen, disc, cfg, additional)
    stats = additional["statistics"]
    stats.reset()
    if graph:
        graphed = train_utils.GraphedTrainStep(state, bs[1], xmc_gan, gen, disc, cfg, additional)
        state = graphed.state
        assert int(stats.info.cpu()[0]) == 0                         # the capture executed nothing
        for tb in bs[1:]:
            state, _ = graphed(state, tb)
    else:
        for tb in bs[1:]:
            state, _ = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
    return _window(stats)


def test_three_replays_accumulate_what_three_eager_steps_accumulate():
    from tests import stats_reference as SR
    ref = SR.reference(4)
    eager, graph = _eager_then(ref, "float32", False), _eager_then(ref, "float32", True)
    assert eager["info"].tolist()[:2] == [3, 0]
    for k in eager:
        assert eager[k].numpy().tobytes() == graph[k].numpy().tobytes(), k


def test_bf16_at_the_c1_shapes():
    """C1 network (gf = df = 96, z = 128, 128 px), B = 8, bf16: every statistic finite, accuracies in [0, 1], and one replay of the
    captured step accumulates what one eager step does"""
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.train_statistics import TrainStatistics
    cfg = coco_xmc.get_c1_config()
    cfg.pretrained_image_contrastive = False
    cfg.batch_size = 8
    assert cfg.dtype == "bfloat16"
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    ref = dict(cfg=cfg, gp=gp, gs=gs, dp=dp, ds=ds)
    eager, graph = _eager_then(ref, "bfloat16", False, n=1), _eager_then(ref, "bfloat16", True, n=1)
    vec = dict(zip(TrainStatistics.NAMES, eager["vec"].tolist()))
    print(vec)
    assert bool(torch.isfinite(eager["vec"]).all()) and bool(torch.isfinite(eager["win_gsq"]).all()) and not eager["win_bad"].any()
    assert all(0.0 <= v <= 1.0 for k, v in vec.items() if k.endswith("_acc") or k.endswith("_frac"))
    assert vec["d_grad_norm"] > 0 and vec["g_grad_norm"] > 0 and vec["d_param_norm"] > 0 and 0 < vec["d_sigma_min"] <= vec["d_sigma_max"]
    for k in eager:
        assert eager[k].numpy().tobytes() == graph[k].numpy().tobytes(), k
