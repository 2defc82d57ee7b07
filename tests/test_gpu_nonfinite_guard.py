"""config.skip_nonfinite_updates on the MI355X: ``xmc_nonfinite_verdict`` against NumPy's ``~isfinite``, every guarded entry point
against its unguarded form (verdict 0: the same bits; verdict 1: nothing but the gradient's zeroing), the three state properties
of tests/test_nonfinite_guard.py on ``HipOps`` in float32 and bfloat16 (with and without the optimiser emitting the prepared
weights), and ``GraphedTrainStep`` replaying clean, poisoned, clean against the same steps run eagerly.

The poison is always a VALUE in an input tensor (``z[row, 0] = NaN`` or one ``image`` pixel = +inf).  The case-running bodies
(``body_*``) are also what tests/test_gpu_nonfinite_guard_bands.py runs inside the guard-band allocator."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_fused_opt as FO
from tests.cpu_ops_guard import assert_same, counters, leaves, poison

pytestmark = pytest.mark.gpu

CHUNK = 4 * 256 * 8                          # NFG_CHUNK: elements per workgroup trip of the scan kernel
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK + 1]
BAD = {"nan": np.float32("nan"), "+inf": np.float32("inf"), "-inf": np.float32("-inf")}


def _ops(dtype=torch.float32):
    from xmcgan_image_generation_amd.ops import HipOps
    return HipOps(dtype=dtype)


def _guard_buffers():
    verdict = torch.zeros((4,), dtype=torch.int32).cuda()
    cnt = torch.zeros((4,), dtype=torch.int32).cuda()
    return verdict, cnt


def _verdict_of(ops, arrays, verdict, cnt):
    segs = [torch.from_numpy(a).cuda() for a in arrays]
    ws = torch.empty((ops.nonfinite_verdict_ws_bytes([a.size for a in arrays]),), dtype=torch.uint8, device="cuda")
    ops.nonfinite_verdict(segs, verdict, cnt, ws)
    first = verdict.cpu().tolist()
    ops.nonfinite_verdict(segs, verdict, cnt, ws)                      # two launches: the same bits
    assert verdict.cpu().tolist() == first
    return first


def _want(arrays):
    bad = [int((~np.isfinite(a)).sum()) for a in arrays]
    return [int(sum(bad) > 0), sum(bad), next((i for i, k in enumerate(bad) if k), -1), 0]


def _benign(n, rng):
    """finite values only, with every pattern that must NOT count: denormals, the largest finite magnitudes, -0.0"""
    a = rng.standard_normal(n).astype(np.float32)
    special = np.array([0x00000001, 0x807fffff, 0x7f7fffff, 0xff7fffff, 0x80000000, 0x00000000], dtype=np.uint32).view(np.float32)
    a[:min(n, 6)] = special[:min(n, 6)]
    if n > 16:
        a[-6:] = special
    return a


def body_verdict(kind):
    """every size of SIZES in two- and three-segment tables; ``kind`` = None: benign buffers only; else one bad value at the first
    element, the last element and in the scalar tail of one segment.  Also the counters' arithmetic over the whole sequence."""
    ops = _ops()
    rng = np.random.default_rng(7)
    verdict, cnt = _guard_buffers()
    total = run = longest = 0
    for i, n0 in enumerate(SIZES):
        sizes = [n0, SIZES[(i + 5) % len(SIZES)], SIZES[(i + 9) % len(SIZES)]][:2 + i % 2]
        for target in range(len(sizes)):
            n = sizes[target]
            spots = [None] if kind is None else sorted({0, n - 1, (n // 4) * 4 if n % 4 else n - 1}) if n else []
            for at in spots:
                arrays = [_benign(k, rng) for k in sizes]
                if at is not None:
                    arrays[target][at] = BAD[kind]
                want = _want(arrays)
                got = _verdict_of(ops, arrays, verdict, cnt)
                assert got == want, (sizes, target, at, got, want)
                for _ in range(2):                                     # (_verdict_of launches twice)
                    if want[0]:
                        total, run = total + 1, run + 1
                        longest = max(longest, run)
                    else:
                        run = 0
        if kind is not None and i % 4 == 3:                            # a clean verdict in between resets the run
            assert _verdict_of(ops, [_benign(7, rng)], verdict, cnt) == [0, 0, -1, 0]
            run = 0
    assert cnt.cpu().tolist() == [total, run, longest, 0]
    assert (total > 0) == (kind is not None)


@pytest.mark.parametrize("kind", [None, "nan", "+inf", "-inf"], ids=["benign", "nan", "+inf", "-inf"])
def test_verdict_kernel_against_numpy(kind):
    body_verdict(kind)


def body_verdict_many_chunks():
    """more chunks than workgroups (the round-robin wraps) and several bad values in several segments: count, first segment"""
    ops = _ops()
    rng = np.random.default_rng(11)
    verdict, cnt = _guard_buffers()
    big = 1024 * CHUNK + CHUNK + 5
    arrays = [rng.standard_normal(big).astype(np.float32), _benign(0, rng), rng.standard_normal(3 * CHUNK + 2).astype(np.float32)]
    assert _verdict_of(ops, arrays, verdict, cnt) == [0, 0, -1, 0]
    arrays[2][[0, CHUNK, 3 * CHUNK + 1]] = BAD["nan"]
    assert _verdict_of(ops, arrays, verdict, cnt) == [1, 3, 2, 0]
    arrays[0][[big - 1, 1024 * CHUNK, 17]] = [BAD["+inf"], BAD["-inf"], BAD["nan"]]
    assert _verdict_of(ops, arrays, verdict, cnt) == [1, 6, 0, 0]
    assert cnt.cpu().tolist() == [4, 4, 4, 0]


def test_verdict_kernel_more_chunks_than_workgroups():
    body_verdict_many_chunks()


def test_verdict_rejects_bad_arguments():
    ops = _ops()
    verdict, cnt = _guard_buffers()
    x = torch.zeros((64,), dtype=torch.float32).cuda()
    ws = torch.empty((64,), dtype=torch.uint8, device="cuda")
    s = ops._stream()
    call = lambda ptrs, ns, k, wsb=64: ops.lib.xmc_nonfinite_verdict((C.c_void_p * len(ptrs))(*ptrs), (C.c_int64 * len(ns))(*ns), k,
                                                                      verdict.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, s)
    assert call([x.data_ptr()], [64], 1) == 0
    assert call([x.data_ptr() + 4], [8], 1) == -22                     # a base that is not 16-byte aligned
    assert call([x.data_ptr()], [-1], 1) == -22
    assert call([x.data_ptr()] * 9, [1] * 9, 9) == -22
    assert call([x.data_ptr()], [64], 0) == -22
    assert call([None], [4], 1) == -22 and call([None], [0], 1) == 0   # a null pointer only with n = 0
    assert call([x.data_ptr()], [64], 1, wsb=8) == -22                 # a workspace below the query's answer
    assert ops.lib.xmc_nonfinite_verdict_workspace_bytes((C.c_int64 * 2)(3 * CHUNK + 1, 0), 2) == 16 * 4
    assert ops.lib.xmc_nonfinite_verdict_workspace_bytes((C.c_int64 * 1)(0), 1) == 16
    assert ops.lib.xmc_nonfinite_verdict_workspace_bytes((C.c_int64 * 1)(-1), 1) == -22
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]                          # refused calls launched nothing


# ------------------------------------------------------------------------------------------------------ guarded entry points
def _verdicts():
    good = torch.zeros((4,), dtype=torch.int32).cuda()
    bad = torch.tensor([1, 3, 0, 0], dtype=torch.int32).cuda()
    return good, bad


def _arena(n, seed, ema=True):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn((n,), generator=g).cuda()
    gr = (torch.randn((n,), generator=g) * 1e-2).cuda()
    m = (torch.randn((n,), generator=g) * 1e-3).cuda()
    v = (torch.rand((n,), generator=g) * 1e-4 + 1e-8).cuda()
    e = torch.randn((n,), generator=g).cuda() if ema else None
    step = torch.zeros((4,), dtype=torch.float32).cuda()
    return [p, gr, m, v, e, step]


def _copy(ts):
    out = []
    for t in ts:
        if t is None:
            out.append(None)
        else:
            c = torch.empty(t.shape, dtype=t.dtype, device=t.device)
            c.copy_(t)
            out.append(c)
    return out


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (what, i)


def body_adam_dev(n):
    """xmc_adam_ema_dev_guarded and xmc_adam_ema_dev_sn_guarded (no spectral table; zero_grads on and off) on an arena of n elements"""
    ops = _ops()
    good, bad = _verdicts()
    kw = dict(lr=2e-4, beta1=0.5, beta2=0.999, grad_scale=0.5, ema_decay=0.999)
    for form, extra in (("dev", {}), ("sn", dict(zero_grads=True)), ("sn", dict(zero_grads=False))):
        fn = ops.adam_ema_dev if form == "dev" else ops.adam_ema_dev_sn
        start = _arena(n, n)
        ref, ok, skip = _copy(start), _copy(start), _copy(start)
        for _ in range(2):                               # two updates: the second one reads an advanced counter
            fn(*ref, **kw, **extra)
            fn(*ok, **kw, **extra, verdict=good)
            fn(*skip, **kw, **extra, verdict=bad)
        _same(ok, ref, (form, extra, "verdict 0"))
        assert int(ref[5].view(torch.int32)[0]) == 2 and not torch.equal(ref[0], start[0])
        for i in (0, 2, 3, 4, 5):                        # p, m, v, ema, step_state untouched
            _same([skip[i]], [start[i]], (form, extra, "verdict 1", i))
        _same([skip[1]], [ref[1]], (form, extra, "gradient"))      # zeroed exactly where the unguarded form zeroes it
        if extra.get("zero_grads"):
            assert not ref[1].any()


@pytest.mark.parametrize("n", [4099, 4096, 3, 1023 * 5 + 2])
def test_guarded_flat_adam(n):
    body_adam_dev(n)


def body_adam_sn_and_tiles(zero_grads):
    """a small discriminator's arena: xmc_adam_ema_dev_sn_guarded with the sigma term and the skip map, then
    xmc_adam_wprep_tiles_guarded -- outputs, emitted copies and partial rows"""
    cfg, gen, disc, state = FO._small_d()
    d = disc(train=True)
    ops = d.ops
    params, sn = state.d_optimizer.target, state.discriminator_state["spectral_norm_stats"]
    arena = d._bind(params)
    d.prepare(params, sn)
    _, u_new, v, scal = d._sn_ctx[:4]
    good, bad = _verdicts()
    skipmap = ops.wprep_skip_map(d.wp, arena.size, base=d.sn_map)
    assert int((skipmap == -2).sum()) > 0
    g = torch.Generator().manual_seed(5)
    n = arena.size
    start = [arena.params, (torch.randn((n,), generator=g) * 1e-3).cuda(), (torch.randn((n,), generator=g) * 1e-4).cuda(),
             (torch.rand((n,), generator=g) * 1e-6 + 1e-9).cuda(), torch.randn((n,), generator=g).cuda(),
             torch.zeros((4,), dtype=torch.float32).cuda()]
    kw = dict(lr=1e-3, beta1=0.5, beta2=0.999, ema_decay=0.99, zero_grads=zero_grads)
    res = {}
    for mode, vd in (("ref", None), ("ok", good), ("skip", bad)):
        t = _copy(start)
        out = ops.wprep_alloc(d.wp)
        for b in list(out[0]) + [out[1]]:
            if b is not None:
                b.fill_(3.0)                             # a skipped launch must leave the prepared copies as they were
        gk = {} if vd is None else dict(verdict=vd)
        kvec = ops.sn_bank_dot(d.bank, t[0], t[1], scal)
        ops.adam_ema_dev_sn(*t, **kw, fix=(skipmap, d.bank, kvec, scal, u_new, v), **gk)
        ops.adam_wprep(d.wp, out, *t, **kw, fix=(kvec, scal, u_new, v), **gk)
        res[mode] = (t, [b for b in out[0] if b is not None] + [out[1]])
    _same(res["ok"][0], res["ref"][0], "verdict 0")
    _same(res["ok"][1], res["ref"][1], "verdict 0, prepared copies")
    assert not torch.equal(res["ref"][0][0], start[0]) and int(res["ref"][0][5].view(torch.int32)[0]) == 1
    for i in (0, 2, 3, 4, 5):
        _same([res["skip"][0][i]], [start[i]], ("verdict 1", i))
    for b in res["skip"][1]:
        assert bool((b.float() == 3.0).all()), "a skipped launch wrote a prepared copy"
    _same([res["skip"][0][1]], [res["ref"][0][1]], "gradient")
    assert bool(res["ref"][0][1].any()) != bool(zero_grads)


@pytest.mark.parametrize("zero_grads", [True, False], ids=["zeroing", "first-write"])
def test_guarded_sigma_adam_and_tiles(zero_grads):
    body_adam_sn_and_tiles(zero_grads)


def body_commit_and_metrics():
    ops = _ops()
    good, bad = _verdicts()
    for n in (1, 3, 4, 5, 255, 4099):
        for skew in (0, 1):                              # skew 1: a 4-byte aligned pair (the scalar kernel)
            src_b, dst_b = torch.randn((n + 1,)).cuda(), torch.zeros((n + 1,), dtype=torch.float32).cuda()
            src, dst = src_b[skew:skew + n], dst_b[skew:skew + n]
            ops.commit_if(dst, src, bad)
            assert not dst_b.any(), (n, skew)
            ops.commit_if(dst, src, good)
            assert torch.equal(dst, src) and float(dst_b[n * (1 - skew)]) == 0.0, (n, skew)
    vals = [torch.full((1,), float(i) + 0.25).cuda() for i in range(5)]
    sums, info = torch.zeros((5,), dtype=torch.float64).cuda(), torch.zeros((2,), dtype=torch.int32).cuda()
    rs, ri = torch.zeros((5,), dtype=torch.float64).cuda(), torch.zeros((2,), dtype=torch.int32).cuda()
    ops.metrics_accum_if(vals, sums, info, bad)
    assert not sums.any() and not info.any()             # a skipped half step adds nothing and is not a call
    vals[2].fill_(float("nan"))
    ops.metrics_accum_if(vals, sums, info, bad)
    assert not sums.any() and not info.any()
    vals[2].fill_(2.25)
    for _ in range(3):
        ops.metrics_accum_if(vals, sums, info, good)
        ops.metrics_accum(vals, rs, ri)
    assert torch.equal(sums, rs) and torch.equal(info, ri) and info.cpu().tolist() == [3, 0]


def test_commit_if_and_metrics_accum_if():
    body_commit_and_metrics()


def test_abi_version_is_36():
    from xmcgan_image_generation_amd import _lib
    assert _lib.load().xmc_abi_version() == _lib.ABI_VERSION == 36


# ---------------------------------------------------------------------------------------------- the state tests on HipOps
MODES = ["float32", "bfloat16", "bfloat16-fuse_prep"]


def _cfg(mode, **kw):
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.dtype = mode.split("-")[0]
    cfg.batch_size = 2
    cfg.skip_nonfinite_updates = True
    cfg.update(kw)
    return cfg


def _batch(cfg, seed):
    from xmcgan_image_generation_amd import synthetic as syn
    return {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size, seed=seed).items()}


def _warm(cfg, mode):
    """state S: one clean step from the seed-3 initialisation; bfloat16 runs the product optimiser mode (fuse_opt, first-write
    arenas), ``-fuse_prep`` also lets the optimiser kernel emit the prepared weights"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    gen, disc, state = train_utils.create_train_state(cfg, 3)
    ops = gen(train=True).ops
    if cfg.dtype == "bfloat16":
        assert ops.fuse_opt and ops.first_write and state.d_optimizer.arena.first_write
        ops.fuse_prep = mode.endswith("fuse_prep")
    state, _ = train_utils.train_step(1, state, _batch(cfg, 1), xmc_gan, gen, disc, cfg, {})
    return gen, disc, state


def _step(state, batch, gen, disc, cfg, rng=9):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    return train_utils.train_step(rng, state, batch, xmc_gan, gen, disc, cfg, {})


@pytest.mark.parametrize("how", ["z", "image"])
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_step_leaves_state_intact(mode, how):
    cfg = _cfg(mode)
    gen, disc, state = _warm(cfg, mode)
    before, step = leaves(state), int(state.step)
    state, _ = _step(state, poison(_batch(cfg, 9), cfg, (0, 1), how), gen, disc, cfg)
    assert_same(leaves(state), before)
    assert int(state.step) == step + 1 and counters(state) == [2, 2, 2]
    if how == "z":                                       # the same step with the switch off ends with non-finite parameters
        off = _cfg(mode, skip_nonfinite_updates=False)
        gen, disc, state = _warm(off, mode)
        state, _ = _step(state, poison(_batch(off, 9), off, (0, 1), how), gen, disc, off)
        assert not (bool(torch.isfinite(state.g_optimizer.arena.params).all()) and bool(torch.isfinite(state.d_optimizer.arena.params).all()))


@pytest.mark.parametrize("how", ["z", "image"])
@pytest.mark.parametrize("mode", MODES)
def test_clean_step_after_skip_equals_clean_step(mode, how):
    cfg = _cfg(mode)
    x = _batch(cfg, 11)
    gen, disc, a = _warm(cfg, mode)
    a, _ = _step(a, poison(_batch(cfg, 9), cfg, (0, 1), how), gen, disc, cfg)
    a, ma = _step(a, x, gen, disc, cfg, rng=10)
    gen_b, disc_b, b = _warm(cfg, mode)                  # S again: the same seed, the same clean step
    b, mb = _step(b, x, gen_b, disc_b, cfg, rng=10)
    assert_same(leaves(a), leaves(b))
    for k in ma:
        assert np.float32(float(ma[k])).tobytes() == np.float32(float(mb[k])).tobytes(), k
    assert int(a.step) == int(b.step) + 1 and counters(a) == [2, 0, 2] and counters(b) == [0, 0, 0]


@pytest.mark.parametrize("how", ["z", "image"])
@pytest.mark.parametrize("mode", MODES)
def test_only_the_bad_half_is_skipped(mode, how):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(mode)
    batch = _batch(cfg, 9)
    gen, disc, state = _warm(cfg, mode)
    before = leaves(state)
    state, _ = _step(state, poison(batch, cfg, (1,), how), gen, disc, cfg)
    got = leaves(state)
    gen_b, disc_b, ref = _warm(cfg, mode)
    first_half = train_utils.split_input_dict(batch, cfg.d_step_per_g_step)[0]
    ref = xmc_gan.train_d(9 * cfg.d_step_per_g_step, ref, first_half, gen_b, disc_b, cfg)
    want = leaves(ref)
    for k in want:
        if k.startswith("d/") or k.startswith("sn/"):
            assert np.array_equal(got[k], want[k]), k
        else:
            assert np.array_equal(got[k], before[k]), k
    assert not np.array_equal(got["d/params"], before["d/params"]) and int(got["d/t"]) == int(before["d/t"]) + 1
    assert counters(state) == [1, 1, 1]


@pytest.mark.parametrize("mode", MODES)
def test_switch_on_with_clean_data_is_bit_equal_to_switch_off(mode):
    runs = []
    for on in (False, True):
        cfg = _cfg(mode, skip_nonfinite_updates=on)
        gen, disc, state = _warm(cfg, mode)
        ms = []
        for s in (2, 3):
            state, m = _step(state, _batch(cfg, s), gen, disc, cfg, rng=s)
            ms.append({k: np.float32(float(v)).tobytes() for k, v in m.items()})
        runs.append((leaves(state), ms))
    assert_same(runs[1][0], runs[0][0])
    assert runs[1][1] == runs[0][1]


# ------------------------------------------------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("mode", ["float32", "bfloat16"])
def test_graph_replays_clean_poisoned_clean_like_the_eager_steps(mode):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(mode)
    batches = [_batch(cfg, 2), poison(_batch(cfg, 3), cfg, (0, 1)), _batch(cfg, 4)]
    gen, disc, eager = _warm(cfg, mode)
    em = []
    for tb in batches:
        eager, m = _step(eager, tb, gen, disc, cfg, rng=0)
        em.append({k: np.float32(float(v)).tobytes() for k, v in m.items()})
    gen2, disc2, st = _warm(cfg, mode)
    ops = gen2(train=True).ops
    acc = train_utils.MetricAccumulator(xmc_gan.metric_keys(cfg), ops)
    graphed = train_utils.GraphedTrainStep(st, batches[0], xmc_gan, gen2, disc2, cfg, {}, accumulator=acc)
    st = graphed.state
    assert counters(st) == [0, 0, 0]                     # the capture executed nothing
    kept = []
    for tb in batches:                                   # no host read between the replays: the metrics are cloned on the device
        st, m = graphed(st, tb)
        kept.append({k: v.clone() for k, v in m.items()})
    assert counters(st) == [2, 0, 2]
    assert_same(leaves(st), leaves(eager))
    for i in (0, 2):
        assert {k: np.float32(float(v)).tobytes() for k, v in kept[i].items()} == em[i], i
    sums, count, first_bad = acc.read()
    assert count == 2 and first_bad == 0 and all(np.isfinite(v) for v in sums.values())
    assert st.g_optimizer.arena.opt_step == 3 and st.d_optimizer.arena.opt_step == 6      # leaves() synchronised the mirrors
    assert int(st.step) == int(eager.step) == 4


# ----------------------------------------------------------------------------------------------------------- the loop
def test_train_survives_a_poisoned_batch_inside_the_replayed_graph(tmp_path):
    """``train`` on HipOps (bf16): step 1 eager, steps 2 .. 5 replay the captured graph; the batch of step 3 is poisoned.  The run
    finishes, the window that holds step 3 reports its two skipped half steps and finite means, the checkpoint carries Adam's t =
    the applied updates and the counters; with every batch poisoned and nonfinite_max_consecutive = 2 the run stops"""
    import json
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.utils import checkpoint, task_manager

    def datasets(poisoned):
        def hook(config, data_rng, start_step, rank, world, device):
            def batches():
                s = start_step
                while True:
                    b = _batch(config, s)
                    yield poison(b, config, (0, 1)) if (poisoned == "all" or s in poisoned) else b
                    s += 1
            return batches(), iter(()), 1000
        return hook
    cfg = _cfg("bfloat16", num_train_steps=5, checkpoint_every_steps=5, eval_every_steps=2, pretrained_image_contrastive=False)
    state = train_utils.train(cfg, str(tmp_path / "a"), datasets=datasets({3}))
    lines = [json.loads(l) for l in open(tmp_path / "a" / "metrics.jsonl")]
    assert [l["step"] for l in lines] == [2, 4, 5]
    assert [l["guard/skipped_half_steps"] for l in lines] == [0, 2, 0] and [l["guard/longest_run"] for l in lines] == [0, 2, 0]
    assert all(np.isfinite(v) for l in lines for v in l.values())
    assert int(state.step) == 5 and counters(state) == [2, 0, 0]
    (path,) = task_manager.list_checkpoints(str(tmp_path / "a" / "checkpoints-0"))
    _, _, fresh = train_utils.create_train_state(cfg, 99)
    fresh = checkpoint.restore(path, fresh)
    assert fresh.g_optimizer.arena.opt_step == 4 and fresh.d_optimizer.arena.opt_step == 8 and counters(fresh) == [2, 0, 0]
    assert bool(torch.isfinite(fresh.g_optimizer.arena.params).all()) and bool(torch.isfinite(fresh.d_optimizer.arena.params).all())
    cfg2 = _cfg("bfloat16", num_train_steps=4, checkpoint_every_steps=100, eval_every_steps=2, nonfinite_max_consecutive=2,
                pretrained_image_contrastive=False)
    with pytest.raises(FloatingPointError, match="consecutive half steps"):
        train_utils.train(cfg2, str(tmp_path / "b"), datasets=datasets("all"))
