"""config.ada_target, config.lecam_weight and config.skip_nonfinite_updates with data-parallel replicas, without a GPU
(DESIGN.md 9f.3): the NumPy specifications of the three ``_rows`` kernels, ``GradSync.gather_rows`` and the refusals that stay,
and two gloo ranks on the CPU operator table (whose ``_rows`` ops are the specifications)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.cpu_ops import CpuOps
from xmcgan_image_generation_amd import dp
from xmcgan_image_generation_amd import synthetic as syn
from xmcgan_image_generation_amd import train_utils, xmc_gan
from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.libml import ada as ADA
from xmcgan_image_generation_amd.libml import diff_augment as DA
from xmcgan_image_generation_amd.libml import lecam as LC
from xmcgan_image_generation_amd.libml import nonfinite_guard as NG
from xmcgan_image_generation_amd.nets import xmc_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = "color,translation,cutout"
B = 2                                                 # the per-device batch
MIN_NORMAL32, MIN_NORMAL64 = float(np.finfo(np.float32).tiny), float(np.finfo(np.float64).tiny)


def _u64(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def _u32(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32).tolist()


def _hinge_dld(x, b, denom=None):
    """the gradient ``xmc_hinge`` writes for the logits [real; fake]: -+ 1 / denom where the hinge is active"""
    d = np.float32(b if denom is None else denom)
    return np.concatenate([-(1 - x[:b] > 0).astype(np.float32) / d, (1 + x[b:] > 0).astype(np.float32) / d])


# ------------------------------------------------------------------------------------------------- 1. the specifications at w = 1
@pytest.mark.parametrize("one_sided", [False, True])
@pytest.mark.parametrize("b", [1, 3, 257])
def test_lecam_step_rows_with_one_row_is_step(b, one_sided):
    """random states: warm-up by ticks, warm-up by updates, active; a clean batch and one with a non-finite logit"""
    rng = np.random.default_rng(31 * b + one_sided)
    for case, (ticks, updates) in enumerate([(0.0, 0.0), (5.0, 0.0), (1.0, 4.0), (6.0, 6.0), (9.0, 2.0)]):
        for bad in (None, np.nan, -np.inf):
            s = LC.initial_state()
            s[:5] = rng.standard_normal(), rng.standard_normal(), ticks, 0.25, updates
            s[5:] = 1.5, -2.5, 7.0
            x = (rng.standard_normal(2 * b) * 10.0 ** rng.uniform(-2, 2, 2 * b)).astype(np.float32)
            if bad is not None:
                x[int(rng.integers(2 * b))] = bad
            dld = _hinge_dld(x, b)
            want = LC.step(s, x, b, dld, 0.3, 0.9, 3, one_sided)
            got = LC.step_rows(s, x[None], 0, dld, 0.3, 0.9, 3, one_sided)
            assert _u64(got[0]) == _u64(want[0]) and _u32(got[1]) == _u32(want[1]) and _u32(got[2]) == _u32(want[2]), (case, bad)
            assert got[0][LC.TICKS] == ticks + 1 and (got[0][LC.UPDATES] == updates + (bad is None))


def test_ada_update_rows_with_one_row_is_update():
    rng = np.random.default_rng(5)
    for b in (1, 3, 257):
        s = ADA.initial_state()
        s[ADA.P] = 0.3
        for call in range(6):
            x = rng.standard_normal(2 * b).astype(np.float32)
            x[rng.integers(2 * b, size=3)] = [0.0, -0.0, np.nan]
            x[b:] = np.inf                            # the generated half is not read
            for interval in (1, 4):
                want = ADA.update(s, x[:b], 0.6, 50.0, interval, 0.8)
                assert _u64(ADA.update_rows(s, x[None], b, 0.6, 50.0, interval, 0.8)) == _u64(want)
            s = want
    with pytest.raises(ValueError):
        ADA.update_rows(s, np.zeros((2, 5), np.float32), 2, 0.6, 50.0, 1, 0.8)


def _torch_rule(verdicts):
    """the torch rule of the CPU operator table's ``nonfinite_verdict`` over a sequence of single-rank verdicts"""
    g, out = NG.NonfiniteGuard(torch.device("cpu")), []
    for bad_count, first in verdicts:
        seg = torch.ones(max(bad_count, 1))
        seg[:bad_count] = float("nan")
        segments = [torch.ones(2)] * first + [seg] if bad_count else [torch.ones(2)]
        out.append((g.judge(CpuOps(), segments).tolist(), g.counters.tolist()))
    return out


def test_merge_rows_with_one_row_is_the_torch_verdict_rule():
    seq = [(2, 1), (1, 0), (0, 0), (5, 3), (0, 0)]
    counters = [0, 0, 0, 0]
    for (bad, first), (v_want, c_want) in zip(seq, _torch_rule(seq)):
        row = [int(bad > 0), bad, first if bad else -1, 0]
        verdict, counters = NG.merge_rows([row], counters)
        assert verdict == v_want == row and counters == c_want
    assert NG.merge_rows([[1, 3, 2, 0]], [2147483647, 2147483647, 5, 9])[1] == [2147483647, 2147483647, 2147483647, 9]


def test_merge_rows_takes_the_lowest_bad_rank_and_saturates():
    clean, c0 = [0, 0, -1, 0], [4, 2, 3, 0]
    assert NG.merge_rows([clean] * 3, c0) == ([0, 0, -1, 0], [4, 0, 3, 0])
    assert NG.merge_rows([clean, [1, 7, 2, 0], [1, 1, 0, 0]], c0) == ([1, 8, 2, 1], [5, 3, 3, 0])
    assert NG.merge_rows([[1, 2147483647, 1, 0], clean, [1, 5, 3, 0]], c0) == ([1, 2147483647, 1, 0], [5, 3, 3, 0])
    with pytest.raises(ValueError):
        NG.merge_rows(np.zeros((0, 4), np.int32), c0)


# ------------------------------------------------------------------------------------------------------- 2. LeCam at w = 2, b = 3
def _two_ranks(bad=None):
    rng = np.random.default_rng(17)
    rows = rng.uniform(-2.0, 2.0, (2, 6)).astype(np.float32)
    if bad is not None:
        rows[1, 4] = bad
    return rows


@pytest.mark.parametrize("one_sided", [False, True])
def test_lecam_two_ranks_are_the_concatenated_batch(one_sided):
    """both ranks write the same state and the same R -- those of ``step`` on [real0; real1; fake0; fake1] with b = 6 -- and each
    rank's dld is exactly 2 x its slice of that call's: hinge gradients -+ 1 / 3 against -+ 1 / 6, c = 2 lam / 3 against 2 lam / 6.
    (Scaling by 2 is exact where nothing is subnormal, which is asserted.)"""
    b, lam = 3, 0.3
    state = LC.initial_state()
    state[:5] = 0.75, -0.4, 6.0, 0.0, 6.0
    rows = _two_ranks()
    cat = np.concatenate([rows[0, :b], rows[1, :b], rows[0, b:], rows[1, b:]])
    dld_cat = _hinge_dld(cat, 2 * b)
    s_want, g_want, r_want = LC.step(state, cat, 2 * b, dld_cat, lam, 0.9, 0, one_sided)
    assert r_want > 0 and not np.array_equal(g_want, dld_cat)
    outs = []
    for rank in range(2):
        dld = _hinge_dld(rows[rank], b)
        own_cat = np.concatenate([dld_cat[rank * b:(rank + 1) * b], dld_cat[2 * b + rank * b:2 * b + (rank + 1) * b]])
        assert _u32(dld) == _u32(np.float32(2) * own_cat)
        s, g, r = LC.step_rows(state, rows, rank, dld, lam, 0.9, 0, one_sided)
        outs.append((s, r))
        want = np.concatenate([g_want[rank * b:(rank + 1) * b], g_want[2 * b + rank * b:2 * b + (rank + 1) * b]])
        assert _u32(g) == _u32(np.float32(2) * want), rank
        for v in (g, want, dld, own_cat):
            assert ((v == 0) | (np.abs(v) >= MIN_NORMAL32)).all()
    assert _u64(outs[0][0]) == _u64(outs[1][0]) == _u64(s_want) and _u32(outs[0][1]) == _u32(outs[1][1]) == _u32(r_want)
    c = 2.0 * lam / b
    assert c >= MIN_NORMAL64 and c / 2 == 2.0 * lam / (2 * b)
    assert all(abs(v) >= MIN_NORMAL64 for v in s_want[:2]) and abs(float(r_want)) >= MIN_NORMAL32


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_logit_in_the_other_ranks_row_freezes_this_ranks_anchors(bad):
    state = LC.initial_state()
    state[:5] = 0.75, -0.4, 6.0, 0.0, 6.0
    rows = _two_ranks(bad)                            # the bad logit sits in rank 1's generated half
    for rank in range(2):
        s, g, r = LC.step_rows(state, rows, rank, _hinge_dld(rows[rank], 3), 0.3, 0.9, 0)
        assert _u64(s[[0, 1, 4]]) == _u64(state[[0, 1, 4]]) and s[LC.TICKS] == 7.0
        assert np.isfinite(g).all() == (rank == 0)    # rank 0's gradient holds its own (finite) logits only
    with pytest.raises(ValueError):
        LC.step_rows(state, rows, 2, np.zeros(6, np.float32), 0.3, 0.9, 0)


# ------------------------------------------------------------------------------------------------------------------ 3. refusal
def _cfg(**kw):
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = B
    cfg.update(kw)
    return cfg


SWITCHES = dict(diff_augment=FULL, ada_target=0.6, ada_interval=1, ada_kimg=0.05, lecam_weight=0.3, lecam_start=0,
                skip_nonfinite_updates=True)


def _fresh(cfg):
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp_, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp_, ds)


def _batch(cfg, step, rank=0, device=None):
    batch = {k: torch.as_tensor(v) for k, v in syn.make_batch(cfg, per_device_batch=B, rank=rank, seed=1234 + step).items()}
    rows, h, w = batch["image"].shape[:3]
    batch["d_aug"] = torch.from_numpy(DA.draw_plan(11, step, rank, rows, h, w, FULL))
    batch["d_aug_u"] = torch.from_numpy(ADA.draw_gates(11, step, rank, rows))
    return batch if device is None else {k: v.to(device) for k, v in batch.items()}


def _controller_bytes(state):
    return [state.ada.state.numpy().tobytes(), state.lecam.state.numpy().tobytes(), state.guard.counters.numpy().tobytes(),
            state.g_optimizer.arena.params.numpy().tobytes(), state.d_optimizer.arena.params.numpy().tobytes()]


@pytest.fixture
def one_rank_group(tmp_path):
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_gather_rows_needs_the_exclusive_schedule(one_rank_group):
    row = torch.arange(5, dtype=torch.float32)
    with pytest.raises(ValueError, match="exclusive"):
        dp.GradSync(schedule="overlapped").gather_rows(row)
    sync = dp.GradSync(schedule="exclusive")
    assert sync.rank == 0 and sync.world == 1
    for t in (row, torch.tensor([1, -2, 3, 0], dtype=torch.int32)):
        out = sync.gather_rows(t)
        assert out.shape == (1, t.numel()) and out.dtype == t.dtype and torch.equal(out[0], t)
    with pytest.raises(ValueError, match="float32 or int32"):
        sync.gather_rows(row.double())


@pytest.mark.parametrize("key", ["ada_target", "lecam_weight", "skip_nonfinite_updates"])
def test_the_checks_still_refuse_anything_but_an_exclusive_exchange(key, one_rank_group):
    xmc_net.set_ops_factory(lambda dtype: CpuOps(dtype))
    try:
        kw = {k: v for k, v in SWITCHES.items() if k.split("_")[0] == key.split("_")[0] or k == "diff_augment"}
        cfg = _cfg(**kw)
        gen, disc, state = _fresh(cfg)
        if key == "skip_nonfinite_updates":
            assert state.guard is not None
        before = [t.clone() for t in (state.g_optimizer.arena.params, state.d_optimizer.arena.params)]
        small = [c.state if hasattr(c, "state") else c.counters for c in (state.ada, state.lecam, state.guard) if c is not None]
        batch = _batch(cfg, 1)
        for sync in (object(), dp.GradSync(schedule="overlapped")):
            for call in (lambda: train_utils.train_step(1, state, batch, xmc_gan, gen, disc, cfg, {}, grad_sync=sync),
                         lambda: xmc_gan.train_d(1, state, train_utils.split_input_dict(batch, 2)[0], gen, disc, cfg, grad_sync=sync),
                         lambda: xmc_gan.train_g_d(1, state, train_utils.split_input_dict(batch, 2)[1], gen, disc, cfg, {},
                                                   grad_sync=sync)):
                with pytest.raises(ValueError) as e:
                    call()
                assert all(word in str(e.value) for word in ("replicas", key, "GradSync(schedule='exclusive')"))
        assert torch.equal(state.g_optimizer.arena.params, before[0]) and torch.equal(state.d_optimizer.arena.params, before[1])
        assert small and not any(t.any() for t in small)
        xmc_gan.check_replica_controllers(cfg, None)
        xmc_gan.check_replica_controllers(cfg, dp.GradSync(schedule="exclusive"))
    finally:
        xmc_net.set_ops_factory(None)


def test_the_drift_check_names_the_controller(one_rank_group):
    sync = dp.GradSync(schedule="exclusive")
    states = {"ada": torch.arange(8, dtype=torch.float64), "lecam": None, "guard": torch.zeros(4, dtype=torch.int32)}
    train_utils.check_replica_drift(states, sync)     # one rank cannot differ from itself
    sync.world = 2                                    # (what rank 1 would have sent: another p)

    def two_rows(out, bits, group=None):
        out.view(2, -1).copy_(torch.stack([bits, bits + (bits.numel() == 16)]))
    real, dist.all_gather_into_tensor = dist.all_gather_into_tensor, two_rows
    try:
        with pytest.raises(RuntimeError, match="ada controller's state on rank 1"):
            train_utils.check_replica_drift(states, sync)
        train_utils.check_replica_drift({"guard": states["guard"]}, sync)
    finally:
        dist.all_gather_into_tensor = real


# ------------------------------------------------------------------------------------ 4. two gloo ranks on the CPU operator table
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _snapshot(state):
    return dict(g=state.g_optimizer.arena.params.clone(), d=state.d_optimizer.arena.params.clone(), ada=state.ada.state.clone(),
                lecam=state.lecam.state.clone(), counters=state.guard.counters.clone())


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    xmc_net.set_ops_factory(lambda dtype: CpuOps(dtype))
    cfg = _cfg(**SWITCHES)
    out = {}
    for scenario in ("clean", "nan"):
        gen, disc, state = _fresh(cfg)
        sync = dp.GradSync(bucket_elems=1 << 20, schedule="exclusive")
        snaps = []
        for step in (1, 2, 3):
            batch = _batch(cfg, step, rank)
            if scenario == "nan" and step == 2 and rank == 1:
                batch["z"] = batch["z"].clone()
                batch["z"][:, 0] = float("nan")       # every half step of this rank's step 2
            state, metrics = train_utils.train_step(step, state, batch, xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
            snaps.append(dict(_snapshot(state), metrics={k: float(v) for k, v in metrics.items()}))
        train_utils.check_replica_drift({"ada": state.ada.state, "lecam": state.lecam.state, "guard": state.guard.counters}, sync)
        out[scenario] = snaps
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_gloo_ranks_hold_the_same_controllers_and_skip_together(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for scenario in ("clean", "nan"):
        for step, (a, b) in enumerate(zip(r0[scenario], r1[scenario]), 1):
            for key in ("g", "d", "ada", "lecam", "counters"):
                # (bit for bit -- stricter than torch.equal, which a NaN R of the skipped step would fail against itself)
                assert a[key].numpy().tobytes() == b[key].numpy().tobytes(), (scenario, step, key)
            assert np.array_equal(a["metrics"][LC.METRIC_KEY], b["metrics"][LC.METRIC_KEY], equal_nan=True), (scenario, step)
    clean, nan = r0["clean"], r0["nan"]
    last = clean[-1]
    assert last["counters"].tolist() == [0, 0, 0, 0] and all(np.isfinite(v) for s in clean for v in s["metrics"].values())
    assert float(last["ada"][ADA.P]) > 0 and last["ada"][ADA.ADJUSTMENTS] == 6            # ada_interval = 1: every half step
    assert float(last["lecam"][LC.ANCHOR_REAL]) != 0 and float(last["lecam"][LC.ANCHOR_FAKE]) != 0 and last["lecam"][LC.UPDATES] == 6
    assert last["metrics"][LC.METRIC_KEY] > 0
    # rank 1's NaN in step 2: neither rank applied anything, both counted the two half steps, and step 3 proceeds
    assert torch.equal(nan[0]["g"], clean[0]["g"]) and torch.equal(nan[0]["d"], clean[0]["d"])
    for r in (r0, r1):
        s1, s2, s3 = r["nan"]
        assert torch.equal(s2["g"], s1["g"]) and torch.equal(s2["d"], s1["d"])
        assert s2["counters"].tolist() == [2, 2, 2, 0] and s3["counters"].tolist() == [2, 0, 2, 0]
        assert not torch.equal(s3["g"], s2["g"]) and not torch.equal(s3["d"], s2["d"])
        assert bool(torch.isfinite(s3["g"]).all()) and bool(torch.isfinite(s3["d"]).all())
        assert s2["lecam"][LC.UPDATES] == 2 and s2["lecam"][LC.TICKS] == 4                # a non-finite logit froze the anchors
