"""config.ada_target on the MI355X: ``xmc_ada_gate`` / ``xmc_ada_update`` (csrc/ada.hip) against their NumPy specification
(libml/ada.py) -- bit for bit: the gate is a select on a float64 comparison, the controller counts integers and then does five IEEE
double operations in a fixed order, so no tolerance is needed -- inside guard bands, and the switch through the training step, a
captured graph, the training loop and a resumed run at C0 (``coco_xmc.get_test_config()``, batch 2)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.guard import Guard, guarded
from xmcgan_image_generation_amd.libml import ada as ADA
from xmcgan_image_generation_amd.libml import diff_augment as DA

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"
DTYPES = ("float32", "bfloat16")
EINVAL = -22


@pytest.fixture(scope="module")
def ops():
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.float32)


def _faulted(e):
    return "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e)


# ------------------------------------------------------------------------------------------------------------ xmc_ada_gate
GATE_P = (0.0, 2.0 ** -24, 0.3, 0.5, 1.0 - 2.0 ** -53, 1.0)


def _gate_inputs(b):
    """a drawn plan (with a -0.0 and the largest float32 in it: the gate moves bits) and uniforms seeded with zeros and with ties
    against every float32-representable p of ``GATE_P``"""
    plan = DA.draw_plan(11, b, 0, b, 128, 128, FULL)
    plan[0, 0, 3], plan[0, 1, 0] = -0.0, np.finfo(np.float32).max
    u = ADA.draw_gates(11, b, 0, b)
    flat = u.reshape(-1)
    special = np.array([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 0.3, np.nextafter(np.float32(0.3), np.float32(0))], np.float32)
    flat[:: 7][: len(special)] = special[: len(flat[:: 7])]
    flat[-1] = 0.0
    return plan, u


@pytest.mark.parametrize("b", [1, 2, 32, 33, 128, 129, 300])
def test_gate_is_bit_equal_to_the_specification_inside_guard_bands(ops, b):
    """2b straddles a wave at 32 / 33, a 256-thread workgroup at 128 / 129, and spans several workgroups at 300"""
    plan_h, u_h = _gate_inputs(b)
    g = Guard("cuda", skew=16)
    try:
        with guarded(g):
            plan, u = torch.from_numpy(plan_h).to("cuda"), torch.from_numpy(u_h).to("cuda")
            state = torch.zeros((8,), dtype=torch.float64, device="cuda")
            got = []
            for p in GATE_P:
                state[0] = p
                got.append((p, ops.ada_gate(plan, u, state), ops.ada_gate(plan, u, state)))
            assert not g.fallthrough, g.fallthrough
            torch.cuda.synchronize()
            rows = [(p, a.cpu().numpy(), c.cpu().numpy()) for p, a, c in got]
        assert g.served >= 3 + 2 * len(GATE_P)
        g.check()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in xmc_ada_gate (b = {b}): {e}", returncode=3)
        raise
    for p, a, c in rows:
        want = ADA.gate(plan_h, u_h, p)
        assert a.shape == (2 * b, 8) and a.dtype == np.float32
        assert a.tobytes() == want.tobytes(), (b, p, np.argwhere(a.view(np.uint32) != want.view(np.uint32))[:4])
        assert c.tobytes() == want.tobytes()
    assert rows[0][1].tobytes() == np.tile(np.asarray(DA.IDENTITY_ROW, np.float32), (2 * b, 1)).tobytes()
    assert rows[-1][1].tobytes() == plan_h.transpose(1, 0, 2).reshape(2 * b, 8).tobytes()


def test_gate_rejects_what_is_outside_its_domain_and_writes_nothing(ops):
    b = 4
    plan_h, u_h = _gate_inputs(b)
    plan, u = torch.from_numpy(plan_h).to("cuda"), torch.from_numpy(u_h).to("cuda")
    state = torch.zeros((8,), dtype=torch.float64, device="cuda")
    rows = torch.full((2 * b, 8), 7.0, device="cuda")
    lib, s = ops.lib, ops._stream()
    ptr = lambda t: t.data_ptr()                                          # noqa: E731
    assert lib.xmc_ada_gate(ptr(plan), ptr(u), ptr(state), ptr(rows), 0, s) == EINVAL
    assert lib.xmc_ada_gate(ptr(plan), ptr(u), ptr(state), ptr(rows), -1, s) == EINVAL
    assert lib.xmc_ada_gate(ptr(plan), ptr(u), ptr(state), ptr(rows), 32768, s) == EINVAL      # 2b > 65535
    for hole in range(4):
        args = [ptr(plan), ptr(u), ptr(state), ptr(rows)]
        args[hole] = None
        assert lib.xmc_ada_gate(*args, b, s) == EINVAL
    assert lib.xmc_ada_gate(ptr(plan) + 4, ptr(u), ptr(state), ptr(rows), b - 1, s) == EINVAL   # the plan is read in 16-byte pieces
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all())


# ---------------------------------------------------------------------------------------------------------- xmc_ada_update
def _logits(b, call, kind):
    """(2b,) float32: the real half holds both signs, +-0, denormals, NaN and +-inf; the generated half is all NaN (it must not
    be read).  ``kind`` "mixed": mostly positive in calls 0-3, mostly negative in calls 4-7; "blank": calls 4-7 hold no finite
    logit at all"""
    rng = np.random.default_rng(1000 * b + call)
    x = rng.standard_normal(b).astype(np.float32) + np.float32(1.0 if call < 4 else -1.0)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -3.0, 2.0], np.float32)
    at = rng.permutation(b)[: min(b, len(special))]
    x[at] = rng.permutation(special)[: len(at)]
    if kind == "blank" and 4 <= call < 8:
        x[:] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), b)
    return np.concatenate([x, np.full(b, np.nan, np.float32)])


@pytest.mark.parametrize("kind", ["mixed", "blank"])
@pytest.mark.parametrize("b", [1, 63, 64, 65, 257, 1025])
def test_update_is_bit_equal_to_the_specification(ops, b, kind):
    """nine calls at interval 4: two adjustments and one half step into the third interval, the state compared as uint64 after
    every call"""
    target, full, interval = 0.6, 7.0 * b, 4
    for p_max in (ADA.P_MAX, 1.0):
        g = Guard("cuda", skew=16)
        want = ADA.initial_state()
        want[ADA.P] = 0.75                                                # (room to move both ways, and p_max within reach)
        try:
            with guarded(g):
                state = torch.from_numpy(want.copy()).to("cuda")
                for call in range(9):
                    x = _logits(b, call, kind)
                    ops.ada_update(torch.from_numpy(x).to("cuda"), b, state, target, full, interval, p_max)
                    got = state.cpu().numpy()
                    want = ADA.update(want, x[:b], target, full, interval, p_max)
                    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist(), (b, kind, p_max, call, got, want)
            g.check()
        except Exception as e:
            if _faulted(e):
                pytest.exit(f"GPU fault in xmc_ada_update (b = {b}): {e}", returncode=3)
            raise
        assert want[ADA.TICKS] == 1 and want[ADA.ADJUSTMENTS] == (2 if kind == "mixed" else 1)
        assert want[ADA.P] != 0.75


def test_update_at_the_target_exactly_and_at_both_clamps(ops):
    state = torch.zeros((8,), dtype=torch.float64, device="cuda")
    state[0] = 0.25
    x = torch.tensor([2.0, 0.5, -1.0, 3.0, float("nan"), float("nan"), float("nan"), float("nan")], device="cuda")
    ops.ada_update(x, 4, state, 0.5, 100.0, 1, ADA.P_MAX)                 # r = (3 - 1) / 4 = 0.5 = the target
    want = ADA.update(np.array([0.25, 0, 0, 0, 0, 0, 0, 0.0]), x[:4].cpu().numpy(), 0.5, 100.0, 1, ADA.P_MAX)
    assert state.cpu().numpy().tobytes() == want.tobytes() and want[ADA.P] == 0.25 and want[ADA.ADJUSTMENTS] == 1
    ones = torch.ones((8,), device="cuda")
    for _ in range(3):
        ops.ada_update(ones, 4, state, 0.5, 8.0, 1, ADA.P_MAX)            # + 0.5 per call: clamped at p_max
        want = ADA.update(want, np.ones(4, np.float32), 0.5, 8.0, 1, ADA.P_MAX)
    assert state.cpu().numpy().tobytes() == want.tobytes() and want[ADA.P] == ADA.P_MAX
    for _ in range(3):
        ops.ada_update(-ones, 4, state, 0.5, 8.0, 1, ADA.P_MAX)           # - 0.5 per call: clamped at 0
        want = ADA.update(want, -np.ones(4, np.float32), 0.5, 8.0, 1, ADA.P_MAX)
    assert state.cpu().numpy().tobytes() == want.tobytes() and want[ADA.P] == 0.0 and want[ADA.ADJUSTMENTS] == 7


def test_update_rejects_what_is_outside_its_domain_and_leaves_the_state(ops):
    before = np.array([0.3, 2.0, 6.0, 1.0, 0.25, 9.0, 0.0, 0.0])
    state = torch.from_numpy(before.copy()).to("cuda")
    x = torch.ones((8,), device="cuda")
    lib, s = ops.lib, ops._stream()
    assert lib.xmc_ada_update(x.data_ptr(), 0, state.data_ptr(), 0.6, 100.0, 4, 0.8, s) == EINVAL
    assert lib.xmc_ada_update(x.data_ptr(), -3, state.data_ptr(), 0.6, 100.0, 4, 0.8, s) == EINVAL
    assert lib.xmc_ada_update(None, 4, state.data_ptr(), 0.6, 100.0, 4, 0.8, s) == EINVAL
    assert lib.xmc_ada_update(x.data_ptr(), 4, None, 0.6, 100.0, 4, 0.8, s) == EINVAL
    assert lib.xmc_ada_update(x.data_ptr(), 4, state.data_ptr(), 0.6, 100.0, 0, 0.8, s) == EINVAL
    assert lib.xmc_ada_update(x.data_ptr(), 4, state.data_ptr(), 0.6, 0.0, 4, 0.8, s) == EINVAL
    assert lib.xmc_ada_update(x.data_ptr(), 4, state.data_ptr(), float("nan"), 100.0, 4, 0.8, s) == EINVAL
    torch.cuda.synchronize()
    assert state.cpu().numpy().tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------------- through the step
B = 2


def _cfg(dtype, policy, **kw):
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.dtype, cfg.batch_size, cfg.pretrained_image_contrastive, cfg.diff_augment = dtype, B, False, policy
    cfg.update(kw)
    return cfg


def _fresh(cfg):
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp, ds)


def _rows(cfg):
    return B * cfg.d_step_per_g_step


def _batch(cfg, step, with_u):
    from xmcgan_image_generation_amd import synthetic as syn
    tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=B, rank=step).items()}
    if cfg.diff_augment:
        tb["d_aug"] = torch.from_numpy(DA.draw_plan(3, step, 0, _rows(cfg), cfg.image_size, cfg.image_size, cfg.diff_augment))
    if with_u:
        tb["d_aug_u"] = torch.from_numpy(ADA.draw_gates(3, step, 0, _rows(cfg)))
    return tb


def _floats(metrics):
    return {k: float(v) for k, v in metrics.items()}


def _one_step(dtype, policy, ada_p=None, identity=False):
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(dtype, policy, **({"ada_target": 0.6} if ada_p is not None else {}))
    gen, disc, state = _fresh(cfg)
    if ada_p is not None:
        assert hasattr(gen(train=True).ops, "ada_gate") and hasattr(gen(train=True).ops, "ada_update")
        state.ada.state[0] = ada_p
    tb = _batch(cfg, 0, ada_p is not None)
    if identity:
        tb["d_aug"] = torch.from_numpy(DA.identity_plan(_rows(cfg)))
    state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    torch.cuda.synchronize()
    return (_floats(metrics), state.g_optimizer.arena.params.clone(), state.d_optimizer.arena.params.clone(),
            state.ada.state.cpu().numpy() if state.ada is not None else None)


def _same(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_p_zero_and_p_one_steps_equal_the_parents_steps(dtype):
    """p = 0 under "translation,cutout": the switch-off step.  p = 0 under the full policy: the parent's step fed the identity plan.
    p = 1: the parent's step fed the drawn plan.  All bit for bit; and the controller counted two half steps of B real logits"""
    try:
        assert _same(_one_step(dtype, "translation,cutout", ada_p=0.0), _one_step(dtype, ""))
        zero = _one_step(dtype, FULL, ada_p=0.0)
        assert _same(zero, _one_step(dtype, FULL, identity=True))
        one, drawn = _one_step(dtype, FULL, ada_p=1.0), _one_step(dtype, FULL)
        assert _same(one, drawn) and not _same(zero, drawn)
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in a training step with config.ada_target ({dtype}): {e}", returncode=3)
        raise
    for got, p in ((zero, 0.0), (one, 1.0)):
        s = got[3]
        assert s[ADA.P] == p and s[ADA.TICKS] == 2 and s[ADA.COUNT] == 2 * B and s[ADA.ADJUSTMENTS] == 0
        assert abs(s[ADA.SIGN_SUM]) <= 2 * B and s[ADA.SIGN_SUM] == round(s[ADA.SIGN_SUM])


# p moves by 4 / 20 at every second half step; over four logits r is a multiple of 0.5, never the target: every adjustment moves p
FAST = dict(ada_target=0.25, ada_kimg=0.02, ada_interval=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager_steps_over_several_intervals(dtype):
    """a graph captured once and replayed three times (six half steps, three adjustments) against four eager steps: metrics, both
    parameter arenas and the controller's state, bit for bit -- p is read and written by the graph's own launches"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(dtype, FULL, **FAST)
    bs = [_batch(cfg, s, True) for s in range(4)]
    try:
        gen, disc, st = _fresh(cfg)
        st.ada.state[0] = 0.4                                             # (room to move both ways)
        eager = []
        for tb in bs:
            st, m = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {})
            eager.append((_floats(m), st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone(),
                          st.ada.state.cpu().numpy()))
        gen2, disc2, st2 = _fresh(cfg)
        st2.ada.state[0] = 0.4
        st2, m = train_utils.train_step(0, st2, bs[0], xmc_gan, gen2, disc2, cfg, {})
        assert _floats(m) == eager[0][0]
        graphed = train_utils.GraphedTrainStep(st2, bs[1], xmc_gan, gen2, disc2, cfg, {})
        st2 = graphed.state
        assert st2.ada.state.cpu().numpy().tobytes() == eager[0][3].tobytes()      # the capture ran nothing
        for i, tb in enumerate(bs[1:], start=1):
            st2, m = graphed(st2, tb)
            got = _floats(m)
            print(dtype, "step", i, "eager", eager[i][0], eager[i][3][:6], "graph", got, st2.ada.state.cpu().numpy()[:6])
            assert got == eager[i][0], i
            assert torch.equal(st2.g_optimizer.arena.params, eager[i][1]) and torch.equal(st2.d_optimizer.arena.params, eager[i][2]), i
            assert st2.ada.state.cpu().numpy().tobytes() == eager[i][3].tobytes(), i
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in a captured step with config.ada_target ({dtype}): {e}", returncode=3)
        raise
    final = eager[-1][3]
    assert final[ADA.ADJUSTMENTS] == 4 and final[ADA.TICKS] == 0
    assert len({e[3][ADA.P] for e in eager}) > 1                          # p did move, so the later steps ran gated plans


@pytest.mark.parametrize("switch", ["skip_nonfinite_updates", "train_statistics", "conv_fp8"])
def test_one_step_beside_the_other_switches(switch):
    from xmcgan_image_generation_amd import _lib, train_utils, xmc_gan
    cfg = _cfg("bfloat16", FULL, **FAST, **{switch: True})
    try:
        additional = xmc_gan.create_additional_data(cfg)
        gen, disc, state = _fresh(cfg)
        state.ada.state[0] = 0.5
        state, m = train_utils.train_step(0, state, _batch(cfg, 0, True), xmc_gan, gen, disc, cfg, additional)
        torch.cuda.synchronize()
        s = state.ada.state.cpu().numpy()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in a step with config.ada_target and config.{switch}: {e}", returncode=3)
        raise
    finally:
        if switch == "conv_fp8":
            _lib.check(_lib.load().xmc_set_tuning(b"mx8_scale_floor", -1), "reset")      # (the scale rule is a process-wide knob)
    assert all(np.isfinite(v) for v in _floats(m).values()), m
    assert s[ADA.ADJUSTMENTS] == 1 and s[ADA.TICKS] == 0 and s[ADA.P] in (0.5 - 4.0 / 20.0, 0.5 + 4.0 / 20.0)
    assert bool(torch.isfinite(state.g_optimizer.arena.params).all()) and bool(torch.isfinite(state.d_optimizer.arena.params).all())


# ------------------------------------------------------------------------------------------------------- the training loop
def _loop_cfg(**kw):
    return _cfg("bfloat16", FULL, ada_target=0.25, ada_kimg=0.02, ada_interval=3, eval_every_steps=2, checkpoint_every_steps=100, **kw)


def _final(state):
    return (state.g_optimizer.arena.params.clone(), state.d_optimizer.arena.params.clone(), state.ema_buffer.clone(),
            state.ada.state.clone())


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """4 steps in one ``train`` call (step 1 eager, 2-4 replayed): eight half steps, an adjustment at every third"""
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    workdir = str(tmp_path_factory.mktemp("ada_run_a"))
    state = train_utils.train(_loop_cfg(num_train_steps=4), workdir, datasets=synthetic_datasets)
    return workdir, _final(state)


def test_training_loop_writes_p_and_runs_twice_to_the_same_bits(run_a, tmp_path):
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    workdir, final_a = run_a
    with open(os.path.join(workdir, "metrics.jsonl")) as f:
        lines = [json.loads(line) for line in f]
    assert [line["step"] for line in lines] == [2, 4]
    for line in lines:
        assert np.isfinite(line["ada/p"]) and 0.0 <= line["ada/p"] <= ADA.P_MAX and -1.0 <= line["ada/r_t"] <= 1.0
        assert all(np.isfinite(v) for v in line.values())
    assert [line["ada/adjustments"] for line in lines] == [1, 2]
    s = final_a[3].cpu().numpy()
    print("train(): ada/p, ada/r_t at steps 2 and 4:", [(line["ada/p"], line["ada/r_t"]) for line in lines], "final state", s[:6])
    assert s[ADA.ADJUSTMENTS] == 2 and s[ADA.TICKS] == 2 and s[ADA.COUNT] == 2 * B
    state = train_utils.train(_loop_cfg(num_train_steps=4), str(tmp_path), datasets=synthetic_datasets)
    for x, y in zip(final_a, _final(state)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_resumed_run_ends_where_the_uninterrupted_one_does(run_a, tmp_path):
    """run B stops after step 2 -- four half steps, one tick into the controller's second interval -- and resumes from its
    checkpoint: the counts in flight travel with it"""
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.utils import checkpoint
    _, final_a = run_a
    workdir = str(tmp_path)
    train_utils.train(_loop_cfg(num_train_steps=2), workdir, datasets=synthetic_datasets)
    saved = checkpoint.msgpack_restore(open(os.path.join(workdir, "checkpoints-0", "ckpt-1.flax"), "rb").read())["ada"]["state"]
    assert saved[ADA.TICKS] == 1 and saved[ADA.COUNT] == B and saved[ADA.ADJUSTMENTS] == 1
    state = train_utils.train(_loop_cfg(num_train_steps=4), workdir, datasets=synthetic_datasets)
    assert int(state.step) == 4
    for x, y in zip(final_a, _final(state)):
        assert torch.equal(x, y)
