"""config.lecam_weight on the MI355X: ``xmc_lecam`` (csrc/lecam.hip) against its NumPy specification (libml/lecam.py) -- bit for bit:
IEEE double in a fixed order, the sums included, so no tolerance is needed -- inside guard bands, and the switch through the training
step, a captured graph, the training loop and a resumed run at C0 (``coco_xmc.get_test_config()``, batch 4)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.guard import Guard, guarded
from xmcgan_image_generation_amd.libml import ada as ADA
from xmcgan_image_generation_amd.libml import diff_augment as DA
from xmcgan_image_generation_amd.libml import lecam as LC

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16")
EINVAL = -22
TAIL = (1.5, -2.5, 7.0)                               # state[5 .. 7]: never touched


@pytest.fixture(scope="module")
def ops():
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.float32)


def _faulted(e):
    return "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e)


def _u64(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def _u32(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32).tolist()


def _state(a_r=0.0, a_f=0.0, ticks=0.0, updates=0.0):
    s = LC.initial_state()
    s[LC.ANCHOR_REAL], s[LC.ANCHOR_FAKE], s[LC.TICKS], s[LC.UPDATES] = a_r, a_f, ticks, updates
    s[5:] = TAIL
    return s


def _hinge_dld(x, b):
    r, f = x[:b], x[b:]
    return np.concatenate([-(1 - r > 0).astype(np.float32) / np.float32(b), (1 + f > 0).astype(np.float32) / np.float32(b)])


TIE = np.float32(0.375)


def _logits(b, call):
    """(2b,) float32, magnitudes from 1e-3 to 1e3, with +0 and -0 in it.  Call 1's generated half is the constant ``TIE``: its
    fixed-order sum and mean are exact, so a_F == TIE after that (warm-up) call, and call 2 holds the tie real_0 == a_F"""
    rng = np.random.default_rng(977 * b + call)
    x = (rng.standard_normal(2 * b) * 10.0 ** rng.uniform(-3, 3, 2 * b)).astype(np.float32)
    x[b + (b - 1) // 2] = -0.0
    if b > 1:
        x[b - 1] = 0.0
    if call == 1:
        x[b:] = TIE
    if call == 2:
        x[0] = TIE
    return x


def _launch_and_compare(ops, b, one_sided, calls, state0, lam=0.3, decay=0.9, start=2):
    """``calls``: the logit vectors of chained calls on one device state.  Every call's dld, loss and state against the
    specification, bit for bit, inside guard bands.  -> the specification's history [(state, dld, r)]"""
    g = Guard("cuda", skew=16)
    want, hist, got = state0.copy(), [], []
    try:
        with guarded(g):
            state = torch.from_numpy(state0.copy()).to("cuda")
            for x in calls:
                dld_h = _hinge_dld(x, b)
                logit, dld = torch.from_numpy(x).to("cuda"), torch.from_numpy(dld_h.copy()).to("cuda")
                loss = ops.lecam(logit, dld, b, state, lam, decay, start, one_sided)
                got.append((dld.cpu().numpy(), loss.cpu().numpy(), state.cpu().numpy(), logit.cpu().numpy()))
                want, g_want, r_want = LC.step(want, x, b, dld_h, lam, decay, start, one_sided)
                hist.append((want.copy(), g_want, r_want, dld_h))
            assert not g.fallthrough, g.fallthrough
        assert g.served >= 1 + 3 * len(calls)
        g.check()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in xmc_lecam (b = {b}): {e}", returncode=3)
        raise
    for i, ((dld, loss, state, logit), (s_want, g_want, r_want, _), x) in enumerate(zip(got, hist, calls)):
        assert _u32(logit) == _u32(x), (b, i)                                              # the input is only read
        bad = np.flatnonzero(dld.view(np.uint32) != g_want.view(np.uint32))
        assert not len(bad), (b, one_sided, i, bad[:4], dld[bad[:4]], g_want[bad[:4]])
        assert loss.shape == (1,) and _u32(loss) == _u32(r_want), (b, one_sided, i, loss, r_want)
        assert _u64(state) == _u64(s_want), (b, one_sided, i, state, s_want)
    return hist


# --------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("one_sided", [False, True])
@pytest.mark.parametrize("b", [1, 2, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_kernel_is_bit_equal_to_the_specification_inside_guard_bands(ops, b, one_sided):
    """b = 1, 2: an empty tree half; 255 / 256 / 257: one element per lane and one over; 513, 1025: the strided loop's third and
    fifth pass.  start = 2: call 0 is the first update (copies the means), call 1 a warm-up copy with updates > 0, call 2 active"""
    hist = _launch_and_compare(ops, b, one_sided, [_logits(b, c) for c in range(3)], _state())
    (s0, g0, r0, d0), (s1, g1, r1, d1), (s2, g2, r2, d2) = hist
    assert r0 == 0 and r1 == 0 and _u32(g0) == _u32(d0) and _u32(g1) == _u32(d1)
    assert s1[LC.ANCHOR_FAKE] == float(TIE) and s2[LC.UPDATES] == 3 and s2[LC.TICKS] == 3 and tuple(s2[5:]) == TAIL
    assert r2 > 0 or (one_sided and b <= 2)
    assert _u32(g2[0]) == _u32(np.float32(np.float64(d2[0]) + 0.0))                       # the tie takes no gradient
    if b >= 63:
        assert (g2 != d2).mean() > (0.1 if one_sided else 0.9)


@pytest.mark.parametrize("half", [0, 1])
def test_non_finite_logits_leave_the_anchors_and_still_tick(ops, half):
    b = 65
    for bad in (np.nan, np.inf, -np.inf):
        for one_sided in (False, True):
            for state0 in (_state(0.75, -0.4, 6.0, 6.0), _state()):
                x = _logits(b, 0)
                x[half * b + 64] = bad
                ((s, g, r, dld),) = _launch_and_compare(ops, b, one_sided, [x], state0, start=0)
                assert _u64(s[[0, 1, 4]]) == _u64(state0[[0, 1, 4]]) and s[LC.TICKS] == state0[LC.TICKS] + 1
                if state0[LC.UPDATES] == 0:
                    assert r == 0 and _u32(g) == _u32(dld)


def test_rejections_return_einval_and_write_nothing(ops):
    b = 4
    before = _state(0.3, -0.2, 5.0, 4.0)
    state = torch.from_numpy(before.copy()).to("cuda")
    x = torch.from_numpy(_logits(b, 0)).to("cuda")
    dld = torch.full((2 * b,), 7.0, device="cuda")
    loss = torch.full((1,), 9.0, device="cuda")
    lib, s = ops.lib, ops._stream()
    ok = dict(logit=x.data_ptr(), dld=dld.data_ptr(), b=b, state=state.data_ptr(), loss=loss.data_ptr(), lam=0.3, decay=0.99, start=0,
              one_sided=0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(b=0), dict(b=-1), dict(b=1 << 30), dict(logit=None), dict(dld=None), dict(state=None), dict(loss=None),
           dict(lam=-0.1), dict(lam=nan), dict(lam=inf), dict(decay=1.0), dict(decay=-0.01), dict(decay=nan), dict(start=-1),
           dict(one_sided=2), dict(one_sided=-1), dict(logit=x.data_ptr() + 2), dict(dld=dld.data_ptr() + 2),
           dict(loss=loss.data_ptr() + 2), dict(state=state.data_ptr() + 4)]
    for change in bad:
        a = dict(ok, **change)
        assert lib.xmc_lecam(a["logit"], a["dld"], a["b"], a["state"], a["loss"], a["lam"], a["decay"], a["start"], a["one_sided"],
                             s) == EINVAL, change
    torch.cuda.synchronize()
    assert state.cpu().numpy().tobytes() == before.tobytes() and bool((dld == 7.0).all()) and float(loss[0]) == 9.0
    # ... and the same arguments unchanged are inside the domain (lam = 0 included: the term adds c * d = 0)
    assert lib.xmc_lecam(*[ok[k] for k in ("logit", "dld", "b", "state", "loss")], 0.0, 0.0, 0, 1, s) == 0
    torch.cuda.synchronize()
    assert state.cpu().numpy()[LC.TICKS] == 6.0


# ------------------------------------------------------------------------------------------------------- through the step
B = 4
ACTIVE = np.array([0.75, -0.4, 6.0, 0.0, 6.0, 0.0, 0.0, 0.0])


def _cfg(dtype, **kw):
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.dtype, cfg.batch_size, cfg.pretrained_image_contrastive = dtype, B, False
    cfg.update(kw)
    return cfg


def _fresh(cfg):
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp, ds)


def _batch(cfg, step):
    from xmcgan_image_generation_amd import synthetic as syn
    tb = {k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=B, rank=step).items()}
    rows = B * cfg.d_step_per_g_step
    if cfg.get("diff_augment", ""):
        tb["d_aug"] = torch.from_numpy(DA.draw_plan(3, step, 0, rows, cfg.image_size, cfg.image_size, cfg.diff_augment))
    if cfg.get("ada_target", 0):
        tb["d_aug_u"] = torch.from_numpy(ADA.draw_gates(3, step, 0, rows))
    return tb


def _floats(metrics):
    return {k: float(v) for k, v in metrics.items()}


def _arenas(state):
    return [t.clone() for a in (state.d_optimizer.arena, state.g_optimizer.arena) for t in (a.params, a.m, a.v)] + [state.ema_buffer.clone()]


@pytest.mark.parametrize("one_sided", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_step_takes_the_term_exactly(dtype, one_sided, monkeypatch):
    """run A: one train_step with the switch on.  Run B: the key absent, and ``losses.hinge_loss`` wrapped: the wrapper reads the
    logits back, runs the SPECIFICATION with a state of its own across the two half steps and writes the resulting dld.  The same
    dld bits go into the same deterministic kernels: parameters and Adam moments of D and G are bit-identical"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.libml import losses
    kw = dict(lecam_weight=0.3, lecam_decay=0.9, lecam_one_sided=one_sided)
    try:
        cfg = _cfg(dtype, **kw)
        gen, disc, state = _fresh(cfg)
        assert hasattr(gen(train=True).ops, "lecam")
        state.lecam.load_state_dict({"state": ACTIVE})
        state, metrics_a = train_utils.train_step(0, state, _batch(cfg, 0), xmc_gan, gen, disc, cfg, {})
        torch.cuda.synchronize()
        a, state_a, metrics_a = _arenas(state), state.lecam.state.cpu().numpy(), _floats(metrics_a)

        spec = {"state": ACTIVE.copy(), "r": []}
        plain = losses.hinge_loss

        def wrapped(ops, logit, batch, d_acc, g_acc):
            dld, dlg = plain(ops, logit, batch, d_acc, g_acc)
            spec["state"], new, r = LC.step(spec["state"], logit.float().cpu().numpy(), batch, dld.cpu().numpy(), 0.3, 0.9, 0, one_sided)
            dld.copy_(torch.from_numpy(new))
            spec["r"].append(float(r))
            return dld, dlg
        monkeypatch.setattr(losses, "hinge_loss", wrapped)
        off = _cfg(dtype)
        gen0, disc0, state0 = _fresh(off)
        assert state0.lecam is None
        state0, metrics_b = train_utils.train_step(0, state0, _batch(off, 0), xmc_gan, gen0, disc0, off, {})
        torch.cuda.synchronize()
        monkeypatch.setattr(losses, "hinge_loss", plain)
        b_ = _arenas(state0)
        # and the parent's own step, for the record: the term does move D
        gen1, disc1, state1 = _fresh(off)
        state1, _ = train_utils.train_step(0, state1, _batch(off, 0), xmc_gan, gen1, disc1, off, {})
        torch.cuda.synchronize()
        parent = _arenas(state1)
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in a training step with config.lecam_weight ({dtype}): {e}", returncode=3)
        raise
    assert len(spec["r"]) == cfg.d_step_per_g_step and all(r > 0 for r in spec["r"])
    for name, x, y in zip(("d.params", "d.m", "d.v", "g.params", "g.m", "g.v", "ema"), a, b_):
        assert torch.equal(x, y), name
    assert not torch.equal(a[0], parent[0])
    assert state_a.tobytes() == spec["state"].tobytes()
    assert metrics_a.pop("d_loss_lecam") == spec["r"][-1]
    assert metrics_a == _floats(metrics_b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager_over_steps_that_cross_lecam_start(dtype):
    """lecam_start = 3: the first step's two half steps and the second step's first are warm-up, the term switches on inside the
    second step.  A graph captured once and replayed three times against four eager steps: metrics, parameters and the controller's
    state, bit for bit -- the anchors are read and written by the graph's own launches"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(dtype, lecam_weight=0.3, lecam_decay=0.9, lecam_start=3)
    bs = [_batch(cfg, s) for s in range(4)]
    try:
        gen, disc, st = _fresh(cfg)
        eager = []
        for tb in bs:
            st, m = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {})
            eager.append((_floats(m), st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone(),
                          st.lecam.state.cpu().numpy()))
        gen2, disc2, st2 = _fresh(cfg)
        st2, m = train_utils.train_step(0, st2, bs[0], xmc_gan, gen2, disc2, cfg, {})
        assert _floats(m) == eager[0][0]
        graphed = train_utils.GraphedTrainStep(st2, bs[1], xmc_gan, gen2, disc2, cfg, {})
        st2 = graphed.state
        assert st2.lecam.state.cpu().numpy().tobytes() == eager[0][3].tobytes()    # the capture ran nothing
        for i, tb in enumerate(bs[1:], start=1):
            st2, m = graphed(st2, tb)
            got = _floats(m)
            print(dtype, "step", i, "eager", eager[i][0], eager[i][3][:5], "graph", got, st2.lecam.state.cpu().numpy()[:5])
            assert got == eager[i][0], i
            assert torch.equal(st2.g_optimizer.arena.params, eager[i][1]) and torch.equal(st2.d_optimizer.arena.params, eager[i][2]), i
            assert st2.lecam.state.cpu().numpy().tobytes() == eager[i][3].tobytes(), i
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in a captured step with config.lecam_weight ({dtype}): {e}", returncode=3)
        raise
    assert eager[0][0]["d_loss_lecam"] == 0 and all(e[0]["d_loss_lecam"] > 0 for e in eager[1:])
    final = eager[-1][3]
    assert final[LC.TICKS] == 8 and final[LC.UPDATES] == 8 and final[LC.LAST_R] > 0


@pytest.mark.parametrize("switch", ["skip_nonfinite_updates", "train_statistics", "ada", "conv_fp8"])
def test_one_step_beside_the_other_switches(switch):
    from xmcgan_image_generation_amd import _lib, train_utils, xmc_gan
    other = dict(diff_augment="color,translation,cutout", ada_target=0.6) if switch == "ada" else {switch: True}
    cfg = _cfg("bfloat16", lecam_weight=0.3, **other)
    try:
        additional = xmc_gan.create_additional_data(cfg)
        gen, disc, state = _fresh(cfg)
        state.lecam.load_state_dict({"state": ACTIVE})
        if switch == "ada":
            state.ada.state[0] = 0.5
        state, m = train_utils.train_step(0, state, _batch(cfg, 0), xmc_gan, gen, disc, cfg, additional)
        torch.cuda.synchronize()
        s = state.lecam.state.cpu().numpy()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in a step with config.lecam_weight and {switch}: {e}", returncode=3)
        raise
    finally:
        if switch == "conv_fp8":
            _lib.check(_lib.load().xmc_set_tuning(b"mx8_scale_floor", -1), "reset")      # (the scale rule is a process-wide knob)
    m = _floats(m)
    assert all(np.isfinite(v) for v in m.values()) and m["d_loss_lecam"] > 0, m
    assert s[LC.TICKS] == 8 and s[LC.UPDATES] == 8 and np.isfinite(s).all()
    assert bool(torch.isfinite(state.g_optimizer.arena.params).all()) and bool(torch.isfinite(state.d_optimizer.arena.params).all())


# ------------------------------------------------------------------------------------------------------- the training loop
def _loop_cfg(**kw):
    return _cfg("bfloat16", lecam_weight=0.3, lecam_decay=0.9, lecam_start=3, eval_every_steps=2, checkpoint_every_steps=100, **kw)


def _final(state):
    return (state.g_optimizer.arena.params.clone(), state.d_optimizer.arena.params.clone(), state.ema_buffer.clone(),
            state.lecam.state.clone())


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """4 steps in one ``train`` call (step 1 eager, 2-4 replayed): eight half steps, the term on from the fourth"""
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    workdir = str(tmp_path_factory.mktemp("lecam_run_a"))
    state = train_utils.train(_loop_cfg(num_train_steps=4), workdir, datasets=synthetic_datasets)
    return workdir, _final(state)


def test_training_loop_writes_the_anchors_and_runs_twice_to_the_same_bits(run_a, tmp_path):
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    workdir, final_a = run_a
    with open(os.path.join(workdir, "metrics.jsonl")) as f:
        lines = [json.loads(line) for line in f]
    assert [line["step"] for line in lines] == [2, 4]
    for line in lines:
        assert all(np.isfinite(v) for v in line.values())
        assert {"lecam/anchor_real", "lecam/anchor_fake", "lecam/updates", "d_loss_lecam"} <= set(line)
    assert [line["lecam/updates"] for line in lines] == [4, 8]
    s = final_a[3].cpu().numpy()
    print("train(): anchors at steps 2 and 4:", [(line["lecam/anchor_real"], line["lecam/anchor_fake"]) for line in lines], "final", s[:5])
    assert s[LC.TICKS] == 8 and s[LC.UPDATES] == 8 and s[LC.LAST_R] > 0
    assert lines[-1]["lecam/anchor_real"] == s[LC.ANCHOR_REAL] and lines[-1]["lecam/anchor_fake"] == s[LC.ANCHOR_FAKE]
    assert lines[-1]["d_loss_lecam"] > 0
    state = train_utils.train(_loop_cfg(num_train_steps=4), str(tmp_path), datasets=synthetic_datasets)
    for x, y in zip(final_a, _final(state)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_resumed_run_ends_where_the_uninterrupted_one_does(run_a, tmp_path):
    """run B stops after step 2 -- four half steps, the term just switched on -- and resumes from its checkpoint: the anchors and
    their counts travel with it"""
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    from xmcgan_image_generation_amd.utils import checkpoint
    _, final_a = run_a
    workdir = str(tmp_path)
    train_utils.train(_loop_cfg(num_train_steps=2), workdir, datasets=synthetic_datasets)
    saved = checkpoint.msgpack_restore(open(os.path.join(workdir, "checkpoints-0", "ckpt-1.flax"), "rb").read())["lecam"]["state"]
    assert saved[LC.TICKS] == 4 and saved[LC.UPDATES] == 4 and saved[LC.LAST_R] > 0
    state = train_utils.train(_loop_cfg(num_train_steps=4), workdir, datasets=synthetic_datasets)
    assert int(state.step) == 4
    for x, y in zip(final_a, _final(state)):
        assert torch.equal(x, y)
