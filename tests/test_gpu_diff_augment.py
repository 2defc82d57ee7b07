"""config.diff_augment on the MI355X: ``xmc_diffaug_fwd`` / ``xmc_diffaug_bwd`` (csrc/diff_augment.hip) against their float64
NumPy specification (libml/diff_augment.py) inside guard bands, their determinism, the adjoint identity on the device, the
library's plan validation, and the switch through the training step, a captured graph and the training loop.

Error bounds of the kernel tests (inputs |x| <= 1, plan parameters inside the drawn ranges b in [-0.5, 0.5), s in [0, 2),
k in [0.5, 1.5)).  Intermediates: after brightness |u| <= 1.5; after saturation |u - m| s + |m| <= 2 * 2 + 1.5 = 5.5; after
contrast |u - mu| k + |mu| <= 7 * 1.5 + 1.5 = 12.  The float32 kernel makes about ten roundings of at most 2^-24 * 12 on the
way (7.2e-6 together), and its mean comes out of a reduction tree of at most 16 levels (2^-24 * 1.5 per level, times |1 - k|
<= 0.5 and k: under 1e-6): under 1e-5 in all, 2e-5 absolute is allowed.  The backward steps have coefficients |k| + |1 - k| <= 2 and
|s| + |1 - s| <= 3, together at most 6 in front of max|g|: the same count of roundings gives 2e-5 * max|g|.  bf16 tensors add the one rounding on store, 2^-8 |want|.  With
bits 0-2 clear both kernels only move data: bit-equal.

Measured on one MI355X (worst error / bound over every shape, flag set and plan of the tests below): float32 0.013 - 0.029 of the
bound; bf16 0.98 - 0.99 -- that is the store's own rounding, whose half ulp reaches 2^-8 |want| just above a power of two by the
format's definition, with the float32 part (under 3 % of 2e-5) on top; it cannot exceed the bound while the float32 part holds."""
import json
import os

import numpy as np
import pytest
import torch

from tests.guard import Guard, guarded
from tests.test_diff_augment import FULL, edge_rows
from xmcgan_image_generation_amd.libml import diff_augment as DA

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (5, 8, 8), (3, 6, 10), (2, 16, 16), (4, 128, 128)]
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
FLAG_SETS = (0, 1, 2, 4, 7)


@pytest.fixture(scope="module")
def ops():
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.float32)


def _faulted(e):
    return "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e)


def _plans(rows, h, w):
    """plans of ``rows`` rows that together hold every row of ``edge_rows`` (shifts at -r, 0, +r in both axes, a box clipped at
    each border, a box of side 0, a box over the whole image), in order, wrapping around"""
    edge = edge_rows(h, w)
    count = -(-len(edge) // rows)
    return [np.ascontiguousarray(edge[(np.arange(rows) + k * rows) % len(edge)]) for k in range(count)]


_DATA = {}


def _data(b, h, w, dtype):
    """(real, fake, g) host tensors of one case, values in [-1, 1], made once"""
    key = (b, h, w, dtype)
    if key not in _DATA:
        gen = torch.Generator().manual_seed(1000 * b + 10 * h + w)
        _DATA[key] = tuple((torch.rand((b, h, w, 3), generator=gen) * 2 - 1).to(DTYPES[dtype]) for _ in range(3))
    return _DATA[key]


def _check(got, want, dtype, flags, scale, what):
    got = got.float().cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), what
    if flags == 0:
        assert np.array_equal(got, want), what
        return 0.0
    err = np.abs(got - want)
    bound = 2e-5 * scale + (2.0 ** -8 * np.abs(want) if dtype == "bfloat16" else 0.0)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (what, float(err.max()), worst)
    return worst


def _run_case(ops, b, h, w, dtype):
    """forward and backward of one (shape, dtype) for every flag set and every plan, each launched twice -> worst error / bound"""
    real_h, fake_h, g_h = _data(b, h, w, dtype)
    real, fake, g = real_h.to("cuda"), fake_h.to("cuda"), g_h.to("cuda")
    x64 = torch.cat([real_h, fake_h]).double().numpy()
    g64 = g_h.double().numpy()
    gmax = float(np.abs(g64).max())
    worst = 0.0
    for flags in FLAG_SETS:
        for host in _plans(2 * b, h, w):
            plan = torch.from_numpy(host).to("cuda")
            out = ops.diff_augment(real, fake, plan, host, flags)
            again = ops.diff_augment(real, fake, plan, host, flags)
            assert out.shape == (2 * b, h, w, 3) and out.dtype == DTYPES[dtype]
            assert torch.equal(out.view(torch.uint8), again.view(torch.uint8)), "two forward launches differ"
            worst = max(worst, _check(out, DA.apply(x64, host, flags), dtype, flags, 1.0, ("fwd", b, h, w, dtype, flags)))
        for host in _plans(b, h, w):
            plan = torch.from_numpy(host).to("cuda")
            dimg = ops.diff_augment_bwd(g, plan, host, flags)
            again = ops.diff_augment_bwd(g, plan, host, flags)
            assert dimg.shape == g.shape and dimg.dtype == g.dtype
            assert torch.equal(dimg.view(torch.uint8), again.view(torch.uint8)), "two backward launches differ"
            worst = max(worst, _check(dimg, DA.adjoint(g64, host, flags), dtype, flags, gmax, ("bwd", b, h, w, dtype, flags)))
    return worst


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_kernels_match_the_specification(ops, b, h, w, dtype):
    """the bounds of the module docstring; with no colour bit bit-equal; every launch repeated with the same bits"""
    try:
        worst = _run_case(ops, b, h, w, dtype)
        torch.cuda.synchronize()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in the diff_augment kernels ({b}, {h}, {w}) {dtype}: {e}", returncode=3)
        raise
    print(f"diff_augment ({b}, {h}, {w}) {dtype}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_kernels_stay_inside_their_buffers(ops, b, h, w, dtype):
    """the same cases with every tensor (inputs, plan, output, workspace) between bands of 0xFF bytes, at the weakest alignment the
    allocator hands out (skew 16): no band byte changes and no NaN from a band reaches an output"""
    g = Guard("cuda", skew=16)
    try:
        with guarded(g):
            _run_case(ops, b, h, w, dtype)
            assert not g.fallthrough, g.fallthrough
        assert g.served >= 3 + 4 * len(FLAG_SETS)
        g.check()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in the diff_augment kernels under guard bands ({b}, {h}, {w}) {dtype}: {e}", returncode=3)
        raise


def test_adjoint_identity_on_the_device(ops):
    """<fwd(x) - fwd(0), g> == <x, bwd(g)> to 1e-5 of |x| |g| per sample, float32 at (2, 16, 16), every colour bit set"""
    b, h, w = 2, 16, 16
    real_h, fake_h, g_h = _data(b, h, w, "float32")
    host = _plans(2 * b, h, w)[0]
    plan = torch.from_numpy(host).to("cuda")
    real, fake, g = real_h.to("cuda"), fake_h.to("cuda"), g_h.to("cuda")
    zero = torch.zeros_like(fake)
    lin = (ops.diff_augment(real, fake, plan, host, 7)[b:] - ops.diff_augment(real, zero, plan, host, 7)[b:]).double().cpu()
    back = ops.diff_augment_bwd(g, plan[b:], host[b:], 7).double().cpu()
    lhs = (lin * g_h.double()).reshape(b, -1).sum(1)
    rhs = (fake_h.double() * back).reshape(b, -1).sum(1)
    scale = fake_h.double().reshape(b, -1).norm(dim=1) * g_h.double().reshape(b, -1).norm(dim=1)
    print("adjoint identity, |lhs - rhs| / (|x| |g|):", ((lhs - rhs).abs() / scale).tolist())
    assert ((lhs - rhs).abs() <= 1e-5 * scale).all()


def test_bad_host_plan_is_an_error_and_launches_nothing(ops):
    b, h, w = 2, 8, 8
    real_h, fake_h, g_h = _data(b, h, w, "float32")
    real, fake, g = real_h.to("cuda"), fake_h.to("cuda"), g_h.to("cuda")
    good = np.ascontiguousarray(DA.identity_plan(b).transpose(1, 0, 2).reshape(2 * b, 8))
    plan = torch.from_numpy(good).to("cuda")                     # the DEVICE plan is fine: only the host copy is bad
    out = torch.full((2 * b, h, w, 3), 7.0, device="cuda")
    dimg = torch.full((b, h, w, 3), 7.0, device="cuda")
    ws = torch.zeros(2 * b * 64, device="cuda")
    for col, val in ((3, float(h)), (3, -float(h)), (4, float(w) + 3)):
        bad = good.copy()
        bad[b, col] = val
        rc = ops.lib.xmc_diffaug_fwd(real.data_ptr(), fake.data_ptr(), plan.data_ptr(), bad.ctypes.data, out.data_ptr(), b, h, w, 7, 0,
                                     ws.data_ptr(), ops._stream())
        assert rc == -22
        rc = ops.lib.xmc_diffaug_bwd(g.data_ptr(), plan[b:].data_ptr(), bad[b:].ctypes.data, dimg.data_ptr(), b, h, w, 7, 0,
                                     ws.data_ptr(), ops._stream())
        assert rc == -22
        from xmcgan_image_generation_amd._lib import XmcError
        with pytest.raises(XmcError):
            ops.diff_augment(real, fake, plan, bad, 7)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dimg == 7.0).all()) and not ws.any()


def test_device_plan_that_differs_from_the_host_copy_stays_in_bounds(ops):
    """what protects a graph replay: the kernels clamp and bounds-check what the DEVICE plan holds -- shifts far outside the
    image, a NaN, an infinite box -- and the guard bands stay intact"""
    b, h, w = 2, 8, 8
    real_h, fake_h, g_h = _data(b, h, w, "float32")
    good = np.ascontiguousarray(DA.identity_plan(b).transpose(1, 0, 2).reshape(2 * b, 8))
    wild = good.copy()
    wild[0, 3:5], wild[1, 3:5], wild[2, 3:], wild[3, 5:] = (1e9, -1e9), (-300, 300), np.nan, (-np.inf, -np.inf, np.inf)
    g = Guard("cuda", skew=16)
    try:
        with guarded(g):
            real, fake, gg = real_h.to("cuda"), fake_h.to("cuda"), g_h.to("cuda")
            plan = torch.from_numpy(wild).to("cuda")
            out = ops.diff_augment(real, fake, plan, good, 7)
            dimg = ops.diff_augment_bwd(gg, plan[b:].contiguous(), good[b:], 7)
            torch.cuda.synchronize()
        g.check()
    except Exception as e:
        if _faulted(e):
            pytest.exit(f"GPU fault in the diff_augment kernels on a wild device plan: {e}", returncode=3)
        raise
    assert out.shape == (2 * b, h, w, 3) and dimg.shape == (b, h, w, 3)


# ------------------------------------------------------------------------------------------------------- through the step
B = 2


def _cfg(dtype, policy):
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.dtype, cfg.batch_size, cfg.pretrained_image_contrastive, cfg.diff_augment = dtype, B, False, policy
    return cfg


def _fresh(cfg):
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp, ds)


def _batches(cfg, n):
    from xmcgan_image_generation_amd import synthetic as syn
    return [{k: torch.as_tensor(v).cuda() for k, v in syn.make_batch(cfg, per_device_batch=B, rank=r).items()} for r in range(n)]


def _rows(cfg):
    return B * cfg.d_step_per_g_step


def _plan(cfg, real_row=None, fake_row=None):
    plan = DA.identity_plan(_rows(cfg))
    if real_row is not None:
        plan[:, 0] = np.asarray(real_row, np.float32)
    if fake_row is not None:
        plan[:, 1] = np.asarray(fake_row, np.float32)
    return torch.from_numpy(plan)


_STEPS = {}


def _one_step(dtype, which):
    """one train_step from the same state and batch: "off", "identity", "fake_cut", "real_cut" -> tensors after the step"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    if (dtype, which) in _STEPS:
        return _STEPS[dtype, which]
    cfg = _cfg(dtype, "" if which == "off" else "translation,cutout")
    cut = (0, 1, 1, 0, 0, 0, 0, cfg.image_size)                  # a box over the whole image
    gen, disc, state = _fresh(cfg)
    d_before = state.d_optimizer.arena.params.clone()
    tb = _batches(cfg, 1)[0]
    if which != "off":
        tb["d_aug"] = _plan(cfg, **{"identity": {}, "fake_cut": {"fake_row": cut}, "real_cut": {"real_row": cut}}[which])
    state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    torch.cuda.synchronize()
    _STEPS[dtype, which] = dict(g=state.g_optimizer.arena.params.clone(), d=state.d_optimizer.arena.params.clone(),
                                g_grads=state.g_optimizer.arena.grads.clone(), d_before=d_before,
                                metrics={k: float(v) for k, v in metrics.items()})
    return _STEPS[dtype, which]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_identity_plan_step_is_bit_equal_to_the_switch_off(keep_grads, dtype):
    off, ident = _one_step(dtype, "off"), _one_step(dtype, "identity")
    assert ident["metrics"] == off["metrics"]
    for k in ("g", "d", "g_grads"):
        assert torch.equal(ident[k], off[k]), k
    assert bool(off["g_grads"].any())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_cutting_the_generated_images_zeroes_every_generator_gradient(keep_grads, dtype):
    """generated rows with a box over the whole image, real rows untouched: D sees black generated images, nothing flows back to
    G -- every generator gradient is exactly zero -- while D's own parameters still change"""
    got = _one_step(dtype, "fake_cut")
    assert not bool(got["g_grads"].any()) and bool(torch.isfinite(got["g_grads"]).all())
    assert not torch.equal(got["d"], got["d_before"])
    assert all(np.isfinite(v) for v in got["metrics"].values())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_cutting_the_real_images_leaves_the_generator_gradient(keep_grads, dtype):
    off, got = _one_step(dtype, "identity"), _one_step(dtype, "real_cut")
    assert bool(got["g_grads"].any()) and bool(torch.isfinite(got["g_grads"]).all())
    assert not torch.equal(got["g_grads"], off["g_grads"])
    assert got["metrics"]["d_loss"] != off["metrics"]["d_loss"]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_graph_replays_new_plans_like_eager_steps(dtype):
    """a graph captured with one plan and replayed with that plan and two others: bit-equal to three eager steps with the same
    three plans (the plan travels in the static batch like z)"""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    cfg = _cfg(dtype, FULL)
    bs = _batches(cfg, 4)
    for s, tb in enumerate(bs):
        tb["d_aug"] = torch.from_numpy(DA.draw_plan(3, s, 0, _rows(cfg), cfg.image_size, cfg.image_size, FULL))
    gen, disc, st = _fresh(cfg)
    eager = []
    for tb in bs:
        st, m = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {})
        eager.append(({k: float(v) for k, v in m.items()}, st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone()))
    gen2, disc2, st2 = _fresh(cfg)
    st2, m = train_utils.train_step(0, st2, bs[0], xmc_gan, gen2, disc2, cfg, {})
    assert {k: float(v) for k, v in m.items()} == eager[0][0]
    graphed = train_utils.GraphedTrainStep(st2, bs[1], xmc_gan, gen2, disc2, cfg, {})
    st2 = graphed.state
    for i, tb in enumerate(bs[1:], start=1):
        st2, m = graphed(st2, tb)
        got = {k: float(v) for k, v in m.items()}
        print(dtype, "step", i, "eager", eager[i][0], "graph", got)
        assert got == eager[i][0], i
        assert torch.equal(st2.g_optimizer.arena.params, eager[i][1]) and torch.equal(st2.d_optimizer.arena.params, eager[i][2]), i


def test_fp8_mode_takes_the_augmented_input_as_it_is():
    """config.conv_fp8: D's RGB layer (3 input channels) is a bf16 convolution in that mode too, so the augmented tensor needs no
    MX packet twin -- an identity plan is bit-equal to the switch-off fp8 step, a drawn plan gives finite, different losses"""
    from xmcgan_image_generation_amd import _lib, train_utils, xmc_gan
    got = {}
    try:
        for which, policy in (("off", ""), ("identity", "translation,cutout"), ("drawn", FULL)):
            cfg = _cfg("bfloat16", policy)
            cfg.conv_fp8 = True
            gen, disc, state = _fresh(cfg)
            assert gen(train=True).ops.fp8
            tb = _batches(cfg, 1)[0]
            if which == "identity":
                tb["d_aug"] = _plan(cfg)
            elif which == "drawn":
                tb["d_aug"] = torch.from_numpy(DA.draw_plan(9, 1, 0, _rows(cfg), cfg.image_size, cfg.image_size, FULL))
            state, m = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
            got[which] = ({k: float(v) for k, v in m.items()}, state.g_optimizer.arena.params.clone(), state.d_optimizer.arena.params.clone())
    finally:
        _lib.check(_lib.load().xmc_set_tuning(b"mx8_scale_floor", -1), "reset")      # (the scale rule is a process-wide knob)
    assert got["identity"][0] == got["off"][0]
    assert torch.equal(got["identity"][1], got["off"][1]) and torch.equal(got["identity"][2], got["off"][2])
    assert all(np.isfinite(v) for v in got["drawn"][0].values()) and got["drawn"][0]["d_loss"] != got["off"][0]["d_loss"]
    assert bool(torch.isfinite(got["drawn"][1]).all()) and bool(torch.isfinite(got["drawn"][2]).all())


def test_training_loop_with_the_full_policy(tmp_path):
    """train() for three steps at C0 (bf16, batch 2) on synthetic data: finite metrics, the policy in config.json, and a second
    identical run ends with bit-identical parameters (the plan is a pure function of seed, step and rank)"""
    from tests.test_gpu_train_loop import synthetic_datasets
    from xmcgan_image_generation_amd import train_utils
    finals = []
    for run in ("a", "b"):
        cfg = _cfg("bfloat16", FULL)
        cfg.num_train_steps, cfg.eval_every_steps, cfg.checkpoint_every_steps = 3, 3, 3
        workdir = str(tmp_path / run)
        state = train_utils.train(cfg, workdir, datasets=synthetic_datasets)
        assert int(state.step) == 3
        finals.append((state.g_optimizer.arena.params.clone(), state.d_optimizer.arena.params.clone(), state.ema_buffer.clone()))
        with open(os.path.join(workdir, "config.json")) as f:
            assert json.load(f)["diff_augment"] == FULL
        with open(os.path.join(workdir, "metrics.jsonl")) as f:
            lines = [json.loads(line) for line in f]
        assert lines and lines[-1]["step"] == 3
        assert all(np.isfinite(v) for line in lines for v in line.values())
    for x, y in zip(*finals):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
