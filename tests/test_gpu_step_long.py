"""The training step at Localized Narratives' caption length (T = 64) on the MI355X against ``oracle.torch_ref.train_step``, with
the gates of the T = 17 tests: float32 losses within 1e-3 (tests/test_gpu_step.py::test_train_step_fp32_tiny) and gradient arenas
within 2e-3 norm-relative (tests/test_host_logic.py); bf16 losses within 5e-2 (test_train_step_bf16_tiny_losses) with the long
MFMA attention and its direct-context route doing the work; graph replay bit-equal to eager, two runs bit-identical.  The batch is
tests/test_ln_dataset.py::ln_batch: max_len 64 and 33 among its rows."""
import numpy as np
import pytest
import torch

from tests.test_gpu_step import _check_grads, _rel_scalar
from tests.test_ln_dataset import ln_batch

pytestmark = pytest.mark.gpu

KEYS = ("d_loss", "g_loss", "c_loss_d", "c_loss_g")


def _setup(cfg, b):
    from oracle import torch_ref as R
    from xmcgan_image_generation_amd import synthetic as syn
    from xmcgan_image_generation_amd import train_utils
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    batch = ln_batch(cfg, b)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, gp, gs, dp, ds)
    return gen, disc, state, R.make_state(gp, gs, dp, ds, torch.float32), batch


@pytest.mark.usefixtures("keep_grads")
def test_train_step_fp32_tiny_t64():
    from oracle import torch_ref as R
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = 2
    gen, disc, state, ref_state, batch = _setup(cfg, 2)
    tb = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}
    new_state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    _, ref_metrics, dbg = R.train_step(ref_state, R.batch_to_torch(batch), cfg, return_debug=True)
    for k in KEYS:
        r = _rel_scalar(metrics[k], ref_metrics[k])
        print("T=64", k, float(metrics[k]), float(ref_metrics[k]), r)
        assert r < 1e-3, (k, float(metrics[k]), float(ref_metrics[k]))
    attn = gen(train=True).last_attn.cpu()
    assert attn.shape[-1] == 64 and torch.equal(attn.argmax(-1), dbg["aux"]["attn"].argmax(-1)), "attention indices must be identical"
    _check_grads(new_state.d_optimizer.arena.tree(new_state.d_optimizer.arena.grads), R.leaves(dbg["d_grad"]), 2e-3, "d_grad T=64")
    _check_grads(new_state.g_optimizer.arena.tree(new_state.g_optimizer.arena.grads), R.leaves(dbg["g_grad"]), 2e-3, "g_grad T=64")


def test_train_step_bf16_tiny_t64_runs_the_long_mfma_attention():
    from oracle import torch_ref as R
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.dtype = "bfloat16"
    gen, disc, state, ref_state, batch = _setup(cfg, 4)
    ops = gen(train=True).ops
    seen = []
    fwd = ops.attn_g_fwd

    def spy(region, words_n, max_len, gamma, ctx_out=None):
        seen.append((tuple(region.shape), words_n.shape[1], bool(ops.attn_g_sliced(region, words_n.shape[1])), ctx_out is not None))
        return fwd(region, words_n, max_len, gamma, ctx_out=ctx_out)
    ops.attn_g_fwd = spy
    try:
        tb = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}
        new_state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    finally:
        del ops.attn_g_fwd
    assert seen and all(t == 64 and sliced and direct for _, t, sliced, direct in seen), seen
    _, ref_metrics = R.train_step(ref_state, R.batch_to_torch(batch), cfg.copy())
    for k in KEYS:
        r = _rel_scalar(metrics[k], ref_metrics[k])
        print("bf16 T=64", k, float(metrics[k]), float(ref_metrics[k]), r)
        assert np.isfinite(float(metrics[k])) and r < 5e-2, k
    assert bool(torch.isfinite(new_state.g_optimizer.arena.params).all())


def test_graph_replay_is_bit_equal_to_eager_at_t64_and_reproducible():
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.configs import coco_xmc
    runs = []
    for mode in ("eager", "graph", "graph"):
        cfg = coco_xmc.get_test_config()
        cfg.dtype = "bfloat16"
        cfg.batch_size = 2
        gen, disc, st, _, batch = _setup(cfg, 2)
        tb = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}
        st, _ = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {})
        if mode == "graph":
            graphed = train_utils.GraphedTrainStep(st, tb, xmc_gan, gen, disc, cfg, {})
            st, m = graphed(graphed.state, tb)
        else:
            st, m = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {})
        torch.cuda.synchronize()
        runs.append(({k: float(v) for k, v in m.items()}, st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone()))
        del st, gen, disc
    for other in runs[1:]:
        assert runs[0][0] == other[0], (runs[0][0], other[0])
        assert torch.equal(runs[0][1], other[1]) and torch.equal(runs[0][2], other[2])
