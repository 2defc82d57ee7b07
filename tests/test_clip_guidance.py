"""config.clip_guidance_weight on the host: the float64 specifications of the image tower's data-gradient kernels
(utils/clip_grad.py) against autograd of the forward statements of tests/clip_ref.py, the differentiable oracle
(tests/clip_grad_ref.py) against clip_ref.encode_image, the switch's configuration checks, and train_g_d / train() with a stand-in
encoder on the CPU mock operator table.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from tests import clip_grad_ref as GR
from tests import clip_ref as R
from tests.cpu_ops_clip import CpuOpsClip
from xmcgan_image_generation_amd import synthetic as syn, train_utils, xmc_gan
from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.libml import clip_bpe
from xmcgan_image_generation_amd.nets import xmc_net
from xmcgan_image_generation_amd.utils import alignment_metrics as A, clip_grad, clip_utils


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ the specifications
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("t", [1, 5, 50])
def test_attention_bwd_spec_is_autograd_of_the_forward_statement(t, causal):
    n, h = 3, 128
    gen = torch.Generator().manual_seed(t + 7 * causal)
    qkv = torch.randn(n * t, 3 * h, generator=gen, dtype=torch.float64).requires_grad_(True)
    bias = 0.1 * torch.randn(3 * h, generator=gen, dtype=torch.float64)
    dctx = torch.randn(n * t, h, generator=gen, dtype=torch.float64)
    lens = np.array([t, 1, max(1, (2 * t) // 3)])
    ctx, _ = R.attention(qkv, bias, lens, t, causal=causal)
    (want,) = torch.autograd.grad(ctx, qkv, dctx)
    got = clip_grad.attention_bwd(qkv.detach().numpy(), bias.numpy(), lens, dctx.numpy(), t, causal)
    assert _rel(got, want.numpy()) <= 1e-12
    masked = got.reshape(n, t, 3, h)[1, 1:, 1:]                              # sequence 1 has one live key: k and v rows 1.. get nothing
    assert not masked.any()


@pytest.mark.parametrize("rows,h", [(7, 4), (9, 1024)])
def test_ln_bwd_spec_is_autograd_of_the_forward_statement(rows, h):
    gen = torch.Generator().manual_seed(rows + h)
    x = (2.0 * torch.randn(rows, h, generator=gen, dtype=torch.float64)).requires_grad_(True)
    gamma, beta = 1 + 0.1 * torch.randn(h, generator=gen, dtype=torch.float64), torch.randn(h, generator=gen, dtype=torch.float64)
    dy, dres = torch.randn(rows, h, generator=gen, dtype=torch.float64), torch.randn(rows, h, generator=gen, dtype=torch.float64)
    y, _ = R.layer_norm(x, gamma, beta)
    (want,) = torch.autograd.grad(y, x, dy)
    assert _rel(clip_grad.ln_bwd_add(x.detach().numpy(), gamma.numpy(), dy.numpy()), want.numpy()) <= 1e-12
    assert _rel(clip_grad.ln_bwd_add(x.detach().numpy(), gamma.numpy(), dy.numpy(), dres.numpy()), (want + dres).numpy()) <= 1e-12


@pytest.mark.parametrize("n,h,t", [(3, 128, 5), (2, 64, 50)])
def test_ln_bwd_row_maps_are_autograd_of_the_forward_statements(n, h, t):
    gen = torch.Generator().manual_seed(n + h + t)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    gamma, beta = 1 + 0.1 * rnd(h), rnd(h)
    # the pooled row: LN of row 0 of every sequence
    x, dy, dres = rnd(n * t, h).requires_grad_(True), rnd(n, h), rnd(n * t, h)
    pooled, _ = R.layer_norm(x.view(n, t, h)[:, 0], gamma, beta)
    (want,) = torch.autograd.grad(pooled, x, dy)
    got = clip_grad.ln_bwd_add(x.detach().numpy(), gamma.numpy(), dy.numpy(), mode="gather", t=t)
    assert _rel(got, want.numpy()) <= 1e-12 and not got.reshape(n, t, h)[:, 1:].any()
    got = clip_grad.ln_bwd_add(x.detach().numpy(), gamma.numpy(), dy.numpy(), dres.numpy(), mode="gather", t=t)
    assert _rel(got, (want + dres).numpy()) <= 1e-12
    # pre_layrnorm of clip_ref.vision_embed: the gradient of the patch products, the class row's dropped
    params = {R.V + "embeddings.class_embedding": rnd(h).numpy(), R.V + "embeddings.position_embedding.weight": rnd(t, h).numpy(),
              R.V + "pre_layrnorm.weight": gamma.numpy(), R.V + "pre_layrnorm.bias": beta.numpy()}
    pe, dyv = rnd(n * (t - 1), h).requires_grad_(True), rnd(n * t, h)
    y, _, _ = R.vision_embed(params, pe, n)
    (want,) = torch.autograd.grad(y, pe, dyv)
    got = clip_grad.ln_bwd_add(pe.detach().numpy(), gamma.numpy(), dyv.numpy(), mode="vision", t=t,
                               pos=params[R.V + "embeddings.position_embedding.weight"])
    assert _rel(got, want.numpy()) <= 1e-12


def test_quick_gelu_bwd_spec_is_autograd_of_the_forward_statement():
    gen = torch.Generator().manual_seed(3)
    x = (4.0 * torch.randn(51, 256, generator=gen, dtype=torch.float64)).requires_grad_(True)
    bias, dy = torch.randn(256, generator=gen, dtype=torch.float64), torch.randn(51, 256, generator=gen, dtype=torch.float64)
    (want,) = torch.autograd.grad(R.quick_gelu(x + bias), x, dy)
    assert _rel(clip_grad.bias_quick_gelu_bwd(x.detach().numpy(), bias.numpy(), dy.numpy()), want.numpy()) <= 1e-12


@pytest.mark.parametrize("hw,size,patch", [(32, 64, 32), (128, 224, 32), (256, 224, 32), (96, 64, 16)])
def test_preprocess_adjoint_is_the_transpose(hw, size, patch):
    rng = np.random.default_rng(hw + size)
    n, g = 2, size // patch
    x, y = rng.random((n, hw, hw, 3)), rng.standard_normal((n * g * g, 3 * patch * patch))
    ax = A.preprocess(x, size, patch) - A.preprocess(np.zeros_like(x), size, patch)       # the linear part
    lhs, rhs = float((ax * y).sum()), float((x * clip_grad.preprocess_adjoint(y, hw, size, patch)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), float(np.abs(ax).ravel() @ np.abs(y).ravel()))
    xt = torch.as_tensor(x).requires_grad_(True)                              # and autograd of the differentiable restatement
    (want,) = torch.autograd.grad(GR.preprocess(xt, size, patch), xt, torch.as_tensor(y))
    assert _rel(clip_grad.preprocess_adjoint(y, hw, size, patch), want.numpy()) <= 1e-12
    with pytest.raises(ValueError, match="multiple"):
        clip_grad.preprocess_adjoint(y, hw, size + 1, patch)


@pytest.mark.parametrize("over", [{}, {"image_size": 224}], ids=["small5", "small50"])
def test_differentiable_oracle_reproduces_clip_ref(over):
    params = R.small_params(**over)
    images = np.random.default_rng(11).random((2, 128 if over else 32, 128 if over else 32, 3)).astype(np.float32)
    want = R.encode_image(params, images)
    got = GR.encode_image(params, torch.as_tensor(images))
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max()) + 2e-15
    assert R.dense is not GR.dense                                           # the swap is undone
    fast = GR.encode_image(params, torch.as_tensor(images), round_bf16=True)       # the rounding dense: clip_ref's forward
    assert float((fast - R.encode_image(params, images, round_bf16=True)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the switch on the host
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB, MERGES = os.path.join(GOLDEN, "clip_bpe_vocab.json"), os.path.join(GOLDEN, "clip_bpe_merges.txt")
WORDS = ["a cat", "the dog sitting on a horse", "cat's dog", "a horse on the cat", "dog", "the cat on the dog", "horse 42",
         "sitting cat"]


def _cfg(lam=None, **kw):
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = 2
    if lam is not None:
        cfg.update(clip_guidance_weight=lam, clip_vocab_path=VOCAB, clip_merges_path=MERGES)
    cfg.update(kw)
    return cfg


def _guidance():
    """the real ``ClipGuidance`` at ``clip_ref.SMALL`` (128 px images shrunk to 64: 5 tokens), float32"""
    return clip_utils.ClipGuidance(R.small_params(), clip_bpe.ClipTokenizer(VOCAB, MERGES), fast=False)


@pytest.fixture()
def clip_table():
    xmc_net.set_ops_factory(lambda dtype: CpuOpsClip(dtype))
    yield
    xmc_net.set_ops_factory(None)


def test_check_config_rejections():
    xmc_net.check_config(_cfg())
    xmc_net.check_config(_cfg(0.0))
    xmc_net.check_config(_cfg(0.5))
    with pytest.raises(ValueError, match="must be >= 0"):
        xmc_net.check_config(_cfg(-0.1))
    for missing in ("clip_vocab_path", "clip_merges_path"):
        with pytest.raises(ValueError, match="clip_vocab_path and clip_merges_path"):
            xmc_net.check_config(_cfg(0.5, **{missing: None}))
    xmc_net.check_config(_cfg(0.0, clip_vocab_path=None, device_dataset_cache=True))      # off: nothing is asked for
    with pytest.raises(ValueError, match="device_dataset_cache=True: the cache carries no caption strings"):
        xmc_net.check_config(_cfg(0.5, device_dataset_cache=True))


def test_metric_keys():
    five = ("d_loss", "g_loss", "c_loss_d", "c_loss_g", "c_loss_g_pretrained")
    assert xmc_gan.METRIC_KEYS == five
    assert xmc_gan.metric_keys(_cfg()) == five and xmc_gan.metric_keys(_cfg(0.0)) == five
    assert xmc_gan.metric_keys(_cfg(0.25)) == five + ("c_loss_g_clip",)
    assert "clip_guidance_weight" not in coco_xmc.get_config() and "clip_guidance_weight" not in coco_xmc.get_c1_config()


def _one_step(lam, batch, text=None, guidance=None):
    cfg = _cfg(lam)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    state = train_utils.load_flax_params(state, gp, gs, dp, ds)
    batch = dict(batch)
    if text is not None:
        batch["clip_text"] = text
    extra = {"clip_guidance": guidance} if guidance is not None else {}
    grads = {}
    keep = xmc_gan._apply_adam

    def spy(ops, opt, *a, **kw):                     # the gradient arenas as the optimiser sees them
        grads[len(grads)] = opt.arena.grads.clone()
        return keep(ops, opt, *a, **kw)
    xmc_gan._apply_adam = spy
    try:
        half = train_utils.split_input_dict(batch, cfg.d_step_per_g_step)[-1]
        state, metrics = xmc_gan.train_g_d(0, state, half, gen, disc, cfg, extra)
    finally:
        xmc_gan._apply_adam = keep
    return metrics, grads[0], grads[1]               # (D's update comes first, then G's)


def test_train_g_d_adds_the_weighted_term_and_leaves_d_alone(clip_table):
    lam = 0.5
    cfg = _cfg()
    batch = {k: torch.as_tensor(v) for k, v in syn.make_batch(cfg, per_device_batch=2).items()}
    rows = batch["image"].shape[0]
    guidance = _guidance()
    text = guidance.embed_text(CpuOpsClip(), [WORDS[i % len(WORDS)] for i in range(rows)])
    assert text.shape == (rows, 64) and text.dtype == torch.float32
    off, d_off, g_off = _one_step(None, batch)
    on, d_on, g_on = _one_step(lam, batch, text, guidance)
    assert set(on) == set(off) | {"c_loss_g_clip"} and "c_loss_g_clip" not in off
    c = float(on["c_loss_g_clip"])
    assert np.isfinite(c) and c > 0.0
    assert abs((float(on["g_loss"]) - float(off["g_loss"])) - lam * c) <= 4 * 2.0 ** -24 * (abs(float(on["g_loss"])) + lam * c)
    assert torch.equal(on["d_loss"], off["d_loss"]) and torch.equal(d_on, d_off)
    assert not torch.equal(g_on, g_off)
    # a batch without the text rows, or with rows of another shape: ValueError naming the key
    with pytest.raises(ValueError, match="'clip_text'"):
        _one_step(lam, batch, None, guidance)
    with pytest.raises(ValueError, match=r"batch\['clip_text'\] must be \(2, 64\)"):
        _one_step(lam, batch, text[:, :32], guidance)


def _datasets(with_text):
    def hook(config, data_rng, start_step, rank, world, device):
        def batches():
            s = start_step
            while True:
                b = {k: torch.as_tensor(v) for k, v in syn.make_batch(config, per_device_batch=config.batch_size, seed=s).items()}
                if with_text:
                    b["text"] = [WORDS[(s + i) % len(WORDS)].encode() for i in range(b["image"].shape[0])]
                yield b
                s += 1
        return batches(), iter(()), 1000
    return hook


def _lines(workdir):
    with open(os.path.join(workdir, "metrics.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_train_writes_the_term_and_nothing_changes_with_the_key_absent(clip_table, tmp_path, monkeypatch):
    monkeypatch.setattr(clip_utils.ClipGuidance, "from_config", classmethod(lambda cls, config: _guidance()))
    on = str(tmp_path / "on")
    train_utils.train(_cfg(0.5, num_train_steps=2), on, datasets=_datasets(True))
    lines = _lines(on)
    assert [ln["step"] for ln in lines] == [1, 2]
    assert all(set(ln) == {"step", *xmc_gan.METRIC_KEYS, "c_loss_g_clip"} and np.isfinite(ln["c_loss_g_clip"]) for ln in lines)
    absent, zero = str(tmp_path / "absent"), str(tmp_path / "zero")
    train_utils.train(_cfg(num_train_steps=2), absent, datasets=_datasets(False))
    train_utils.train(_cfg(0.0, num_train_steps=2), zero, datasets=_datasets(True))
    assert _lines(absent) == _lines(zero) and all(set(ln) == {"step", *xmc_gan.METRIC_KEYS} for ln in _lines(absent))
    assert [ln["d_loss"] for ln in lines][0] == _lines(absent)[0]["d_loss"]    # the first step's D never sees the term
    with pytest.raises(ValueError, match="text"):                             # a stream without caption texts
        train_utils.train(_cfg(0.5, num_train_steps=2), str(tmp_path / "bare"), datasets=_datasets(False))
