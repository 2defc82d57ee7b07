"""config.train_statistics on the CPU operator table (tests/cpu_ops.py; ``TrainStatistics`` restates its two launches in float64
torch there): the per-step vector against the oracle, the switch changing nothing else, and the training loop's two files."""
import json
import os
import re

import pytest
import torch

from tests import stats_reference as SR
from tests.cpu_ops import CpuOps
from xmcgan_image_generation_amd import synthetic as syn
from xmcgan_image_generation_amd import train_utils, xmc_gan
from xmcgan_image_generation_amd.nets import xmc_net
from xmcgan_image_generation_amd.train_statistics import TrainStatistics, arena_leaves


@pytest.fixture(scope="module")
def cpu_table():
    xmc_net.set_ops_factory(lambda dtype: CpuOps(dtype))
    yield
    xmc_net.set_ops_factory(None)


def _step(ref, on):
    cfg = ref["cfg"].copy()
    cfg.train_statistics = on
    additional = xmc_gan.create_additional_data(cfg)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, ref["gp"], ref["gs"], ref["dp"], ref["ds"])
    tb = {k: torch.as_tensor(v) for k, v in ref["batch"].items()}
    state, metrics = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, additional)
    return cfg, additional, disc, state, metrics


def test_names_are_the_statistic_dict_then_the_summaries():
    assert TrainStatistics.NAMES[:15] == tuple(xmc_net.STAT_KEYS) and len(TrainStatistics.NAMES) == 25
    assert TrainStatistics.NAMES[15:] == ("real_logit_mean", "fake_logit_mean", "real_margin_frac", "fake_margin_frac", "d_grad_norm",
                                          "g_grad_norm", "d_param_norm", "g_param_norm", "d_sigma_min", "d_sigma_max")


_STEPPED = {}


def _stepped(b):
    if b not in _STEPPED:
        ref = SR.reference(b)
        _STEPPED[b] = (ref, *_step(ref, True))
    return _STEPPED[b]


@pytest.mark.parametrize("b", [4, 2])
def test_accuracies_match_the_oracle_exactly(cpu_table, b):
    """equal to ``get_statistics`` of the oracle's ten matrices in float64, exactly, no row excluded.  No data seed separates every
    row's two largest entries by 1e-3 at C0 (tests/stats_reference.py has the figures: smallest gaps 7.6e-07 .. 8.1e-06 at B = 4,
    1.8e-06 .. 3.5e-05 at B = 2): the comparison runs on the best of the scanned seeds."""
    ref, _, additional, _, _, _ = _stepped(b)
    stats = additional["statistics"]
    SR.check_accuracies(dict(zip(stats.NAMES, stats.vec.double().tolist())), ref)


@pytest.mark.parametrize("b", [4, 2])
def test_values_match_the_oracle(cpu_table, b):
    """head losses at test_host_logic's loss tolerance (2e-4), entropies within ten times their response to the logit tolerance,
    logit summary from the oracle's logits, gradient norms at test_host_logic's 2e-3, parameter norms against the oracle's
    state in front of train_g_d's update (1e-3: the post-step parameter bar)"""
    ref, _, additional, disc, state, metrics = _stepped(b)
    stats = additional["statistics"]
    got = dict(zip(stats.NAMES, stats.vec.double().tolist()))
    SR.check_values(got, ref, loss_tol=2e-4, grad_tol=2e-3, param_tol=1e-3)
    sigma = disc(train=True)._sn_ctx[3].view(-1, 2)[:, 0]
    assert got["d_sigma_min"] == float(sigma.min()) and got["d_sigma_max"] == float(sigma.max()) and got["d_sigma_min"] > 0
    window = stats.read()
    assert window["count"] == 1 and window["first_bad"] is None
    assert window["sums"] == {k: float(v) for k, v in zip(stats.NAMES, stats.vec.double().tolist())}
    # the per-tensor table: one row per physical tensor, D's first; its sums are the global norms
    d_arena, g_arena = state.d_optimizer.arena, state.g_optimizer.arena
    names = [f"d/{p}" for p, _, _ in arena_leaves(d_arena)] + [f"g/{p}" for p, _, _ in arena_leaves(g_arena)]
    assert list(window["leaves"]) == names
    gsq = sum(v[0] for k, v in window["leaves"].items() if k.startswith("d/"))
    assert abs(gsq ** 0.5 - got["d_grad_norm"]) <= 1e-6 * got["d_grad_norm"]
    assert all(v[2] == 0 for v in window["leaves"].values())
    # the gradient arenas still hold what the updates consumed (the CPU table's optimiser leaves them)
    for which, arena in (("d", d_arena), ("g", g_arena)):
        for p, off, n in arena_leaves(arena):
            want = float(arena.grads[off:off + n].double().pow(2).sum())
            assert abs(window["leaves"][f"{which}/{p}"][0] - want) <= 1e-12 * max(want, 1e-300), p


def test_a_switched_off_head_reports_zero(cpu_table):
    ref = SR.reference(2, dict(word_contrastive=False))
    _, additional, _, _, _ = _step(ref, True)
    stats = additional["statistics"]
    got = dict(zip(stats.NAMES, stats.vec.tolist()))
    for head in ("fake_word", "real_word"):
        assert got[f"{head}_loss"] == 0 and got[f"{head}_acc"] == 0 and got[f"{head}_entropy"] == 0
    SR.check_values(got, ref, loss_tol=2e-4, grad_tol=2e-3, param_tol=1e-3)


def test_off_changes_nothing(cpu_table):
    ref = SR.reference(2)
    cfg_off, additional_off, _, state_off, metrics_off = _step(ref, False)
    assert "statistics" not in additional_off and "statistics" not in xmc_gan.create_additional_data(cfg_off)
    assert cfg_off.train_statistics is False
    from xmcgan_image_generation_amd.configs import coco_xmc
    for make in (coco_xmc.get_config, coco_xmc.get_test_config, coco_xmc.get_c1_config, coco_xmc.get_c3_config, coco_xmc.get_c4_config):
        assert make().train_statistics is False
    _, additional_on, _, state_on, metrics_on = _step(ref, True)
    assert isinstance(additional_on["statistics"], TrainStatistics)
    assert tuple(metrics_on) == tuple(metrics_off) and set(metrics_on) == set(xmc_gan.METRIC_KEYS)
    a, b = SR.snapshot(state_on, metrics_on), SR.snapshot(state_off, metrics_off)
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# --------------------------------------------------------------------------------------------------------------- the loop
def _datasets(poison_step=None):
    def hook(config, data_rng, start_step, rank, world, device):
        def batches():
            s = start_step
            while True:
                batch = {k: torch.as_tensor(v) for k, v in syn.make_batch(config, per_device_batch=config.batch_size, seed=s).items()}
                if s == poison_step:
                    batch["image"][-1, 3, 5, 1] = float("inf")          # (the train_g_d half of the batch)
                yield batch
                s += 1
        return batches(), iter(()), 1000
    return hook


def _loop_cfg(**kw):
    from xmcgan_image_generation_amd.configs import coco_xmc
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = 2
    cfg.update(dict(num_train_steps=4, eval_every_steps=2, checkpoint_every_steps=100, train_statistics=True))
    cfg.update(kw)
    return cfg


def test_loop_writes_window_means_and_layer_stats(cpu_table, tmp_path):
    cfg = _loop_cfg()
    state = train_utils.train(cfg, str(tmp_path), datasets=_datasets())
    lines = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    assert [l["step"] for l in lines] == [2, 4]
    for line in lines:
        assert set(line) == {"step", *xmc_gan.METRIC_KEYS, *(f"stats/{k}" for k in TrainStatistics.NAMES)}
        # the window means of the head losses add up to the window means of the contrastive metrics
        assert abs(line["stats/real_word_loss"] + line["stats/real_sentence_loss"] - line["c_loss_d"]) <= 1e-5 * abs(line["c_loss_d"])
        assert 0.0 <= line["stats/real_sentence_acc"] <= 1.0 and line["stats/d_grad_norm"] > 0 and line["stats/g_param_norm"] > 0
    layers = [json.loads(l) for l in open(tmp_path / "layer_stats.jsonl")]
    assert [l["step"] for l in layers] == [2, 4] and [l["count"] for l in layers] == [2, 2]
    n_tensors = len(arena_leaves(state.d_optimizer.arena)) + len(arena_leaves(state.g_optimizer.arena))
    for line in layers:
        assert len(line["leaves"]) == n_tensors
        assert all(set(v) == {"grad_norm_rms", "param_norm_rms", "nonfinite"} and v["nonfinite"] == 0 for v in line["leaves"].values())
        d_sq = sum(v["grad_norm_rms"] ** 2 for k, v in line["leaves"].items() if k.startswith("d/"))
        assert d_sq > 0
    # the second window was zeroed at the first boundary: its RMS gradient norm is not the first window's
    assert layers[0]["leaves"] != layers[1]["leaves"]


def test_loop_without_the_switch_writes_what_it_wrote(cpu_table, tmp_path):
    train_utils.train(_loop_cfg(train_statistics=False, num_train_steps=2), str(tmp_path), datasets=_datasets())
    line = json.loads(open(tmp_path / "metrics.jsonl").readline())
    assert set(line) == {"step", *xmc_gan.METRIC_KEYS} and not os.path.exists(tmp_path / "layer_stats.jsonl")


def test_non_finite_stop_names_the_first_leaf(cpu_table, tmp_path):
    cfg = _loop_cfg()
    with pytest.raises(FloatingPointError) as e:
        train_utils.train(cfg, str(tmp_path), datasets=_datasets(poison_step=2))
    m = re.search(r"not finite at step 2; .*the first gradient that held a non-finite value was (\S+) at step 2$", str(e.value))
    assert m, str(e.value)
    _, _, state = train_utils.create_train_state(cfg, 0)
    assert m.group(1) == f"d/{arena_leaves(state.d_optimizer.arena)[0][0]}"          # arena order, D before G
    with pytest.raises(FloatingPointError) as e_off:
        train_utils.train(_loop_cfg(train_statistics=False), str(tmp_path / "off"), datasets=_datasets(poison_step=2))
    assert str(e_off.value).endswith(")") and "gradient" not in str(e_off.value)
