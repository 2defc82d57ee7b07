"""KID and improved precision / recall on the host (utils/sample_metrics.py): the specification against brute-force loops, known
answers, the subset draw, ``EvalMetric.calculate_metrics`` against ``calculate_inception_fid``, and ``train_utils.test`` with the
extra columns on the CPU operator table.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_eval_metrics import _Batches, _StubGen, _config, _stub_inception, _stub_state
from xmcgan_image_generation_amd import train_utils
from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.nets import xmc_net
from xmcgan_image_generation_amd.utils import eval_metrics, sample_metrics as S


# ------------------------------------------------------------------------------------------------- brute force
def _brute_d2(a, b):
    return np.array([[float(np.sum((a[i].astype(np.float64) - b[j].astype(np.float64)) ** 2)) for j in range(len(b))]
                     for i in range(len(a))])


def _brute_radii(x, k):
    d = _brute_d2(x, x)
    return np.array([sorted(d[i, j] for j in range(len(x)) if j != i)[k - 1] for i in range(len(x))])


def _brute_hits(a, b, radii):
    d = _brute_d2(a, b)
    return np.array([any(d[i, j] <= radii[j] for j in range(len(b))) for i in range(len(a))])


@pytest.fixture(scope="module")
def small():
    r = np.random.default_rng(3)
    return r.standard_normal((7, 32)).astype(np.float32), (0.8 * r.standard_normal((5, 32)) + 0.2).astype(np.float32)


@pytest.mark.parametrize("k", [1, 3])
def test_spec_matches_brute_force_loops(small, k):
    real, fake = small                                           # n = 7, m = 5, d = 32
    for pool in (real, fake):
        np.testing.assert_allclose(S.knn_radii_spec(pool, k), _brute_radii(pool, k), rtol=0, atol=1e-11)
    for a, b in ((fake, real), (real, fake)):
        radii = _brute_radii(b, k)
        d = _brute_d2(a, b) - radii[None, :]
        assert np.abs(d).min() > 1e-9                            # no pair sits on a ball's surface: the decisions are stable
        assert np.array_equal(S.ball_hits_spec(a, b, radii), _brute_hits(a, b, radii))
    p, q = S.precision_recall_spec(fake, real, k)
    assert p == np.mean(_brute_hits(fake, real, _brute_radii(real, k)))
    assert q == np.mean(_brute_hits(real, fake, _brute_radii(fake, k)))
    assert S.precision_recall(fake, real, k) == (p, q)
    assert S.precision_recall(fake, real, k, real_radii=S.knn_radii_spec(real, k)) == (p, q)


def test_spec_works_across_row_blocks(monkeypatch):
    """the same numbers whether a pool is one block or many (BLOCK = 1024 in production, 3 here)"""
    r = np.random.default_rng(5)
    a, b = r.standard_normal((11, 32)), r.standard_normal((8, 32)) + 0.1
    idx = S.kid_subsets(11, 8, 2, 7, 0)
    want = S.knn_radii_spec(a, 2), S.ball_hits_spec(b, a, S.knn_radii_spec(a, 2)), S.poly3_sums_spec(a, idx[0], b, idx[1])
    monkeypatch.setattr(S, "BLOCK", 3)
    got = S.knn_radii_spec(a, 2), S.ball_hits_spec(b, a, S.knn_radii_spec(a, 2)), S.poly3_sums_spec(a, idx[0], b, idx[1])
    np.testing.assert_allclose(got[0], want[0], rtol=1e-13)
    assert np.array_equal(got[1], want[1])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-13)


def test_radii_need_more_rows_than_k():
    x = np.zeros((3, 32))
    with pytest.raises(ValueError):
        S.knn_radii_spec(x, 3)
    with pytest.raises(ValueError):
        S.knn_radii_spec(x, 0)
    assert S.knn_radii_spec(x, 2).shape == (3,)


# ------------------------------------------------------------------------------------------------- known answers
def test_a_permuted_pool_has_precision_and_recall_one():
    r = np.random.default_rng(0)
    real = r.standard_normal((9, 32))
    assert S.precision_recall_spec(real[r.permutation(9)], real, k=3) == (1.0, 1.0)


def test_far_apart_clusters_have_precision_and_recall_zero():
    r = np.random.default_rng(1)
    real = r.standard_normal((9, 32))
    shift = np.zeros(32)
    shift[0] = 100 * np.linalg.norm(real, axis=1).max()          # 100 norms away
    assert S.precision_recall_spec(real + shift, real, k=3) == (0.0, 0.0)


def test_a_row_repeated_more_than_k_times_has_radius_zero_and_is_still_hit():
    r = np.random.default_rng(2)
    k = 3
    pool = r.integers(-8, 9, (10, 32)).astype(np.float64)        # small integers: norms and dot products are exact in any order
    pool[:k + 1] = pool[0]                                       # one row k + 1 times
    radii = S.knn_radii_spec(pool, k)
    assert np.all(radii[:k + 1] == 0.0) and np.all(radii[k + 1:] > 0.0)
    hits = S.ball_hits_spec(pool[:1], pool[:k + 1], radii[:k + 1])       # against its copies alone: d2 = 0 <= 0
    assert hits.tolist() == [True]


# ------------------------------------------------------------------------------------------------- KID
def _brute_poly3(x, xi, y, yi):
    d = x.shape[1]
    k = lambda u, v: (float(np.dot(u.astype(np.float64), v.astype(np.float64))) / d + 1.0) ** 3         # noqa: E731
    out = []
    for s in range(len(xi)):
        xs, ys = x[xi[s]], y[yi[s]]
        m = len(xs)
        out.append([sum(k(xs[p], xs[q]) for p in range(m) for q in range(m) if p != q),
                    sum(k(ys[p], ys[q]) for p in range(m) for q in range(m) if p != q),
                    sum(k(xs[p], ys[q]) for p in range(m) for q in range(m))])
    return np.array(out)


def test_poly3_sums_match_brute_force(small):
    real, fake = small
    gi, ri = S.kid_subsets(len(fake), len(real), 3, 4, seed=1)
    np.testing.assert_allclose(S.poly3_sums_spec(fake, gi, real, ri), _brute_poly3(fake, gi, real, ri), rtol=1e-13)
    with pytest.raises(ValueError):
        S.poly3_sums_spec(fake, gi + len(fake), real, ri)        # an index outside the pool


def test_kid_of_full_subsets_is_the_same_in_every_subset():
    r = np.random.default_rng(4)
    a, b = np.abs(r.standard_normal((6, 32))), np.abs(r.standard_normal((6, 32)) + 0.3)
    gi, ri = S.kid_subsets(6, 6, 5, 6, seed=9)                   # subset_size = n: every subset is a permutation of the pool
    value, per = S.kid_from_sums(S.poly3_sums_spec(a, gi, b, ri), 6)
    np.testing.assert_allclose(per, per[0], rtol=1e-12)
    v, std = S.kid(a, b, subsets=5, subset_size=6, seed=9)
    assert v == value and std <= 1e-12 * max(1.0, abs(v))
    assert S.kid(a, a, subsets=2, subset_size=6)[0] < 0 < v      # the unbiased estimate of a pool against itself is below zero


def test_kid_is_symmetric_given_swapped_index_arrays(small):
    real, fake = small
    gi, ri = S.kid_subsets(len(fake), len(real), 4, 4, seed=2)
    ab = S.poly3_sums_spec(fake, gi, real, ri)
    ba = S.poly3_sums_spec(real, ri, fake, gi)
    np.testing.assert_allclose(ab[:, [1, 0, 2]], ba, rtol=1e-13)
    np.testing.assert_allclose(S.kid_from_sums(ab, 4)[1], S.kid_from_sums(ba, 4)[1], rtol=1e-12, atol=1e-15)


def test_kid_from_sums_formula():
    sums = np.array([[12.0, 6.0, 8.0], [24.0, 12.0, 16.0]])
    value, per = S.kid_from_sums(sums, 3)
    assert per.tolist() == [12 / 6 + 6 / 6 - 16 / 9, 24 / 6 + 12 / 6 - 32 / 9] and value == per.mean()


def test_kid_subsets_draw():
    a, b = S.kid_subsets(50, 40, 6, 10, seed=7), S.kid_subsets(50, 40, 6, 10, seed=7)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))       # deterministic in the seed
    assert not np.array_equal(a[0], S.kid_subsets(50, 40, 6, 10, seed=8)[0])
    assert a[0].dtype == a[1].dtype == np.int32 and a[0].shape == a[1].shape == (6, 10)
    rng = np.random.default_rng(7)                               # g then r, subset by subset, from one generator
    for s in range(6):
        assert np.array_equal(a[0][s], rng.choice(50, 10, replace=False))
        assert np.array_equal(a[1][s], rng.choice(40, 10, replace=False))
    gi, ri = S.kid_subsets(50, 4, 2, 10, seed=0)                 # clipped to the smaller pool
    assert gi.shape == ri.shape == (2, 4) and gi.max() < 50 and sorted(ri[0]) == [0, 1, 2, 3]
    assert all(len(set(row)) == 4 for row in gi)
    with pytest.raises(ValueError):
        S.kid_subsets(50, 1, 2, 10, seed=0)
    with pytest.raises(ValueError):
        S.kid_subsets(50, 40, 2, 1, seed=0)


def test_dispatch_takes_the_operator_table_when_it_has_the_entry_points(small):
    real, fake = small
    calls = []

    class Table:
        def knn_radii(self, x, k):
            calls.append("knn")
            return S.knn_radii_spec(x, k)

        def ball_hits(self, a, b, r):
            calls.append("hits")
            return S.ball_hits_spec(a, b, r)

        def poly3_sums(self, x, xi, y, yi):
            calls.append("poly3")
            return S.poly3_sums_spec(x, xi, y, yi)

    assert S.precision_recall(fake, real, 1, ops=Table()) == S.precision_recall_spec(fake, real, 1)
    assert calls == ["knn", "hits", "knn", "hits"]
    assert S.precision_recall(fake, real, 1, ops=Table(), real_radii=S.knn_radii_spec(real, 1)) == S.precision_recall_spec(fake, real, 1)
    assert calls[4:] == ["hits", "knn", "hits"]
    assert S.kid(fake, real, 2, 4, 0, ops=Table()) == S.kid(fake, real, 2, 4, 0) and calls[-1] == "poly3"
    assert S.kid(fake, real, 2, 4, 0, ops=object()) == S.kid(fake, real, 2, 4, 0)      # a table without them: the specification


# ------------------------------------------------------------------------------------------------- EvalMetric
def _metric(extras, seed=1, **kw):
    cfg = _config(9, 3, 2)
    cfg.eval_extra_metrics = extras
    cfg.update(kid_subsets=3, kid_subset_size=5, pr_k=2, **kw)
    return eval_metrics.EvalMetric(_Batches(3, seed=seed), cfg, inception=_stub_inception, chunk=4)


def test_calculate_metrics_keeps_the_eight_values_bit_for_bit():
    want = _metric(()).calculate_inception_fid(_StubGen, _stub_state(), 5)
    for extras in ((), ("kid",), ("precision_recall",), ("kid", "precision_recall")):
        got = _metric(extras).calculate_metrics(_StubGen, _stub_state(), 5)
        assert tuple(got[k] for k in train_utils.EVAL_KEYS) == want
        assert set(got) == set(train_utils.EVAL_KEYS) | set(eval_metrics.extra_metric_keys(extras))
    assert set(eval_metrics.extra_metric_keys(("kid",))) == {"kid", "kid_std", "ema_kid", "ema_kid_std"}
    assert set(eval_metrics.extra_metric_keys(("precision_recall",))) == {
        "precision", "precision_std", "recall", "recall_std", "ema_precision", "ema_precision_std", "ema_recall", "ema_recall_std"}


def test_calculate_metrics_extras_are_the_mean_and_std_of_the_spec_over_the_passes():
    em = _metric(("kid", "precision_recall"))
    got = em.calculate_metrics(_StubGen, _stub_state(), 5)
    em2 = _metric(("kid", "precision_recall"))
    kids, ekids, ps, rs = [], [], [], []
    for i in range(2):
        pool, _, epool, _ = em2._get_generated_pool_for_evaluation(_StubGen, _stub_state(), (i, 5))
        gi, ri = S.kid_subsets(9, 9, 3, 5, np.random.SeedSequence([5, i, 0x4B4944]))
        kids.append(S.kid_from_sums(S.poly3_sums_spec(pool, gi, em2._pool, ri), 5)[0])
        ekids.append(S.kid_from_sums(S.poly3_sums_spec(epool, gi, em2._pool, ri), 5)[0])      # the same subsets for the EMA pool
        p, r = S.precision_recall_spec(pool, em2._pool, 2)
        ps.append(p), rs.append(r)
    assert (got["kid"], got["kid_std"]) == (float(np.mean(kids)), float(np.std(kids)))
    assert (got["ema_kid"], got["ema_kid_std"]) == (float(np.mean(ekids)), float(np.std(ekids)))
    assert (got["precision"], got["precision_std"]) == (float(np.mean(ps)), float(np.std(ps)))
    assert (got["recall"], got["recall_std"]) == (float(np.mean(rs)), float(np.std(rs)))
    assert em.calculate_metrics(_StubGen, _stub_state(), 5) == got and em.calculate_metrics(_StubGen, _stub_state(), 6) != got


def test_real_radii_are_computed_once(monkeypatch):
    em = _metric(("precision_recall",))
    seen = []
    real = S.knn_radii
    monkeypatch.setattr(S, "knn_radii", lambda x, k, ops=None: (seen.append(len(x)), real(x, k, ops))[1])
    em.calculate_metrics(_StubGen, _stub_state(), 5)
    em.calculate_metrics(_StubGen, _stub_state(), 6)
    real_calls = [i for i, n in enumerate(seen) if n == 9]
    assert len(seen) == 1 + 2 * 2 * 2             # the real pool once; every generated pool (2 calls x 2 passes x {current, EMA})
    assert real_calls[0] == 0 and np.array_equal(em.real_radii(2), S.knn_radii_spec(em._pool, 2))


# ------------------------------------------------------------------------------------------------- check_config
def test_check_config_rejects_unknown_metrics_and_a_pr_k_that_needs_more_rows():
    cfg = coco_xmc.get_test_config()
    assert tuple(cfg.eval_extra_metrics) == () and (cfg.kid_subsets, cfg.kid_subset_size, cfg.pr_k) == (100, 1000, 3)
    xmc_net.check_config(cfg)
    cfg.eval_extra_metrics = ("kid", "density")
    with pytest.raises(ValueError, match="density"):
        xmc_net.check_config(cfg)
    cfg.eval_extra_metrics = ("precision_recall",)
    cfg.eval_num, cfg.pr_k = 8, 8
    with pytest.raises(ValueError, match="pr_k"):
        xmc_net.check_config(cfg)
    cfg.pr_k = 7
    xmc_net.check_config(cfg)


# ------------------------------------------------------------------------------------------------- test() end to end
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from tests.cpu_ops import CpuOps
    from tests.test_train_loop import _cfg, synthetic_datasets
    xmc_net.set_ops_factory(lambda dtype: CpuOps(dtype))
    try:
        workdir = str(tmp_path_factory.mktemp("extras"))
        cfg = _cfg(num_train_steps=2, checkpoint_every_steps=1, eval_every_steps=2, eval_num=6, eval_batch_size=2, eval_avg_num=2)
        train_utils.train(cfg, workdir, datasets=synthetic_datasets())
        yield cfg, workdir
    finally:
        xmc_net.set_ops_factory(None)


def _features(images):
    x = torch.as_tensor(images).float()
    pool = torch.cat([x.mean(dim=(1, 2)), x.std(dim=(1, 2)), x[:, ::32, ::32, 0].reshape(x.shape[0], -1)], 1).numpy()
    return pool, torch.softmax(torch.as_tensor(pool[:, :5]), 1).numpy()


def _eval_data(config, data_rng, start_step, rank, world, device):
    from xmcgan_image_generation_amd import synthetic as syn

    def batches():
        s = 100
        while True:
            yield {k: torch.as_tensor(v) for k, v in syn.make_batch(config, per_device_batch=config.eval_batch_size, seed=s).items()}
            s += 1
    return iter(()), batches(), 0


def test_test_mode_writes_exactly_the_new_columns(trained, tmp_path):
    import shutil
    cfg, workdir = trained
    plain, extra = str(tmp_path / "plain"), str(tmp_path / "extra")
    shutil.copytree(workdir, plain), shutil.copytree(workdir, extra)
    ecfg = cfg.copy()
    ecfg.update(eval_extra_metrics=("kid", "precision_recall"), kid_subsets=2, kid_subset_size=4, pr_k=2)
    assert train_utils.test(cfg, plain, datasets=_eval_data, inception=_features, timeout=0) == 2
    assert train_utils.test(ecfg, extra, datasets=_eval_data, inception=_features, timeout=0) == 2
    head = lambda d: open(os.path.join(d, "checkpoints-0", "scores.csv"), newline="").read().split("\r\n")[0].split(",")    # noqa: E731
    old = ["checkpoint_path", "step"] + sorted(f"eval/{k}" for k in train_utils.EVAL_KEYS)
    new = sorted(f"eval/{k}" for k in eval_metrics.extra_metric_keys(("kid", "precision_recall")))
    assert head(plain) == old and len(new) == 12
    assert head(extra) == ["checkpoint_path", "step"] + sorted(old[2:] + new)
    rows = lambda d: [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl")) if "eval/fid" in l]                     # noqa: E731
    for a, b in zip(rows(plain), rows(extra)):
        assert set(b) - set(a) == set(new) and all(a[k] == b[k] for k in a)            # FID / IS as without the extras
        assert 0.0 <= b["eval/precision"] <= 1.0 and 0.0 <= b["eval/recall"] <= 1.0 and np.isfinite(b["eval/kid"])
    # a scores.csv started with other columns: ValueError before anything is evaluated, in either direction
    before = open(os.path.join(plain, "metrics.jsonl")).read()
    with pytest.raises(ValueError, match="eval/kid"):
        train_utils.test(ecfg, plain, datasets=_eval_data, inception=_features, timeout=0)
    with pytest.raises(ValueError, match="eval/kid"):
        train_utils.test(cfg, extra, datasets=_eval_data, inception=_features, timeout=0)
    assert open(os.path.join(plain, "metrics.jsonl")).read() == before
