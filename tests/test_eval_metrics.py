"""FID / Inception Score on the CPU: the metric math against closed forms and scipy, the Inception-v3 layer table against
Keras' published counts, the checkpoint loader, the plan of InceptionV3Features against the torch restatement
(tests/inception_ref.py) through the CPU operator table, and the host logic of EvalMetric with stub networks (batch
counts, truncation, chunking, the 8-tuple, a 2-rank gloo run)."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.utils import eval_metrics, inception_arch as A, inception_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ FID / IS math
def _orthonormal_centered(rng, n, d):
    x = rng.standard_normal((n, d))
    q, _ = np.linalg.qr(x - x.mean(0))
    return q                                            # zero-mean orthonormal columns: sample covariance exactly diagonal


def test_fid_of_a_pool_against_itself_is_zero():
    p = np.random.default_rng(0).standard_normal((300, 32)) @ np.random.default_rng(1).standard_normal((32, 32))
    assert abs(U.calculate_fid(p, p)) < 1e-9 * np.trace(np.cov(p, rowvar=False))


def test_fid_of_diagonal_gaussians_matches_the_closed_form():
    rng = np.random.default_rng(2)
    n, d = 400, 24
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    sd1, sd2 = rng.uniform(0.2, 2.0, d), rng.uniform(0.2, 2.0, d)
    p1 = mu1 + np.sqrt(n - 1) * _orthonormal_centered(rng, n, d) * sd1
    p2 = mu2 + np.sqrt(n - 1) * _orthonormal_centered(rng, n, d) * sd2
    want = np.sum((mu1 - mu2) ** 2) + np.sum((sd1 - sd2) ** 2)
    assert U.calculate_fid(p1, p2) == pytest.approx(want, rel=1e-9)


def test_fid_matches_scipy_sqrtm_on_non_commuting_covariances():
    linalg = pytest.importorskip("scipy.linalg")
    rng = np.random.default_rng(3)
    d = 20
    p1 = rng.standard_normal((500, d)) @ rng.standard_normal((d, d)) + 1.0
    p2 = rng.standard_normal((500, d)) @ rng.standard_normal((d, d)) * 0.5
    mu1, mu2 = p1.mean(0), p2.mean(0)
    s1, s2 = np.cov(p1, rowvar=False), np.cov(p2, rowvar=False)
    assert not np.allclose(s1 @ s2, s2 @ s1)
    covmean = linalg.sqrtm(s1 @ s2).real                  # the reference's _calculate_frechet_distance
    want = (mu1 - mu2) @ (mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean)
    assert U.calculate_fid(p1, p2) == pytest.approx(want, rel=1e-6)


def test_inception_score_of_uniform_predictions_is_one():
    m, s = U.calculate_inception_score(np.full((40, 1000), 1e-3), num_splits=4)
    assert m == pytest.approx(1.0, abs=1e-12) and s == pytest.approx(0.0, abs=1e-12)


def test_inception_score_of_evenly_spread_one_hots_is_the_class_count():
    k = 8
    pred = np.full((4 * k, k), 1e-30)
    pred[np.arange(4 * k), np.arange(4 * k) % k] = 1.0
    m, s = U.calculate_inception_score(pred, num_splits=2)
    assert m == pytest.approx(k, rel=1e-9) and s == pytest.approx(0.0, abs=1e-9)


def test_inception_score_split_arithmetic_drops_the_remainder():
    rng = np.random.default_rng(4)
    pred = rng.dirichlet(np.ones(10) * 0.3, size=11)
    m, s = U.calculate_inception_score(pred, num_splits=3)          # chunks of 3: rows 0..8, rows 9, 10 dropped
    scores = []
    for i in range(3):
        c = pred[3 * i:3 * i + 3]
        py = c.mean(0)
        scores.append(np.exp(np.mean([np.sum(r * (np.log(r) - np.log(py))) for r in c])))
    assert m == pytest.approx(np.mean(scores), rel=1e-12) and s == pytest.approx(np.std(scores), rel=1e-9)
    pred2 = pred.copy()
    pred2[9:] = rng.dirichlet(np.ones(10), size=2)
    assert U.calculate_inception_score(pred2, num_splits=3) == (m, s)


# ------------------------------------------------------------------------------------------------ the layer table
def test_layer_table_matches_the_published_counts():
    assert len(A.CONVS) == 94
    assert [c.name for c in A.CONVS] == [f"ConvBatchNormReluBlock_{i}" for i in range(94)]
    assert A.param_counts() == (23_817_352, 17_216, 23_851_784)
    assert A.macs_per_image() == pytest.approx(5.713e9, rel=1e-3)
    assert A.flops_per_image() / 1e9 == pytest.approx(11.43, abs=0.005)
    assert len(A.geometries()) == 43
    params, stats = A.param_shapes()
    assert params["ConvBatchNormReluBlock_0"]["Conv_0"]["kernel"] == (3, 3, 3, 32)
    assert params["ConvBatchNormReluBlock_93"]["Conv_0"]["kernel"] == (1, 1, 2048, 192)
    assert params["Dense_0"] == {"kernel": (2048, 1000), "bias": (1000,)}
    assert stats["ConvBatchNormReluBlock_5"]["BatchNorm_0"]["var"] == (64,)
    assert [A.BUFFERS[m] for m in A.MIXED] == [(35, 35, 256), (35, 35, 288), (35, 35, 288)] + [(17, 17, 768)] * 5 + \
        [(8, 8, 1280), (8, 8, 2048), (8, 8, 2048)]
    # every branch writes a disjoint slice, and the slices of a concatenation tile it exactly
    for m in A.MIXED:
        ranges = sorted((s.dst_off, s.dst_off + (s.cout if isinstance(s, A.ConvSpec) else A.BUFFERS[s.src][2]))
                        for s in A.STEPS if s.dst == m)
        assert ranges[0][0] == 0 and ranges[-1][1] == A.BUFFERS[m][2]
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (m, ranges)
    c0 = A.CONVS[0]
    assert (c0.hi, c0.ho, c0.stride, c0.padding) == (299, 149, 2, "VALID")
    assert sum(1 for s in A.STEPS if isinstance(s, A.PoolSpec) and s.kind == "max") == 4
    assert sum(1 for s in A.STEPS if isinstance(s, A.PoolSpec) and s.kind == "avg") == 9


def test_random_init_keeps_every_mixed_block_alive():
    from tests import inception_ref as R
    p, s = A.init_inception(0)
    img = np.random.default_rng(5).random((1, 64, 64, 3), dtype=np.float32)
    _, logits, mixed = R.forward(p, s, img, torch.float32, return_mixed=True)
    for m in mixed:
        rms, alive = float(m.pow(2).mean().sqrt()), float((m > 0).float().mean())
        assert 0.3 < rms < 5.0 and 0.3 < alive < 0.8, (rms, alive)
    assert float(U.softmax(logits.numpy()).max()) < 0.9


# ------------------------------------------------------------------------------------------------ the loader
def _tiny_tree(with_scale):
    p, s = A.init_inception(1)
    if with_scale:
        for k in p:
            if k.startswith("ConvBatchNorm"):
                p[k]["BatchNorm_0"]["scale"] = np.full_like(p[k]["BatchNorm_0"]["bias"], 7.0)   # the Keras mapping's leaf
    return {"params": p, "batch_stats": s}


@pytest.mark.parametrize("fmt", ["npy", "msgpack"])
def test_loader_round_trips_both_formats(tmp_path, fmt):
    tree = _tiny_tree(with_scale=True)
    path = str(tmp_path / f"inception.{fmt}")
    if fmt == "npy":
        np.save(path, tree, allow_pickle=True)
    else:
        from xmcgan_image_generation_amd.utils.checkpoint import msgpack_serialize
        with open(path, "wb") as f:
            f.write(msgpack_serialize(tree))
    got = U.inception_model(path)
    for spec in A.CONVS[::13]:
        for a, b in zip(U.fold_block(got["params"], got["batch_stats"], spec),
                        U.fold_block(tree["params"], tree["batch_stats"], spec)):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got["params"]["Dense_0"]["kernel"], tree["params"]["Dense_0"]["kernel"])


def test_loader_missing_path_raises_and_none_is_random(tmp_path):
    with pytest.raises(FileNotFoundError):
        U.inception_model(str(tmp_path / "absent.npy"))
    a, b = U.inception_model(None), U.inception_model(None)
    np.testing.assert_array_equal(a["params"]["ConvBatchNormReluBlock_7"]["Conv_0"]["kernel"],
                                  b["params"]["ConvBatchNormReluBlock_7"]["Conv_0"]["kernel"])


def test_bn_fold_ignores_scale_and_matches_float64():
    from tests import inception_ref as R
    tree = _tiny_tree(with_scale=True)
    spec = A.CONVS[12]                                       # the 5x5 of mixed0
    w, b = U.fold_block(tree["params"], tree["batch_stats"], spec)
    x = torch.randn(2, 9, 9, spec.cin, dtype=torch.float64)
    got = R.conv_ref(x, torch.as_tensor(w), torch.as_tensor(b), kh=spec.kh, kw=spec.kw, pad=spec.pad, relu=False)
    p, s = tree["params"][spec.name], tree["batch_stats"][spec.name]["BatchNorm_0"]
    k = torch.as_tensor(p["Conv_0"]["kernel"]).double().permute(3, 2, 0, 1)
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), k, padding=spec.pad)
    t = lambda a: torch.as_tensor(a).double()[None, :, None, None]      # noqa: E731
    want = ((y - t(s["mean"])) / torch.sqrt(t(s["var"]) + 1e-3) + t(p["BatchNorm_0"]["bias"])).permute(0, 2, 3, 1)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ the plan on CPU
def test_plan_matches_the_restatement_and_issues_no_concatenation(monkeypatch):
    from tests import inception_ref as R
    p, s = A.init_inception(2)
    img = np.random.default_rng(6).random((2, 40, 40, 3), dtype=np.float32)
    pool_ref, logits_ref = R.forward(p, s, img, torch.float64)
    ops = R.CountingOps(torch.float64)
    f = U.InceptionV3Features(ops, p, s)

    def no_cat(*a, **k):
        raise AssertionError("the forward concatenates")
    monkeypatch.setattr(torch, "cat", no_cat)
    pool, preds = f(img)
    monkeypatch.undo()
    assert ops.calls == {"inception_resize": 1, "inception_conv": 94, "maxpool3x3s2_valid": 4, "avgpool3x3_same": 9,
                         "mean_hw": 1, "gemm": 1}
    assert pool.shape == (2, 2048) and pool.dtype == np.float32 and preds.shape == (2, 1000)
    # the folded weights are float32 (as on the GPU): agreement to float32 rounding of the weights
    assert np.abs(pool - pool_ref.numpy()).max() <= 1e-5 * np.abs(pool_ref.numpy()).max()
    np.testing.assert_allclose(preds, U.softmax(logits_ref.numpy()), atol=1e-6)
    np.testing.assert_allclose(preds.sum(1), 1.0, atol=1e-5)
    bufs = f._bufs[(2, 40, 40)]
    f(img)
    assert f._bufs[(2, 40, 40)] is bufs and len(f._bufs) == 1          # buffers reused across calls of one shape


# ------------------------------------------------------------------------------------------------ EvalMetric host logic
class _Batches:
    """an endless dataset iterator that counts the batches drawn"""

    def __init__(self, b, hw=8, seed=0):
        self.b, self.hw, self.rng, self.drawn = b, hw, np.random.default_rng(seed), 0

    def __iter__(self):
        return self

    def __next__(self):
        self.drawn += 1
        b = self.b
        return {"image": self.rng.random((b, self.hw, self.hw, 3), dtype=np.float32),
                "sentence_embedding": np.zeros((b, 4), np.float32), "embedding": np.zeros((b, 3, 4), np.float32),
                "max_len": np.full((b,), 3, np.int32)}


def _stub_inception(images):
    """per-image features (so chunking cannot change them): channel means / stds / products, softmax over 6 classes"""
    x = torch.as_tensor(images).double().reshape(images.shape[0], -1, 3)
    m, sd = x.mean(1), x.std(1)
    pool = torch.cat([m, sd, m * sd, m ** 2], 1).numpy().astype(np.float32)
    z = 8 * torch.cat([m, sd], 1).numpy()
    return pool, U.softmax(z).astype(np.float32)


class _StubGen:
    """eval_step's generator: apply(variables, (cond, z)) -> (B, 8, 8, 3) images in [0, 1] from z and the parameters"""

    def __init__(self, train=False):
        pass

    def apply(self, variables, inputs, mutable=False):
        _, z = inputs
        a = float(variables["params"]["a"])
        base = torch.sigmoid(a * z[:, :3])[:, None, None, :]
        ramp = torch.linspace(0, 1, 8)[None, :, None, None] * z[:, 3:4, None, None].abs()
        return torch.clamp(base * 0.8 + 0.2 * ramp.expand(-1, 8, 8, 3), 0, 1)


def _stub_state():
    return types.SimpleNamespace(step=1, g_optimizer=types.SimpleNamespace(target={"a": 1.0}), ema_params={"a": 0.5},
                                 generator_state={})


def _config(eval_num=10, bs=3, avg=2):
    cfg = coco_xmc.get_test_config()
    cfg.eval_num, cfg.eval_batch_size, cfg.eval_avg_num = eval_num, bs, avg
    return cfg


def test_config_carries_the_reference_eval_sizes():
    assert (coco_xmc.get_config().eval_num, coco_xmc.get_config().eval_avg_num) == (30000, 3)
    assert (coco_xmc.get_test_config().eval_num, coco_xmc.get_test_config().eval_avg_num) == (2, 1)


def test_eval_metric_draws_the_reference_batch_counts_and_truncates():
    ds = _Batches(3)
    calls = []
    em = eval_metrics.EvalMetric(ds, _config(10, 3, 2), inception=lambda im: (calls.append(len(im)), _stub_inception(im))[1],
                                 chunk=5)
    assert ds.drawn == 10 // 3 + 1 and em._pool.shape == (10, 12)          # 4 batches = 12 images, truncated to 10
    assert calls == [5, 5, 2]                                              # chunks of 5 whatever the batch size
    out = em.calculate_inception_fid(_StubGen, _stub_state(), 7)
    assert ds.drawn == 4 + 2 * 4
    assert len(out) == 8 and all(np.isfinite(out))


def test_eval_metric_chunking_does_not_change_the_result():
    res = []
    for chunk in (1, 4, 7, 256):
        em = eval_metrics.EvalMetric(_Batches(3), _config(10, 3, 2), inception=_stub_inception, chunk=chunk)
        res.append(em.calculate_inception_fid(_StubGen, _stub_state(), 11))
    assert all(r == res[0] for r in res), res


def test_eval_metric_tuple_is_the_mean_and_std_over_passes():
    cfg = _config(9, 3, 3)
    em = eval_metrics.EvalMetric(_Batches(3, seed=1), cfg, num_splits=2, inception=_stub_inception, chunk=4)
    out = em.calculate_inception_fid(_StubGen, _stub_state(), 5)
    em2 = eval_metrics.EvalMetric(_Batches(3, seed=1), cfg, num_splits=2, inception=_stub_inception, chunk=4)
    fids, iss, efids, eiss = [], [], [], []
    for i in range(3):
        pool, preds, epool, epreds = em2._get_generated_pool_for_evaluation(_StubGen, _stub_state(), (i, 5))
        assert pool.shape == (9, 12) and preds.shape == (9, 6)
        fids.append(U.calculate_fid(pool, em2._pool))
        efids.append(U.calculate_fid(epool, em2._pool))
        iss.append(U.calculate_inception_score(preds, 2)[0])
        eiss.append(U.calculate_inception_score(epreds, 2)[0])
    want = (np.mean(fids), np.std(fids), np.mean(iss), np.std(iss), np.mean(efids), np.std(efids), np.mean(eiss), np.std(eiss))
    np.testing.assert_allclose(out, want, rtol=1e-12)
    assert out[1] > 0 and out[0] != out[4]                                # passes differ; EMA images differ
    assert em.calculate_inception_fid(_StubGen, _stub_state(), 5) == out  # same rng, same numbers
    assert em.calculate_inception_fid(_StubGen, _stub_state(), 6) != out
    assert len({eval_metrics.batch_seed(5, i, s) for i in range(3) for s in range(4)}) == 12


# ------------------------------------------------------------------------------------------------ 2 ranks, gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests.test_eval_metrics import _Batches, _StubGen, _config, _stub_inception, _stub_state
    em = eval_metrics.EvalMetric(_Batches(3, seed=10 + rank), _config(14, 3, 2), inception=_stub_inception, chunk=4,
                                 group=dist.group.WORLD)
    out = em.calculate_inception_fid(_StubGen, _stub_state(), 3)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pool=em._pool, out=np.asarray(out))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_gloo_ranks_agree_on_the_gathered_pools(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    np.testing.assert_array_equal(r0["pool"], r1["pool"])
    np.testing.assert_array_equal(r0["out"], r1["out"])
    # the real pool is rank 0's 15 images then rank 1's, truncated to eval_num = 14
    local = []
    for rank in range(2):
        ds = _Batches(3, seed=10 + rank)
        local.append(np.concatenate([_stub_inception(next(ds)["image"])[0] for _ in range(14 // 3 + 1)], 0))
    np.testing.assert_array_equal(r0["pool"], np.concatenate(local, 0)[:14])
    assert np.all(np.isfinite(r0["out"]))
