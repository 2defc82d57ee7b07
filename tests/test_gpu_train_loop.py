"""The training and evaluation loops on the MI355X: the metric-accumulation kernel (eager launches, graph replays, guard bands),
a resumed run against an uninterrupted one bit for bit, the accumulator inside the replayed graph against per-step reads, and
``train`` + ``test`` end to end on TFRecord shards.

Configuration: ``coco_xmc.get_test_config()`` (128 px, gf = df = 16, z 8), batch 2, bf16, no ResNet-50 term.  The injected
``datasets`` hook hands out ``synthetic.make_batch(cfg, seed=step)`` for step ``step``."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests.guard import Guard, guarded
from tests.test_input_pipeline import _write_shards
from xmcgan_image_generation_amd import synthetic as syn
from xmcgan_image_generation_amd import train_utils, xmc_gan
from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.utils import checkpoint, eval_metrics, task_manager

pytestmark = pytest.mark.gpu

KEYS = xmc_gan.METRIC_KEYS
F32 = torch.float32


def _cfg(**kw):
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = 2
    cfg.dtype = "bfloat16"
    cfg.pretrained_image_contrastive = False
    cfg.update(kw)
    return cfg


def _batch(cfg, step):
    return {k: torch.as_tensor(v) for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size, seed=step).items()}


def synthetic_datasets(config, data_rng, start_step, rank, world, device):
    def batches():
        s = start_step
        while True:
            yield {k: v.to(device) for k, v in _batch(config, s).items()}
            s += 1
    return batches(), iter(()), 1000


@pytest.fixture(scope="module")
def ops():
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------- the kernel
LAUNCHES, EAGER = 6, 3


def _values(n, bad=()):
    """(6, n) float32 inputs of mixed magnitude and sign: the float64 sum of a column differs from its float32 sum"""
    gen = torch.Generator().manual_seed(100 + n)
    v = torch.randn(LAUNCHES, n, generator=gen) * torch.tensor([10.0 ** (3 * (i % 3) - 2) for i in range(n)])
    for launch, column, value in bad:
        v[launch - 1, column] = value
    return v


def _accumulate(ops, values):
    """3 eager launches, then 3 replays of a captured graph that holds the one launch -> (sums, info after each launch)"""
    dev = ops.device
    n = values.shape[1]
    staged = values.to(dev)
    vals = [torch.zeros(1, dtype=F32, device=dev) for _ in range(n)]
    sums = torch.zeros((n,), dtype=torch.float64, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    seen = torch.zeros((LAUNCHES, 2), dtype=torch.int32, device=dev)

    def load(k):
        for i, v in enumerate(vals):
            v.copy_(staged[k, i:i + 1])

    for k in range(EAGER):
        load(k)
        ops.metrics_accum(vals, sums, info)
        seen[k].copy_(info)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.metrics_accum(vals, sums, info)
    for k in range(EAGER, LAUNCHES):
        load(k)
        graph.replay()
        seen[k].copy_(info)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), seen.cpu().numpy()


def _sequential(values):
    want = np.zeros(values.shape[1], np.float64)
    for row in values.numpy():
        for i, x in enumerate(row):
            want[i] = want[i] + np.float64(x)
    return want


def _check_clean(ops, n):
    values = _values(n)
    sums, seen = _accumulate(ops, values)
    want = _sequential(values)
    assert sums.tobytes() == want.tobytes(), (sums, want)
    assert seen[:, 0].tolist() == list(range(1, LAUNCHES + 1)) and not seen[:, 1].any()
    return sums


def _check_nan(ops, n):
    """NaN in the last column before launch 4 (the first replay), an infinity in the first before launch 5"""
    values = _values(n, bad=[(4, n - 1, float("nan")), (5, 0, float("inf"))])
    sums, seen = _accumulate(ops, values)
    assert seen[:, 0].tolist() == list(range(1, LAUNCHES + 1))
    assert seen[:, 1].tolist() == [0, 0, 0, 4, 4, 4]
    want = _sequential(values)
    assert np.isnan(sums[n - 1]) and (n == 1 or sums[0] == np.inf)
    assert sums[1:n - 1].tobytes() == want[1:n - 1].tobytes()


def test_metrics_accum_sums_in_float64_over_eager_launches_and_replays(ops):
    sums = _check_clean(ops, 5)
    f32 = _values(5).numpy().astype(np.float32)
    acc = np.zeros(5, np.float32)
    for row in f32:
        acc = acc + row
    assert (sums != acc.astype(np.float64)).any()           # the inputs tell a float32 accumulation from a float64 one


def test_metrics_accum_records_the_first_non_finite_call(ops):
    _check_nan(ops, 5)


def test_metrics_accum_rejects_bad_arguments(ops):
    from xmcgan_image_generation_amd import _lib
    import ctypes as C
    sums = torch.zeros((9,), dtype=torch.float64, device=ops.device)
    info = torch.zeros((2,), dtype=torch.int32, device=ops.device)
    v = torch.zeros(1, dtype=F32, device=ops.device)
    ptrs = (C.c_void_p * 9)(*[v.data_ptr()] * 9)
    s = ops._stream()
    assert ops.lib.xmc_metrics_accum(ptrs, 9, sums.data_ptr(), info.data_ptr(), s) == -22
    assert ops.lib.xmc_metrics_accum(ptrs, 0, sums.data_ptr(), info.data_ptr(), s) == -22
    assert ops.lib.xmc_metrics_accum(ptrs, 2, None, info.data_ptr(), s) == -22
    ptrs[1] = None
    assert ops.lib.xmc_metrics_accum(ptrs, 2, sums.data_ptr(), info.data_ptr(), s) == -22
    torch.cuda.synchronize()
    assert not sums.any() and not info.any() and _lib.ABI_VERSION >= 27


@pytest.mark.parametrize("skew", [0, 16])
@pytest.mark.parametrize("n", [1, 8])
def test_metrics_accum_inside_guard_bands(ops, n, skew):
    """the n inputs, ``sums`` and ``info`` each between bands of 0xFF bytes (NaN as float32 / float64): the sums stay bit-equal
    to the sequential float64 sum, so nothing next to an input was read, and no band byte changes"""
    g = Guard("cuda", skew=skew)
    try:
        with guarded(g):
            _check_clean(ops, n)
            _check_nan(ops, n)
    except Exception as e:                                   # a faulted device answers every later call with the same error
        if "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e):
            pytest.exit(f"GPU fault in xmc_metrics_accum (n = {n}, skew {skew}): {e}", returncode=3)
        raise
    assert g.served >= 2 * (n + 4)
    g.check()
    assert g.fallthrough == [], g.fallthrough


# --------------------------------------------------------------------------------------------- resume, graph + accumulator
def _flat(tree, prefix=""):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flat(tree[k], f"{prefix}/{k}")
    else:
        yield prefix, tree


@pytest.fixture(scope="module")
def uninterrupted(tmp_path_factory):
    """run A: 4 steps in one ``train`` call (step 1 eager, 2-4 replayed); scalars, grids and a checkpoint at step 4 only"""
    workdir = str(tmp_path_factory.mktemp("run_a"))
    cfg = _cfg(num_train_steps=4, eval_every_steps=100, checkpoint_every_steps=100)
    train_utils.train(cfg, workdir, datasets=synthetic_datasets)
    return cfg, workdir


def test_resumed_run_equals_an_uninterrupted_one_bit_for_bit(uninterrupted, tmp_path):
    cfg, workdir_a = uninterrupted
    workdir_b = str(tmp_path)
    train_utils.train(_cfg(num_train_steps=2, eval_every_steps=100, checkpoint_every_steps=100), workdir_b, datasets=synthetic_datasets)
    ckpt_b = os.path.join(workdir_b, "checkpoints-0")
    assert sorted(os.listdir(ckpt_b)) == ["TRAIN_DONE", "ckpt-1.flax"]
    train_utils.train(cfg, workdir_b, datasets=synthetic_datasets)       # new networks, a new graph: steps 3 (eager) and 4 (replayed)
    assert sorted(os.listdir(ckpt_b)) == ["TRAIN_DONE", "ckpt-1.flax", "ckpt-2.flax"]
    a = checkpoint.msgpack_restore(open(os.path.join(workdir_a, "checkpoints-0", "ckpt-1.flax"), "rb").read())
    b = checkpoint.msgpack_restore(open(os.path.join(ckpt_b, "ckpt-2.flax"), "rb").read())
    la, lb = dict(_flat(a)), dict(_flat(b))
    assert sorted(la) == sorted(lb) and len(la) > 100
    assert int(la["/step"]) == 4 and int(la["/g_optimizer/state/step"]) == 4 and int(la["/d_optimizer/state/step"]) == 8
    groups = set()
    different = []
    for name in la:
        x, y = np.asarray(la[name]), np.asarray(lb[name])
        groups.add(name.split("/")[1] + ("/" + name.split("/")[-1] if name.endswith(("grad_ema", "grad_sq_ema", "u0")) else ""))
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            different.append(name)
    assert not different, (len(different), different[:8])
    # every part of the state was compared: parameters, both Adam moments and the counters, EMA, BatchNorm statistics, u0
    assert {"step", "g_optimizer", "d_optimizer", "g_optimizer/grad_ema", "d_optimizer/grad_sq_ema", "ema_params", "generator_state",
            "discriminator_state/u0"} <= groups, groups
    first = checkpoint.msgpack_restore(open(os.path.join(ckpt_b, "ckpt-1.flax"), "rb").read())
    moved = [n for n, v in _flat(first) if np.asarray(v).tobytes() != np.asarray(la[n]).tobytes()]
    assert len(moved) > len(la) // 2                         # (steps 3 and 4 did change the state the comparison looks at)


def test_accumulator_in_the_replayed_graph_equals_per_step_reads(uninterrupted):
    """the means ``train`` wrote at step 4 (accumulated on the device: one eager step, three replays) against a second,
    identical run whose metrics are read with a synchronisation after every step"""
    cfg, workdir = uninterrupted
    (line,) = [json.loads(l) for l in open(os.path.join(workdir, "metrics.jsonl"))]
    assert line["step"] == 4
    streams = train_utils.rng_streams(cfg.seed)
    gen, disc, state = train_utils.create_train_state(cfg, streams["model"])
    dev = gen.ops.device
    batches = [{k: v.to(dev) for k, v in _batch(cfg, s).items()} for s in range(1, 5)]
    per_step = []

    def read(metrics):
        torch.cuda.synchronize()
        per_step.append({k: np.float32(float(metrics[k])) for k in KEYS})

    state, metrics = train_utils.train_step(train_utils.fold_in(streams["train"], 1), state, batches[0], xmc_gan, gen, disc, cfg, {})
    read(metrics)
    graphed = train_utils.GraphedTrainStep(state, batches[0], xmc_gan, gen, disc, cfg, {})
    state = graphed.state
    for b in batches[1:]:
        state, metrics = graphed(state, b)
        read(metrics)
    assert int(state.step) == 4
    for k in KEYS:
        total = np.float64(0.0)
        for m in per_step:
            total = total + np.float64(m[k])
        assert line[k] == float(total / 4), (k, line[k], float(total / 4))
    assert len({m["d_loss"] for m in per_step}) == 4         # four different steps, not one value four times


# ------------------------------------------------------------------------------------------------------ end to end on shards
def test_train_and_test_end_to_end_on_shards(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    _write_shards(data, n=12)
    _write_shards(data, n=4, split="val")
    workdir = str(tmp_path / "work")
    cfg = _cfg(num_train_steps=2, eval_every_steps=100, checkpoint_every_steps=100, data_dir=str(data) + "/")
    state = train_utils.train(cfg, workdir)                  # the real pipeline, uploading to the GPU
    assert int(state.step) == 2
    ckpt_dir = os.path.join(workdir, "checkpoints-0")
    assert sorted(os.listdir(ckpt_dir)) == ["TRAIN_DONE", "ckpt-1.flax"]
    (line,) = [json.loads(l) for l in open(os.path.join(workdir, "metrics.jsonl"))]
    assert line["step"] == 2 and all(np.isfinite(line[k]) for k in KEYS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)         # random Inception weights
        assert train_utils.test(cfg, workdir) == 1
        # the same evaluation by hand: the same eval stream, the restored state, the same rng
        streams = train_utils.rng_streams(cfg.seed)
        gen, _, template = train_utils.create_train_state(cfg, streams["model"])
        _, eval_iter, _ = train_utils.default_datasets(cfg, streams["data"], 1, 0, 1, gen.ops.device)
        em = eval_metrics.EvalMetric(eval_iter, cfg, chunk=256)
        restored = checkpoint.restore(os.path.join(ckpt_dir, "ckpt-1.flax"), template)
        want = em.calculate_inception_fid(gen, restored, streams["eval"])
    rows = open(os.path.join(ckpt_dir, "scores.csv"), newline="").read().split("\r\n")
    assert len(rows) == 3 and rows[2] == ""                  # header, one row
    cells = dict(zip(rows[0].split(","), rows[1].split(",")))
    assert cells["checkpoint_path"] == os.path.join(ckpt_dir, "ckpt-1.flax") and cells["step"] == "1"
    assert np.all(np.isfinite(want))
    for k, v in zip(train_utils.EVAL_KEYS, want):
        assert cells[f"eval/{k}"] == "%.3f" % v, (k, cells[f"eval/{k}"], v)
    evals = [json.loads(l) for l in open(os.path.join(workdir, "metrics.jsonl")) if "eval/fid" in l]
    assert len(evals) == 1 and evals[0]["step"] == 2 and evals[0]["eval/fid"] == want[0]
    slept = []
    assert train_utils.test(cfg, workdir, task_manager_kw=dict(sleep=slept.append)) == 0        # nothing left: returns at once
    assert slept == [] and open(os.path.join(ckpt_dir, "scores.csv"), newline="").read().split("\r\n") == rows
    assert task_manager.TaskManagerWithCsvResults(os.path.join(workdir, "checkpoints")).is_training_done()
