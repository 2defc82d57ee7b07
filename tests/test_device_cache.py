"""Device-resident dataset cache (libml/device_cache.py, config.device_dataset_cache) on the host: the plan drawn without an image
and executed by the NumPy executor -- the specification of xmc_cache_gather -- against COCODataset.preprocess, the cached stream
against create_datasets(procs=0) batch for batch, decode counts, the memory budget and the plan checks.  CPU only."""
import ctypes

import numpy as np
import pytest

from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.libml import _io, coco_dataset, device_cache, input_pipeline, png, tfrecord

FIELDS = ("image", "image_aug", "embedding", "max_len", "sentence_embedding", "z")


def _features(rng, s, t, e=768):
    h, w = int(rng.integers(40, 91)), int(rng.integers(40, 91))
    return {"image": rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "image/filename": b"img.jpg",
            "caption/text": [f"caption {k}".encode() for k in range(s)],
            "caption/embedding": rng.standard_normal((s, t, e)).astype(np.float32),
            "caption/max_len": rng.integers(3, t + 1, size=s).astype(np.int64)}


@pytest.mark.parametrize("size", [16, 128])
@pytest.mark.parametrize("version,return_text", [("2014", False), ("2014", True), ("ln", False)])
def test_plan_example_reproduces_preprocess(size, version, return_text):
    """200 example generators: the plan executed on the UNFLIPPED resize is preprocess's output, bit for bit, in every field"""
    ds = coco_dataset.COCODataset(image_size=size, z_dim=8, coco_version=version, return_text=return_text)
    s, t, e = ds.embedding_shape
    assert (s, t) == ((1, 64) if version == "ln" else (5, 17))
    rng = np.random.default_rng(size)
    feats = [_features(rng, s, t) for _ in range(4)]
    caches = []
    for f in feats:                                   # what the fill stores per record
        ml = f["caption/max_len"].astype(np.float32)[:, None]
        caches.append((_io.resize_bilinear_rgb(f["image"], size, False)[None], f["caption/embedding"][None],
                       (f["caption/embedding"].sum(axis=-2) / ml)[None], ml[None, :, 0]))
    seen = set()
    for i in range(200):
        f, c = feats[i % 4], caches[i % 4]
        want = ds.preprocess(f, np.random.default_rng([7, 0, 0, i]))
        fields, z = device_cache.plan_example(np.random.default_rng([7, 0, 0, i]), s, 8, size, f["caption/max_len"], return_text)
        plan = np.array([[0, *fields, 0, 0]], np.int32)
        got = device_cache.execute_plan(*c, plan)
        got["z"] = z[None]
        for k in FIELDS:
            assert got[k].dtype == want[k].dtype == np.float32 and np.array_equal(got[k][0], want[k]), (i, k)
        if return_text:
            assert want["text"] == f["caption/text"][fields[0]]
        seen.add(fields[1:])
    assert len({v[0] for v in seen}) == 2 and len({v[3] for v in seen}) == 2      # both flips, both augmentation flips
    assert {v[1] for v in seen} == set(range(9)) == {v[2] for v in seen}          # every shift 0 .. 2 * pad


def _write_three_shards(tmp_path, split="train", seed=3):
    """4 + 5 + 4 records in three shards, written with the public tfrecord / png modules"""
    rng = np.random.default_rng(seed)
    name = {"train": "train", "val": "validation"}[split]
    k = 0
    for shard, n in enumerate((4, 5, 4)):
        recs = []
        for _ in range(n):
            f = _features(rng, 5, 17)
            recs.append(tfrecord.serialize_example({
                "image": [png.encode_rgb(f["image"], np.arange(f["image"].shape[0]) % 5)], "image/filename": [f"img{k}.jpg".encode()],
                "caption/text": [f"caption {k}.{j}".encode() for j in range(5)],
                "caption/embedding": f["caption/embedding"].reshape(-1), "caption/max_len": f["caption/max_len"]}))
            k += 1
        tfrecord.write_records(str(tmp_path / f"coco2014_{name}.tfrecord-{shard}-of-3"), recs)


def _config(tmp_path, **kw):
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = 2
    cfg.image_size = 16
    cfg.update(data_dir=str(tmp_path) + "/", coco_version="2014", shuffle_buffer_size=4, train_shuffle=True, eval_batch_size=2,
               dataset="mscoco")
    cfg.update(kw)
    return cfg


def _same_batches(a, b, n):
    for step in range(n):
        x, y = next(a), next(b)
        assert list(x) == list(y), step                                            # same keys, same order
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), (step, k)
            else:
                assert x[k] == y[k], (step, k)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = tmp_path_factory.mktemp("cache_shards")
    _write_three_shards(d, "train")
    _write_three_shards(d, "val", seed=5)
    return d


@pytest.mark.parametrize("kw,rank,world", [(dict(train_shuffle=True), 0, 1), (dict(train_shuffle=False), 0, 1),
                                           (dict(train_shuffle=True), 1, 2),
                                           (dict(train_shuffle=True, return_text=True, return_filename=True), 0, 1)],
                         ids=["shuffle", "in-order", "rank1of2", "text+filename"])
def test_cached_stream_equals_the_host_pipeline(shards, kw, rank, world):
    """13 records, 4 per training batch, 12 batches = more than three epochs: the cached stream (device=None) is the stream of
    create_datasets(procs=0) batch for batch, train and eval"""
    cfg = _config(shards, **kw)
    cfg.batch_size = 2 * world
    host_tr, host_ev, n = input_pipeline.create_datasets(cfg, data_rng=11, rank=rank, world=world, procs=0)
    cfg.device_dataset_cache = True
    tr, ev, n2 = input_pipeline.create_datasets(cfg, data_rng=11, rank=rank, world=world, procs=0)
    assert n == n2
    _same_batches(host_tr, tr, 12)
    _same_batches(host_ev, ev, 24)


def test_fill_through_worker_processes_fills_the_same_cache(shards):
    """num_decode_procs only sets the fill's parallelism in cache mode: same slots, same bits"""
    ds = coco_dataset.COCODataset(image_size=16, z_dim=8, data_dir=str(shards) + "/", return_filename=True)
    a = device_cache.DeviceDatasetCache(ds, ds.files("train"), None, workers=2, procs=0, chunk=3)
    b = device_cache.DeviceDatasetCache(ds, ds.files("train"), None, workers=1, procs=2, chunk=3)
    assert a.slots == b.slots == 13 and a.filenames == b.filenames == [f"img{k}.jpg".encode() for k in range(13)]
    for k in a.arrays:
        assert np.array_equal(a.arrays[k], b.arrays[k]), k
    assert np.array_equal(a.max_len, b.max_len) and a.texts == b.texts


def test_no_decode_after_the_fill(shards, monkeypatch):
    """the fill decodes each record exactly once, three further epochs decode nothing (with the config key ignored the stream
    would decode every example again)"""
    calls = []
    real = png.decode_rgb
    monkeypatch.setattr(png, "decode_rgb", lambda data: (calls.append(1), real(data))[1])
    cfg = _config(shards, device_dataset_cache=True)
    tr, ev, _ = input_pipeline.create_datasets(cfg, data_rng=2, prefetch=1)
    first = next(tr)                                  # the iterators exist: both fills are complete
    assert len(calls) == 13 + 13                      # train + val, once each
    assert first["image"].shape == (4, 16, 16, 3) and first["image_aug"].shape == (4, 16, 16, 3)
    for _ in range(11):                               # 48 examples > three epochs of 13
        next(tr)
    next(ev)
    assert len(calls) == 26


def test_budget_refusal_names_both_sizes(shards, monkeypatch):
    ds = coco_dataset.COCODataset(image_size=16, z_dim=8, data_dir=str(shards) + "/")
    need = 13 * 4 * (16 * 16 * 3 + 5 * 17 * 768 + 5 * 768 + 5)
    for free, total in ((need - 1, 100 * need), (need, 2 * need - 2)):            # above what is free; above half of the total
        monkeypatch.setattr(device_cache, "_device_memory", lambda device, v=(free, total): v)
        with pytest.raises(ValueError) as err:
            device_cache.DeviceDatasetCache(ds, ds.files("train"), None)
        assert str(need) in str(err.value) and str(total) in str(err.value) and str(free) in str(err.value)
    monkeypatch.setattr(device_cache, "_device_memory", lambda device: (need, 2 * need))
    assert device_cache.DeviceDatasetCache(ds, ds.files("train"), None).nbytes == need


BAD_PLANS = [("slot past the end", dict(slot=3), {}), ("negative slot", dict(slot=-1), {}), ("caption >= S", dict(cap=5), {}),
             ("shift > 2 * pad", dict(dy=9), {}), ("column shift > 2 * pad", dict(dx=9), {}), ("H <= pad", {}, dict(h=4))]


@pytest.mark.parametrize("what,fields,dims", BAD_PLANS, ids=[b[0] for b in BAD_PLANS])
def test_rejected_plans(what, fields, dims):
    """a plan that would index outside the cache: the NumPy executor raises, the library returns XMC_EINVAL from both entry points
    -- xmc_cache_gather before it touches a pointer or launches (there is no GPU here, and none of the addresses is real)"""
    from xmcgan_image_generation_amd import _lib
    lib = _lib.load()
    slots, s, t, e, pad = 3, 5, 17, 8, 4
    h = w = dims.get("h", 8)
    good = np.array([[2, 4, 1, 8, 0, 1, 0, 0], [0, 0, 0, 0, 8, 0, 0, 0]], np.int32)
    plan = good.copy()
    plan[1, 0] = fields.get("slot", 0)
    plan[1, 1] = fields.get("cap", 0)
    plan[1, 3] = fields.get("dy", 0)
    plan[1, 4] = fields.get("dx", 8)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)                                   # noqa: E731
    assert lib.xmc_cache_plan_check(hp(good), 2, slots, s, 8, 8, pad) == 0
    assert lib.xmc_cache_plan_check(hp(plan), 2, slots, s, h, w, pad) == -22
    fake = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(10)]                    # never dereferenced on the host
    rc = lib.xmc_cache_gather(fake[0], fake[1], fake[2], fake[3], slots, fake[4], hp(plan), fake[5], fake[6], fake[7], fake[8],
                              fake[9], 2, h, w, s, t, e, pad, None)
    assert rc == -22
    rng = np.random.default_rng(0)
    img, emb = rng.random((slots, h, w, 3), np.float32), rng.random((slots, s, t, e), np.float32)
    with pytest.raises(ValueError):
        device_cache.execute_plan(img, emb, emb.sum(2), rng.random((slots, s), np.float32), plan, pad)
    if not dims:
        assert device_cache.execute_plan(img, emb, emb.sum(2), rng.random((slots, s), np.float32), good, pad)["image"].shape == (2, 8, 8, 3)
