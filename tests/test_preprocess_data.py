"""The dataset builder (xmcgan_image_generation_amd/preprocess_data.py) on a three-image tree, with the NumPy specification
doing the pixel work and a stub in place of BERT.  No GPU."""
import json
import os

import numpy as np
import pytest

import jpeg_ref as R
from xmcgan_image_generation_amd import preprocess_data as P
from xmcgan_image_generation_amd.libml import coco_dataset, png, tfrecord
from xmcgan_image_generation_amd.utils import bert_utils

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_vocab_small.txt")
FIXTURE_OF = dict(R.TREE)


def _encoder():
    return bert_utils.TextEncoder(VOCAB, None, encoder=R.stub_encoder)


def _run(tmp_path, records=None, **kw):
    images, ann, recs = R.make_tree(tmp_path)
    out = tmp_path / "data"
    args = dict(split="train", coco_version="2014", num_shards=2, batch=2, procs=0, device=False, log=lambda *_: None)
    args.update(kw)
    return out, recs, P.run(images, recs if records is None else records, str(out), _encoder(), **args)


def test_annotation_readers_keep_the_files_order(tmp_path):
    images, ann, recs = R.make_tree(tmp_path)
    got = P.read_coco_captions([ann])
    assert got == recs and [n for n, _ in got] == [R.TREE[2][0], R.TREE[0][0], R.TREE[1][0]]
    man = tmp_path / "manifest.tsv"
    man.write_text("".join(f"{n}\t{c}\n" for k in range(5) for n, caps in recs for c in [caps[k]]))
    assert P.read_manifest(str(man)) == recs
    man.write_text("no tab here\n")
    with pytest.raises(P.PreprocessError, match="manifest.tsv:1"):
        P.read_manifest(str(man))


def test_shards_records_and_done_file(tmp_path):
    out, recs, summary = _run(tmp_path)
    assert sorted(os.listdir(out)) == ["PREPROCESS_DONE", "coco2014_train.tfrecord-0-of-2", "coco2014_train.tfrecord-1-of-2", "skipped.txt"]
    assert summary["records"] == 3 and summary["skipped"] == 0 and summary["records_per_shard"] == [2, 1]
    assert json.load(open(out / "PREPROCESS_DONE")) == {"coco2014_train": summary}
    shards = dict(R.read_shards(out, "2014", "train", 2))
    # record r -> shard r mod N, ascending r within a shard
    placed = {0: [0, 2], 1: [1]}
    ds = coco_dataset.COCODataset(data_dir=str(out) + "/", return_text=True, return_filename=True)
    enc = _encoder()
    for shard, rs in placed.items():
        assert len(shards[shard]) == len(rs)
        for data, r in zip(shards[shard], rs):
            name, caps = recs[r]
            ex = ds.parse_example(data)
            assert ex["image/filename"] == name.encode()
            assert ex["caption/text"] == [c.encode() for c in caps[:5]]                 # the annotation file's order
            want = enc.caption_features(caps[:5])
            assert np.array_equal(ex["caption/embedding"].reshape(-1), want["caption/embedding"])
            assert np.array_equal(ex["caption/max_len"], want["caption/max_len"])
            assert np.array_equal(ex["image"], R.decoded(FIXTURE_OF[name])[3])         # the specification's pixels
            raw = tfrecord.parse_example(data)
            assert sorted(raw) == ["caption/embedding", "caption/max_len", "caption/text", "image", "image/filename"]
            assert raw["caption/embedding"].size == 5 * 17 * 768 and raw["image"][0][:8] == b"\x89PNG\r\n\x1a\n"
    assert [os.path.basename(p) for p in ds.files("train")] == ["coco2014_train.tfrecord-0-of-2", "coco2014_train.tfrecord-1-of-2"]
    # a finished directory is left alone
    assert P.run(str(tmp_path / "images"), recs, str(out), _encoder(), num_shards=2, procs=0, device=False, log=lambda *_: None) == summary


def test_worker_processes_write_the_same_bytes(tmp_path):
    out0, _, s0 = _run(tmp_path / "a")
    out1, _, s1 = _run(tmp_path / "b", procs=2, batch=3)
    assert s0 == s1
    for n in ("coco2014_train.tfrecord-0-of-2", "coco2014_train.tfrecord-1-of-2"):
        assert (out0 / n).read_bytes() == (out1 / n).read_bytes()


def test_localized_narratives_shape(tmp_path):
    out, recs, summary = _run(tmp_path, coco_version="ln", split="validation", num_shards=1)
    assert summary["sentence_num"] == 1 and summary["max_text_length"] == 64
    (_, data), = R.read_shards(out, "ln", "validation", 1)
    ds = coco_dataset.COCODataset(data_dir=str(out) + "/", coco_version="ln", return_text=True)
    for d, (name, caps) in zip(data, recs):
        ex = ds.parse_example(d)
        assert ex["caption/embedding"].shape == (1, 64, 768) and ex["caption/max_len"].shape == (1,)
        assert ex["caption/text"] == [caps[0].encode()]
    assert len(ds.files("val")) == 1


def test_too_few_captions_names_the_image(tmp_path):
    images, ann, recs = R.make_tree(tmp_path)
    short = [recs[0], (recs[1][0], recs[1][1][:4]), recs[2]]
    with pytest.raises(P.PreprocessError, match=recs[1][0] + r": 4 caption"):
        P.run(images, short, str(tmp_path / "data"), _encoder(), num_shards=2, procs=0, device=False, log=lambda *_: None)
    assert not os.path.exists(tmp_path / "data" / "PREPROCESS_DONE")


def test_unsupported_and_damaged_files_stop_or_are_skipped(tmp_path):
    images, ann, recs = R.make_tree(tmp_path)
    caps = recs[0][1]
    with open(os.path.join(images, "cmyk.jpg"), "wb") as f:
        f.write(R.jpeg_bytes("cmyk_8x8"))
    with open(os.path.join(images, "cut.jpg"), "wb") as f:
        f.write(R.jpeg_bytes("q90_444")[:900])
    more = [recs[0], ("cmyk.jpg", caps), recs[1], ("cut.jpg", caps), recs[2]]
    kw = dict(num_shards=2, batch=4, procs=0, device=False, log=lambda *_: None)
    with pytest.raises(P.PreprocessError, match=r"cmyk\.jpg: .*\(-13\)"):
        P.run(images, more, str(tmp_path / "stop"), _encoder(), **kw)
    assert os.listdir(tmp_path / "stop") == []                                       # no shard, no temporary file
    with pytest.raises(P.PreprocessError, match=r"cut\.jpg: .*\(-2\)"):
        P.run(images, [m for m in more if m[0] != "cmyk.jpg"], str(tmp_path / "stop2"), _encoder(), **kw)
    with pytest.raises(P.PreprocessError, match="missing.jpg: cannot be read"):
        P.run(images, [("missing.jpg", caps)], str(tmp_path / "stop3"), _encoder(), skip_unsupported=True, **kw)
    summary = P.run(images, more, str(tmp_path / "skip"), _encoder(), skip_unsupported=True, **kw)
    assert summary["records"] == 3 and summary["skipped"] == 2 and summary["images"] == 5
    assert [ln.split("\t")[:3] for ln in open(tmp_path / "skip" / "skipped.txt").read().splitlines()] == \
        [["coco2014_train", "cmyk.jpg", "-13"], ["coco2014_train", "cut.jpg", "-2"]]
    names = [tfrecord.parse_example(d)["image/filename"][0].decode() for r in range(3)
             for d in [dict(R.read_shards(tmp_path / "skip", "2014", "train", 2))[r % 2][r // 2]]]
    assert names == [recs[0][0], recs[1][0], recs[2][0]]                               # r counts the records written


def test_train_and_validation_share_a_directory_and_rebuilds_leave_no_stale_shards(tmp_path):
    images, ann, recs = R.make_tree(tmp_path)
    out = tmp_path / "data"
    with open(os.path.join(images, "cmyk.jpg"), "wb") as f:
        f.write(R.jpeg_bytes("cmyk_8x8"))
    kw = dict(procs=0, device=False, log=lambda *_: None)
    train = P.run(images, recs + [("cmyk.jpg", recs[0][1])], str(out), _encoder(), split="train", num_shards=3, skip_unsupported=True, **kw)
    val = P.run(images, recs[:2], str(out), _encoder(), split="validation", num_shards=2, **kw)
    assert json.load(open(out / "PREPROCESS_DONE")) == {"coco2014_train": train, "coco2014_validation": val}
    assert open(out / "skipped.txt").read().startswith("coco2014_train\tcmyk.jpg\t-13\t")     # the train run's list survives
    # the train shards are still "done": a second train run touches nothing
    before = {n: os.stat(out / n).st_mtime_ns for n in os.listdir(out)}
    assert P.run(images, recs, str(out), _encoder(), split="train", num_shards=3, **kw) == train
    assert {n: os.stat(out / n).st_mtime_ns for n in os.listdir(out)} == before
    ds = coco_dataset.COCODataset(data_dir=str(out) + "/")
    assert len(ds.files("train")) == 3 and len(ds.files("val")) == 2
    # leftovers of a killed run carry names the reader's pattern does not match, and the next run removes them
    (out / "part-coco2014_train-0-of-3").write_bytes(b"half a record")
    assert len(ds.files("train")) == 3
    # a forced rebuild with another shard count replaces the old set instead of standing beside it
    again = P.run(images, recs, str(out), _encoder(), split="train", num_shards=2, force=True, **kw)
    assert again["records_per_shard"] == [2, 1] and again["skipped"] == 0
    assert [os.path.basename(p) for p in ds.files("train")] == ["coco2014_train.tfrecord-0-of-2", "coco2014_train.tfrecord-1-of-2"]
    assert len(ds.files("val")) == 2 and not [n for n in os.listdir(out) if n.startswith("part-")]
    assert json.load(open(out / "PREPROCESS_DONE")) == {"coco2014_train": again, "coco2014_validation": val}
    assert "coco2014_train" not in open(out / "skipped.txt").read()


def test_command_line(tmp_path, monkeypatch, capsys):
    images, ann, recs = R.make_tree(tmp_path)
    seen, stub = {}, _encoder()

    def fake_text_encoder(vocab, ckpt):
        seen["args"] = (vocab, ckpt)
        return stub
    monkeypatch.setattr(bert_utils, "TextEncoder", fake_text_encoder)
    rc = P.main(["--images", images, "--captions", ann, "--split", "train", "--out", str(tmp_path / "data"), "--vocab", VOCAB,
                 "--num-shards", "3", "--procs", "0", "--no-device"])
    assert rc == 0 and seen["args"] == (VOCAB, None)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["records_per_shard"] == [1, 1, 1]
    image = tfrecord.parse_example(next(tfrecord.read_records(str(tmp_path / "data" / "coco2014_train.tfrecord-1-of-3"))))["image"][0]
    assert np.array_equal(png.decode_rgb(image), R.decoded(FIXTURE_OF[recs[1][0]])[3])
