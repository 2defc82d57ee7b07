"""Caption encoder, host side (no GPU): the WordPiece tokenizer against ``transformers.BertTokenizer`` and against hand-written
answers, the float64 oracle tests/bert_ref.py against ``transformers.BertModel``, the weight loader, and ``TextEncoder`` with a
fake network (return convention, the sentence-embedding quirk, ``caption_features`` through the TFRecord codec).

Fixtures written for this test: tests/golden/bert_vocab_small.txt (74 entries) and tests/golden/bert_sentences.txt (one JSON
string per line: accents, CJK, punctuation runs, tabs, control characters, a 101-character word, an empty string)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import bert_ref as R
from xmcgan_image_generation_amd.libml import tfrecord, wordpiece
from xmcgan_image_generation_amd.utils import bert_arch, bert_utils

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB = os.path.join(GOLDEN, "bert_vocab_small.txt")


def _sentences():
    with open(os.path.join(GOLDEN, "bert_sentences.txt"), encoding="ascii") as f:
        return [json.loads(line) for line in f if line.strip()]


@pytest.fixture(scope="module")
def tok():
    return wordpiece.FullTokenizer(VOCAB, do_lower_case=True)


# ------------------------------------------------------------------------------------------------------------ tokenizer
def test_fixture_sentences_cover_the_hard_cases():
    s = _sentences()
    assert "" in s and any("\t" in x for x in s) and any("\x00" in x for x in s) and any("猫" in x for x in s)
    assert any("é" in x for x in s) and any("?!?!" in x for x in s)
    assert any(len(w) == 101 for x in s for w in x.split()) and any(len(w) == 100 for x in s for w in x.split())


def test_tokenizer_equals_transformers(tok):
    transformers = pytest.importorskip("transformers")
    hf = transformers.BertTokenizer(VOCAB, do_lower_case=True)
    for s in _sentences():
        want = hf.tokenize(s)
        assert tok.tokenize(s) == want, s
        assert tok.convert_tokens_to_ids(want) == hf.convert_tokens_to_ids(want)


def test_tokenizer_known_answers(tok):
    assert tok.tokenize("A man riding a horse on the beach.") == ["a", "man", "riding", "a", "horse", "on", "the", "beach", "."]
    assert tok.tokenize("Café tables, naïve résumé!") == ["cafe", "table", "##s", ",", "naive", "resume", "!"]
    assert tok.tokenize("猫と犬 sitting") == ["猫", "[UNK]", "犬", "sitting"]          # CJK split, kana unknown
    assert tok.tokenize("a\tdog\nand\ra  cat") == ["a", "dog", "and", "a", "cat"]
    assert tok.tokenize("d\x00o\x07g\u200b \ufffdcat") == ["dog", "cat"]                        # dropped characters
    assert tok.tokenize("Unbelievably") == ["un", "##believ", "##ably"]
    assert tok.tokenize("unbelievabl") == ["[UNK]"]                                # one position without a match: the whole token
    assert tok.tokenize("x" * 100) == ["x"] + ["##x"] * 99 and tok.tokenize("x" * 101) == ["[UNK]"]
    assert tok.tokenize("") == [] and tok.tokenize(" \t ") == []
    # a special token's spelling in raw text is ordinary text
    assert tok.tokenize("a [SEP] dog") == ["a", "[", "sep", "]", "dog"]
    assert tok.convert_tokens_to_ids(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a"]) == [0, 1, 2, 3, 5]


def test_encode_rows(tok):
    long = "two dogs sitting on a red table with pizza and a cat on the street riding the horse"
    ids, max_len = tok.encode(["", "a man", long, "a [SEP] dog"], 17)
    assert ids.dtype == np.int32 and ids.shape == (4, 17) and max_len.dtype == np.int64
    assert max_len.tolist() == [2, 4, 17, 7]
    assert ids[0].tolist() == [2, 3] + [0] * 15
    assert ids[1].tolist() == [2, 5, 12, 3] + [0] * 13
    pieces = tok.tokenize(long)
    assert len(pieces) == 19                                                       # cut to T - 2 = 15 pieces
    assert ids[2].tolist() == [2] + tok.convert_tokens_to_ids(pieces[:15]) + [3]
    assert ids[3].tolist()[:7] == [2, 5] + tok.convert_tokens_to_ids(["[", "sep", "]"]) + [16, 3]
    ids5, ml5 = tok.encode([long], 5)
    assert ids5[0].tolist() == [2] + tok.convert_tokens_to_ids(pieces[:3]) + [3] and ml5.tolist() == [5]
    assert (wordpiece.encode(tok, ["a man"], 17)[0] == ids[1]).all()


# ------------------------------------------------------------------------------------------------------------ the oracle
SMALL = dict(layers=2, hidden=128, ffn=512, vocab=64, max_pos=40)


def _batch(vocab, n=5, t=17, seed=0):
    rng = np.random.default_rng(seed)
    max_len = np.array([2, 9, 17, 5, 12][:n], np.int64)
    ids = np.zeros((n, t), np.int64)
    for i, m in enumerate(max_len):
        ids[i, :m] = rng.integers(1, vocab, size=m)
    return ids, max_len


def test_oracle_equals_transformers_bert_model():
    transformers = pytest.importorskip("transformers")
    params = bert_arch.init_bert(3, **SMALL)
    cfg = transformers.BertConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
                                  max_position_embeddings=40, type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12,
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = transformers.BertModel(cfg, add_pooling_layer=False).double().eval()
    sd = {k: torch.as_tensor(v).double() for k, v in params.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    ids, max_len = _batch(64)
    mask = (np.arange(17)[None, :] < max_len[:, None]).astype(np.int64)
    with torch.no_grad():
        want = model(input_ids=torch.as_tensor(ids), attention_mask=torch.as_tensor(mask),
                     token_type_ids=torch.zeros_like(torch.as_tensor(ids))).last_hidden_state
    got = R.forward(params, ids, max_len)
    assert got.dtype == torch.float64 and got.shape == (5, 17, 128)
    assert float((got - want).abs().max()) <= 1e-10


def test_oracle_switches():
    params = bert_arch.init_bert(3, **SMALL)
    ids, max_len = _batch(64)
    ref = R.forward(params, ids, max_len)
    f32 = R.forward(params, ids, max_len, torch.float32)
    bf = R.forward(params, ids, max_len, round_bf16=True)
    assert f32.dtype == torch.float32
    e32, ebf = float((f32.double() - ref).abs().max()), float((bf - ref).abs().max())
    assert 0 < e32 < 1e-4 < ebf < 0.3                      # float32 rounding << bf16 operand rounding << the outputs' scale
    # a padded key has no influence: changing the ids behind max_len changes the padded ROWS only
    ids2 = ids.copy()
    ids2[1, 9:] = 7
    ref2 = R.forward(params, ids2, max_len)
    assert torch.equal(ref2[1, :9], ref[1, :9]) and not torch.equal(ref2[1, 9:], ref[1, 9:])


# ------------------------------------------------------------------------------------------------------------ the loader
def test_loader_round_trip_and_errors(tmp_path):
    params = bert_arch.init_bert(1, **SMALL)
    path = str(tmp_path / "bert.npz")
    extra = dict(params)
    extra["pooler.dense.weight"] = np.zeros((128, 128), np.float32)
    extra["embeddings.position_ids"] = np.arange(40)[None]
    np.savez(path, **extra)
    got = bert_utils.bert_model(path)
    assert sorted(got) == sorted(params) and all(np.array_equal(got[k], params[k]) and got[k].dtype == np.float32 for k in params)
    assert bert_utils.infer_dims(got) == bert_arch.BertDims(2, 128, 512, 64, 40, 2)

    with pytest.raises(FileNotFoundError):
        bert_utils.bert_model(str(tmp_path / "absent.npz"))
    key = "encoder.layer.1.output.LayerNorm.bias"
    np.savez(path, **{k: v for k, v in params.items() if k != key})
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        bert_utils.bert_model(path)
    bad = dict(params)
    bad["encoder.layer.0.intermediate.dense.bias"] = np.zeros((511,), np.float32)
    np.savez(path, **bad)
    with pytest.raises(ValueError, match=r"encoder\.layer\.0\.intermediate\.dense\.bias"):
        bert_utils.bert_model(path)
    np.savez(path, **{k: v for k, v in params.items() if k != "embeddings.word_embeddings.weight"})
    with pytest.raises(ValueError, match=r"embeddings\.word_embeddings\.weight"):
        bert_utils.bert_model(path)
    # None: the explicit opt-in to random weights
    rnd = bert_utils.bert_model(None, seed=1, **SMALL)
    assert all(np.array_equal(rnd[k], params[k]) for k in params)


def test_base_size_shapes():
    shapes = bert_arch.expected_shapes(bert_arch.BertDims(12, 768, 3072, 30522, 512, 12))
    assert len(shapes) == 5 + 12 * 16
    assert shapes["encoder.layer.11.intermediate.dense.weight"] == (3072, 768)
    assert shapes["embeddings.word_embeddings.weight"] == (30522, 768)


# ------------------------------------------------------------------------------------------------------------ TextEncoder
def _fake_encoder(ids, max_len):
    """embedding[n, t, c] = id + c / 1000 + 1 at every position, padding included"""
    ids = np.asarray(ids, np.float32)
    return ids[:, :, None] + 1.0 + np.arange(768, dtype=np.float32)[None, None, :] / 1000.0


def test_text_encoder_convention():
    te = bert_utils.TextEncoder(VOCAB, None, encoder=_fake_encoder)
    caps = ["a man riding a horse", "", "two dogs"]
    out = te.get_bert_for_captions(caps)
    assert isinstance(out, tuple) and len(out) == 3
    emb, sent, max_len = out
    assert emb.shape == (3, 17, 768) and emb.dtype == np.float32
    assert sent.shape == (3, 768) and sent.dtype == np.float32
    assert max_len.dtype == np.int64 and max_len.tolist() == [7, 2, 5]
    # the quirk: all 17 positions are summed, the divisor counts the real tokens only
    want = emb.astype(np.float64).sum(axis=1) / max_len[:, None]
    np.testing.assert_allclose(sent, want, rtol=1e-6)
    masked = np.stack([emb[i, :m].astype(np.float64).sum(axis=0) / m for i, m in enumerate(max_len)])
    assert np.abs(sent - masked).max() > 1.0
    emb5, _, ml5 = te.get_bert_for_captions(caps, max_text_length=5)
    assert emb5.shape == (3, 5, 768) and ml5.tolist() == [5, 2, 5]


def test_caption_features_through_the_tfrecord_codec():
    te = bert_utils.TextEncoder(VOCAB, None, encoder=_fake_encoder)
    caps = ["a man", "a dog", "a cat", "Café!", ""]
    feats = te.caption_features(caps)
    assert sorted(feats) == ["caption/embedding", "caption/max_len", "caption/text"]
    back = tfrecord.parse_example(tfrecord.serialize_example(feats))
    emb, _, max_len = te.get_bert_for_captions(caps)
    assert np.array_equal(np.asarray(back["caption/embedding"], np.float32).reshape(5, 17, 768), emb)
    assert np.array_equal(back["caption/max_len"], max_len) and back["caption/max_len"].dtype == np.int64
    assert back["caption/text"] == [c.encode("utf-8") for c in caps]


def test_random_weights_warn_and_bad_ids_are_rejected_on_the_host():
    with pytest.raises(ValueError, match="token id 64"):
        bert_utils.check_ids(np.array([[2, 64, 3]]), np.array([3]), vocab=64, max_pos=40)
    with pytest.raises(ValueError, match="token id -1"):
        bert_utils.check_ids(np.array([[2, -1, 3]]), np.array([3]), vocab=64, max_pos=40)
    with pytest.raises(ValueError, match="max_len"):
        bert_utils.check_ids(np.array([[2, 5, 3]]), np.array([1]), vocab=64, max_pos=40)
    with pytest.raises(ValueError, match="max_text_length"):
        bert_utils.check_ids(np.zeros((1, 33), np.int64), np.array([2]), vocab=64, max_pos=40)
    bert_utils.check_ids(np.array([[2, 63, 3]]), np.array([3]), vocab=64, max_pos=40)
    if not torch.cuda.is_available():                      # without a GPU the default network cannot be built: no fallback
        from xmcgan_image_generation_amd import _lib
        with pytest.warns(UserWarning, match="random BERT"), pytest.raises(_lib.XmcError):
            bert_utils.TextEncoder(VOCAB, None)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_check_their_domain_before_any_launch():
    """the argument checks of csrc/bert.hip run on the host before the first HIP call: without a GPU, with pointers that are never
    dereferenced (only ``max_len_host`` is read), every call outside a kernel's domain returns XMC_EINVAL"""
    import ctypes as C
    from xmcgan_image_generation_amd import _lib
    lib = _lib.load()
    p, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)

    def attention(t, h, max_len):
        ml = np.array(max_len, np.int32)
        return lib.xmc_bert_attention(p, p, p, C.c_void_p(ml.ctypes.data), p, len(max_len), t, h, None)

    einval = lib.xmc_bert_attention(None, p, p, p, p, 1, 17, 128, None)
    assert einval < 0 and einval > -1000                                              # XMC_EINVAL, not a HIP error
    assert attention(33, 128, [5, 33]) == einval and attention(17, 128, [9, 1]) == einval
    assert attention(17, 128, [18, 9]) == einval and attention(17, 96, [9, 9]) == einval and attention(1, 128, [1]) == einval
    assert lib.xmc_bias_residual_ln(p, p, p, p, p, p, 4, 1028, 1e-12, None) == einval     # row longer than a wave holds
    assert lib.xmc_bias_residual_ln(p, p, p, p, p, p, 4, 6, 1e-12, None) == einval        # not a multiple of 4
    assert lib.xmc_bias_residual_ln(p, p, p, p, p, odd, 4, 128, 1e-12, None) == einval    # 4-byte aligned output
    assert lib.xmc_bias_gelu(p, p, p, 4, 6, None) == einval and lib.xmc_bias_gelu(odd, p, p, 4, 8, None) == einval
    assert lib.xmc_bert_embed_ln(p, p, p, p, p, p, p, 34, 17, 128, 64, 16, 1e-12, None) == einval      # T beyond the position table
    assert lib.xmc_bert_embed_ln(p, p, p, p, p, p, p, 0, 17, 128, 64, 40, 1e-12, None) == einval
    assert lib.xmc_bert_sentence(p, p, p, 3, 17, 130, None) == einval
    with pytest.raises(_lib.XmcError, match="invalid argument"):
        _lib.check(einval, "xmc_bert_attention")
