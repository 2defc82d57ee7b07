"""Writes the small CLIP BPE fixture of tests/test_clip_text.py: ``clip_bpe_vocab.json`` and ``clip_bpe_merges.txt`` in the format
of CLIP's ``vocab.json`` / ``merges.txt``.  Ids 0..255 are the byte symbols in the order of the GPT-2 byte table, 256..511 their
``</w>`` forms, then one symbol per merge in rank order, then the two special tokens -- the layout of the real vocabulary, with
21 merges chosen for the test sentences instead of 48,894 learnt ones.

    python tests/golden/make_clip_bpe_fixture.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from xmcgan_image_generation_amd.libml import clip_bpe  # noqa: E402

MERGES = [("t", "h"), ("th", "e</w>"), ("a", "n"), ("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>"), ("i", "n"),
          ("in", "g</w>"), ("o", "n</w>"), ("'", "s</w>"), ("s", "i"), ("si", "t"), ("r", "e"), ("e", "r</w>"), ("h", "o"),
          ("ho", "r"), ("hor", "s"), ("hors", "e</w>"), ("'", "t</w>"), ("Ã", "©</w>")]


def main():
    symbols = list(clip_bpe.bytes_to_unicode().values())
    vocab = symbols + [s + "</w>" for s in symbols] + [a + b for a, b in MERGES] + [clip_bpe.START, clip_bpe.END]
    assert len(set(vocab)) == len(vocab)
    with open(os.path.join(HERE, "clip_bpe_vocab.json"), "w", encoding="utf-8") as f:
        json.dump({s: i for i, s in enumerate(vocab)}, f, ensure_ascii=False)
    with open(os.path.join(HERE, "clip_bpe_merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in MERGES))


if __name__ == "__main__":
    main()
