#!/usr/bin/env python
"""Captions in (one per line), BERT features out: the reference's get_bert_for_captions (preprocess_data.py:36-58) on the HIP encoder.

usage: python tools/encode_captions.py --vocab vocab.txt --checkpoint bert_base_uncased.npz captions.txt out.npz [--fast] [--chunk 1024]

out.npz holds ``embedding`` (N, T, 768) float32, ``sentence_embedding`` (N, 768) float32 and ``max_len`` (N,) int64.
``--checkpoint`` is the np.savez of a Hugging Face BertModel's state_dict(); ``--random-weights`` is the explicit
opt-in to meaningless embeddings (plumbing checks).  ``--max-text-length`` (2..64, default 17): 64 for Localized Narratives."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("captions")
    ap.add_argument("out")
    ap.add_argument("--vocab", required=True)
    ap.add_argument("--checkpoint")
    ap.add_argument("--random-weights", action="store_true")
    ap.add_argument("--max-text-length", type=int, default=17, help="tokens per caption, [CLS]/[SEP] included: 17 (COCO), 64 (LN-COCO)")
    ap.add_argument("--fast", action="store_true", help="GEMM operands rounded to bf16 (bf16 MFMA); float32 otherwise")
    ap.add_argument("--chunk", type=int, default=1024)
    a = ap.parse_args()
    if (a.checkpoint is None) != a.random_weights:
        ap.error("give --checkpoint PATH, or --random-weights on purpose")
    from xmcgan_image_generation_amd.utils import bert_utils
    with open(a.captions, encoding="utf-8") as f:
        captions = [line.rstrip("\n") for line in f]
    enc = bert_utils.TextEncoder(a.vocab, a.checkpoint, fast=a.fast, chunk=a.chunk)
    embedding, sentence, max_len = enc.get_bert_for_captions(captions, a.max_text_length)
    np.savez(a.out, embedding=embedding, sentence_embedding=sentence, max_len=max_len)
    print(f"{len(captions)} captions -> {a.out}: embedding {embedding.shape}, max_len {int(max_len.min())}..{int(max_len.max())}")


if __name__ == "__main__":
    main()
