"""WordPiece tokenizer of the caption encoder (host, pure Python).

The reference tokenizes captions with ``bert.tokenization.FullTokenizer(vocab_file, do_lower_case)`` and builds the id rows in
``preprocess_data.py:38-56``.  This module restates that algorithm:

1. clean: U+0000, U+FFFD and the control / format characters (category Cc, Cf) other than tab, newline and carriage return are
   dropped; tab, newline, carriage return, space and category Zs become one space;
2. every CJK ideograph gets a space on both sides, so it is a word of its own;
3. split on whitespace; each word is lower-cased, decomposed (NFD) and stripped of its combining marks (category Mn), then cut
   so that every punctuation character -- the four ASCII symbol runs and every category P* -- is a token of its own;
4. WordPiece: a token of more than 100 characters is ``[UNK]``; otherwise the longest vocabulary entry that matches at the
   current position is taken, greedily, non-initial pieces spelled with a leading ``##``; one position without a match makes
   the whole token ``[UNK]``.

A special token's spelling in the raw text is ordinary text: ``"[SEP]"`` becomes ``[``, ``sep``, ``]``.
"""
from __future__ import annotations

import unicodedata
from typing import Dict, List, Sequence, Tuple

import numpy as np

CLS_TOKEN, SEP_TOKEN, UNK_TOKEN = "[CLS]", "[SEP]", "[UNK]"
MAX_CHARS_PER_WORD = 100

_CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
               (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
_ASCII_PUNCT = ((33, 47), (58, 64), (91, 96), (123, 126))


def _is_whitespace(ch: str) -> bool:
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch: str) -> bool:
    return ch not in "\t\n\r" and unicodedata.category(ch) in ("Cc", "Cf")


def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    return any(lo <= cp <= hi for lo, hi in _ASCII_PUNCT) or unicodedata.category(ch).startswith("P")


def _is_cjk(ch: str) -> bool:
    cp = ord(ch)
    return any(lo <= cp <= hi for lo, hi in _CJK_RANGES)


def load_vocab(vocab_file: str) -> Dict[str, int]:
    """one token per line, id = line number; a token's surrounding whitespace is not part of it"""
    vocab: Dict[str, int] = {}
    with open(vocab_file, "r", encoding="utf-8") as f:
        for index, line in enumerate(f):
            vocab[line.strip()] = index
    return vocab


class FullTokenizer:
    """``FullTokenizer(vocab_file, do_lower_case=True)``: ``tokenize(text)`` -> WordPiece tokens, ``convert_tokens_to_ids``."""

    def __init__(self, vocab_file: str, do_lower_case: bool = True):
        self.vocab = load_vocab(vocab_file)
        self.inv_vocab = {i: t for t, i in self.vocab.items()}
        self.do_lower_case = do_lower_case
        for tok in (CLS_TOKEN, SEP_TOKEN, UNK_TOKEN):
            if tok not in self.vocab:
                raise ValueError(f"{vocab_file}: the vocabulary has no {tok}")

    # ------------------------------------------------------------------------------- words
    def basic_tokenize(self, text: str) -> List[str]:
        chars = []
        for ch in text:
            if ch in "\x00\ufffd" or _is_control(ch):
                continue
            if _is_whitespace(ch):
                chars.append(" ")
            elif _is_cjk(ch):
                chars.append(f" {ch} ")
            else:
                chars.append(ch)
        out: List[str] = []
        for word in "".join(chars).split():
            if self.do_lower_case:
                word = "".join(c for c in unicodedata.normalize("NFD", word.lower()) if unicodedata.category(c) != "Mn")
            piece = ""
            for ch in word:
                if _is_punctuation(ch):
                    if piece:
                        out.append(piece)
                    out.append(ch)
                    piece = ""
                else:
                    piece += ch
            if piece:
                out.append(piece)
        # a word can come out of the folding with whitespace in it or as nothing at all: split once more
        return " ".join(out).split()

    # ------------------------------------------------------------------------------- pieces
    def wordpiece(self, token: str) -> List[str]:
        if len(token) > MAX_CHARS_PER_WORD:
            return [UNK_TOKEN]
        pieces, start = [], 0
        while start < len(token):
            end = len(token)
            while end > start:
                sub = ("##" if start else "") + token[start:end]
                if sub in self.vocab:
                    break
                end -= 1
            if end == start:
                return [UNK_TOKEN]
            pieces.append(sub)
            start = end
        return pieces

    def tokenize(self, text: str) -> List[str]:
        return [p for tok in self.basic_tokenize(text) for p in self.wordpiece(tok)]

    def convert_tokens_to_ids(self, tokens: Sequence[str]) -> List[int]:
        return [self.vocab[t] for t in tokens]

    def convert_ids_to_tokens(self, ids: Sequence[int]) -> List[str]:
        return [self.inv_vocab[int(i)] for i in ids]

    # ------------------------------------------------------------------------------- id rows
    def encode(self, captions: Sequence[str], max_text_length: int = 17) -> Tuple[np.ndarray, np.ndarray]:
        """preprocess_data.py:38-56 -> (ids int32 (N, T), max_len int64 (N,)): pieces cut to T - 2, ``[CLS] .. [SEP]``, zero
        padding; ``max_len`` counts the non-pad positions (2 for an empty caption)"""
        if max_text_length < 2:
            raise ValueError("max_text_length must hold [CLS] and [SEP]")
        if isinstance(captions, (str, bytes)):
            raise TypeError("captions is a list of strings, not one string")
        ids = np.zeros((len(captions), max_text_length), np.int32)
        max_len = np.zeros((len(captions),), np.int64)
        for i, text in enumerate(captions):
            if isinstance(text, bytes):
                text = text.decode("utf-8")
            toks = [CLS_TOKEN] + self.tokenize(text)[:max_text_length - 2] + [SEP_TOKEN]
            ids[i, :len(toks)] = self.convert_tokens_to_ids(toks)
            max_len[i] = len(toks)
        return ids, max_len


def encode(tokenizer: FullTokenizer, captions: Sequence[str], max_text_length: int = 17):
    return tokenizer.encode(captions, max_text_length)
