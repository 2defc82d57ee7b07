"""CLIP's byte-level BPE tokenizer in pure Python (OpenAI's ``simple_tokenizer.py`` / ``transformers.CLIPTokenizer`` without ftfy):
NFC, whitespace collapsed, lower-cased; split by

    <|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|\\p{L}+|\\p{N}|[^\\s\\p{L}\\p{N}]+

(the scanner below walks ``unicodedata`` categories: the ``regex`` package is not required); every piece goes through the GPT-2
byte-to-unicode table, gets ``</w>`` on its last symbol and is merged by rank.  ``vocab.json`` (symbol -> id) and ``merges.txt``
are the files of ``openai/clip-vit-base-patch32``; nothing is downloaded.
"""
from __future__ import annotations

import json
import unicodedata

import numpy as np

START, END = "<|startoftext|>", "<|endoftext|>"
_SUFFIXES = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def bytes_to_unicode():
    """GPT-2's reversible byte -> printable unicode character table"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def _kind(ch):
    """'L' letter, 'N' number, 'S' whitespace, 'O' anything else"""
    if ch.isspace():
        return "S"
    cat = unicodedata.category(ch)[0]
    return cat if cat in "LN" else "O"


def split(text: str):
    """the pieces the pattern above finds in ``text``, in order (leftmost alternative first, runs greedy)"""
    out, i, n = [], 0, len(text)
    while i < n:
        for lit in (START, END) + _SUFFIXES:
            if text.startswith(lit, i):
                out.append(lit)
                i += len(lit)
                break
        else:
            k = _kind(text[i])
            j = i + 1
            if k == "L":
                while j < n and _kind(text[j]) == "L":
                    j += 1
            elif k == "O":
                while j < n and _kind(text[j]) == "O":
                    j += 1
            if k != "S":                             # (a number is one character: digits split singly)
                out.append(text[i:j])
            i = j
    return out


def clean(text) -> str:
    if isinstance(text, bytes):
        text = text.decode("utf-8")
    return " ".join(unicodedata.normalize("NFC", text).split()).lower()


class ClipTokenizer:
    def __init__(self, vocab_file, merges_file):
        with open(vocab_file, encoding="utf-8") as f:
            self.encoder = {k: int(v) for k, v in json.load(f).items()}
        with open(merges_file, encoding="utf-8") as f:
            lines = [ln.rstrip("\n") for ln in f]
        merges = [tuple(ln.split()) for ln in lines if ln.strip() and not ln.startswith("#version")]
        bad = [m for m in merges if len(m) != 2]
        if bad:
            raise ValueError(f"{merges_file}: a merge is two symbols, got {bad[0]}")
        for tok in (START, END):
            if tok not in self.encoder:
                raise ValueError(f"{vocab_file}: no {tok} entry")
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        self.start_id, self.end_id = self.encoder[START], self.encoder[END]
        self.pad_id = self.end_id                    # transformers.CLIPTokenizer pads with <|endoftext|>
        self.vocab_size = max(self.encoder.values()) + 1
        self._cache = {START: (START,), END: (END,)}

    def bpe(self, token: str):
        """the symbols of one piece (already in the byte alphabet) after every applicable merge, lowest rank first"""
        got = self._cache.get(token)
        if got is not None:
            return got
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            new, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    new.append(a + b)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        self._cache[token] = word
        return word

    def tokenize(self, text):
        """-> list of vocabulary symbols (no start / end)"""
        out = []
        for piece in split(clean(text)):
            if piece not in (START, END):
                piece = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
            out.extend(self.bpe(piece))
        return out

    def encode(self, captions, context: int = 77):
        """-> (ids int32 (n, context), eot int32 (n,)): <|startoftext|>, at most ``context - 2`` tokens, <|endoftext|>, then the pad id
        (= <|endoftext|>'s); ``eot[i]`` is the position of the first <|endoftext|> of row i.  A symbol the vocabulary lacks maps
        to <|endoftext|>, transformers' unknown token."""
        if isinstance(captions, (str, bytes)):
            captions = [captions]
        if context < 2:
            raise ValueError(f"context {context}: a row holds at least the start and the end token")
        ids = np.full((len(captions), context), self.pad_id, np.int32)
        eot = np.zeros((len(captions),), np.int32)
        for r, cap in enumerate(captions):
            toks = [self.encoder.get(s, self.end_id) for s in self.tokenize(cap)][:context - 2]
            row = [self.start_id] + toks + [self.end_id]
            ids[r, :len(row)] = row
            eot[r] = row.index(self.end_id)
        return ids, eot
