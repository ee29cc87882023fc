"""The host side of vocabulary control (`WhisperModel(contextual_bias=True)`): `sequence_bias`, `bad_words_ids` and `hotwords` compiled
into the one table ccx_whisper_set_bias_options takes (include/ccx.h: ccx_decode_bias_options; the kernel: csrc/dec_bias.hip).

A table is an ordered list of entries (ids, bias): the bias is added to the logit of ids[-1] whenever the tokens the decode has just
sampled end in ids[:-1] (entries of one id always apply).  Hugging Face's names and forms: `sequence_bias` is a dict tuple -> float or
a list of [ids, float]; `bad_words_ids` is a list of id lists, each an entry with bias -inf.  `hotwords` (faster-whisper's name; the
rule here is this project's) are phrases the caller wants to see: each is encoded as written and with a leading space, and every
prefix of each encoding becomes an entry with `hotword_boost` -- the first token is always boosted, each next one once the ones before
it were sampled.  `hotword_boost` has no default: no real checkpoint was at hand to tune one.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_ENTRIES, MAX_IDS, MAX_LEN = 8192, 65536, 32      # CCX_BIAS_MAX_* (include/ccx.h)


def _ids(seq, what: str) -> Tuple[int, ...]:
    if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
        raise ValueError(f"{what} = {seq!r} must be a sequence of token ids")
    out = []
    for t in seq:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"{what} = {seq!r} holds {t!r}, which is no token id")
        out.append(int(t))
    if not 1 <= len(out) <= MAX_LEN:
        raise ValueError(f"{what} has {len(out)} ids; an entry holds 1 to {MAX_LEN}")
    return tuple(out)


def _bias(value, what: str) -> np.float32:
    try:
        b = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what} = {value!r} must be a finite number or -inf") from e
    if isinstance(value, bool) or math.isnan(b) or b == math.inf or (math.isfinite(b) and abs(b) > 3.4028234e38):
        raise ValueError(f"{what} = {value!r} must be a finite number (in float32) or -inf")
    return np.float32(b)


def compile_bias_table(sequence_bias=None, bad_words_ids=None, hotwords=None, hotword_boost: Optional[float] = None,
                       encode: Optional[Callable[[str], Sequence[int]]] = None, *, eot: int,
                       n_vocab: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (offsets int32 [n + 1], ids int32 [offsets[n]], bias float32 [n]): the arrays of ccx_decode_bias_options, n = 0 when nothing
    is given.  Compiled in this order: hotwords, then sequence_bias, then bad_words_ids; a sequence that appears in more than one of
    the three gets the float32 sum of its values, in that order, at the place of its first appearance.  ValueError, saying why, for: a
    sequence named twice in the list form of sequence_bias; an entry that is empty or longer than 32 ids (a hotword phrase of more than
    32 tokens included); an id that is negative (or >= n_vocab where that is given); a target -- the last id -- that is >= eot (eot,
    the specials and the timestamps are never edited: `[eot]` cannot be a bad word); a bias that is NaN or +inf; hotwords without
    hotword_boost, or with one that is not finite and > 0, or without `encode`; more than 8192 entries or 65536 ids."""
    eot = int(eot)
    table: Dict[Tuple[int, ...], np.float32] = {}          # insertion-ordered

    def check(seq: Tuple[int, ...], what: str):
        for t in seq:
            if t < 0 or (n_vocab is not None and t >= n_vocab):
                raise ValueError(f"{what} = {list(seq)} holds the id {t}, outside the vocabulary")
        if seq[-1] >= eot:
            raise ValueError(f"{what} = {list(seq)} ends in {seq[-1]} >= eot = {eot}: <|endoftext|>, the special tokens and the "
                             f"timestamps are never edited, so they cannot be the target of a bias or a bad word")

    def add(seq: Tuple[int, ...], b: np.float32, what: str):
        check(seq, what)
        if seq in table:
            s = np.float32(table[seq] + b)
            if np.isnan(s) or s == np.inf:
                raise ValueError(f"{what} = {list(seq)}: its values sum to {s}")
            table[seq] = s
        else:
            table[seq] = b

    if hotwords is not None:
        phrases = [hotwords] if isinstance(hotwords, str) else list(hotwords)
        if hotword_boost is None:
            raise ValueError("hotwords need hotword_boost: it has no default (no real checkpoint was at hand to tune one)")
        boost = _bias(hotword_boost, "hotword_boost")
        if not (np.isfinite(boost) and boost > 0):
            raise ValueError(f"hotword_boost = {hotword_boost!r} must be finite and > 0")
        if encode is None:
            raise ValueError("hotwords need the tokenizer's `encode`")
        seen = set()
        for ph in phrases:
            if not isinstance(ph, str) or not ph.strip():
                raise ValueError(f"hotwords holds {ph!r}, which is no phrase")
            for text in (ph, " " + ph):
                toks = [int(t) for t in encode(text)]
                if len(toks) > MAX_LEN:
                    raise ValueError(f"the hotword {ph!r} encodes to {len(toks)} tokens; a phrase holds at most {MAX_LEN}")
                for k in range(1, len(toks) + 1):
                    seq = tuple(toks[:k])
                    if seq not in seen:                     # identical expanded sequences are kept once
                        seen.add(seq)
                        add(seq, boost, f"the hotword {ph!r}: its tokens")
    if sequence_bias is not None:
        if isinstance(sequence_bias, dict):
            items = list(sequence_bias.items())
        else:
            items, named = [], set()
            for i, it in enumerate(sequence_bias):
                if not hasattr(it, "__len__") or len(it) != 2:
                    raise ValueError(f"sequence_bias[{i}] = {it!r} must be [ids, bias]")
                seq = _ids(it[0], f"sequence_bias[{i}][0]")
                if seq in named:
                    raise ValueError(f"sequence_bias names the sequence {list(seq)} twice")
                named.add(seq)
                items.append((seq, it[1]))
        for seq, b in items:
            seq = _ids(seq, "a key of sequence_bias")
            add(seq, _bias(b, f"sequence_bias[{list(seq)}]"), "sequence_bias: the sequence")
    if bad_words_ids is not None:
        for i, seq in enumerate(bad_words_ids):
            add(_ids(seq, f"bad_words_ids[{i}]"), np.float32(-np.inf), f"bad_words_ids[{i}]")
    n = len(table)
    total = sum(len(s) for s in table)
    if n > MAX_ENTRIES or total > MAX_IDS:
        raise ValueError(f"the bias table holds {n} entries and {total} ids; the limits are {MAX_ENTRIES} and {MAX_IDS}")
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in table], dtype=np.int64)
    ids = np.array([t for s in table for t in s], dtype=np.int32)
    bias = np.array(list(table.values()), dtype=np.float32)
    return offsets, ids, bias
