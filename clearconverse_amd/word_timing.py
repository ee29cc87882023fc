"""Host half of word timestamps: what openai-whisper's timing.py does around the cross-attention DTW, and the tokenizer's word
splitting it relies on.  The reference asks for it with `word_timestamps=True` (back/api.py:1435, 1477) and never reads the words;
here it is OPT-IN (`WhisperModel(word_alignment=True)`).  The device half -- the teacher-forced pass, the alignment matrix and the
DTW -- is `WhisperModel.align` (csrc/align.hip); this module only turns its jump frames into words.

Every rule below is restated from recollection [UPSTREAM-RECALL: whisper/timing.py, tokenizer.py]; **parity unpinned**: the
reference holds no fixture for it and the tests do not import openai-whisper.  A word's `probability` (the mean of its tokens'
softmax probabilities over the text ids, timing.py::find_alignment) is OPT-IN on top (`WhisperModel(word_probabilities=True)`; the
reference never reads it): without it the words carry no such key.  Not restated: the unicode-only split of the languages without
spaces.
"""
from __future__ import annotations

import string
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

HOP, SAMPLE_RATE = 160, 16000
TOKENS_PER_SECOND = 50           # audio.py: exact_div(SAMPLE_RATE, N_SAMPLES_PER_TOKEN), one encoder position = 20 ms
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END_MARKS = ".。!！?？"


@dataclass
class WordTiming:
    word: str
    tokens: List[int] = field(default_factory=list)
    start: float = 0.0
    end: float = 0.0
    probability: Optional[float] = None     # only with token probabilities (find_alignment(token_probs=))


def split_tokens_on_unicode(tokenizer, tokens: Sequence[int]) -> Tuple[List[str], List[List[int]]]:
    """[UPSTREAM-RECALL: tokenizer.py::split_tokens_on_unicode] a word ends where the tokens so far decode without a replacement
    character (or where the full text has one at that place too).  Special tokens (>= eot) decode to '' here and end a word."""
    decoded_full = tokenizer.decode(tokens)
    replacement = "�"
    words, word_tokens, current, offset = [], [], [], 0
    for t in tokens:
        current.append(int(t))
        decoded = tokenizer.decode(current)
        if replacement not in decoded or decoded_full[offset + decoded.index(replacement)] == replacement:
            words.append(decoded)
            word_tokens.append(current)
            current = []
            offset += len(decoded)
    return words, word_tokens


def split_to_word_tokens(tokenizer, tokens: Sequence[int], eot: int) -> Tuple[List[str], List[List[int]]]:
    """[UPSTREAM-RECALL: tokenizer.py::split_to_word_tokens -> split_tokens_on_spaces] (English): the unicode-safe split, then
    subwords are glued to the word before them unless they are special, start with a space or are punctuation."""
    subwords, subword_tokens = split_tokens_on_unicode(tokenizer, tokens)
    words: List[str] = []
    word_tokens: List[List[int]] = []
    for sw, st in zip(subwords, subword_tokens):
        special = st[0] >= eot
        with_space = sw.startswith(" ")
        punctuation = sw.strip() in string.punctuation
        if special or with_space or punctuation or len(words) == 0:
            words.append(sw)
            word_tokens.append(list(st))
        else:
            words[-1] = words[-1] + sw
            word_tokens[-1].extend(st)
    return words, word_tokens


def merge_punctuations(alignment: List[WordTiming], prepended: str = PREPEND_PUNCTUATIONS, appended: str = APPEND_PUNCTUATIONS) -> None:
    """[UPSTREAM-RECALL: timing.py::merge_punctuations] in place; a merged-away entry keeps word '' and no tokens.  Word and tokens
    only: the surviving entry keeps its own probability, as upstream's does."""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:
        previous, following = alignment[i], alignment[j]
        if previous.word.startswith(" ") and previous.word.strip() in prepended:
            following.word = previous.word + following.word
            following.tokens = previous.tokens + following.tokens
            previous.word, previous.tokens = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        previous, following = alignment[i], alignment[j]
        if not previous.word.endswith(" ") and following.word in appended:
            previous.word = previous.word + following.word
            previous.tokens = previous.tokens + following.tokens
            following.word, following.tokens = "", []
        else:
            i = j
        j += 1


def alignment_tokens(text_tokens: Sequence[int], rules, sot_sequence: Optional[Sequence[int]] = None) -> List[int]:
    """[UPSTREAM-RECALL: find_alignment] the teacher-forced sequence [*sot_sequence, no_timestamps, *text_tokens, eot]; sot_sequence
    defaults to [sot] (the English-only models; [sot, <|language|>, <|task|>] on a multilingual one).  Rows len(sot_sequence) .. -1
    go to the DTW."""
    sot_sequence = [rules.sot] if sot_sequence is None else [int(t) for t in sot_sequence]
    return [*sot_sequence, rules.no_timestamps, *[int(t) for t in text_tokens], rules.eot]


def find_alignment(tokenizer, rules, text_tokens: Sequence[int], jump_frame: Sequence[int],
                   token_probs: Optional[Sequence[float]] = None) -> List[WordTiming]:
    """[UPSTREAM-RECALL: find_alignment], the host half.  jump_frame: the DTW's jump frames of rows 1 .. -1 of alignment_tokens
    (len(text_tokens) + 1 entries: the encoder position at which each row starts).  Word boundaries are cumulative word-token
    counts; start / end are jump_frame / 50 seconds from the window's start.  token_probs (len(text_tokens) entries,
    WhisperModel.align(token_probs=True)): every word's `probability` is the mean of its tokens' over the same boundaries
    [`np.mean(text_token_probs[i:j]) for i, j in zip(word_boundaries[:-1], word_boundaries[1:])`]."""
    if len(text_tokens) == 0:
        return []
    words, word_tokens = split_to_word_tokens(tokenizer, list(text_tokens) + [rules.eot], rules.eot)
    if len(word_tokens) <= 1:
        return []
    boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jump_times = np.asarray(jump_frame, dtype=np.float64)[: len(text_tokens) + 1] / TOKENS_PER_SECOND
    starts, ends = jump_times[boundaries[:-1]], jump_times[boundaries[1:]]
    timings = [WordTiming(w, list(t), float(s), float(e)) for w, t, s, e in zip(words, word_tokens, starts, ends)]
    if token_probs is not None:
        tp = np.asarray(token_probs, dtype=np.float64)
        if tp.shape != (len(text_tokens),):
            raise ValueError(f"find_alignment: {tp.shape} token probabilities for {len(text_tokens)} text tokens")
        for timing, i, j in zip(timings, boundaries[:-1], boundaries[1:]):
            timing.probability = float(np.mean(tp[i:j]))
    return timings


def add_word_timestamps(segments: List[dict], tokenizer, rules, align_fn: Callable[[List[int]], Sequence[int]],
                        last_speech_timestamp: float = 0.0, prepend_punctuations: str = PREPEND_PUNCTUATIONS,
                        append_punctuations: str = APPEND_PUNCTUATIONS,
                        prob_fn: Optional[Callable[[List[int]], Sequence[float]]] = None) -> float:
    """[UPSTREAM-RECALL: timing.py::add_word_timestamps] for the segments of ONE window, in place: `words` on every segment and the
    segment bounds moved to their first / last word.  align_fn(text_tokens) -> jump frames (WhisperModel.align for this window).
    prob_fn(text_tokens) -> one probability per text token: every word dict gains `probability`; without it the dicts have no such
    key.  Returns the new last_speech_timestamp."""
    if len(segments) == 0:
        return last_speech_timestamp
    per_segment = [[t for t in s["tokens"] if t < rules.eot] for s in segments]
    text_tokens = [t for ts in per_segment for t in ts]
    alignment = []
    if text_tokens:
        alignment = find_alignment(tokenizer, rules, text_tokens, align_fn(text_tokens),
                                   token_probs=prob_fn(text_tokens) if prob_fn is not None else None)
    durations = np.array([t.end - t.start for t in alignment])
    durations = durations[durations.nonzero()]
    median_duration = min(0.7, float(np.median(durations))) if len(durations) > 0 else 0.0
    max_duration = median_duration * 2
    # "hack: truncate long words at sentence boundaries"
    if len(durations) > 0:
        for i in range(1, len(alignment)):
            if alignment[i].end - alignment[i].start > max_duration:
                if alignment[i].word in SENTENCE_END_MARKS:
                    alignment[i].end = alignment[i].start + max_duration
                elif alignment[i - 1].word in SENTENCE_END_MARKS:
                    alignment[i].start = alignment[i].end - max_duration
    merge_punctuations(alignment, prepend_punctuations, append_punctuations)
    time_offset = segments[0]["seek"] * HOP / SAMPLE_RATE
    word_index = 0
    for segment, toks in zip(segments, per_segment):
        saved, words = 0, []
        while word_index < len(alignment) and saved < len(toks):
            timing = alignment[word_index]
            if timing.word:
                words.append(dict(word=timing.word, start=round(time_offset + timing.start, 2), end=round(time_offset + timing.end, 2)))
                if prob_fn is not None:
                    words[-1]["probability"] = timing.probability
            saved += len(timing.tokens)
            word_index += 1
        if len(words) > 0:
            # "ensure the first and second word after a pause is not longer than twice the median word duration"
            if words[0]["end"] - last_speech_timestamp > median_duration * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            # "prefer the segment-level start timestamp if the first word is too long"
            if segment["start"] < words[0]["end"] and segment["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median_duration, segment["start"]))
            else:
                segment["start"] = words[0]["start"]
            # "prefer the segment-level end timestamp if the last word is too long"
            if segment["end"] > words[-1]["start"] and segment["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median_duration, segment["end"])
            else:
                segment["end"] = words[-1]["end"]
            last_speech_timestamp = segment["end"]
        segment["words"] = words
    return last_speech_timestamp


def get_end(segments: List[dict]) -> Optional[float]:
    """[UPSTREAM-RECALL: transcribe.py::get_end] end of the last word of the last segment that has one, else the last segment's end"""
    for s in reversed(segments):
        for w in reversed(s.get("words", [])):
            return w["end"]
    return segments[-1]["end"] if segments else None
