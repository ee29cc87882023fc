"""Temperature fallback and best_of: the host rules, free of any GPU state.

[UPSTREAM-RECALL: whisper/transcribe.py::decode_with_fallback, decoding.py::MaximumLikelihoodRanker, DecodingResult]; parity unpinned, as
for every other upstream rule of this package.  `WhisperModel.transcribe_batch` owns the device work (one `decode` for round 0, one
`decode_rows` per later round over the windows still failing) and asks this module what a round decodes and what a window keeps;
tests/test_fallback_reference_cpu.py drives the same functions against tests/fallback_reference.py.

The walk, per window: the temperatures of the schedule in order; the window is accepted at the first temperature at which it needs no
fallback, and at the last one whatever it scores.  At temperature 0 there is one row per window (best_of is dropped); above 0 with
best_of = n there are n, ranked by mean log-probability.  On an instance built with `beam_search=True` a temperature-0 round with
`beam_size` set decodes every window by beam search instead (`WhisperModel.decode_beam`), `beam_size` and `patience` are dropped above 0
as `best_of` is at 0, and `length_penalty` applies to both.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, List, Optional, Sequence, Tuple


def normalize_schedule(temperature) -> Tuple[float, ...]:
    """A float or a sequence of floats -> the schedule as a tuple (at least one entry, every one >= 0)."""
    sched = tuple(float(t) for t in temperature) if isinstance(temperature, (tuple, list)) else (float(temperature),)
    if not sched or not all(t >= 0.0 for t in sched):
        raise ValueError("temperature: a float >= 0 or a non-empty sequence of them")
    return sched


def rows_per_window(temperature: float, best_of: Optional[int]) -> int:
    """[UPSTREAM-RECALL: decode_with_fallback] `best_of` is dropped at temperature 0: one row per window; above 0, best_of rows."""
    if temperature == 0.0 or best_of is None:
        return 1
    if int(best_of) < 1:
        raise ValueError("best_of must be >= 1")
    return int(best_of)


def compression_ratio(text_bytes: bytes) -> float:
    """[UPSTREAM-RECALL: utils.py::compression_ratio] len(b) / len(zlib.compress(b)), b = the window's text .strip().encode("utf-8")
    (`text_compression_ratio` takes the tokens)."""
    return len(text_bytes) / len(zlib.compress(text_bytes))


def text_compression_ratio(tokenizer, tokens: Sequence[int]) -> float:
    return compression_ratio(tokenizer.decode(list(tokens)).strip().encode("utf-8"))


def needs_fallback(compression: float, avg_logprob: float, no_speech_prob: float, compression_ratio_threshold: Optional[float],
                   logprob_threshold: Optional[float], no_speech_threshold: Optional[float]) -> bool:
    """[UPSTREAM-RECALL: decode_with_fallback] too repetitive (compression ratio above its threshold) or too improbable (mean
    log-probability below its threshold) -- except a window that is silence by both of the window loop's measures (no_speech_prob above
    and mean log-probability below their thresholds, both set): the loop skips it anyway.  A threshold that is None tests nothing."""
    need = False
    if compression_ratio_threshold is not None and compression > compression_ratio_threshold:
        need = True
    if logprob_threshold is not None and avg_logprob < logprob_threshold:
        need = True
    if (no_speech_threshold is not None and logprob_threshold is not None and no_speech_prob > no_speech_threshold
            and avg_logprob < logprob_threshold):
        need = False
    return need


def rank_candidates(candidates: Sequence[dict], eot: int, length_penalty: Optional[float] = None) -> int:
    """[UPSTREAM-RECALL: decoding.py::MaximumLikelihoodRanker] index of the candidate a window keeps: tokens cut at the first eot,
    score = sum_logprob / len(tokens) with length_penalty None (the default: today's arithmetic), else sum_logprob /
    ((5 + len) / 6) ** length_penalty (the Google NMT penalty); an empty candidate scores -inf, the first maximum wins."""
    best, best_score = 0, None
    for k, c in enumerate(candidates):
        toks = list(c["tokens"])
        if eot in toks:
            toks = toks[:toks.index(eot)]
        if not toks:
            score = -math.inf
        elif length_penalty is None:
            score = c["sum_logprob"] / len(toks)
        else:
            score = c["sum_logprob"] / (((5 + len(toks)) / 6) ** length_penalty)
        if best_score is None or score > best_score:
            best, best_score = k, score
    return best


def stream_id(window: int, candidate: int, n_rows: int) -> int:
    """Noise stream of candidate `candidate` of the group's window `window` in a round of n_rows rows per window: a function of the
    window's place in its group alone, so a window's draws do not depend on which other windows are decoded with it."""
    return window * n_rows + candidate


def plan_round(failing: Sequence[int], prompts: Sequence[Sequence[int]], n_rows: int, max_batch: int) -> List[dict]:
    """One round over the windows `failing` (indices into the group, which is what is encoded), n_rows rows each, as decode_rows calls
    of at most max_batch rows: [dict(prompts, windows, stream_ids, owners)], owners[r] = (window, candidate).  Rows are window-major:
    the candidates of a window are consecutive (a window's rows may still straddle two calls)."""
    if max_batch < 1 or n_rows < 1:
        raise ValueError("plan_round: max_batch and n_rows must be >= 1")
    rows = [(w, c) for w in failing for c in range(n_rows)]
    chunks = []
    for at in range(0, len(rows), max_batch):
        part = rows[at:at + max_batch]
        chunks.append(dict(prompts=[list(prompts[w]) for w, _ in part], windows=[w for w, _ in part],
                           stream_ids=[stream_id(w, c, n_rows) for w, c in part], owners=part))
    return chunks


def window_result(candidates: Sequence[dict], temperature: float, tokenizer, eot: int, length_penalty: Optional[float] = None) -> dict:
    """What a window keeps of one round's rows [UPSTREAM-RECALL: DecodingTask.run / DecodingResult]: the ranker's pick, avg_logprob =
    sum_logprob / (n_tokens + 1), no_speech_prob of the group's FIRST row, compression_ratio of the pick's text.  Every other key of
    the pick comes along as it is: its `token_logprobs` / `top_logprobs` (a decode with logprobs=n) are the picked candidate's."""
    k = rank_candidates(candidates, eot, length_penalty)
    c = candidates[k]
    toks = list(c["tokens"])
    if eot in toks:
        toks = toks[:toks.index(eot)]
    out = dict(c)
    out.update(tokens=toks, avg_logprob=c["sum_logprob"] / (len(toks) + 1), no_speech_prob=candidates[0]["no_speech_prob"],
               temperature=float(temperature), compression_ratio=text_compression_ratio(tokenizer, toks), candidate=k)
    return out


class FallbackWalk:
    """The schedule walk of one group of windows [UPSTREAM-RECALL: decode_with_fallback, batched]: `pending()` = the windows the
    current round decodes at `temperature()`, `submit(results)` = what each of them kept (it moves on to the next round), until `done()`.  accepted[w] holds window w's
    result (with `temperature`, `compression_ratio`) once it is accepted; `trace[w]` every round's result, for tests.  `clips` / `seeks`:
    set by the caller -- which clip and which seek each window of the group is."""

    def __init__(self, n_windows: int, schedule: Sequence[float], compression_ratio_threshold: Optional[float],
                 logprob_threshold: Optional[float], no_speech_threshold: Optional[float]):
        self.schedule = tuple(schedule)
        self.thresholds = (compression_ratio_threshold, logprob_threshold, no_speech_threshold)
        self.round = 0
        self.failing: List[int] = list(range(n_windows))
        self.accepted: Dict[int, dict] = {}
        self.trace: Dict[int, List[dict]] = {w: [] for w in range(n_windows)}
        self.clips: List[int] = []
        self.seeks: List[int] = []

    def temperature(self) -> float:
        return self.schedule[self.round]

    def pending(self) -> List[int]:
        return list(self.failing)

    def done(self) -> bool:
        return not self.failing

    def submit(self, results: Dict[int, dict]) -> None:
        last = self.round == len(self.schedule) - 1
        still = []
        for w in self.failing:
            r = results[w]
            self.trace[w].append(r)
            if last or not needs_fallback(r["compression_ratio"], r["avg_logprob"], r["no_speech_prob"], *self.thresholds):
                self.accepted[w] = r
            else:
                still.append(w)
        self.failing = still
        self.round += 1
