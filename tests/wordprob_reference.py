"""numpy / fp64 restatements for word probabilities and hallucination-silence skipping (tests/test_wordprob_reference_cpu.py,
tests/test_pick_probs_gpu.py, tests/test_word_probs_gpu.py).  Written from the rule's statement, not from the product code.

* `pick_probs_ref`: what dec_pick_probs_kernel (csrc/dec_probs.hip) computes, in fp64 on the same fp32 logits.
* `word_probs_ref`: a word's probability = mean of its tokens' [UPSTREAM-RECALL: timing.py::find_alignment].
* `anomaly_score_ref`, `segment_anomaly_ref`, `silence_rule_ref`: [UPSTREAM-RECALL: whisper/transcribe.py, the
  hallucination_silence_threshold block]; parity unpinned.  `silence_rule_ref` is a pure function of one window.
"""
import math
import string

import numpy as np

FPS = 100      # mel frames per second


def pick_probs_ref(logits, hi, picks):
    """logits [rows, ld] fp32, picks [rows] (-1: skipped) -> (p, log p) fp64 [rows]; NaN where skipped.  Softmax over the columns
    [0, hi) only; -inf inside contributes 0; a picked -inf has p = 0 and log p = -inf."""
    lg = np.asarray(logits)
    p = np.full(lg.shape[0], np.nan)
    logp = np.full(lg.shape[0], np.nan)
    for r, k in enumerate(picks):
        k = int(k)
        if k < 0:
            continue
        assert k < hi
        x = lg[r, :hi].astype(np.float64)
        m = x.max()
        lse = m + math.log(np.exp(x - m).sum())
        logp[r] = x[k] - lse
        p[r] = math.exp(logp[r]) if np.isfinite(logp[r]) else 0.0
    return p, logp


def word_probs_ref(token_probs, word_token_counts):
    """token_probs: one per text token; word_token_counts: tokens of every word, in order -> one mean per word"""
    tp = [float(x) for x in token_probs]
    out, at = [], 0
    for n in word_token_counts:
        out.append(math.fsum(tp[at:at + n]) / n)
        at += n
    assert at == len(tp)
    return out


def anomaly_score_ref(word):
    p = word["probability"] if "probability" in word else 0.0
    d = word["end"] - word["start"]
    s = 1.0 if p < 0.15 else 0.0
    if d < 0.133:
        s = s + (0.133 - d) * 15
    if d > 2.0:
        s = s + (d - 2.0)
    return s


def segment_anomaly_ref(segment):
    if segment is None:
        return False
    ws = segment.get("words") or []
    if len(ws) == 0:
        return False
    counted = []
    for w in ws:
        if w["word"] in string.punctuation:
            continue
        counted.append(w)
        if len(counted) == 8:
            break
    score = 0.0
    for w in counted:
        score += anomaly_score_ref(w)
    return score >= 3 or score + 0.01 >= len(counted)


def _first_with_words(segs):
    for s in segs:
        if s.get("words"):
            return s
    return None


def _end_of(segs):
    """get_end: the end of the last word of the last segment that has one, else the last segment's end, else None"""
    for s in segs[::-1]:
        if s.get("words"):
            return s["words"][-1]["end"]
    return segs[-1]["end"] if len(segs) else None


def silence_rule_ref(segments, previous_seek, seek_in, content, single_timestamp_ending, last_word_end, last_speech_timestamp,
                     threshold):
    """One window.  segments: the window's, words attached.  previous_seek: where the window started; seek_in: the next seek by the
    rules before this one (timestamp tokens, then the last-word rule); content: frames of the clip; last_word_end: get_end of the
    segments; last_speech_timestamp: the previous window's.
    -> dict(seek, segments (kept), dropped, last_speech_timestamp, branches: set of names of what fired).
    The last statement is the product's never-loop guard: a seek that did not move forward goes to the window's end."""
    size = min(3000, content - previous_seek)
    t0 = previous_seek / FPS
    dur = size / FPS
    t_end = (previous_seek + size) / FPS
    seek, fired = seek_in, set()

    def guard(s):
        return previous_seek + size if s <= previous_seek else s

    if not single_timestamp_ending and last_word_end is not None and last_word_end > t0:
        if t_end - last_word_end > threshold:
            seek = round(last_word_end * FPS)
            fired.add("remaining_long")
        else:
            seek = previous_seek + size
            fired.add("remaining_short")
    first = _first_with_words(segments)
    if first is not None and segment_anomaly_ref(first) and first["start"] - t0 > threshold:
        fired.add("leading_gap_drop")
        return dict(seek=guard(previous_seek + round((first["start"] - t0) * FPS)), segments=[], dropped=True,
                    last_speech_timestamp=last_speech_timestamp, branches=fired)
    kept = list(segments)
    last_end = last_speech_timestamp
    for si in range(len(segments)):
        s = segments[si]
        if not s.get("words"):
            continue
        if segment_anomaly_ref(s):
            nxt = _first_with_words(segments[si + 1:])
            next_start = nxt["words"][0]["start"] if nxt is not None else t0 + dur
            before = (s["start"] - last_end > threshold) or (s["start"] < threshold) or (s["start"] - t0 < 2.0)
            after = (next_start - s["end"] > threshold) or segment_anomaly_ref(nxt) or (t_end - s["end"] < 2.0)
            if before and after:
                seek = round(max(t0 + 1, s["start"]) * FPS)
                fired.add("truncate")
                if content / FPS - s["end"] < threshold:
                    seek = content
                    fired.add("seek_content")
                kept = list(segments[:si])
                break
            fired.add("anomaly_kept")
        else:
            fired.add("normal_moves_hal_last_end")
        last_end = s["end"]
    end = _end_of(kept)
    return dict(seek=guard(seek), segments=kept, dropped=False,
                last_speech_timestamp=last_speech_timestamp if end is None else end, branches=fired)
