"""CPU: word probabilities (clearconverse_amd/word_timing.py) and the hallucination-silence rule of `WindowLoop.advance(...,
hallucination_silence_threshold=)` against tests/wordprob_reference.py and hand-derived answers
[UPSTREAM-RECALL: whisper/timing.py::find_alignment, whisper/transcribe.py; parity unpinned]."""
import copy

import numpy as np
import pytest

from clearconverse_amd import word_timing as WT
from clearconverse_amd.tokenizer import IdTokenizer
from clearconverse_amd.whisper import WindowLoop, is_segment_anomaly, word_anomaly_score
from tests import align_reference as AR
from tests import wordprob_reference as WR
from tests.test_align_reference_cpu import DictTokenizer
from tests.test_transcribe_loop_cpu import A, B_, C_, CASES, RULES, R, run_product, ts


def W(word, start, end, p):
    return dict(word=word, start=start, end=end, probability=p)


def good(start, n=3, d=0.5):
    """n likely words of d seconds from `start`: score 0 each"""
    return [W(f" w{i}", round(start + i * d, 2), round(start + (i + 1) * d, 2), 0.9) for i in range(n)]


def bad(start, n=2, d=0.5):
    """n improbable words: score 1 each, so the segment is anomalous (score + 0.01 >= n)"""
    return [W(f" x{i}", round(start + i * d, 2), round(start + (i + 1) * d, 2), 0.05) for i in range(n)]


def run_window(tokens, words_per_segment, content=6000, seek=0, thr=2.0, last_speech=0.0, use_threshold=True):
    """One window through the product and through the reference.  words_per_segment[i] is attached to the i-th segment the
    window yields and the segment's bounds go to its first / last word, as add_word_timestamps leaves them."""
    loop = WindowLoop(RULES, IdTokenizer(), content, None, 448)
    loop.seek, loop.last_speech_timestamp = seek, last_speech
    r = dict(tokens=list(tokens), avg_logprob=-0.3, no_speech_prob=0.0)
    segs, single, seek_in = loop.window_segments(r)
    assert len(segs) == len(words_per_segment), [(s["start"], s["end"]) for s in segs]
    for s, ws in zip(segs, words_per_segment):
        s["words"] = copy.deepcopy(ws)
        if ws:
            s["start"], s["end"] = ws[0]["start"], ws[-1]["end"]
    lwe = WT.get_end(segs)
    if not single and lwe > seek / 100:
        seek_in = round(lwe * 100)              # the last-word rule that runs before this one
    ref = WR.silence_rule_ref(copy.deepcopy(segs), seek, seek_in, content, single, lwe, last_speech, thr)
    n_tokens, n_reset = len(loop.all_tokens), loop.reset
    kw = dict(hallucination_silence_threshold=thr) if use_threshold else {}
    loop.advance(r, 0.0, last_word_end=lwe, segments=copy.deepcopy(segs), **kw)
    if use_threshold:
        assert loop.seek == ref["seek"], (loop.seek, ref)
        assert [(s["start"], s["end"], s["words"]) for s in loop.segments] == [(s["start"], s["end"], s["words"]) for s in ref["segments"]]
        assert loop.last_speech_timestamp == ref["last_speech_timestamp"]
        if ref["dropped"]:
            assert loop.segments == [] and len(loop.all_tokens) == n_tokens and loop.reset == n_reset
    return loop, ref


def test_word_anomaly_score_known_answers():
    cases = [(W(" a", 1.0, 1.5, 0.9), 0.0), (W(" a", 1.0, 1.5, 0.1), 1.0), (W(" a", 1.0, 1.5, 0.15), 0.0),
             (W(" a", 1.0, 1.033, 0.9), 1.5), (W(" a", 1.0, 4.5, 0.9), 1.5), (W(" a", 2.0, 2.0, 0.0), 1.0 + 0.133 * 15),
             (dict(word=" a", start=0.0, end=0.5), 1.0)]                       # no probability key counts as 0
    for w, want in cases:
        assert word_anomaly_score(w) == pytest.approx(want, abs=1e-9), w
        assert WR.anomaly_score_ref(w) == pytest.approx(want, abs=1e-9), w


def test_segment_anomaly_punctuation_filter_and_eight_word_cap():
    for fn in (is_segment_anomaly, WR.segment_anomaly_ref):
        assert fn(None) is False and fn(dict(words=[])) is False
        assert fn(dict(words=good(0.0, 3))) is False
        assert fn(dict(words=bad(0.0, 2))) is True                     # 2 + 0.01 >= 2
        assert fn(dict(words=bad(0.0, 3))) is True                     # 3 >= 3
        assert fn(dict(words=good(0.0, 3) + bad(1.5, 2))) is False     # 2 < 3 and 2.01 < 5
        assert fn(dict(words=good(0.0, 1) + bad(0.5, 3))) is True      # 3 >= 3
        # two instantaneous improbable punctuation marks would score 2 x 2.995 on their own: they are not counted
        marks = [W(",", 1.0, 1.0, 0.01), W(".", 2.0, 2.0, 0.01)]
        assert fn(dict(words=good(0.0, 2) + marks)) is False
        assert fn(dict(words=good(0.0, 2) + [W(" ,", 1.0, 1.0, 0.01), W(" .", 2.0, 2.0, 0.01)])) is True      # not bare marks: counted, 5.99 >= 3
        # only the first 8 counted words: five improbable words behind eight likely ones do not make it anomalous, ...
        assert fn(dict(words=good(0.0, 8) + bad(4.0, 5))) is False
        # ... marks in between do not use up the eight, and three improbable words among the first eight do
        assert fn(dict(words=good(0.0, 5) + marks + bad(2.5, 3) + good(4.0, 4))) is True
        assert fn(dict(words=good(0.0, 6) + marks + bad(3.0, 3))) is False             # the third improbable word is the ninth


def test_remaining_duration_branch_both_ways():
    toks = [ts(0), A, ts(5), ts(5)]                                     # ends on a pair: not a single-timestamp ending
    # the last word ends at 20.0 s, 10 s before the window's end: resume there
    loop, ref = run_window(toks, [good(18.5, 3)])
    assert loop.seek == 2000 and ref["branches"] >= {"remaining_long"}
    # the last word ends at 29.0 s, 1 s <= 2 s before the end: the window's end, not the last-word rule's 2900
    loop, ref = run_window(toks, [good(27.5, 3)])
    assert loop.seek == 3000 and ref["branches"] >= {"remaining_short"}
    assert run_window(toks, [good(27.5, 3)], use_threshold=False)[0].seek == 2900
    # on a single-timestamp ending the branch does not apply
    loop, ref = run_window([ts(0), A, ts(5)], [good(18.5, 3)])
    assert loop.seek == 3000 and not ref["branches"] & {"remaining_long", "remaining_short"}


def test_leading_gap_before_an_anomalous_first_segment_drops_the_window():
    loop, ref = run_window([ts(10), A, B_, ts(12)], [bad(10.0, 2)], last_speech=3.0)
    assert ref["dropped"] and ref["branches"] >= {"leading_gap_drop"}
    assert loop.seek == 1000 and loop.segments == [] and loop.all_tokens == [] and loop.last_speech_timestamp == 3.0
    # a gap of exactly the threshold is not "longer": the window stays (and the segment, next to the window's start, is cut instead)
    loop, ref = run_window([ts(2), A, B_, ts(4)], [bad(2.0, 2)])
    assert not ref["dropped"]
    # a likely first segment behind the same gap stays whole
    loop, ref = run_window([ts(10), A, B_, ts(12)], [good(10.0, 2)])
    assert not ref["dropped"] and loop.seek == 3000 and len(loop.segments) == 1 and loop.last_speech_timestamp == 11.0


def test_anomalous_segment_between_silences_truncates_the_window():
    toks = [ts(0), A, ts(5), ts(10), B_, ts(11), ts(15), C_, ts(20)]
    loop, ref = run_window(toks, [good(3.5, 3), bad(10.0, 2), good(15.0, 3)])
    # 10.0 - 5.0 > 2 before, 15.0 - 11.0 > 2 after: seek = max(0 + 1, 10.0) s, the first segment stays
    assert ref["branches"] >= {"truncate", "normal_moves_hal_last_end"} and "seek_content" not in ref["branches"]
    assert loop.seek == 1000 and [(s["start"], s["end"]) for s in loop.segments] == [(3.5, 5.0)]
    assert loop.last_speech_timestamp == 5.0 and loop.all_tokens == [ts(0), A, ts(5)]
    # speech right behind it (12.0 - 11.0 <= 2, likely, far from the window's end): kept
    loop, ref = run_window(toks, [good(3.5, 3), bad(10.0, 2), good(12.0, 3)])
    assert "truncate" not in ref["branches"] and "anomaly_kept" in ref["branches"] and loop.seek == 3000 and len(loop.segments) == 3
    # another anomaly behind it counts as silence
    loop, ref = run_window(toks, [good(3.5, 3), bad(10.0, 2), bad(12.0, 2)])
    assert "truncate" in ref["branches"] and loop.seek == 1000
    # the window's first second is never decoded again: seek = time_offset + 1 for an anomaly at the very start
    loop, ref = run_window([ts(0), A, ts(1), ts(5), B_, ts(8)], [bad(0.0, 2), good(5.0, 3)], content=9000, seek=3000, last_speech=29.0)
    assert "truncate" in ref["branches"] and loop.seek == 3100 and loop.segments == [] and loop.last_speech_timestamp == 29.0


def test_truncation_near_the_end_of_the_clip_seeks_to_content():
    toks = [ts(0), A, ts(5), ts(10), B_, ts(11)]
    # 12 s clip: nothing follows (12.0 - 11.0 <= 2 but the window ends within 2 s), and 12.0 - 11.0 < 2: the clip is finished
    loop, ref = run_window(toks, [good(3.5, 3), bad(10.0, 2)], content=1200)
    assert ref["branches"] >= {"truncate", "seek_content"} and loop.seek == 1200 and len(loop.segments) == 1
    # 14 s clip: 14.0 - 11.0 > 2 of silence behind it, so it is cut, but 3 s of the clip are left: seek stays at the segment's start
    loop, ref = run_window(toks, [good(3.5, 3), bad(10.0, 2)], content=1400)
    assert "truncate" in ref["branches"] and "seek_content" not in ref["branches"] and loop.seek == 1000 and len(loop.segments) == 1
    # 13 s clip: exactly 2 s behind it on both counts, which is neither "longer" nor "less": the segment stays
    loop, ref = run_window(toks, [good(3.5, 3), bad(10.0, 2)], content=1300)
    assert "truncate" not in ref["branches"] and loop.seek == 1300 and len(loop.segments) == 2


def test_a_likely_segment_moves_hal_last_end():
    """The second window of a 90 s clip (30 s .. 60 s), threshold 3 s, the previous window's speech ended at 25.0 s.  Segments
    [30.5, 32.0], [32.5, 33.5] (improbable words) and [37.0, ...]: 37.0 - 33.5 > 3 of silence behind the anomaly; its leading gap of
    2.5 s is no longer than the threshold, so the window is not dropped."""
    toks = [ts(0.5), A, ts(2), ts(2.5), B_, ts(3.5), ts(7), C_, ts(12)]
    kw = dict(content=9000, seek=3000, thr=3.0, last_speech=25.0)
    # measured from 25.0 the anomaly at 32.5 would have silence before it (7.5 > 3); the likely segment that ends at 32.0 takes that
    # away (0.5 <= 3, 32.5 >= 3, 2.5 s into the window >= 2)
    loop, ref = run_window(toks, [good(30.5, 3), bad(32.5, 2), good(37.0, 3)], **kw)
    assert "truncate" not in ref["branches"] and ref["branches"] >= {"normal_moves_hal_last_end", "anomaly_kept"}
    assert loop.seek == 6000 and len(loop.segments) == 3 and loop.last_speech_timestamp == 38.5
    # a segment without words does not move it: cut at the anomaly; the segment before it stays and gives the last speech time
    loop, ref = run_window(toks, [[], bad(32.5, 2), good(37.0, 3)], **kw)
    assert "truncate" in ref["branches"] and "normal_moves_hal_last_end" not in ref["branches"]
    assert loop.seek == 3250 and [(s["start"], s["end"]) for s in loop.segments] == [(30.5, 32.0)] and loop.last_speech_timestamp == 32.0


def _random_words(g, start, end):
    n = int(g.integers(1, 11))
    t, out = start, []
    for i in range(n):
        kind = int(g.integers(0, 6))
        d = [0.3, 0.5, 0.05, 0.0, 3.0, 0.2][kind]
        p = float(g.choice([0.02, 0.1, 0.2, 0.6, 0.95]))
        word = str(g.choice([" a", " word", ",", ".", " (", "-", " long"]))
        out.append(W(word, round(t, 2), round(t + d, 2), p))
        t += d + float(g.choice([0.0, 0.0, 0.1, 2.5]))
    return out


def test_advance_equals_the_reference_on_seeded_scripted_windows():
    g = np.random.default_rng(7)
    seen, n_windows = set(), 0
    for case in range(400):
        content = int(g.integers(100, 9000))
        seek = int(g.integers(0, max(1, content - 50)))
        size = min(3000, content - seek)
        toks, t = [], float(g.integers(0, 600)) * 0.02
        for _ in range(int(g.integers(1, 5))):
            toks.append(ts(t))
            toks += [int(x) for x in g.integers(1000, 40000, int(g.integers(1, 4)))]
            t = min(t + float(g.integers(1, 500)) * 0.02, 30.0)
            toks.append(ts(t))
            t = min(t + float(g.choice([0.0, 0.0, 1.0, 4.0])), 30.0)
        tail = int(g.integers(0, 3))
        if tail == 1:
            toks += [ts(t), int(g.integers(1000, 40000))]
        elif tail == 2:
            toks.append(toks[-1])
        loop = WindowLoop(RULES, IdTokenizer(), content, None, 448)
        loop.seek = seek
        segs = loop.window_segments(dict(tokens=toks, avg_logprob=-0.3, no_speech_prob=0.0))[0]
        words = [[] if g.integers(0, 5) == 0 else _random_words(g, s["start"], s["end"]) for s in segs]
        thr = float(g.choice([0.0, 0.5, 2.0, 5.0]))
        last_speech = float(g.choice([0.0, seek / 100 - 1.0, seek / 100 - 6.0]))
        _, ref = run_window(toks, words, content=content, seek=seek, thr=thr, last_speech=max(0.0, last_speech))
        seen |= ref["branches"]
        n_windows += 1
    assert n_windows >= 200
    assert seen == {"remaining_long", "remaining_short", "leading_gap_drop", "truncate", "seek_content", "anomaly_kept",
                    "normal_moves_hal_last_end"}, seen


def test_threshold_none_leaves_every_scripted_case_unchanged():
    """advance(..., hallucination_silence_threshold=None) is advance(...)"""
    advance = WindowLoop.advance
    for name, c in CASES.items():
        tk = c.get("tokenizer") or IdTokenizer()
        base = run_product(c["content"], c["script"], tk, c.get("prompt"), c.get("temperature", 0.0), **c.get("kw", {}))
        try:
            WindowLoop.advance = lambda self, r, temperature=0.0, **kw: advance(self, r, temperature, hallucination_silence_threshold=None, **kw)
            got = run_product(c["content"], c["script"], tk, c.get("prompt"), c.get("temperature", 0.0), **c.get("kw", {}))
        finally:
            WindowLoop.advance = advance
        assert got == base, name
    # ... and with words and a last-word end as well
    toks = [ts(0), A, ts(5), ts(10), B_, ts(11), ts(15), C_, ts(20), ts(20)]
    words = [good(3.5, 3), bad(10.0, 2), good(15.0, 3)]
    a, _ = run_window(toks, words, use_threshold=False)
    loop = WindowLoop(RULES, IdTokenizer(), 6000, None, 448)
    r = dict(tokens=toks, avg_logprob=-0.3, no_speech_prob=0.0)
    segs = loop.window_segments(r)[0]
    for s, ws in zip(segs, words):
        s["words"], s["start"], s["end"] = copy.deepcopy(ws), ws[0]["start"], ws[-1]["end"]
    loop.advance(r, 0.0, last_word_end=WT.get_end(segs), segments=segs, hallucination_silence_threshold=None)
    assert (loop.seek, loop.segments, loop.all_tokens, loop.last_speech_timestamp) == (a.seek, a.segments, a.all_tokens, a.last_speech_timestamp)
    assert loop.seek == 1650 and len(loop.segments) == 3


def test_word_probabilities_are_refused_without_word_alignment():
    from clearconverse_amd._lib import CcxError
    from clearconverse_amd.weights import WhisperDims
    from clearconverse_amd.whisper import WhisperModel
    with pytest.raises(CcxError, match="word_alignment"):
        WhisperModel(WhisperDims.mini(2, 128), {}, word_probabilities=True)


def test_word_timing_keeps_positional_construction():
    t = WT.WordTiming(" a", [1], 0.0, 0.5)
    assert t.probability is None and WT.WordTiming(" a", [1], 0.0, 0.5, 0.25).probability == 0.25


def test_add_word_timestamps_with_and_without_prob_fn():
    tk = DictTokenizer({1: " Hi", 2: ".", 3: " th", 4: "ere", 5: " friend", 6: " (", 7: " you", 8: ")"})
    text = [1, 2, 3, 4, 5, 6, 7, 8]
    jumps = [0, 10, 20, 35, 50, 60, 70, 80, 90]
    probs = [0.9, 0.5, 0.4, 0.2, 0.7, 0.1, 0.6, 0.3]

    def seg():
        return dict(seek=500, start=5.0, end=8.0, tokens=[ts(0), *text, ts(3)], text="x")
    plain = seg()
    WT.add_word_timestamps([plain], tk, RULES, lambda toks: jumps)
    assert all(set(w) == {"word", "start", "end"} for w in plain["words"]) and len(plain["words"]) == 4
    with_p = seg()
    asked = []
    WT.add_word_timestamps([with_p], tk, RULES, lambda toks: jumps, prob_fn=lambda toks: asked.append(list(toks)) or probs)
    assert asked == [text]
    # everything but the new key is what it is without prob_fn
    assert [{k: v for k, v in w.items() if k != "probability"} for w in with_p["words"]] == plain["words"]
    assert (with_p["start"], with_p["end"]) == (plain["start"], plain["end"])
    # the reference: per-word means over the word-token counts, and a merged entry keeps the probability of the entry that survives
    # (" Hi" + ".", " (" + " you" + ")": the surviving entries are " Hi" and " you")
    words = [" Hi", ".", " there", " friend", " (", " you", ")"]
    means = WR.word_probs_ref(probs, [1, 1, 2, 1, 1, 1, 1])
    assert means == pytest.approx([0.9, 0.5, 0.3, 0.7, 0.1, 0.6, 0.3], abs=1e-15)
    merged = AR.merge_punctuations_ref([[w, [i]] for i, w in enumerate(words)])
    want = [(w, means[i]) for i, (w, _) in enumerate(merged) if w]
    assert [w for w, _ in want] == [" Hi.", " there", " friend", " ( you)"]
    assert [(w["word"], w["probability"]) for w in with_p["words"]] == [(w, pytest.approx(p, abs=1e-12)) for w, p in want]
    assert [w["probability"] for w in with_p["words"]] == pytest.approx([0.9, 0.3, 0.7, 0.6], abs=1e-12)
    # find_alignment on its own, and a wrong number of probabilities is refused
    al = WT.find_alignment(tk, RULES, text, jumps, token_probs=probs)
    assert [a.probability for a in al] == pytest.approx(means, abs=1e-12)
    assert all(a.probability is None for a in WT.find_alignment(tk, RULES, text, jumps))
    with pytest.raises(ValueError):
        WT.find_alignment(tk, RULES, text, jumps, token_probs=probs[:-1])


def test_pick_probs_reference_known_answers():
    lg = np.array([[0.0, np.log(3.0), np.nan, np.inf], [1.0, -np.inf, 1.0, 7.0], [5.0, 5.0, 5.0, 5.0]], dtype=np.float32)
    p, logp = WR.pick_probs_ref(lg, 2, [1, -1, 0])
    assert p[0] == pytest.approx(0.75, abs=1e-7) and np.isnan(p[1]) and p[2] == pytest.approx(0.5, abs=1e-12)
    p, logp = WR.pick_probs_ref(lg[1:2], 3, [1])
    assert p[0] == 0.0 and logp[0] == -np.inf
    p, _ = WR.pick_probs_ref(lg[1:2], 3, [2])
    assert p[0] == pytest.approx(0.5, abs=1e-12)
