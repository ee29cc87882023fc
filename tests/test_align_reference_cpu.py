"""CPU: the references of tests/align_reference.py against an independent implementation and hand-derived answers, the host word rules
of clearconverse_amd/word_timing.py on hand-derived cases, and `WindowLoop.advance(..., last_word_end=)` against
oracle/whisper_transcribe_ref.py driven with the same last-word ends (the seek rule of transcribe(word_timestamps=True), reference
back/api.py:1435, 1477)."""
import numpy as np
import pytest
import torch

from clearconverse_amd import word_timing as WT
from clearconverse_amd.tokenizer import IdTokenizer
from clearconverse_amd.whisper import WindowLoop
from tests import align_reference as AR
from tests.test_transcribe_loop_cpu import B_, C_, CASES, RULES, R, run_oracle, run_product, table, ts


def test_median_filter_and_dtw_equal_the_transformers_implementation():
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    g = torch.Generator().manual_seed(0)
    for case in range(20):
        H, T, M = int(torch.randint(1, 4, (1,), generator=g)), int(torch.randint(1, 12, (1,), generator=g)), int(torch.randint(1, 40, (1,), generator=g))
        x = torch.randn(H, T, M, generator=g)
        if case % 4 == 0:
            x = (x * 2).round() / 2                      # ties inside the median windows
        assert torch.equal(AR.median_filter_ref(x, 7), gw._median_filter(x[None], 7)[0]), case
        c = x[0].numpy() if case % 2 else (x[0] * 4).round().numpy() / 4       # every other case: a grid, so that costs tie
        for fn in (AR.dtw_ref, AR.dtw_ref_fast):
            ti, tj = fn(c)
            ri, rj = gw._dynamic_time_warping(c.astype(np.float32))
            assert np.array_equal(ti, ri) and np.array_equal(tj, rj), (case, fn.__name__)


def test_dtw_hand_derived_answers():
    # 3 x 5, cost 1 everywhere but on the staircase (0,0) (0,1) (1,2) (2,3) (2,4): the only path of cost 0
    x = np.ones((3, 5), dtype=np.float32)
    for i, j in ((0, 0), (0, 1), (1, 2), (2, 3), (2, 4)):
        x[i, j] = 0
    for fn in (AR.dtw_ref, AR.dtw_ref_fast):
        ti, tj = fn(x)
        assert ti.tolist() == [0, 0, 1, 2, 2] and tj.tolist() == [0, 1, 2, 3, 4]
        assert AR.jump_frames(ti, tj).tolist() == [0, 2, 3]
    # all ties (3 x 4 zeros): every inner cell takes "left", so the backtrace runs along the last row to the border column, then up
    for fn in (AR.dtw_ref, AR.dtw_ref_fast):
        ti, tj = fn(np.zeros((3, 4), dtype=np.float32))
        assert ti.tolist() == [0, 1, 2, 2, 2, 2] and tj.tolist() == [0, 0, 0, 1, 2, 3]
        assert AR.jump_frames(ti, tj).tolist() == [0, 0, 0]


def test_matrix_reference_statistics():
    """population std over ALL token rows, per (head, frame); M <= 3 stays unfiltered"""
    g = torch.Generator().manual_seed(1)
    P = torch.rand(2, 5, 3, generator=g)
    A = AR.matrix_ref(P)
    z = (P.double() - P.double().mean(1, keepdim=True)) / P.double().var(1, unbiased=False, keepdim=True).sqrt()
    assert torch.allclose(A, z.mean(0), atol=1e-12)
    P = torch.rand(1, 4, 9, generator=g)
    A = AR.matrix_ref(P)
    z = ((P.double() - P.double().mean(1, keepdim=True)) / P.double().var(1, unbiased=False, keepdim=True).sqrt())[0]
    win = torch.stack([z[:, [3, 2, 1, 0, 1, 2, 3]], z[:, [5, 6, 7, 8, 7, 6, 5]]])       # frames 0 and 8 with reflect padding (5 .. 8, 7, 6, 5)
    assert torch.allclose(A[:, 0], win[0].sort(-1)[0][:, 3]) and torch.allclose(A[:, 8], win[1].sort(-1)[0][:, 3])


class DictTokenizer:
    """ids -> fixed strings; ids >= eot decode to nothing, as the product's tokenizers do"""
    def __init__(self, table_):
        self.t = table_

    def decode(self, ids):
        return "".join(self.t[int(i)] for i in ids if int(i) < RULES.eot)


def _timings(words):
    return [WT.WordTiming(w, list(t), 0.0, 0.0) for w, t in words]


def test_merge_punctuations_hand_derived():
    words = [(" Hello", [1]), (",", [2]), (" (", [3]), ("world", [4]), (")", [5]), (' "', [6]), (" quoted", [7]), (".", [8])]
    al = _timings(words)
    WT.merge_punctuations(al)
    assert [(a.word, a.tokens) for a in al if a.word] == [(" Hello,", [1, 2]), (" (world)", [3, 4, 5]), (' " quoted.', [6, 7, 8])]
    assert [a.tokens for a in al if not a.word] == [[]] * 5
    assert [(w, t) for w, t in AR.merge_punctuations_ref([[w, t] for w, t in words])] == [(a.word, a.tokens) for a in al]
    g = np.random.default_rng(0)
    vocab = [" a", "b", " (", ")", ".", ",", ' "', " -", " word", "'", " ", "?"]
    for _ in range(200):
        ws = [(vocab[int(i)], [k]) for k, i in enumerate(g.integers(0, len(vocab), int(g.integers(0, 9))))]
        al = _timings(ws)
        WT.merge_punctuations(al)
        assert [[a.word, a.tokens] for a in al] == AR.merge_punctuations_ref([[w, t] for w, t in ws])


def test_split_to_word_tokens_and_find_alignment():
    tk = DictTokenizer({1: " Hi", 2: ".", 3: " th", 4: "ere", 5: " friend"})
    words, toks = WT.split_to_word_tokens(tk, [1, 2, 3, 4, 5, RULES.eot], RULES.eot)
    assert words == [" Hi", ".", " there", " friend", ""] and toks == [[1], [2], [3, 4], [5], [RULES.eot]]
    assert WT.alignment_tokens([1, 2], RULES) == [RULES.sot, RULES.no_timestamps, 1, 2, RULES.eot]
    # jump frames of the rows [no_timestamps, 1, 2, 3, 4, 5]: a word starts at its first token's frame and ends at the next word's
    al = WT.find_alignment(tk, RULES, [1, 2, 3, 4, 5], [0, 10, 20, 35, 50, 60])
    assert [(a.word, a.start, a.end) for a in al] == [(" Hi", 0.0, 0.2), (".", 0.2, 0.4), (" there", 0.4, 1.0), (" friend", 1.0, 1.2)]
    assert WT.find_alignment(tk, RULES, [], []) == []


def test_long_word_truncation_and_segment_bounds_hand_derived():
    """Durations 0.2, 0.2, 2.0, 0.2 s: median 0.2, so a word may last 0.4 s; ' there' follows a sentence end and is cut to its last
    0.4 s.  The segment's bounds move to its first and last word; the '.' joins ' Hi' without changing its times."""
    tk = DictTokenizer({1: " Hi", 2: ".", 3: " there", 4: " friend"})
    seg = dict(seek=500, start=5.0, end=8.0, tokens=[ts(0), 1, 2, 3, 4, ts(3)], text=" Hi. there friend")
    last = WT.add_word_timestamps([seg], tk, RULES, lambda toks: [0, 10, 20, 120, 130], last_speech_timestamp=4.9)
    assert seg["words"] == [dict(word=" Hi.", start=5.0, end=5.2), dict(word=" there", start=7.0, end=7.4), dict(word=" friend", start=7.4, end=7.6)]
    assert (seg["start"], seg["end"], last) == (5.0, 7.6, 7.6)
    # a sentence-end mark that is itself too long keeps its first 0.4 s (then merges into the word before it, whose times stay)
    seg = dict(seek=0, start=0.0, end=3.0, tokens=[ts(0), 1, 2, 3, 4, ts(3)], text="")
    WT.add_word_timestamps([seg], tk, RULES, lambda toks: [0, 10, 110, 120, 130])
    assert [(w["word"], w["start"], w["end"]) for w in seg["words"]] == [(" Hi.", 0.0, 0.2), (" there", 2.2, 2.4), (" friend", 2.4, 2.6)]
    # two segments of one window share one alignment; a segment without text gets no words
    a = dict(seek=0, start=0.0, end=1.0, tokens=[ts(0), 1, ts(1)], text=" Hi")
    b = dict(seek=0, start=1.0, end=2.0, tokens=[ts(1), ts(2)], text="")
    c = dict(seek=0, start=2.0, end=3.0, tokens=[ts(2), 3, 4, ts(3)], text=" there friend")
    WT.add_word_timestamps([a, b, c], tk, RULES, lambda toks: [0, 10, 100, 120])
    assert [w["word"] for w in a["words"]] == [" Hi"] and b["words"] == [] and [w["word"] for w in c["words"]] == [" there", " friend"]


def test_get_end_hand_derived():
    assert WT.get_end([]) is None and AR.get_end_ref([]) is None
    segs = [dict(end=5.0, words=[dict(end=4.2)]), dict(end=9.0, words=[])]
    assert WT.get_end(segs) == 4.2 == AR.get_end_ref(segs)
    segs = [dict(end=5.0, words=[]), dict(end=9.0, words=[])]
    assert WT.get_end(segs) == 9.0 == AR.get_end_ref(segs)


def _run_product_with_word_ends(content, script, tk, last_word_end_fn, prompt=None):
    loop = WindowLoop(RULES, tk, content, prompt, 448)
    while loop.active():
        r = script(loop.seek)
        rd = dict(tokens=list(r.tokens), avg_logprob=r.avg_logprob, no_speech_prob=r.no_speech_prob)
        built = loop.window_segments(rd)
        loop.advance(rd, 0.0, last_word_end=None if built is None else last_word_end_fn(built[0]))
        assert len(loop.seeks) < 100
    out = loop.result()
    out["seeks"] = loop.seeks
    return out


def test_window_loop_with_last_word_end_equals_the_transcribe_restatement():
    tk = IdTokenizer()
    c = CASES["consecutive_unfinished_tail"]
    script = table({0: c["script"](0), 200: c["script"](200), 236: R([ts(0), B_, C_, ts(2.5)])})
    # the aligned last word of the unfinished tail ends at 2.36 s: the next window starts at frame 236, not at the timestamp's 200
    got = _run_product_with_word_ends(c["content"], script, tk, lambda segs: 2.36)
    ref = run_oracle(c["content"], script, tk, word_timestamps=True, last_word_end_fn=lambda segs: 2.36)
    assert got["seeks"] == ref["seeks"] == [0, 236]
    assert got["text"] == ref["text"] and got["tokens"] == ref["tokens"]
    # without the argument: the timestamp-token rule, as before
    assert run_product(c["content"], script, tk)["seeks"] == [0, 200]
    # a last word that ends before the window's start does not move seek
    c2 = CASES["ends_on_a_pair"]
    got = _run_product_with_word_ends(c2["content"], c2["script"], tk, lambda segs: 0.0)
    ref = run_oracle(c2["content"], c2["script"], tk, word_timestamps=True, last_word_end_fn=lambda segs: 0.0)
    assert got["seeks"] == ref["seeks"] == [0, 300]
    # inert where the window ends on a single timestamp
    for name in ("single_timestamp_ending", "consecutive_then_single_ending", "long_initial_prompt_truncated"):
        c = CASES[name]
        fn = lambda segs: segs[-1]["end"] - 0.3
        got = _run_product_with_word_ends(c["content"], c["script"], tk, fn, c.get("prompt"))
        ref = run_oracle(c["content"], c["script"], tk, c.get("prompt"), word_timestamps=True, last_word_end_fn=fn)
        assert got["seeks"] == ref["seeks"] and got["text"] == ref["text"], name
        assert got["seeks"] == run_product(c["content"], c["script"], tk, c.get("prompt"))["seeks"], name
