"""GPU: repetition_penalty and no_repeat_ngram_size in WhisperModel.transcribe / transcribe_batch (opt-in:
WhisperModel(repetition_control=True)) on two short synthetic clips at the mini dims.

  * with the flag and n = 3: no window repeats a 3-gram that ends in a text id, and the call is not the default call
  * with the flag and the default values (1.0, 0): what an instance built without it returns
  * without the flag: the two arguments are accepted and change nothing
  * a fallback schedule plus n = 2 on an instance that also has temperature_fallback=True: the rounds above temperature 0 -- best_of
    rows over the window map -- keep the invariant too (the round that is kept is looked at)
A window's history is its own decode: the invariant is stated per window (the segments of one `seek`), never across windows.
"""
import pytest

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from tests import history_rules_reference as HR

pytestmark = pytest.mark.gpu

EOT = DecodeRules().eot
CLIP_S = [4.0, 7.5]
KW = dict(temperature=0.0, no_speech_threshold=None, logprob_threshold=None)


def _clips():
    return [synthetic_clip(50 + i, 30.0)[: int(CLIP_S[i] * 16000)] for i in range(2)]


def _build(ccx_ctx, **kw):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=8, ctx=ccx_ctx, **kw)


@pytest.fixture(scope="module")
def models(ccx_ctx):
    m, d = _build(ccx_ctx, repetition_control=True, temperature_fallback=True), _build(ccx_ctx)
    yield m, d
    m.close()
    d.close()


def _windows(out):
    """the token runs of one result that came out of ONE window's decode: each segment, and a window's segments joined where none of
    them was cleared (a cleared segment's tokens are gone: joining across it would invent n-grams)"""
    runs, by_seek = [], {}
    for s in out["segments"]:
        runs.append(list(s["tokens"]))
        by_seek.setdefault(s["seek"], []).append(s)
    for segs in by_seek.values():
        if all(s["tokens"] for s in segs):
            runs.append([t for s in segs for t in s["tokens"]])
    return runs


def _same(a, b):
    return [(o["text"], o["tokens"], o["segments"], o["language"]) for o in a] == [(o["text"], o["tokens"], o["segments"], o["language"]) for o in b]


def test_ngram_ban_holds_in_every_window_and_shows(models):
    m, d = models
    clips = _clips()
    plain = m.transcribe_batch(clips, **KW)
    out = m.transcribe_batch(clips, no_repeat_ngram_size=3, **KW)
    n_runs = 0
    for o in out:
        for run in _windows(o):
            assert not HR.ngram_invariant_violations(run, EOT, 3), run
            n_runs += 1
    assert n_runs >= 2
    # the default transcripts of this model loop: they break the invariant, and the call with the rule is another call
    assert any(HR.ngram_invariant_violations(run, EOT, 3) for o in plain for run in _windows(o))
    assert [o["text"] for o in out] != [o["text"] for o in plain] and [o["tokens"] for o in out] != [o["tokens"] for o in plain]
    one = m.transcribe(clips[1], no_repeat_ngram_size=3, repetition_penalty=1.3, **KW)
    for run in _windows(one):
        assert not HR.ngram_invariant_violations(run, EOT, 3), run
    # the setting does not outlive the call
    assert _same(m.transcribe_batch(clips, **KW), plain)
    with pytest.raises(ValueError):
        m.transcribe_batch(clips, repetition_penalty=0.0, **KW)
    with pytest.raises(ValueError):
        m.transcribe(clips[0], no_repeat_ngram_size=-2, **KW)
    assert _same(m.transcribe_batch(clips, **KW), plain)


def test_default_values_and_missing_flag_change_nothing(models):
    m, d = models
    clips = _clips()
    base = d.transcribe_batch(clips, **KW)
    assert _same(m.transcribe_batch(clips, repetition_penalty=1.0, no_repeat_ngram_size=0, **KW), base)
    assert _same(m.transcribe_batch(clips, **KW), base)
    assert m.history_graph_count() == 0 or m.graph_count() > m.history_graph_count()
    # without the flag: accepted and ignored, whatever they hold
    assert _same(d.transcribe_batch(clips, repetition_penalty=1.5, no_repeat_ngram_size=2, **KW), base)
    assert d.transcribe(clips[0], repetition_penalty=1.5, no_repeat_ngram_size=2, **KW)["tokens"] == base[0]["tokens"]
    assert d.history_graph_count() == 0
    prompts = [[d.rules.sot]] * 2
    a = d.decode(prompts, sample_len=12)
    b = d.decode(prompts, sample_len=12, repetition_penalty=2.0, no_repeat_ngram_size=1)
    assert [r["tokens"] for r in a] == [r["tokens"] for r in b] and d.history_graph_count() == 0


def test_fallback_rounds_get_the_calls_values(models):
    m, d = models
    clips = _clips()
    # no window passes a log-probability threshold of +100: every window walks the whole schedule and keeps its last round
    out = m.transcribe_batch(clips, temperature=(0.0, 0.4), best_of=2, logprob_threshold=100.0, compression_ratio_threshold=None,
                             no_speech_threshold=None, no_repeat_ngram_size=2)
    walks = list(m.fallback_walks)
    assert walks
    kept = 0
    for walk in walks:
        for w, r in walk.accepted.items():
            assert r["temperature"] == 0.4 and len(walk.trace[w]) == 2
            for rnd in walk.trace[w]:                       # the temperature-0 round and the best_of round alike
                assert not HR.ngram_invariant_violations(rnd["tokens"], EOT, 2), (w, rnd["temperature"], rnd["tokens"])
            kept += 1
    assert kept >= 2
    for o in out:
        for run in _windows(o):
            assert not HR.ngram_invariant_violations(run, EOT, 2), run
    # the same call without the rule breaks it somewhere: the values did reach the rounds
    m.transcribe_batch(clips, temperature=(0.0, 0.4), best_of=2, logprob_threshold=100.0, compression_ratio_threshold=None, no_speech_threshold=None)
    assert any(HR.ngram_invariant_violations(rnd["tokens"], EOT, 2) for walk in m.fallback_walks for w in walk.trace for rnd in walk.trace[w])
