"""GPU: sequence_bias, bad_words_ids and hotwords in WhisperModel.transcribe / transcribe_batch (opt-in:
WhisperModel(contextual_bias=True)) on two short synthetic clips at the mini dims.

  * bad_words_ids built from what the default transcripts hold: no window holds a banned sequence, and the call is not the default call
  * sequence_bias (dict and list form) with the same bans is the same call; a finite bias changes the call too
  * hotwords: the boosted id shows up in every window; hotwords without hotword_boost raise
  * without the flag: all four arguments are accepted and change nothing, bit for bit
  * a fallback schedule plus bad_words_ids on an instance that also has temperature_fallback=True: every round of every window, the
    best_of rows above temperature 0 included, keeps clear of the banned sequences
A window matches over its own decode only: the invariant is stated per window (the segments of one `seek`), never across windows.
"""
import pytest

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from tests import bias_reference as BR

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
EOT = RULES.eot
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
    m, d = _build(ccx_ctx, contextual_bias=True, temperature_fallback=True), _build(ccx_ctx)
    yield m, d
    m.close()
    d.close()


def _windows(out):
    """the token runs of one result that came out of ONE window's decode: each segment, and a window's segments joined where none of
    them was cleared (a cleared segment's tokens are gone: joining across it would invent sequences)"""
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


def _text_bigrams(outs, k=3):
    """the first k distinct text bigrams of every transcript: sequences a segment's own decode emitted"""
    words = []
    for o in outs:
        n = 0
        for s in o["segments"]:
            text = [t for t in s["tokens"] if t < EOT]
            for x, y in zip(text, text[1:]):
                if [x, y] not in words and n < k:
                    words.append([x, y])
                    n += 1
    return words


def test_each_argument_reaches_every_window(models):
    m, d = models
    clips = _clips()
    plain = m.transcribe_batch(clips, **KW)
    words = _text_bigrams(plain)
    assert len(words) >= 2 and any(BR.banned_occurrences(run, words) for o in plain for run in _windows(o))
    out = m.transcribe_batch(clips, bad_words_ids=words, **KW)
    n_runs = 0
    for o in out:
        for run in _windows(o):
            assert not BR.banned_occurrences(run, words), run
            n_runs += 1
    assert n_runs >= 2
    assert [o["tokens"] for o in out] != [o["tokens"] for o in plain]
    # the same bans as sequence_bias, in both forms
    assert _same(m.transcribe_batch(clips, sequence_bias={tuple(w): float("-inf") for w in words}, **KW), out)
    assert _same(m.transcribe_batch(clips, sequence_bias=[[w, float("-inf")] for w in words], **KW), out)
    one = m.transcribe(clips[1], bad_words_ids=words, **KW)
    for run in _windows(one):
        assert not BR.banned_occurrences(run, words), run
    # a finite bias: the call changes, and differently
    fin = m.transcribe_batch(clips, sequence_bias={tuple(w): -6.0 for w in words}, **KW)
    assert not _same(fin, plain)
    # hotwords: an id no default window holds is in every window once it is boosted by 40
    used = {t for o in plain for t in o["tokens"]}
    word = next(t for t in range(3000, 3100) if t not in used and t not in RULES.suppress)
    hot = m.transcribe_batch(clips, hotwords=m.tokenizer.decode([word]), hotword_boost=40.0, **KW)
    for o in hot:
        assert word in o["tokens"], o["tokens"]
    assert _same(m.transcribe_batch(clips, hotwords=[m.tokenizer.decode([word])], hotword_boost=40.0, **KW), hot)
    # nothing outlives a call; what the compile refuses raises before anything is set
    assert _same(m.transcribe_batch(clips, **KW), plain)
    with pytest.raises(ValueError, match="hotword_boost"):
        m.transcribe_batch(clips, hotwords="<3000>", **KW)
    with pytest.raises(ValueError, match="hotword_boost"):
        m.transcribe(clips[0], hotwords=["<3000>"], **KW)
    with pytest.raises(ValueError, match="eot"):
        m.transcribe_batch(clips, bad_words_ids=[[EOT]], **KW)
    assert _same(m.transcribe_batch(clips, **KW), plain)
    assert m.bias_graph_count() >= 1 and m.graph_count() > m.bias_graph_count()


def test_missing_flag_changes_nothing(models):
    m, d = models
    clips = _clips()
    base = d.transcribe_batch(clips, **KW)
    assert _same(m.transcribe_batch(clips, **KW), base)
    assert _same(m.transcribe_batch(clips, sequence_bias={}, bad_words_ids=[], **KW), base)
    words = _text_bigrams(base)
    # without the flag: accepted and ignored, whatever they hold -- a missing hotword_boost included
    got = d.transcribe_batch(clips, sequence_bias={(5,): 9.0}, bad_words_ids=words, hotwords="<3000>", hotword_boost=40.0, **KW)
    assert _same(got, base)
    assert _same(d.transcribe_batch(clips, hotwords="<3000>", **KW), base)
    assert d.transcribe(clips[0], bad_words_ids=words, **KW)["tokens"] == base[0]["tokens"]
    assert d.bias_graph_count() == 0
    prompts = [[d.rules.sot]] * 2
    a = d.decode(prompts, sample_len=12)
    b = d.decode(prompts, sample_len=12, sequence_bias={(5,): 9.0}, bad_words_ids=[[a[0]["tokens"][0], a[0]["tokens"][1]]])
    assert [(r["tokens"], r["sum_logprob"]) for r in a] == [(r["tokens"], r["sum_logprob"]) for r in b] and d.bias_graph_count() == 0


def test_fallback_rounds_get_the_calls_table(models):
    m, d = models
    clips = _clips()
    kw = dict(temperature=(0.0, 0.4), best_of=2, logprob_threshold=100.0, compression_ratio_threshold=None, no_speech_threshold=None)
    # no window passes a log-probability threshold of +100: every window walks the whole schedule and keeps its last round
    m.transcribe_batch(clips, **kw)
    rounds = [rnd for walk in m.fallback_walks for w in walk.trace for rnd in walk.trace[w]]
    words = []
    for rnd in rounds:                                       # ban a text bigram of every round, the sampled ones included
        pair = next(([x, y] for x, y in zip(rnd["tokens"], rnd["tokens"][1:]) if y < EOT), None)
        if pair is not None and pair not in words:
            words.append(pair)
    assert len(words) >= 2
    out = m.transcribe_batch(clips, bad_words_ids=words, **kw)
    walks = list(m.fallback_walks)
    assert walks
    kept = 0
    for walk in walks:
        for w, r in walk.accepted.items():
            assert r["temperature"] == 0.4 and len(walk.trace[w]) == 2
            for rnd in walk.trace[w]:                       # the temperature-0 round and the best_of round alike
                assert not BR.banned_occurrences(rnd["tokens"], words), (w, rnd["temperature"], rnd["tokens"])
            kept += 1
    assert kept >= 2
    for o in out:
        for run in _windows(o):
            assert not BR.banned_occurrences(run, words), run
