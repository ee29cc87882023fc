"""GPU: top_k / top_p / min_p in WhisperModel.transcribe / transcribe_batch (opt-in: WhisperModel(truncated_sampling=True)) on two
short synthetic clips at the mini dims, with a fallback schedule and best_of on an instance that also has temperature_fallback=True.

  * the rounds above temperature 0 -- best_of rows over the window map -- honour the values: every token of every window that failed
    its temperature-0 round and was decoded again lies in the reference kept set (tests/truncation_reference.py) computed from the
    instance's own teacher-forced logits of that window (enlarged by the deltas of tests/test_decode_truncate_gpu.py)
  * the temperature-0 round, and a temperature-0 call, are identical with and without the values
  * the values do not outlive the call; every refusal
"""
import numpy as np
import pytest

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import decoding_options_reference as DO
from tests import truncation_reference as TR
from tests.test_decode_truncate_gpu import _enlarged

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
ORULES = R.Rules(suppress=tuple(RULES.suppress))
EOT, SOT = RULES.eot, RULES.sot
CLIP_S = [4.0, 7.5]
# no window passes a log-probability threshold of +100: every window walks the whole schedule and keeps its last round
WALK = dict(temperature=(0.0, 0.4), best_of=2, logprob_threshold=100.0, compression_ratio_threshold=None, no_speech_threshold=None)
TRUNC = dict(top_k=5, top_p=0.9, min_p=0.02)
PRM = TR.Params(0.4, 5, 0.9, 0.02)


def _clips():
    return [synthetic_clip(50 + i, 30.0)[: int(CLIP_S[i] * 16000)] for i in range(2)]


def _build(ccx_ctx, **kw):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=8, ctx=ccx_ctx, **kw)


@pytest.fixture(scope="module")
def models(ccx_ctx):
    m, d = _build(ccx_ctx, truncated_sampling=True, temperature_fallback=True), _build(ccx_ctx, temperature_fallback=True)
    yield m, d
    m.close()
    d.close()


def _call(model, clips, **kw):
    """transcribe_batch from the same Philox seed and call counter, so that two calls (and two instances) draw the same noise"""
    model.sample_seed, model._sample_calls = 7, 0
    return model.transcribe_batch(clips, **kw)


def _same(a, b):
    return [(o["text"], o["tokens"], o["segments"], o["language"]) for o in a] == [(o["text"], o["tokens"], o["segments"], o["language"]) for o in b]


def _rounds(m):
    return [(w, [(r["temperature"], list(r["tokens"]), r["sum_logprob"]) for r in walk.trace[w]]) for walk in m.fallback_walks for w in sorted(walk.trace)]


def _outside(m, window, tokens, prm):
    """the steps of one window's decode whose token is outside the (enlarged) reference kept set of the instance's own logits"""
    toks = list(tokens) + ([EOT] if len(tokens) < 224 else [])
    seq = np.array([[SOT] + toks[:-1]] * (window + 1), dtype=np.int32)
    lg = m.decoder_logits(seq)[window].cpu()
    bad = []
    for i, tok in enumerate(toks):
        x = DO.apply_filters(lg[i], toks[:i], ORULES).numpy()
        if not _enlarged(x, prm)[tok]:
            bad.append(i)
    return bad, len(toks)


def test_warm_rounds_honour_the_values_and_the_cold_round_does_not_see_them(models):
    m, d = models
    clips = _clips()
    out = _call(m, clips, **WALK, **TRUNC)
    rounds = _rounds(m)                                   # both clips are one window each: one group, still encoded
    assert len(rounds) == 2
    checked = 0
    for w, rnds in rounds:
        assert [t for t, _, _ in rnds] == [0.0, 0.4]      # failed at 0, retried warmer
        bad, n = _outside(m, w, rnds[1][1], PRM)
        assert not bad, (w, bad)
        checked += n
    assert checked >= 8
    # the same call without the values: the temperature-0 round is the same round, bit for bit; the warm round draws from the whole
    # vocabulary and leaves the kept set somewhere
    plain = _call(m, clips, **WALK)
    plain_rounds = _rounds(m)
    assert [r[1][0] for r in plain_rounds] == [r[1][0] for r in rounds]
    assert any(_outside(m, w, rnds[1][1], PRM)[0] for w, rnds in plain_rounds)
    assert [o["tokens"] for o in out] != [o["tokens"] for o in plain]
    # an instance without the opt-in, default values: the plain call
    assert _same(_call(d, clips, **WALK), plain)
    assert _same(_call(m, clips, **WALK, top_k=0, top_p=1.0, min_p=0.0), plain)


def test_a_temperature_0_call_is_identical_and_nothing_outlives_a_call(models):
    m, d = models
    clips = _clips()
    kw = dict(temperature=0.0, no_speech_threshold=None, logprob_threshold=None)
    base = d.transcribe_batch(clips, **kw)
    assert _same(m.transcribe_batch(clips, **kw, **TRUNC), base)
    assert m.sampling_graph_count() == 0 or m.graph_count() > m.sampling_graph_count()
    one = m.transcribe(clips[1], temperature=0.4, top_k=1, no_speech_threshold=None, logprob_threshold=None)
    assert one["tokens"] == base[1]["tokens"]            # top_k = 1: the greedy transcript at any temperature
    assert _same(m.transcribe_batch(clips, **kw), base)
    # a single positive temperature without a schedule is honoured too: another transcript than the plain sampler's, reproducibly
    warm = dict(temperature=0.4, no_speech_threshold=None, logprob_threshold=None)
    a, b, c = _call(m, clips, **warm, **TRUNC), _call(m, clips, **warm, **TRUNC), _call(m, clips, **warm)
    assert _same(a, b) and not _same(a, c)


def test_refusals(models):
    m, d = models
    clips = _clips()
    for kw in (dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.1), dict(top_p=float("nan")), dict(min_p=-0.1),
               dict(min_p=2.0), dict(min_p=float("nan"))):
        for model in (m, d):
            with pytest.raises(ValueError, match=list(kw)[0]):
                model.transcribe_batch(clips, **kw)
            with pytest.raises(ValueError, match=list(kw)[0]):
                model.transcribe(clips[0], **kw)
    for kw in (dict(top_k=5), dict(top_p=0.9), dict(min_p=0.1)):      # without the opt-in a value off its default is refused
        with pytest.raises(ValueError, match="truncated_sampling=True"):
            d.transcribe_batch(clips, **kw)
        with pytest.raises(ValueError, match="truncated_sampling=True"):
            d.transcribe(clips[0], **kw)
        with pytest.raises(ValueError, match="truncated_sampling=True"):
            d.decode([[SOT]], sample_len=4, **kw)
        with pytest.raises(ValueError, match="truncated_sampling=True"):
            d.decode_rows([[SOT]], [0], sample_len=4, **kw)
    assert d.sampling_graph_count() == 0
