"""CPU: the host side of the multilingual Whisper checkpoints -- id tables, language list, suppress list, the SOT sequence in the
window loop, the per-sequence sample cap and the grouping of a pass by cap, and that an English-only model ignores language / task.
The device side is tests/test_token_probs_gpu.py and tests/test_multilingual_gpu.py."""
import numpy as np
import pytest
import torch

from clearconverse_amd import tokenizer as T
from clearconverse_amd.tokenizer import DecodeRules, IdTokenizer
from clearconverse_amd.weights import WhisperDims
from clearconverse_amd.whisper import WhisperModel, WindowLoop, decode_cap, groups_by_cap
from clearconverse_amd.word_timing import alignment_tokens
from tests import lang_reference as LR


@pytest.mark.parametrize("n_lang, n_vocab", [(99, 51865), (100, 51866)])
def test_multilingual_id_table(n_lang, n_vocab):
    r = DecodeRules.multilingual(n_lang)
    assert (r.eot, r.sot, r.language_begin) == (50257, 50258, 50259)
    assert r.translate == 50259 + n_lang
    assert [r.transcribe, r.sot_lm, r.sot_prev, r.no_speech, r.no_timestamps, r.timestamp_begin] == [r.translate + i for i in range(1, 7)]
    assert r.timestamp_begin == 50265 + n_lang and r.timestamp_begin + 1501 == n_vocab
    if n_lang == 99:
        assert r.timestamp_begin == 50364
    assert r.is_multilingual and r.num_languages == n_lang and len(r.languages) == n_lang
    # every English-only id is one lower
    e = DecodeRules()
    assert (e.eot, e.sot, e.translate, e.transcribe, e.sot_lm, e.sot_prev, e.no_speech, e.no_timestamps, e.timestamp_begin) == \
        (50256, 50257, 50357, 50358, 50359, 50360, 50361, 50362, 50363)
    if n_lang == 99:
        m = (r.eot, r.sot, r.translate, r.transcribe, r.sot_lm, r.sot_prev, r.no_speech, r.no_timestamps, r.timestamp_begin)
        assert m == tuple(x + 1 for x in (50256, 50257, 50357, 50358, 50359, 50360, 50361, 50362, 50363))
    assert not e.is_multilingual and e.sot_sequence("de", "translate") == [e.sot]
    assert r.sot_sequence("de", "translate") == [r.sot, r.language_begin + 2, r.translate]
    assert r.sot_sequence("German") == [r.sot, r.language_begin + 2, r.transcribe]
    assert r.sot_sequence() == [r.sot, r.language_begin, r.transcribe]
    assert r.language_code(r.language_begin + 2) == "de"
    with pytest.raises(ValueError):
        r.sot_sequence("xx")
    with pytest.raises(ValueError):
        r.sot_sequence("de", "summarise")


def test_for_dims_follows_the_vocabulary():
    e = DecodeRules.for_dims(WhisperDims.mini())
    assert not e.is_multilingual and e.eot == 50256 and list(e.suppress) == list(DecodeRules().suppress)
    for n_vocab, n_lang in ((51865, 99), (51866, 100)):
        d = WhisperDims.mini(n_vocab=n_vocab)
        assert d.is_multilingual and d.num_languages == n_lang
        r = DecodeRules.for_dims(d)
        assert r.num_languages == n_lang and r.timestamp_begin + 1501 == n_vocab
    assert not WhisperDims.small_en().is_multilingual and WhisperDims.small_en().num_languages == 99
    assert WhisperDims.mini(2, 128) == WhisperDims.mini(n_layer=2, n_state=128, n_vocab=51864)       # backward compatible
    for preset, (state, head, layer) in dict(tiny=(384, 6, 4), base=(512, 8, 6), small=(768, 12, 12), medium=(1024, 16, 24)).items():
        d = getattr(WhisperDims, preset)()
        assert (d.n_vocab, d.n_audio_state, d.n_text_head, d.n_text_layer, d.n_audio_layer) == (51865, state, head, layer, layer)
        assert d.n_audio_state // d.n_audio_head == 64 and d.n_audio_state <= 1024 and d.n_mels == 80


def test_languages_and_suppress_list_against_transformers():
    try:
        from transformers.models.whisper import tokenization_whisper as TW
        from transformers.models.whisper.configuration_whisper import NON_SPEECH_TOKENS, NON_SPEECH_TOKENS_MULTI
    except ImportError:
        pytest.skip("transformers is not importable")
    assert list(T.LANGUAGES.items()) == list(TW.LANGUAGES.items())            # codes, names AND order (the order is the token order)
    assert T.TO_LANGUAGE_CODE == TW.TO_LANGUAGE_CODE
    r = DecodeRules.multilingual()
    assert T.NON_SPEECH_TEXT_TOKENS_MULTI == [t for t in NON_SPEECH_TOKENS_MULTI if t < r.eot]
    assert T.NON_SPEECH_TEXT_TOKENS == [t for t in NON_SPEECH_TOKENS if t < DecodeRules().eot]
    specials = [r.transcribe, r.translate, r.sot, r.sot_prev, r.sot_lm, r.no_speech]
    assert list(r.suppress) == sorted(T.NON_SPEECH_TEXT_TOKENS_MULTI + specials)
    # the same six specials as the English-only list, by their multilingual ids
    e = DecodeRules()
    assert sorted(set(e.suppress) - set(T.NON_SPEECH_TEXT_TOKENS)) == sorted(s - 1 for s in specials)
    # transformers lists the specials it suppresses itself: each of them is one of ours
    assert set(t for t in NON_SPEECH_TOKENS_MULTI if t >= r.eot) <= set(specials)


def test_tokenizers_filter_text_with_the_eot_they_are_given():
    assert IdTokenizer().decode([5, 50256, 50257, 7]) == " <5> <7>"
    assert IdTokenizer(50257).decode([5, 50256, 50257, 7]) == " <5> <50256> <7>"
    assert T.get_tokenizer("/nonexistent", rules=DecodeRules.multilingual()).eot == 50257
    assert T.get_tokenizer("/nonexistent").eot == 50256


@pytest.mark.parametrize("n_prompt", [0, 5, 400])
def test_window_loop_with_a_three_token_sot_sequence(n_prompt):
    r = DecodeRules.multilingual()
    tok = IdTokenizer(r.eot)
    seq = r.sot_sequence("fr", "translate")
    ids = list(range(1000, 1000 + n_prompt))
    prompt = "".join(f" <{i}>" for i in ids) or None
    loop = WindowLoop(r, tok, 1000, prompt, 448, sot_sequence=seq, language="fr")
    it = loop.initial_tokens()
    if n_prompt == 0:
        assert it == seq and loop.sample_cap() == 224
    else:
        assert it == [r.sot_prev] + ids[-223:] + seq
        assert len(it) == 1 + min(n_prompt, 223) + 3
        assert loop.sample_cap() == (224 if n_prompt == 5 else 222)
    assert len(it) + loop.sample_cap() - 1 <= 448
    assert loop.result()["language"] == "fr"
    # the default stays the English-only loop
    e = DecodeRules()
    assert WindowLoop(e, IdTokenizer(), 1000, None, 448).initial_tokens() == [e.sot]
    assert WindowLoop(e, IdTokenizer(), 1000, None, 448).result()["language"] == "en"
    assert alignment_tokens([7, 8], r, seq) == [*seq, r.no_timestamps, 7, 8, r.eot]
    assert alignment_tokens([7, 8], e) == [e.sot, e.no_timestamps, 7, 8, e.eot]


def test_cap_rule():
    # upstream's loop stops once tokens.shape[-1] > n_ctx: from P initial tokens at most n_ctx + 1 - P are sampled, and never more than n_ctx // 2
    assert [decode_cap(p, 448) for p in (1, 3, 225, 226, 227)] == [224, 224, 224, 223, 222]
    for p in range(1, 228):
        assert p + decode_cap(p, 448) - 1 <= 448
    assert groups_by_cap([0, 1, 2, 3, 4], [224, 222, 224, 223, 224], 2) == [(224, [0, 2]), (224, [4]), (223, [3]), (222, [1])]
    assert groups_by_cap([3, 5], [224, 224], 8) == [(224, [3, 5])]


class _Stub(WhisperModel):
    """WhisperModel.transcribe_batch with the device calls scripted: which groups are decoded, with which prompts and sample_len."""

    def __init__(self, rules, max_batch=8, detected="ja"):
        self.rules, self.tokenizer, self.dims = rules, IdTokenizer(rules.eot), WhisperDims.mini(n_vocab=51865 if rules.is_multilingual else 51864)
        self.max_batch, self.device, self.max_audio_seconds = max_batch, torch.device("cpu"), 30.0
        self.word_alignment, self.sample_seed, self._sample_calls, self.handle = False, 0, 0, None
        self.detected, self.calls, self.detect_calls = detected, [], []

    def log_mel(self, audio, n_samples, seek=None, return_mel=False):
        return None

    def encode(self, B, return_xa=False):
        return None

    def detect_language(self, B):
        self.detect_calls.append(B)
        return [self.detected] * B, np.zeros((B, self.rules.num_languages), dtype=np.float32)

    def decode(self, prompts, sample_len=None, temperature=0.0, seed=0):
        self.calls.append(dict(sample_len=sample_len, prompts=[list(p) for p in prompts]))
        tsb = self.rules.timestamp_begin
        return [dict(tokens=[tsb, 1234, tsb + 100], sum_logprob=-1.0, avg_logprob=-0.25, no_speech_prob=0.01) for _ in prompts]


def _prompt(n):
    return "".join(f" <{1000 + i}>" for i in range(n)) or None


def test_transcribe_groups_by_cap_and_detects_the_language():
    r = DecodeRules.multilingual()
    m = _Stub(r, max_batch=2)
    clips = [np.zeros(16000 * 3, dtype=np.float32)] * 5
    # initial tokens: 3, 226, 227, 3, 227 -> caps 224, 223, 222, 224, 222
    out = m.transcribe_batch(clips, [None, _prompt(222), _prompt(300), None, _prompt(223)], languages=[None, "de", None, "de", None])
    assert [(c["sample_len"], [len(p) for p in c["prompts"]]) for c in m.calls] == [(224, [3, 3]), (223, [226]), (222, [227, 227])]
    for c in m.calls:
        for p in c["prompts"]:
            assert len(p) + c["sample_len"] - 1 <= 448 and c["sample_len"] == decode_cap(len(p), 448)
    # detection once per group that holds a clip without a language, before its decode; a given language is kept
    assert m.detect_calls == [2, 2]
    assert [o["language"] for o in out] == ["ja", "de", "ja", "de", "ja"]
    ja, de = r.language_token("ja"), r.language_token("de")
    assert m.calls[0]["prompts"][0][-3:] == [r.sot, ja, r.transcribe] and m.calls[0]["prompts"][1][-3:] == [r.sot, de, r.transcribe]
    assert m.calls[1]["prompts"][0][-3:] == [r.sot, de, r.transcribe] and m.calls[1]["prompts"][0][0] == r.sot_prev
    m2 = _Stub(r)
    res = m2.transcribe(clips[0], language="de", task="translate")
    assert m2.detect_calls == [] and res["language"] == "de" and m2.calls[0]["prompts"] == [[r.sot, de, r.translate]]


def test_english_only_ignores_language_and_task():
    e = DecodeRules()
    clip = np.zeros(16000 * 3, dtype=np.float32)
    a, b = _Stub(e), _Stub(e)
    ra = a.transcribe(clip, initial_prompt=_prompt(300))
    rb = b.transcribe(clip, initial_prompt=_prompt(300), language="de", task="translate")
    assert a.calls == b.calls and ra == rb and rb["language"] == "en"
    assert a.detect_calls == b.detect_calls == []
    assert a.calls[0]["sample_len"] == 224 and a.calls[0]["prompts"][0][-1] == e.sot and len(a.calls[0]["prompts"][0]) == 225


def test_reference_self_check():
    LR.self_check()
    r = DecodeRules.multilingual()
    o = LR.oracle_rules(r)
    assert (o.eot, o.sot, o.no_speech, o.timestamp_begin) == (50257, 50258, r.no_speech, 50364) and tuple(o.suppress) == tuple(r.suppress)


def test_batch_pipeline_refuses_a_multilingual_model():
    """the pinned batch driver builds English-only prompts with one sample_len and never detects a language"""
    from types import SimpleNamespace
    from clearconverse_amd import _lib
    from clearconverse_amd.batch import BatchPipeline
    multi, english = SimpleNamespace(rules=DecodeRules.multilingual()), SimpleNamespace(rules=DecodeRules())
    BatchPipeline({"ctx": None, "whisper_model": english, "whisper_models": [english]})
    BatchPipeline({"ctx": None, "whisper_model": english})
    for models in ({"ctx": None, "whisper_model": multi}, {"ctx": None, "whisper_model": english, "whisper_models": [english, multi]}):
        with pytest.raises(_lib.CcxError, match="English-only"):
            BatchPipeline(models)
