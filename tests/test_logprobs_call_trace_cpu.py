"""The library-call sequence of `decode`, `decode_rows` and `transcribe_batch` with `logprobs`, pinned without a GPU over the fake
library of tests/test_decode_call_trace_cpu.py: None is the default trace, with and without the opt-in; an int sets
ccx_whisper_set_logprob_options last and takes it back first, with the fetch right behind every decode; every refusal reaches the
library not at all."""
import numpy as np
import pytest

from clearconverse_amd import _lib
from tests import test_decode_call_trace_cpu as T

LOGP, FETCH = "ccx_whisper_set_logprob_options", "ccx_whisper_token_logprobs"
KINDS = ("decode", "decode_rows")
ON = dict(T.ALL_ON, truncated_sampling=True, token_logprobs=True)
SAMPLING = "ccx_whisper_set_sampling_options"


@pytest.fixture(autouse=True)
def _no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: 0)


def _top_n(entry):
    """the payload of a ccx_whisper_set_logprob_options record: NULL -> None, else the struct's top_n"""
    ref = entry[1][0]
    return None if ref is None else ref._obj.top_n


def _fetch(entry):
    """(R, sample_len, top_n, whether the two top arrays are given) of a ccx_whisper_token_logprobs record"""
    R, sample_len, lp, n, tid, tlp, _ = entry[1]
    assert lp is not None
    return (R, sample_len, n, tid is not None and tlp is not None)


@pytest.mark.parametrize("opt_in", [False, True])
@pytest.mark.parametrize("kind", KINDS + ("decode_beam",))
def test_none_is_the_default_trace(kind, opt_in):
    m = T._Traced(token_logprobs=opt_in)
    out = T._call(m, kind) if kind == "decode_beam" else T._call(m, kind, logprobs=None)
    assert m.lib.trace == T._default_trace(kind)
    if kind != "decode_beam":
        assert out == [dict(tokens=[], sum_logprob=0.0, avg_logprob=0.0, no_speech_prob=0.0, cross_path="kv16")] * 2


@pytest.mark.parametrize("kind", KINDS)
def test_an_int_sets_last_fetches_behind_the_decode_and_resets_first(kind):
    m = T._Traced(**ON)
    out = T._call(m, kind, logprobs=3, temperature=0.5, top_k=4, repetition_penalty=1.3, bad_words_ids=[[7]], without_timestamps=True)
    names = [e[0] for e in m.lib.trace]
    at = names.index(T.DECODES[KINDS.index(kind)])
    # applied after `sampling`, the last of the setters; the decode, its path query, the fetch; taken back first
    assert names[at - 2:at + 4] == [SAMPLING, LOGP, names[at], T.PATH, FETCH, LOGP]
    assert set(names[:at - 2]) == {T.OPTIONS, T.HISTORY, T.BIAS} and names[at + 4] == SAMPLING
    assert _top_n(m.lib.trace[at - 1]) == 3 and _top_n(m.lib.trace[at + 3]) is None
    assert _fetch(m.lib.trace[at + 2]) == (2, 4, 3, True)
    assert names.count(LOGP) == 2 and names.count(FETCH) == 1
    # a library that writes nothing: no tokens, so one entry (the eot's step), which the fetch's fill leaves NaN / empty
    for r in out:
        assert len(r["token_logprobs"]) == 1 and np.isnan(r["token_logprobs"][0]) and r["top_logprobs"] == [[]]


@pytest.mark.parametrize("kind", KINDS)
def test_zero_fetches_the_chosen_tokens_only(kind):
    m = T._Traced(token_logprobs=True)
    out = T._call(m, kind, logprobs=0)
    names = [e[0] for e in m.lib.trace]
    assert names == [LOGP, T.DECODES[KINDS.index(kind)], T.PATH, FETCH, LOGP]
    assert _top_n(m.lib.trace[0]) == 0 and _fetch(m.lib.trace[3]) == (2, 4, 0, False)
    assert all("token_logprobs" in r and "top_logprobs" not in r for r in out)


@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_decode_takes_the_setting_back_and_fetches_nothing(kind):
    m = T._Traced(token_logprobs=True)
    m.lib.fail_at = {T.DECODES[KINDS.index(kind)]: 0}
    with pytest.raises(_lib.CcxError):
        T._call(m, kind, logprobs=2)
    assert [e[0] for e in m.lib.trace] == [LOGP, T.DECODES[KINDS.index(kind)], LOGP] and _top_n(m.lib.trace[-1]) is None


REFUSALS = [("no opt-in", dict(), 3, "token_logprobs=True"), ("-1", ON, -1, "logprobs"), ("9", ON, 9, "logprobs"),
            ("True", ON, True, "logprobs"), ("2.5", ON, 2.5, "logprobs")]


@pytest.mark.parametrize("name,opt_ins,value,word", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("kind", KINDS + ("transcribe",))
def test_every_refusal_reaches_the_library_not_at_all(kind, name, opt_ins, value, word):
    m = T._Traced(**opt_ins)
    with pytest.raises(ValueError, match=word):
        if kind == "transcribe":
            m.transcribe_batch([T.CLIP], logprobs=value)
        else:
            T._call(m, kind, logprobs=value, bad_words_ids=[[7]])
    assert m.lib.trace == [] and m.ctx.checked == []


def test_beam_size_with_logprobs_is_refused():
    m = T._Traced(**dict(ON, beam_search=True, temperature_fallback=True))
    with pytest.raises(ValueError, match="beam"):
        m.transcribe_batch([T.CLIP], beam_size=2, logprobs=2)
    with pytest.raises(ValueError, match="beam"):
        m.transcribe([T.CLIP][0], beam_size=2, logprobs=0)
    with pytest.raises(ValueError, match="beam"):
        m.decode(T.PROMPTS, sample_len=4, beam_size=2, logprobs=2)
    assert m.lib.trace == [] and m.ctx.checked == []
    # without beam_search the argument is accepted and ignored, as always: the call records
    m = T._Traced(token_logprobs=True)
    m.transcribe_batch([T.CLIP], beam_size=2, logprobs=2)
    assert [e[0] for e in m.lib.trace] == [LOGP, "ccx_whisper_decode", T.PATH, FETCH, LOGP]


def test_transcribe_sets_once_fetches_behind_every_decode_and_restores():
    m = T._Traced(**dict(T.FIVE_ON, token_logprobs=True))
    m.lib.sum_logprob = {"ccx_whisper_decode": -10.0}      # round 0 is too improbable: the window decodes again, warmer, best_of rows
    out = m.transcribe_batch([T.CLIP], temperature=(0.0, 0.4), best_of=2, logprobs=2, **T.CALL)
    names = [e[0] for e in m.lib.trace]
    at = names.index("ccx_whisper_decode")
    assert names[at - 1] == LOGP and _top_n(m.lib.trace[at - 1]) == 2 and set(names[:at - 1]) == set(T.CALL_SETS)
    assert names[at:at + 7] == ["ccx_whisper_decode", T.PATH, FETCH, "ccx_whisper_decode_rows", T.PATH, FETCH, LOGP]
    assert _fetch(m.lib.trace[at + 2]) == (1, 224, 2, True) and _fetch(m.lib.trace[at + 5]) == (2, 224, 2, True)
    assert _top_n(m.lib.trace[at + 6]) is None and names.count(LOGP) == 2
    held = T._left_behind(m.lib.trace)
    assert held == T.CLEAN
    seg = out[0]["segments"][0]
    assert seg["tokens"] == [] and seg["token_logprobs"] == [] and seg["top_logprobs"] == []
    # the walk's accepted candidate carries the lists
    acc = m.fallback_walks[0].accepted[0]
    assert len(acc["token_logprobs"]) == 1 and acc["top_logprobs"] == [[]]


def test_transcribe_without_logprobs_is_todays_call():
    m = T._Traced(token_logprobs=True)
    out = m.transcribe_batch([T.CLIP])
    assert m.lib.trace == [T._plain(1, [[T.SOT]]), (T.PATH, (), 0)]
    assert set(out[0]) == {"text", "segments", "language", "tokens"}
    assert set(out[0]["segments"][0]) == {"seek", "start", "end", "tokens", "text"}
