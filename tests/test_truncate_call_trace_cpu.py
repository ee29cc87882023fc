"""The library-call sequence of a call with top_k / top_p / min_p, pinned without a GPU over the fake library of
tests/test_decode_call_trace_cpu.py: ccx_whisper_set_sampling_options is the LAST setting applied and the FIRST taken back (the fixed
order of `WhisperModel._settings`: options, SOT tail, prefix length, history, bias, sampling), a refused call reaches the library not at
all, and a setter that fails -- this one, or one behind which this one was already applied -- leaves nothing set."""
import numpy as np
import pytest

from clearconverse_amd import _lib
from tests import test_decode_call_trace_cpu as T

SAMPLING = "ccx_whisper_set_sampling_options"
ON = dict(T.ALL_ON, truncated_sampling=True)
F32 = T.F32
KINDS = ("decode", "decode_rows")
ARGS = dict(top_k=5, top_p=0.9, min_p=0.1)
WANT = (5, F32(0.9), F32(0.1))


@pytest.fixture(autouse=True)
def _no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: 0)


def _payload(entry):
    """(top_k, top_p, min_p) of a recorded ccx_whisper_set_sampling_options, None for its NULL"""
    ref = entry[1][0]
    return None if ref is None else (ref._obj.top_k, ref._obj.top_p, ref._obj.min_p)


def _names(trace):
    return [e[0] for e in trace]


@pytest.mark.parametrize("kind", KINDS)
def test_set_last_and_taken_back_first(kind):
    m = T._Traced(**ON)
    T._call(m, kind, temperature=0.5, seed=3, **ARGS, **T.FAMILIES["all"][0])
    names = _names(m.lib.trace)
    decode = T.DECODES[KINDS.index(kind)]
    assert names == [T.OPTIONS, T.HISTORY, T.BIAS, SAMPLING, decode, T.PATH, SAMPLING, T.BIAS, T.HISTORY, T.OPTIONS]
    assert _payload(m.lib.trace[3]) == WANT and _payload(m.lib.trace[6]) is None
    assert m.lib.trace[4][1]["temperature"] == 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_alone_and_with_values_that_set_nothing(kind):
    m = T._Traced(truncated_sampling=True)
    T._call(m, kind, top_k=40)
    assert _names(m.lib.trace) == [SAMPLING, T.DECODES[KINDS.index(kind)], T.PATH, SAMPLING]
    assert _payload(m.lib.trace[0]) == (40, 1.0, 0.0)
    for model in (T._Traced(truncated_sampling=True), T._Traced()):      # the defaults set nothing, with or without the opt-in
        T._call(model, kind, top_k=0, top_p=1.0, min_p=0.0)
        assert model.lib.trace == T._default_trace(kind)


BAD = [(dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"), (dict(top_k=True), "top_k"), (dict(top_p=0.0), "top_p"),
       (dict(top_p=1.0001), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(top_p="x"), "top_p"), (dict(min_p=-0.1), "min_p"),
       (dict(min_p=1.5), "min_p"), (dict(min_p=float("nan")), "min_p"), (dict(min_p=None), "min_p")]


@pytest.mark.parametrize("bad,word", BAD, ids=[f"{w}={list(b.values())[0]!r}" for b, w in BAD])
@pytest.mark.parametrize("kind", KINDS + ("transcribe",))
def test_a_refused_call_makes_no_library_call(kind, bad, word):
    for opt_in in (True, False):                         # a value outside its range is refused with or without the opt-in
        m = T._Traced(**dict(ON, truncated_sampling=opt_in))
        with pytest.raises(ValueError, match=word):
            if kind == "transcribe":
                m.transcribe_batch([T.CLIP], temperature=0.5, **T.CALL, **bad)
            else:
                T._call(m, kind, temperature=0.5, **T.GOOD["bias"], **T.GOOD["history"], **bad)
        assert m.lib.trace == [] and m.ctx.checked == []


@pytest.mark.parametrize("kind", KINDS + ("transcribe",))
def test_without_the_opt_in_a_value_off_its_default_is_refused(kind):
    m = T._Traced(**T.ALL_ON)
    with pytest.raises(ValueError, match="truncated_sampling=True"):
        if kind == "transcribe":
            m.transcribe_batch([T.CLIP], top_p=0.9, **T.CALL)
        else:
            T._call(m, kind, top_p=0.9, **T.GOOD["options"])
    assert m.lib.trace == [] and m.ctx.checked == []


@pytest.mark.parametrize("kind", KINDS)
def test_a_later_refusal_comes_before_this_setting_is_applied(kind):
    m = T._Traced(**ON)
    with pytest.raises(_lib.CcxError, match="temperature"):
        T._call(m, kind, temperature=-1.0, **ARGS)
    with pytest.raises(TypeError, match="beam_width"):
        T._call(m, kind, beam_width=3, **ARGS)
    assert m.lib.trace == []


@pytest.mark.parametrize("kind", KINDS)
def test_this_setter_failing_takes_back_the_ones_before_it(kind):
    m = T._Traced(**ON)
    m.lib.fail_at = {SAMPLING: 0}
    with pytest.raises(_lib.CcxError):
        T._call(m, kind, temperature=0.5, **ARGS, **T.FAMILIES["all"][0])
    assert _names(m.lib.trace) == [T.OPTIONS, T.HISTORY, T.BIAS, SAMPLING, T.BIAS, T.HISTORY, T.OPTIONS]      # not reset: it was never set
    assert T._left_behind(m.lib.trace) == T.CLEAN


@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_decode_takes_it_back(kind):
    m = T._Traced(**ON)
    decode = T.DECODES[KINDS.index(kind)]
    m.lib.fail_at = {decode: 0}
    with pytest.raises(_lib.CcxError):
        T._call(m, kind, temperature=0.5, **ARGS)
    assert _names(m.lib.trace) == [SAMPLING, decode, SAMPLING] and _payload(m.lib.trace[-1]) is None


def test_the_beam_decode_does_not_take_the_arguments():
    m = T._Traced(**ON)
    with pytest.raises(TypeError, match="top_k"):
        T._call(m, "decode_beam", top_k=3)
    assert m.lib.trace == []


def test_transcribe_sets_it_once_for_every_round_and_restores_it():
    m = T._Traced(**dict(T.FIVE_ON, truncated_sampling=True))
    m.lib.sum_logprob = {"ccx_whisper_decode": -10.0}      # round 0 is too improbable: the window decodes again, warmer, best_of rows
    m.transcribe_batch([T.CLIP], temperature=(0.0, 0.4), best_of=2, **ARGS, **T.CALL)
    names = _names(m.lib.trace)
    at = [i for i, n in enumerate(names) if n == SAMPLING]
    decodes = [i for i, n in enumerate(names) if n in T.DECODES]
    assert len(at) == 2 and [names[i] for i in decodes] == ["ccx_whisper_decode", "ccx_whisper_decode_rows"]
    assert at[0] == decodes[0] - 1 and _payload(m.lib.trace[at[0]]) == WANT          # the last setting before the first decode ...
    assert names[decodes[-1] + 1] == T.PATH and at[1] == decodes[-1] + 2 and _payload(m.lib.trace[at[1]]) is None      # ... the first taken back
    held = T._left_behind([e for e in m.lib.trace if e[0] != SAMPLING])
    assert held == T.CLEAN and (m.sot_tail, m.prefix_len) == (0, 0)


def test_transcribe_a_later_failing_setter_cannot_exist_and_an_earlier_one_keeps_it_unset():
    """sampling is the last setter: one that fails before it means it is never applied"""
    m = T._Traced(**dict(T.FIVE_ON, truncated_sampling=True))
    m.lib.fail_at = {T.BIAS: 0}
    with pytest.raises(_lib.CcxError):
        m.transcribe_batch([T.CLIP], temperature=0.3, **ARGS, **T.CALL)
    assert SAMPLING not in _names(m.lib.trace) and not [e for e in m.lib.trace if e[0] in T.DECODES]
    assert T._left_behind(m.lib.trace) == T.CLEAN
    m = T._Traced(**dict(T.FIVE_ON, truncated_sampling=True))
    m.lib.fail_at = {SAMPLING: 0}
    with pytest.raises(_lib.CcxError):
        m.transcribe_batch([T.CLIP], temperature=0.3, **ARGS, **T.CALL)
    assert not [e for e in m.lib.trace if e[0] in T.DECODES] and T._left_behind(m.lib.trace) == T.CLEAN
    assert (m.sot_tail, m.prefix_len) == (0, 0)


def test_transcribe_forwards_the_three_arguments():
    m = T._Traced(truncated_sampling=True)
    m.transcribe(T.CLIP, temperature=0.2, top_k=7, min_p=0.25)
    assert _payload(m.lib.trace[0]) == (7, 1.0, 0.25) and np.isclose(m.lib.trace[1][1]["temperature"], 0.2)
