"""The library-call sequence of `WhisperModel.decode`, `decode_rows`, `decode_beam` and `transcribe_batch`, pinned without a GPU and
without libccx: the real methods run over a fake `lib` that records every entry point it is asked for (scalars, the fields of the
structs behind `byref`, the packed arrays read back through their pointers) and returns 0 unless a test tells it otherwise.

What is pinned: which settings a call puts on the instance and with which values, that each is set once before the first decode and
taken back after the last, that a refused call reaches the library not at all, which exception a bad argument raises and which one
wins when two are bad, and that a setter or a decode that fails leaves no setting behind.  The order among the independent setters
is not pinned (include/ccx.h: they are independent fields of the handle)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.tokenizer import DecodeRules, IdTokenizer
from clearconverse_amd.weights import WhisperDims
from clearconverse_amd.whisper import WhisperModel

R = DecodeRules()
EOT, SOT, NOTS = R.eot, R.sot, R.no_timestamps
OPTIONS, HISTORY, BIAS = "ccx_whisper_set_decode_options", "ccx_whisper_set_history_options", "ccx_whisper_set_bias_options"
TAIL, PREFIX = "ccx_whisper_set_sot_tail", "ccx_whisper_set_prefix_len"
PATH = "ccx_whisper_last_cross_path"
STRUCT_SETTERS, INT_SETTERS = (OPTIONS, HISTORY, BIAS), (TAIL, PREFIX)
DECODES = ("ccx_whisper_decode", "ccx_whisper_decode_rows", "ccx_whisper_decode_beam")
CLEAN = {OPTIONS: None, HISTORY: None, BIAS: None, TAIL: 0, PREFIX: 0}      # what an English instance holds between calls


def _array(p, *shape):
    return None if p is None else np.ctypeslib.as_array(p, shape=shape).tolist()


def _fields(name, ref):
    """NULL -> None; a byref'd struct -> its fields"""
    if ref is None:
        return None
    o = ref._obj
    if name == OPTIONS:
        return dict(without_timestamps=o.without_timestamps, suppress_blank=o.suppress_blank,
                    max_initial_timestamp_index=o.max_initial_timestamp_index,
                    suppress=[o.suppress[i] for i in range(o.n_suppress)] if o.suppress else None)
    if name == HISTORY:
        return (o.repetition_penalty, o.no_repeat_ngram_size)
    n = o.n_entries
    return dict(offsets=[o.offsets[i] for i in range(n + 1)], ids=[o.ids[i] for i in range(o.offsets[n])],
                bias=[o.bias[i] for i in range(n)])


class _FakeLib:
    """every attribute is an entry point: it records (name, payload, return code) in `trace` and returns 0, or 1 at the call
    `fail_at[name]` (0-based) names.  `sum_logprob[name]`: written to every row of that decode's sum_logprob output."""

    def __init__(self):
        self.trace, self.fail_at, self.sum_logprob, self._count = [], {}, {}, {}

    def __getattr__(self, name):
        return functools.partial(self._call, name)

    def _call(self, name, *a):
        k = self._count.get(name, 0)
        self._count[name] = k + 1
        rc = int(self.fail_at.get(name) == k)
        if name in STRUCT_SETTERS:
            payload = _fields(name, a[1])
        elif name in INT_SETTERS:
            payload = a[1]
        elif name == "ccx_whisper_decode":
            _, ids, lens, mp, n, sample_len, temperature, seed, _, _, slp = a[:11]
            payload = dict(ids=_array(ids, n, mp), lens=_array(lens, n), sample_len=sample_len, temperature=temperature, seed=seed)
        elif name == "ccx_whisper_decode_rows":
            _, ids, lens, mp, n, win, nw, sid, sample_len, temperature, seed, _, _, slp = a[:14]
            payload = dict(ids=_array(ids, n, mp), lens=_array(lens, n), windows=_array(win, n), n_windows=nw,
                           stream_ids=_array(sid, n), sample_len=sample_len, temperature=temperature, seed=seed)
        elif name == "ccx_whisper_decode_beam":
            _, ids, lens, mp, n, win, nw, bs, mc, sample_len, _, _, slp = a[:13]
            payload = dict(ids=_array(ids, n, mp), lens=_array(lens, n), windows=_array(win, n), n_windows=nw, beam_size=bs,
                           max_candidates=mc, sample_len=sample_len)
        else:
            payload = a[1:]
        if name in self.sum_logprob:
            np.ctypeslib.as_array(slp, shape=(n,))[:] = self.sum_logprob[name]
        self.trace.append((name, payload, rc))
        return rc


class _FakeCtx:
    def __init__(self):
        self.checked = []

    def check(self, code, what):
        self.checked.append(what)
        if code != 0:
            raise _lib.CcxError(f"{what} failed")


class _Traced(WhisperModel):
    """the real decode methods and transcribe_batch over the fake library; log_mel / encode / detect_language scripted"""

    def __init__(self, max_batch=8, **opt_ins):
        self.rules, self.tokenizer, self.dims = R, IdTokenizer(EOT), WhisperDims.mini(n_vocab=51864)
        self.max_batch, self.device, self.max_audio_seconds = max_batch, torch.device("cpu"), 30.0
        self.word_alignment, self.word_probabilities = False, False
        self.sample_seed, self._sample_calls, self.handle = 0, 0, None
        self.sot_tail, self.prefix_len = 0, 0
        self.lib, self.ctx = _FakeLib(), _FakeCtx()
        for k, v in opt_ins.items():
            assert hasattr(WhisperModel, k)
            setattr(self, k, v)

    def __del__(self):
        pass

    def log_mel(self, audio, n_samples, seek=None, return_mel=False, max_frames=None):
        return None

    def encode(self, B, return_xa=False):
        return None

    def detect_language(self, B):
        raise AssertionError("an English-only model detects nothing")


ALL_ON = dict(decoding_options=True, repetition_control=True, contextual_bias=True)
FIVE_ON = dict(ALL_ON, temperature_fallback=True, beam_search=True)


@pytest.fixture(autouse=True)
def _no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: 0)


# ---------------------------------------------------------------------------------------------- single decodes
PROMPTS = [[SOT], [SOT, 11, 12]]
IDS, LENS = [[SOT, EOT, EOT], [SOT, 11, 12]], [1, 3]


def _call(m, kind, **kw):
    if kind == "decode":
        return m.decode(PROMPTS, sample_len=4, **kw)
    if kind == "decode_rows":
        return m.decode_rows(PROMPTS, [1, 0], sample_len=4, **kw)
    return m.decode_beam(PROMPTS, 2, sample_len=4, **kw)


def _default_trace(kind):
    if kind == "decode":
        d = ("ccx_whisper_decode", dict(ids=IDS, lens=LENS, sample_len=4, temperature=0.0, seed=0), 0)
    elif kind == "decode_rows":
        d = ("ccx_whisper_decode_rows", dict(ids=IDS, lens=LENS, windows=[1, 0], n_windows=2, stream_ids=None, sample_len=4,
                                             temperature=0.0, seed=0), 0)
    else:
        d = ("ccx_whisper_decode_beam", dict(ids=IDS, lens=LENS, windows=None, n_windows=2, beam_size=2, max_candidates=2,
                                             sample_len=4), 0)
    return [d, (PATH, (), 0)]


def _bad(kind):
    """an argument the last refusal of the precedence list turns down: temperature, or patience for the beam search"""
    return dict(patience=0.0) if kind == "decode_beam" else dict(temperature=-1.0)


def _split(trace):
    """(entries before the first decode, from the first to the last decode, behind the last decode)"""
    at = [i for i, e in enumerate(trace) if e[0] in DECODES]
    assert at, trace
    end = at[-1] + 1
    if end < len(trace) and trace[end][0] == PATH:
        end += 1
    return trace[:at[0]], trace[at[0]:end], trace[end:]


def _as_dict(entries):
    names = [e[0] for e in entries]
    assert len(names) == len(set(names)), f"an entry point is called twice: {names}"
    assert all(e[2] == 0 for e in entries)
    return {e[0]: e[1] for e in entries}


def _left_behind(trace):
    """the settings the library holds after the calls of `trace`: a call that returned non-zero changed nothing"""
    held = dict(CLEAN)
    for name, payload, rc in trace:
        if name in held and rc == 0:
            held[name] = payload
    return held


F32 = lambda x: float(np.float32(x))
OPT_WT = dict(without_timestamps=1, suppress_blank=1, max_initial_timestamp_index=50, suppress=None)
FAMILIES = {
    "options": (dict(without_timestamps=True), {OPTIONS: OPT_WT}),
    "options_rules_own": (dict(suppress_blank=True), {OPTIONS: dict(OPT_WT, without_timestamps=0)}),      # a single decode sets them too
    "options_suppress": (dict(suppress_tokens=[5, 3], suppress_blank=False, max_initial_timestamp=None),
                         {OPTIONS: dict(without_timestamps=0, suppress_blank=0, max_initial_timestamp_index=-1,
                                        suppress=sorted({3, 5, R.transcribe, R.translate, R.sot, R.sot_prev, R.sot_lm, R.no_speech}))}),
    "history": (dict(repetition_penalty=1.3, no_repeat_ngram_size=2), {HISTORY: (F32(1.3), 2)}),
    "history_ngram_only": (dict(no_repeat_ngram_size=3), {HISTORY: (1.0, 3)}),
    "bias": (dict(bad_words_ids=[[7], [8, 9]], sequence_bias={(5,): 1.5}),
             {BIAS: dict(offsets=[0, 1, 2, 4], ids=[5, 7, 8, 9], bias=[1.5, -np.inf, -np.inf])}),
    "hotwords": (dict(hotwords="<21> <22>", hotword_boost=2.0), {BIAS: dict(offsets=[0, 1, 3], ids=[21, 21, 22], bias=[2.0, 2.0])}),
    "all": (dict(without_timestamps=True, repetition_penalty=1.3, bad_words_ids=[[7]]),
            {OPTIONS: OPT_WT, HISTORY: (F32(1.3), 0), BIAS: dict(offsets=[0, 1], ids=[7], bias=[-np.inf])}),
}
KINDS = ("decode", "decode_rows", "decode_beam")


@pytest.mark.parametrize("kind", KINDS)
def test_default_call_records_the_decode_and_the_path_query(kind):
    m = _Traced()
    out = _call(m, kind)
    assert m.lib.trace == _default_trace(kind) and m.ctx.checked == [DECODES[KINDS.index(kind)]]
    assert m.last_cross_path == "kv16"
    if kind == "decode_beam":
        assert out == [[], []]
    else:
        assert out == [dict(tokens=[], sum_logprob=0.0, avg_logprob=0.0, no_speech_prob=0.0, cross_path="kv16")] * 2


def test_rows_and_beam_pass_their_maps_through():
    m = _Traced()
    m.decode_rows(PROMPTS, [0, 0], stream_ids=[4, 5], sample_len=4, temperature=0.5, seed=-1, n_windows=3)
    assert m.lib.trace[0][1] == dict(ids=IDS, lens=LENS, windows=[0, 0], n_windows=3, stream_ids=[4, 5], sample_len=4, temperature=0.5,
                                     seed=2 ** 64 - 1)
    m = _Traced()
    m.decode_beam(PROMPTS, 2, patience=1.6, sample_len=4, windows=[2, 0])
    assert m.lib.trace[0][1] == dict(ids=IDS, lens=LENS, windows=[2, 0], n_windows=3, beam_size=2, max_candidates=3, sample_len=4)
    m = _Traced()
    m.decode(PROMPTS)      # sample_len: decode_cap of the longest prompt
    assert m.lib.trace[0][1]["sample_len"] == 224


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("kind", KINDS)
def test_opted_in_families_are_set_before_and_reset_behind_the_decode(kind, family):
    kw, expected = FAMILIES[family]
    m = _Traced(**ALL_ON)
    _call(m, kind, **kw)
    before, during, after = _split(m.lib.trace)
    assert _as_dict(before) == expected
    assert during == _default_trace(kind)
    assert _as_dict(after) == {name: None for name in expected}
    assert (m.sot_tail, m.prefix_len) == (0, 0)      # a single decode leaves both to its caller


@pytest.mark.parametrize("kind", KINDS)
def test_opt_ins_off_ignore_their_arguments(kind):
    m = _Traced()
    _call(m, kind, without_timestamps=True, suppress_tokens="x", repetition_penalty=-2.0, no_repeat_ngram_size=2, bad_words_ids=[[EOT]],
          hotwords="<21>")
    assert m.lib.trace == _default_trace(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_opt_ins_on_with_values_that_set_nothing(kind):
    m = _Traced(**ALL_ON)
    _call(m, kind, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=[], sequence_bias={}, hotword_boost=3.0)
    assert m.lib.trace == _default_trace(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_decode_leaves_no_setting_behind(kind):
    m = _Traced(**ALL_ON)
    m.lib.fail_at = {DECODES[KINDS.index(kind)]: 0}
    with pytest.raises(_lib.CcxError):
        _call(m, kind, **FAMILIES["all"][0])
    before, during, after = _split(m.lib.trace)
    assert _as_dict(before) == FAMILIES["all"][1]
    assert [e[0] for e in during] == [DECODES[KINDS.index(kind)]]      # no path query behind a decode that failed
    assert _as_dict(after) == {OPTIONS: None, HISTORY: None, BIAS: None}


@pytest.mark.parametrize("failing", STRUCT_SETTERS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_setter_takes_back_the_ones_before_it_and_decodes_nothing(kind, failing):
    """new with the settings scope"""
    m = _Traced(**ALL_ON)
    m.lib.fail_at = {failing: 0}
    with pytest.raises(_lib.CcxError):
        _call(m, kind, **FAMILIES["all"][0])
    assert not [e for e in m.lib.trace if e[0] in DECODES + (PATH,)]
    assert _left_behind(m.lib.trace) == CLEAN


GOOD = dict(bias=dict(bad_words_ids=[[7]]), history=dict(repetition_penalty=1.3), options=dict(without_timestamps=True))
REFUSED = {      # family -> (a bad argument, the exception, a word of its message)
    "bias": (dict(bad_words_ids=[[EOT]]), ValueError, "bad_words_ids"),
    "history": (dict(repetition_penalty=-1.0), ValueError, "repetition_penalty"),
    "key": (dict(beam_width=3), TypeError, "beam_width"),
    "resolve": (dict(suppress_tokens="x"), _lib.CcxError, "invalid literal"),
}
ORDER = ("bias", "history", "key", "resolve", "last")


def _refusal(kind, family):
    if family == "last":
        return _bad(kind), _lib.CcxError, "patience" if kind == "decode_beam" else "temperature"
    return REFUSED[family]


@pytest.mark.parametrize("family", ORDER)
@pytest.mark.parametrize("kind", KINDS)
def test_exception_type_per_bad_argument(kind, family):
    kw, exc, word = _refusal(kind, family)
    m = _Traced(**ALL_ON)
    with pytest.raises(exc, match=word) as e:
        _call(m, kind, **kw)
    assert type(e.value) is exc and m.lib.trace == [] and m.ctx.checked == []


@pytest.mark.parametrize("kind", KINDS)
def test_unknown_decoding_keys_raise_without_the_opt_in_too(kind):
    m = _Traced()
    with pytest.raises(TypeError, match="beam_width"):
        _call(m, kind, beam_width=3)
    assert m.lib.trace == []


@pytest.mark.parametrize("first,second", [(a, b) for i, a in enumerate(ORDER) for b in ORDER[i + 1:]])
@pytest.mark.parametrize("kind", KINDS)
def test_precedence_when_two_arguments_are_bad(kind, first, second):
    """the bias compile, then the history ranges, then the decoding keys and `resolve`, then temperature / patience"""
    kw, exc, word = _refusal(kind, first)
    m = _Traced(**ALL_ON)
    with pytest.raises(exc, match=word) as e:
        _call(m, kind, **kw, **_refusal(kind, second)[0])
    assert type(e.value) is exc and m.lib.trace == []


@pytest.mark.parametrize("good,bad", [("bias", "history"), ("bias", "key"), ("bias", "resolve"), ("bias", "last"), ("history", "key"),
                                      ("history", "resolve"), ("history", "last"), ("options", "last")])
@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_call_makes_no_library_call(kind, good, bad):
    """new with the resolvers: every refusal comes before anything is set, also behind a family that is fine"""
    kw, exc, word = _refusal(kind, bad)
    m = _Traced(**ALL_ON)
    with pytest.raises(exc, match=word):
        _call(m, kind, **GOOD[good], **kw)
    assert m.lib.trace == [] and m.ctx.checked == []


# ---------------------------------------------------------------------------------------------- transcribe_batch
CLIP = np.zeros(16000 * 3, dtype=np.float32)      # zeros and a library that writes nothing: no tokens, `seek` advances by the window
CALL = dict(without_timestamps=True, prefixes=[[11, 12]], repetition_penalty=1.3, bad_words_ids=[[7]])
CALL_SETS = {OPTIONS: OPT_WT, TAIL: 1, PREFIX: 2, HISTORY: (F32(1.3), 0), BIAS: dict(offsets=[0, 1], ids=[7], bias=[-np.inf])}
WINDOW = [SOT, NOTS, 11, 12]


def _plain(seed, ids=None, lens=None):
    ids = ids or [WINDOW]
    return ("ccx_whisper_decode", dict(ids=ids, lens=lens or [len(p) for p in ids], sample_len=224, temperature=0.0, seed=seed), 0)


def _check_one_set_and_one_restore(m, decodes):
    before, during, after = _split(m.lib.trace)
    assert _as_dict(before) == CALL_SETS
    assert during == decodes
    assert _as_dict(after) == CLEAN
    assert (m.sot_tail, m.prefix_len) == (0, 0)


def test_transcribe_sets_each_of_the_five_once_and_restores_them():
    m = _Traced(**FIVE_ON)
    out = m.transcribe_batch([CLIP], **CALL)
    _check_one_set_and_one_restore(m, [_plain(1), (PATH, (), 0)])
    assert out[0]["text"] == "" and out[0]["tokens"] == [] and [s["seek"] for s in out[0]["segments"]] == [0]
    assert m.fallback_walks == []


def test_transcribe_two_groups_still_one_set_per_family():
    m = _Traced(max_batch=1, **FIVE_ON)
    m.transcribe_batch([CLIP, CLIP], [None, " <1000> <1001>"], prefixes=[[11, 12], [13, 14]],
                       **{k: v for k, v in CALL.items() if k != "prefixes"})
    second = [R.sot_prev, 1000, 1001, SOT, NOTS, 13, 14]
    _check_one_set_and_one_restore(m, [_plain(1), (PATH, (), 0), _plain(2, [second]), (PATH, (), 0)])


def test_transcribe_fallback_rounds_still_one_set_per_family():
    m = _Traced(**FIVE_ON)
    m.lib.sum_logprob = {"ccx_whisper_decode": -10.0}      # round 0 is too improbable: the window decodes again, warmer, best_of rows
    out = m.transcribe_batch([CLIP], temperature=(0.0, 0.4), best_of=2, **CALL)
    rows = ("ccx_whisper_decode_rows", dict(ids=[WINDOW, WINDOW], lens=[4, 4], windows=[0, 0], n_windows=1, stream_ids=[0, 1],
                                            sample_len=224, temperature=0.4, seed=2), 0)
    _check_one_set_and_one_restore(m, [_plain(1), (PATH, (), 0), rows, (PATH, (), 0)])
    assert len(m.fallback_walks) == 1 and [r["temperature"] for r in m.fallback_walks[0].trace[0]] == [0.0, 0.4]
    seg = out[0]["segments"][0]
    assert (seg["temperature"], seg["avg_logprob"], seg["compression_ratio"], seg["no_speech_prob"]) == (0.4, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("failing", (TAIL, PREFIX, HISTORY, BIAS))
def test_transcribe_a_failing_setter_takes_back_the_ones_before_it(failing):
    """new with the settings scope (TAIL is the second setter of the call)"""
    m = _Traced(**FIVE_ON)
    m.lib.fail_at = {failing: 0}
    with pytest.raises(_lib.CcxError):
        m.transcribe_batch([CLIP], **CALL)
    assert OPTIONS in [e[0] for e in m.lib.trace] and not [e for e in m.lib.trace if e[0] in DECODES + (PATH,)]
    assert _left_behind(m.lib.trace) == CLEAN and (m.sot_tail, m.prefix_len) == (0, 0)


def test_transcribe_values_that_set_nothing():
    m = _Traced(**FIVE_ON)
    m.transcribe_batch([CLIP], suppress_blank=True, repetition_penalty=1.0, bad_words_ids=[], hotword_boost=2.0)
    assert m.lib.trace == [_plain(1, [[SOT]]), (PATH, (), 0)]


def test_transcribe_opt_ins_off_touches_the_library_through_the_decode_only():
    plain = _Traced()
    plain.transcribe_batch([CLIP])
    assert plain.lib.trace == [_plain(1, [[SOT]]), (PATH, (), 0)]
    m = _Traced()
    m.transcribe_batch([CLIP], best_of=2, compression_ratio_threshold=0.1, beam_size=4, patience=2.0, length_penalty=1.0, **CALL,
                       suppress_blank=False, suppress_tokens="x", max_initial_timestamp=None, sample_len=3, clip_timestamps="1,2",
                       carry_initial_prompt=True, no_repeat_ngram_size=-1, sequence_bias="x", hotwords=5)
    assert m.lib.trace == plain.lib.trace and m.ctx.checked == ["ccx_whisper_decode"]
