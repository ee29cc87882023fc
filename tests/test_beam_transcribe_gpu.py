"""GPU: beam_size / patience / length_penalty in WhisperModel.transcribe_batch (opt-in: WhisperModel(beam_search=True)).

Without the opt-in the three options change nothing.  With it, a temperature-0 round decodes every window of a group by beam search
(`decode_beam`, chunked to max_batch // beam_size windows per call over the group's window map) and keeps what
`fallback.window_result` keeps of the hypotheses; in a schedule the rounds above 0 stay best_of rounds; word alignment runs afterwards
with one `encode` per group.  Rules only [UPSTREAM-RECALL: transcribe.py::decode_with_fallback]; parity unpinned.
"""
import statistics

import numpy as np
import pytest
import torch

from clearconverse_amd import fallback
from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict

pytestmark = pytest.mark.gpu

CLIP_S = [4.0, 7.5, 3.0, 9.0, 5.5, 6.5]
NEW_KEYS = {"temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}
KW = dict(no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None)


def _clips(n):
    return [synthetic_clip(50 + i, 30.0)[: int(CLIP_S[i] * 16000)] for i in range(n)]


def _build(ccx_ctx, **kw):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=8, ctx=ccx_ctx, **kw)


@pytest.fixture(scope="module")
def model(ccx_ctx):
    m = _build(ccx_ctx, beam_search=True, temperature_fallback=True)
    yield m
    m.close()


def _first_group_hypotheses(m, clips, beam, patience=None):
    """the first pass of transcribe_batch by hand: the six clips' first windows (seek 0, no prompt) encoded as one group, decoded by
    beam search in the chunks the product uses"""
    from clearconverse_amd.whisper import decode_cap
    lens = [len(c) for c in clips]
    host = np.zeros((len(clips), max(lens)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, :lens[i]] = c
    m.log_mel(torch.from_numpy(host).cuda(), lens, [0] * len(clips))
    m.encode(len(clips))
    prompts = [m.rules.sot_sequence()] * len(clips)
    cap = decode_cap(len(prompts[0]), m.dims.n_text_ctx)
    per = m.max_batch // beam
    out = []
    for at in range(0, len(clips), per):
        part = list(range(at, min(at + per, len(clips))))
        out += m.decode_beam([prompts[w] for w in part], beam, patience=patience, sample_len=cap, windows=part, n_windows=len(clips))
    return out


def test_without_the_opt_in_the_options_change_nothing(ccx_ctx):
    clips = _clips(3)
    d = _build(ccx_ctx)
    try:
        base = d.transcribe_batch(clips, temperature=0.0, **KW)
        with_opts = d.transcribe_batch(clips, temperature=0.0, beam_size=5, patience=2.0, length_penalty=0.6, **KW)
        assert with_opts == base                                      # every segment, token and float, bit for bit
        one = d.transcribe(clips[0], temperature=0.0, beam_size=5, patience=2.0, length_penalty=1.0, **KW)
        assert one == base[0] and not (NEW_KEYS & set(one["segments"][0]))
        sampled = d.transcribe(clips[0], temperature=0.3, beam_size=5, **KW)     # ignored: no rejection either
        assert sampled["segments"]
    finally:
        d.close()


@pytest.mark.parametrize("beam,patience,length_penalty", [(2, None, None), (3, 2.0, 0.6)])
def test_window_results_are_the_rankers_pick_of_decode_beam(model, beam, patience, length_penalty):
    m = model
    clips = _clips(6)
    out = m.transcribe_batch(clips, temperature=0.0, beam_size=beam, patience=patience, length_penalty=length_penalty, **KW)
    walk = m.fallback_walks[0]
    assert walk.clips == list(range(6)) and walk.seeks == [0] * 6
    hyps = _first_group_hypotheses(m, clips, beam, patience)
    for w in range(6):
        want = fallback.window_result(hyps[w], 0.0, m.tokenizer, m.rules.eot, length_penalty)
        got = walk.accepted[w]
        assert got == want, (w, got, want)
        assert got["candidate"] == fallback.rank_candidates(hyps[w], m.rules.eot, length_penalty)
        assert beam <= len(hyps[w]) <= max(beam, round(beam * (patience or 1.0)))
    for o in out:
        assert o["segments"] and all(NEW_KEYS <= set(s) for s in o["segments"])


def test_schedule_uses_beam_at_zero_and_best_of_above(model, monkeypatch):
    m = model
    clips = _clips(6)
    m.transcribe_batch(clips, temperature=0.0, beam_size=2, patience=1.5, length_penalty=0.6, **KW)
    lp = [m.fallback_walks[0].accepted[w]["avg_logprob"] for w in range(6)]
    thr = statistics.median(lp)
    calls = []
    beam_fn, rows_fn, plain_fn = m.decode_beam, m.decode_rows, m.decode
    monkeypatch.setattr(m, "decode_beam", lambda p, b, **kw: (calls.append(("beam", len(p), b, kw.get("patience"))), beam_fn(p, b, **kw))[1])
    monkeypatch.setattr(m, "decode_rows", lambda p, w, s=None, **kw: (calls.append(("rows", len(p), kw["temperature"])), rows_fn(p, w, s, **kw))[1])
    monkeypatch.setattr(m, "decode", lambda p, **kw: (calls.append(("plain", len(p), kw.get("temperature"))), plain_fn(p, **kw))[1])
    m.transcribe_batch(clips, temperature=(0.0, 0.4), beam_size=2, patience=1.5, best_of=3, length_penalty=0.6, no_speech_threshold=None,
                       logprob_threshold=thr, compression_ratio_threshold=None)
    walk = m.fallback_walks[0]
    failing = [w for w in range(6) if lp[w] < thr]
    assert 0 < len(failing) < 6
    # round 0 of the first group: six windows by beam search, four windows per call (max_batch 8 // beam_size 2); round 1: the failing
    # windows, best_of rows each, beam_size and patience dropped
    assert calls[:2] == [("beam", 4, 2, 1.5), ("beam", 2, 2, 1.5)]
    n_rows, at = 0, 2
    while n_rows < 3 * len(failing):                                   # (chunked to max_batch rows)
        assert calls[at][0] == "rows" and calls[at][2] == 0.4, calls[at]
        n_rows += calls[at][1]; at += 1
    assert n_rows == 3 * len(failing)
    assert not any(c[0] == "plain" for c in calls)
    for w in range(6):
        tr = walk.trace[w]
        assert tr[0]["temperature"] == 0.0 and len(tr) == (2 if w in failing else 1)
        if w in failing:
            assert tr[1]["temperature"] == 0.4 and tr[1]["candidate"] in range(3) and walk.accepted[w] is tr[1]


def test_word_timestamps_after_a_beam_decode_encode_once_per_group(ccx_ctx, monkeypatch):
    m = _build(ccx_ctx, beam_search=True, word_alignment=True)
    try:
        clips = _clips(3)
        n_enc = []
        enc = m.encode
        monkeypatch.setattr(m, "encode", lambda B, **kw: (n_enc.append(B), enc(B, **kw))[1])
        out = m.transcribe_batch(clips, temperature=0.0, beam_size=2, word_timestamps=True, **KW)
        assert len(n_enc) == len(m.fallback_walks) >= 1               # one encode per group: the alignment reads the group still encoded
        assert any(s.get("words") for o in out for s in o["segments"])
    finally:
        m.close()


def test_rejections(model):
    from clearconverse_amd import _lib
    clips = _clips(1)
    with pytest.raises(_lib.CcxError) as e:
        model.transcribe(clips[0], temperature=0.3, beam_size=2)
    assert "beam_size" in str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        model.transcribe(clips[0], temperature=0.0, patience=2.0)
    assert "patience" in str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        model.transcribe(clips[0], temperature=0.0, beam_size=9)
    assert "beam_size" in str(e.value)
