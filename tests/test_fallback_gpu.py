"""GPU: temperature fallback and best_of in WhisperModel.transcribe_batch (opt-in: WhisperModel(temperature_fallback=True)).

Seeded weights give near-uniform logits, so the thresholds come from the instance's own temperature-0 decode of the test clips: the
median avg_logprob of the windows is the logprob_threshold, so that some windows pass at temperature 0 and some fall back (a second
run does the same with the compression ratio; the id tokenizer's placeholder text is far above upstream's 2.4 everywhere).  Every
window's walk through the schedule is replayed through tests/fallback_reference.py on the per-round results the instance recorded
(`fallback_walks`); rules only -- [UPSTREAM-RECALL: transcribe.py::decode_with_fallback], parity unpinned.
"""
import statistics

import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from tests import fallback_reference as FR

pytestmark = pytest.mark.gpu

SCHEDULE = (0.0, 0.4, 0.8)
NEW_KEYS = {"temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}
CLIP_S = [4.0, 7.5, 3.0, 9.0, 5.5, 6.5]            # a few windows each: a window that ends inside a segment resumes at its last timestamp


def _clips(n):
    return [synthetic_clip(50 + i, 30.0)[: int(CLIP_S[i] * 16000)] for i in range(n)]


def _build(ccx_ctx, **kw):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=8, ctx=ccx_ctx, **kw)


@pytest.fixture(scope="module")
def model(ccx_ctx):
    m = _build(ccx_ctx, temperature_fallback=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def greedy(model):
    """the plain temperature-0 transcripts of the six clips, and the avg_logprob at temperature 0 of every clip's FIRST window (a
    one-entry schedule without thresholds: each window is accepted as it is).  The first pass over the clips is one encoded group of
    six windows at seek 0 without a prompt: what it decodes does not depend on what was accepted before."""
    m = model
    clips = _clips(6)
    plain = m.transcribe_batch(clips, temperature=0.0, no_speech_threshold=None, logprob_threshold=None)
    one = m.transcribe_batch(clips, temperature=(0.0,), no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None)
    first = m.fallback_walks[0]
    assert first.clips == list(range(6)) and first.seeks == [0] * 6
    assert [o["tokens"] for o in one] == [o["tokens"] for o in plain]          # a schedule of temperature 0 alone is the plain call
    lp = [first.accepted[w]["avg_logprob"] for w in range(6)]
    cr = [first.accepted[w]["compression_ratio"] for w in range(6)]
    return clips, plain, lp, cr


def test_a_float_temperature_returns_the_dicts_it_always_did(model, greedy, ccx_ctx):
    clips, plain, _, _ = greedy
    for out in plain:
        assert set(out) == {"text", "segments", "language", "tokens"}
        for s in out["segments"]:
            assert not (NEW_KEYS & set(s)), s.keys()
    # ... and what an instance built without the keyword returns; best_of / compression_ratio_threshold are ignored there
    d = _build(ccx_ctx)
    try:
        base = d.transcribe_batch(clips, temperature=0.0, no_speech_threshold=None, logprob_threshold=None)
        assert [o["tokens"] for o in base] == [o["tokens"] for o in plain] and [o["segments"] for o in base] == [o["segments"] for o in plain]
        one = d.transcribe(clips[0], temperature=0.0, best_of=5, compression_ratio_threshold=0.1, no_speech_threshold=None, logprob_threshold=None)
        assert one["tokens"] == plain[0]["tokens"] and not (NEW_KEYS & set(one["segments"][0]))
        with pytest.raises(Exception) as e:
            d.transcribe(clips[0], temperature=(0.0, 0.2, 0.4))
        assert "temperature_fallback" in str(e.value)
        with pytest.raises(Exception):
            d.transcribe_batch(clips[:2], temperature=[0.0, 0.2])
    finally:
        d.close()
    # a float on the keyword-built instance samples as before: reproducible per seed + call index
    m = model
    m.sample_seed, m._sample_calls = 5, 0
    a = m.transcribe(clips[1], temperature=0.3)
    m.sample_seed, m._sample_calls = 5, 0
    b = m.transcribe(clips[1], temperature=0.3)
    assert a["tokens"] == b["tokens"] and not (NEW_KEYS & set(a["segments"][0])) and m.fallback_walks == []


def _replay(m, walk, out, schedule, cr_thr, lp_thr):
    """every window of one group: its rounds are the ones the reference walks through, it stops where the reference stops, and the
    segments of its clip at its seek carry the accepted result"""
    for w, (clip, seek) in enumerate(zip(walk.clips, walk.seeks)):
        trace = walk.trace[w]
        rounds = []
        for k, r in enumerate(trace):
            assert r["temperature"] == schedule[k]
            assert r["avg_logprob"] == FR.avg_logprob_ref(r["sum_logprob"], len(r["tokens"]))
            assert r["compression_ratio"] == FR.compression_ratio_ref(m.tokenizer.decode(r["tokens"]))
            rounds.append((r["temperature"], r["compression_ratio"], r["avg_logprob"], r["no_speech_prob"]))
        never = (None, 0.0, 0.0, 0.0)                      # stands for the rounds the window was not decoded at: never looked at
        k_ref = FR.walk_ref(rounds + ([never] if len(rounds) < len(schedule) else []), cr_thr, lp_thr, None)
        assert k_ref == len(trace) - 1, (w, rounds)
        acc = walk.accepted[w]
        assert acc is trace[-1]
        segs = [s for s in out[clip]["segments"] if s["seek"] == seek]
        assert segs, (clip, seek)
        for s in segs:
            assert s["temperature"] == acc["temperature"] and s["avg_logprob"] == acc["avg_logprob"]
            assert s["compression_ratio"] == acc["compression_ratio"] and s["no_speech_prob"] == acc["no_speech_prob"]
        flat = [t for s in segs for t in s["tokens"]]
        # the segments hold the accepted tokens up to the window's last closed segment (a cleared segment holds none)
        if all(s["text"] != "" for s in segs):
            assert flat and flat == acc["tokens"][:len(flat)], (clip, seek)


@pytest.mark.parametrize("by", ["logprob", "compression"])
def test_every_window_walks_the_schedule_as_the_reference_says(model, greedy, by):
    """the threshold under test is the median of the six first windows' own temperature-0 values, the other one is None (the id
    tokenizer's placeholder text compresses far better than speech does: 2.4 would send every window through the whole schedule)"""
    m = model
    clips, plain, lp0, cr0 = greedy
    thr = statistics.median(lp0) if by == "logprob" else None
    cr_thr = statistics.median(cr0) if by == "compression" else None
    m.sample_seed, m._sample_calls = 9, 0
    out = m.transcribe_batch(clips, temperature=SCHEDULE, logprob_threshold=thr, compression_ratio_threshold=cr_thr, no_speech_threshold=None)
    walks = list(m.fallback_walks)
    assert len(walks) >= 1 and sum(len(wk.clips) for wk in walks) == sum(len(set(s["seek"] for s in o["segments"])) for o in out)
    for wk in walks:
        _replay(m, wk, out, SCHEDULE, cr_thr, thr)
    walk = walks[0]
    assert walk.clips == list(range(6)) and walk.seeks == [0] * 6
    passed = [w for w in range(6) if len(walk.trace[w]) == 1]
    fell = [w for w in range(6) if len(walk.trace[w]) > 1]
    assert passed and fell, (passed, fell, lp0, thr, cr0, cr_thr)
    for w in range(6):                                                  # round 0 is the plain temperature-0 decode
        assert walk.trace[w][0]["avg_logprob"] == lp0[w] and walk.trace[w][0]["compression_ratio"] == cr0[w]
    for w in passed:                                                    # a window that passes at 0 is what it is without a schedule
        assert walk.accepted[w]["temperature"] == 0.0
        mine = [s["tokens"] for s in out[w]["segments"] if s["seek"] == 0]
        assert mine == [s["tokens"] for s in plain[w]["segments"] if s["seek"] == 0]
    for w in fell:
        assert walk.accepted[w]["temperature"] > 0.0
    # a window's outcome does not depend on which other windows fell back: here every window of the group falls back to the end
    m.sample_seed, m._sample_calls = 9, 0
    m.transcribe_batch(clips, temperature=SCHEDULE, logprob_threshold=max(lp0) + 100.0, compression_ratio_threshold=None, no_speech_threshold=None)
    every = m.fallback_walks[0]
    assert all(len(every.trace[w]) == len(SCHEDULE) for w in range(6))
    for w in fell:
        for k, r in enumerate(walk.trace[w]):
            assert r["tokens"] == every.trace[w][k]["tokens"] and r["sum_logprob"] == every.trace[w][k]["sum_logprob"], (w, k)


def test_best_of_keeps_the_reference_rankers_choice(model):
    m = model
    clips = _clips(4)
    kw = dict(temperature=0.7, best_of=3, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)
    m.sample_seed, m._sample_calls = 3, 0
    a = m.transcribe_batch(clips, **kw)
    walk = m.fallback_walks[0]
    assert walk.clips == [0, 1, 2, 3] and walk.seeks == [0] * 4 and all(len(walk.trace[w]) == 1 for w in range(4))
    seed = (3 << 32) + 1                # the first group's only round: 12 rows in two calls of 8 and 4 rows under ONE seed
    # the first group again (the four clips at seek 0), and the three candidates of every window fetched alone under their stream ids
    host = np.zeros((4, max(len(c) for c in clips)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    m.log_mel(torch.from_numpy(host).cuda(), [len(c) for c in clips], [0] * 4)
    m.encode(4)
    sot, cap = [m.rules.sot], 224
    for w in range(4):
        rows = m.decode_rows([sot] * 3, [w] * 3, [3 * w + c for c in range(3)], sample_len=cap, temperature=0.7, seed=seed, n_windows=4)
        k = FR.rank_ref([(r["tokens"], r["sum_logprob"]) for r in rows], m.rules.eot)
        acc = walk.accepted[w]
        assert acc["candidate"] == k and acc["tokens"] == rows[k]["tokens"] and acc["sum_logprob"] == rows[k]["sum_logprob"], (w, k)
        assert acc["no_speech_prob"] == rows[0]["no_speech_prob"] and acc["temperature"] == 0.7
        assert len({tuple(r["tokens"]) for r in rows}) > 1              # the candidates are different draws
        for s in a[w]["segments"]:
            assert s["temperature"] == 0.7
            if s["seek"] == 0:
                assert s["avg_logprob"] == FR.avg_logprob_ref(rows[k]["sum_logprob"], len(rows[k]["tokens"]))
    m.sample_seed, m._sample_calls = 3, 0
    b = m.transcribe_batch(clips, **kw)
    assert [o["tokens"] for o in a] == [o["tokens"] for o in b] and [o["segments"] for o in a] == [o["segments"] for o in b]
    # best_of is dropped at temperature 0: the plain transcript
    z = m.transcribe_batch(clips, temperature=0.0, best_of=3, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)
    p = m.transcribe_batch(clips, temperature=0.0, logprob_threshold=None, no_speech_threshold=None)
    assert [o["tokens"] for o in z] == [o["tokens"] for o in p]
    assert all(s["temperature"] == 0.0 for o in z for s in o["segments"])


def test_words_are_aligned_after_the_walk_without_a_second_encode(ccx_ctx, greedy):
    clips, _, lp0, _ = greedy
    m = _build(ccx_ctx, temperature_fallback=True, word_alignment=True)
    try:
        thr = statistics.median(lp0)
        ccx_ctx.prof_enable(True)
        try:
            out = m.transcribe_batch(clips, temperature=SCHEDULE, logprob_threshold=thr, compression_ratio_threshold=None, no_speech_threshold=None,
                                     word_timestamps=True)
            names = [r[0] for r in ccx_ctx.prof_records()]
        finally:
            ccx_ctx.prof_enable(False)
        walks = m.fallback_walks
        assert any(len(wk.trace[w]) > 1 for wk in walks for w in wk.trace)          # something did fall back
        # every group was encoded once (one attention launch per encoder layer), whatever fell back, and aligned at most once, on
        # the accepted tokens
        assert names.count("enc_attention_kernel") == m.dims.n_audio_layer * len(walks)
        assert 1 <= names.count("align_dtw_kernel") <= len(walks)
        assert any("words" in s and s["words"] for o in out for s in o["segments"])
        for wk in walks:
            for w, (clip, seek) in enumerate(zip(wk.clips, wk.seeks)):
                for s in out[clip]["segments"]:
                    if s["seek"] == seek:
                        assert s["temperature"] == wk.accepted[w]["temperature"]
    finally:
        m.close()
