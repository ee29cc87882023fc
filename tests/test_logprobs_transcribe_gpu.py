"""GPU: `transcribe_batch(logprobs=n)` on a token_logprobs instance (mini dims, 2 layers, 128 wide).

  * Every segment's lists match its `tokens` in length; the segments of a window, concatenated, are the window's lists over the
    index ranges WindowLoop.window_segments cuts `tokens` with (a cleared segment: empty lists) -- the window decoded again alone.
  * With a temperature schedule and best_of = 2 the lists are the accepted candidate's, replayed from `fallback_walks`.
  * A default call's result and segment keys are exactly what they were; `load_models(whisper_token_logprobs=True)` works; without
    the opt-in the argument raises ValueError."""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import SepDims, WhisperDims, synthetic_whisper_state_dict
from clearconverse_amd.window_loop import HOP, WindowLoop

pytestmark = pytest.mark.gpu

CLIP_S = [4.0, 3.0]
NO_THRESHOLDS = dict(no_speech_threshold=None, logprob_threshold=None)
RESULT_KEYS, SEGMENT_KEYS = {"text", "segments", "language", "tokens"}, {"seek", "start", "end", "tokens", "text"}
N = 2


def _clips():
    return [synthetic_clip(50 + i, 30.0)[: int(CLIP_S[i] * 16000)] for i in range(2)]


@pytest.fixture(scope="module")
def model(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    m = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=8, ctx=ccx_ctx, temperature_fallback=True,
                     token_logprobs=True)
    yield m
    m.close()


def _encode_first_windows(m, clips):
    host = np.zeros((len(clips), max(len(c) for c in clips)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    m.log_mel(torch.from_numpy(host).cuda(), [len(c) for c in clips], [0] * len(clips))
    m.encode(len(clips))


def _check_window(m, clip, window, segments):
    """`segments`: the result's segments of one window; `window`: that window's decode, with its lists"""
    loop = WindowLoop(m.rules, m.tokenizer, len(clip) // HOP, None, m.dims.n_text_ctx, True, None, None, language="en")
    built = loop.window_segments(window)[0]
    assert len(built) == len(segments)
    pos = 0
    for b, s in zip(built, segments):
        n = len(b["tokens"])
        assert b["tokens"] == window["tokens"][pos:pos + n]
        assert b["token_logprobs"] == window["token_logprobs"][pos:pos + n] and b["top_logprobs"] == window["top_logprobs"][pos:pos + n]
        pos += n
        assert len(s["token_logprobs"]) == len(s["top_logprobs"]) == len(s["tokens"])
        if s["tokens"]:
            assert (s["tokens"], s["token_logprobs"], s["top_logprobs"]) == (b["tokens"], b["token_logprobs"], b["top_logprobs"])
        assert all(1 <= len(step) <= N for step in s["top_logprobs"])
    return pos


def test_segments_carry_the_slices_of_their_window(model):
    m = model
    clips = _clips()
    out = m.transcribe_batch(clips, logprobs=N, **NO_THRESHOLDS)
    plain = m.transcribe_batch(clips, **NO_THRESHOLDS)
    assert [o["tokens"] for o in out] == [o["tokens"] for o in plain] and all(set(o) == RESULT_KEYS for o in out)
    assert all(set(s) == SEGMENT_KEYS | {"token_logprobs", "top_logprobs"} for o in out for s in o["segments"])
    for o in out:
        for s in o["segments"]:
            assert len(s["token_logprobs"]) == len(s["top_logprobs"]) == len(s["tokens"])
    # the first window of every clip again, alone: what its segments were cut from
    _encode_first_windows(m, clips)
    windows = m.decode([[m.rules.sot]] * 2, sample_len=224, logprobs=N)
    cut = 0
    for i, w in enumerate(windows):
        cut += _check_window(m, clips[i], w, [s for s in out[i]["segments"] if s["seek"] == 0])
    assert cut >= 1
    n0 = m.transcribe_batch(clips, logprobs=0, **NO_THRESHOLDS)
    assert all(set(s) == SEGMENT_KEYS | {"token_logprobs"} for o in n0 for s in o["segments"])
    assert [[s["token_logprobs"] for s in o["segments"]] for o in n0] == [[s["token_logprobs"] for s in o["segments"]] for o in out]


def test_a_walk_carries_the_accepted_candidates_lists(model):
    m = model
    clips = _clips()
    kw = dict(temperature=(0.7, 1.0), best_of=2, compression_ratio_threshold=None, **NO_THRESHOLDS)
    m.sample_seed, m._sample_calls = 3, 0
    out = m.transcribe_batch(clips, logprobs=N, **kw)
    walk = m.fallback_walks[0]
    assert walk.clips == [0, 1] and walk.seeks == [0, 0] and all(len(walk.trace[w]) == 1 for w in range(2))
    seed = (3 << 32) + 1
    _encode_first_windows(m, clips)
    for w in range(2):
        rows = m.decode_rows([[m.rules.sot]] * 2, [w] * 2, [2 * w, 2 * w + 1], sample_len=224, temperature=0.7, seed=seed, n_windows=2,
                             logprobs=N)
        acc = walk.accepted[w]
        k = acc["candidate"]
        assert acc["tokens"] == rows[k]["tokens"] and acc["sum_logprob"] == rows[k]["sum_logprob"]
        assert acc["token_logprobs"] == rows[k]["token_logprobs"] and acc["top_logprobs"] == rows[k]["top_logprobs"]
        assert rows[0]["token_logprobs"] != rows[1]["token_logprobs"]            # the candidates are different draws
        _check_window(m, clips[w], rows[k], [s for s in out[w]["segments"] if s["seek"] == 0])
    assert all(s["temperature"] == 0.7 for o in out for s in o["segments"])


def test_a_default_call_is_todays_and_the_opt_in_is_needed(model, ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    m = model
    clips = _clips()
    out = m.transcribe_batch(clips, **NO_THRESHOLDS)
    assert all(set(o) == RESULT_KEYS for o in out) and all(set(s) == SEGMENT_KEYS for o in out for s in o["segments"])
    one = m.transcribe(clips[0], logprobs=None, **NO_THRESHOLDS)
    assert one["tokens"] == out[0]["tokens"] and all(set(s) == SEGMENT_KEYS for s in one["segments"])
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    d = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=8, ctx=ccx_ctx)
    try:
        assert [o["tokens"] for o in d.transcribe_batch(clips, **NO_THRESHOLDS)] == [o["tokens"] for o in out]
        for call in (lambda: d.transcribe_batch(clips, logprobs=N), lambda: d.transcribe(clips[0], logprobs=0)):
            with pytest.raises(ValueError, match="token_logprobs=True"):
                call()
    finally:
        d.close()


def test_load_models_hands_the_opt_in_on(ccx_ctx):
    from clearconverse_amd.models import build_state_dicts, load_models
    sds = build_state_dicts(None, whisper_dims=WhisperDims.mini(2, 128), sep_dims=SepDims(n_layers=2), seed=0)
    models = load_models(None, 0, whisper_batch=2, ctx=ccx_ctx, state_dicts=sds, sep_tokens=60_000, max_crops=16, gate_max_clips=2,
                         whisper_token_logprobs=True)
    try:
        w = models["whisper_model"]
        assert w.token_logprobs is True and all(x.token_logprobs is True for x in models["whisper_models"])
        out = w.transcribe_batch([synthetic_clip(1, 30.0)[:16000 * 4]], logprobs=1, **NO_THRESHOLDS)
        assert all("token_logprobs" in s and "top_logprobs" in s for s in out[0]["segments"])
    finally:
        for k in ("whisper_model", "separator", "embedding_model", "diarization_embedder", "segmentation_vad", "segmentation_diar", "denoiser"):
            models[k].close()
