"""GPU: the reduced audio context through `transcribe` / `transcribe_batch` (WhisperModel(audio_ctx="auto")), at the mini dims: clips of
2, 9, 30 and 45 s.
  * every result carries `audio_ctx`, one context per window in order, equal to `audio_ctx.positions_for` of the content frames the
    window staged (recorded at `log_mel`);
  * audio_ctx="full" on the opted-in instance is token-identical to an instance without the opt-in on the same cross-attention path;
  * a batch call reports what the single calls report; `word_timestamps=True` runs on a word_alignment instance;
  * `load_models(whisper_audio_ctx=)` hands the setting on."""
import numpy as np
import pytest

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.audio_ctx import positions_for
from clearconverse_amd.weights import SepDims, WhisperDims, synthetic_whisper_state_dict

pytestmark = pytest.mark.gpu

SECONDS = [2.0, 9.0, 30.0, 45.0]


def _clip(i, seconds):
    reps = int(np.ceil(seconds / 30.0))
    return np.concatenate([synthetic_clip(40 + i + 7 * k, 30.0) for k in range(reps)])[: int(seconds * 16000)]


@pytest.fixture(scope="module")
def pair(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, audio_ctx="auto", word_alignment=True, max_audio_seconds=60.0)
    d = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, word_alignment=True, max_audio_seconds=60.0)
    yield m, d
    m.close(); d.close()


def _recorded(m, monkeypatch):
    """every log_mel call's staged content frames, in order"""
    seen, real = [], m.log_mel

    def log_mel(*a, **k):
        out = real(*a, **k)
        seen.append(list(m._staged_frames))
        return out
    monkeypatch.setattr(m, "log_mel", log_mel)
    return seen


def test_reported_contexts_are_the_policy_per_window(pair, monkeypatch):
    m, d = pair
    clips = [_clip(i, s) for i, s in enumerate(SECONDS)]
    seen = _recorded(m, monkeypatch)
    single = []
    for c in clips:
        del seen[:]
        r = m.transcribe(c)
        assert m.last_cross_path == "xa_stream"
        frames = [f[0] for f in seen]                       # one window per log_mel call
        assert r["audio_ctx"] == [positions_for(f) for f in frames] and len(frames) >= 1
        assert isinstance(r["text"], str) and isinstance(r["segments"], list)
        single.append(r)
    # by hand: 2 s = 200 frames -> 150 -> 192; 9 s = 900 frames -> 500 -> 512; a whole first window -> 1500
    assert single[0]["audio_ctx"] == [192] and single[1]["audio_ctx"] == [512]
    assert single[2]["audio_ctx"][0] == 1500 and single[3]["audio_ctx"][0] == 1500 and len(single[3]["audio_ctx"]) >= 2
    assert single[3]["audio_ctx"][-1] < 1500               # the last window of 45 s holds less than 30 s
    # the four as one batch: a window's numbers do not depend on its batch mates on the X-stream path
    batch = m.transcribe_batch(clips)
    for a, b in zip(single, batch):
        assert a["audio_ctx"] == b["audio_ctx"] and a["tokens"] == b["tokens"]
    # a fixed context for the call
    fixed = m.transcribe(clips[1], audio_ctx=640)
    assert fixed["audio_ctx"] == [640]


def test_full_is_the_default_instance(pair, monkeypatch):
    m, d = pair
    clips = [_clip(i, s) for i, s in enumerate(SECONDS)]
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")        # the opted-in instance's path, on the default instance
    want = d.transcribe_batch(clips)
    assert d.last_cross_path == "xa_stream"
    monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS")
    got = m.transcribe_batch(clips, audio_ctx="full")
    assert m.last_cross_path == "xa_stream"
    for g, w in zip(got, want):
        assert "audio_ctx" not in w and set(g["audio_ctx"]) == {1500}
        assert g["tokens"] == w["tokens"] and g["text"] == w["text"] and g["segments"] == w["segments"]
    auto = m.transcribe_batch(clips)
    assert [r["audio_ctx"][0] for r in auto] == [192, 512, 1500, 1500]
    assert any(len(r["tokens"]) > 0 for r in got)


def test_word_timestamps_run_on_reduced_windows(pair):
    m, d = pair
    clips = [_clip(i, s) for i, s in enumerate(SECONDS[:3])]
    out = m.transcribe_batch(clips, word_timestamps=True)
    # (with words `seek` follows the last aligned word, so a clip may take more windows than without: the first is what it was)
    assert [r["audio_ctx"][0] for r in out] == [192, 512, 1500]
    for r in out:
        assert all(64 <= c <= 1500 and (c % 64 == 0 or c == 1500) for c in r["audio_ctx"])
        for s in r["segments"]:
            assert "words" in s
            for w in s["words"]:
                assert np.isfinite(w["start"]) and np.isfinite(w["end"]) and w["end"] >= w["start"]


def test_load_models_hands_the_setting_on(ccx_ctx):
    from clearconverse_amd.models import build_state_dicts, load_models
    sds = build_state_dicts(None, whisper_dims=WhisperDims.mini(2, 128), sep_dims=SepDims(n_layers=2), seed=0)
    models = load_models(None, 0, whisper_batch=2, ctx=ccx_ctx, state_dicts=sds, sep_tokens=60_000, max_crops=16, gate_max_clips=2,
                         whisper_audio_ctx="auto")
    try:
        w = models["whisper_model"]
        assert w.audio_ctx == "auto" and all(x.audio_ctx == "auto" for x in models["whisper_models"])
        out = w.transcribe_batch([synthetic_clip(1, 30.0)[:16000 * 4], synthetic_clip(2, 30.0)[:16000 * 2]])
        assert [o["audio_ctx"] for o in out] == [[256], [192]]
    finally:
        for k in ("whisper_model", "separator", "embedding_model", "diarization_embedder", "segmentation_vad", "segmentation_diar", "denoiser"):
            models[k].close()
