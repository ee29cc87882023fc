"""GPU: clip_timestamps and without_timestamps through `transcribe`, and the log-mel launcher behind them.

  * ccx_whisper_logmel_ex with max_frames against oracle/whisper_ref.log_mel_spectrogram, cropped, then pad_or_trim: 80 and 128 mel
    bins, caps of 1, 700 and 3000 frames, a seek above 0.  Bound: the 1e-4 of the existing log-mel tests (tests/test_whisper_gpu.py,
    tests/test_large_kernels_gpu.py).  max_frames = NULL is ccx_whisper_logmel, bit for bit.
  * transcribe(clip_timestamps=[2.0, 9.0, 14.0]) on a 20 s clip, replayed window by window through the reference loop
    (tests/decoding_options_reference.transcribe_loop) with the device's own decode results: seeks, segment bounds, prompts, tokens.
  * the same range given as a crop of the audio: the same mel frames wherever both see the same samples (the clip's normalising
    maximum lies inside the range by construction).
  * transcribe(without_timestamps=True) on a 45 s clip: two segments of 30 s and 15 s, no timestamp token in the text tokens.
  * an instance without the opt-in returns what it returns without the arguments.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import decoding_options_reference as DO
from tests.conftest import within

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
ORULES = R.Rules(suppress=tuple(RULES.suppress))
N_MEL = "clip timestamps: log-mel with max_frames, max abs error"
N_CROP = "clip timestamps: log-mel of the clip range against the cropped audio, max abs difference"


def _model(ccx_ctx, n_mels=80, quiet_timestamps=False, **kw):
    """quiet_timestamps: the (tied) embedding rows of the timestamp ids are zero, so their logits are exactly 0 and some text id
    always stands above them -- a checkpoint that has learnt not to emit timestamps behind <|notimestamps|>, which seeded random
    weights have not (without the timestamp rules nothing bans them: upstream does not either)."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128, n_mels=n_mels)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    if quiet_timestamps:
        sd = dict(sd)
        emb = sd["decoder.token_embedding.weight"].clone()
        emb[RULES.timestamp_begin:] = 0.0
        sd["decoder.token_embedding.weight"] = emb
    return WhisperModel(dims, sd, max_batch=3, ctx=ccx_ctx, max_audio_seconds=50.0, **kw)


@pytest.fixture(scope="module")
def opt_model(ccx_ctx):
    m = _model(ccx_ctx, decoding_options=True)
    yield m
    m.close()


@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_ex_crops_like_pad_or_trim(ccx_ctx, opt_model, n_mels):
    m = opt_model if n_mels == 80 else _model(ccx_ctx, n_mels=128)
    try:
        clip = synthetic_clip(5, 30.0)
        n, seek, caps = len(clip), 300, [1, 700, 3000]
        dev = torch.from_numpy(np.stack([clip] * 3)).cuda()
        mel = m.log_mel(dev, [n] * 3, seek=[seek] * 3, return_mel=True, max_frames=caps).cpu()
        full = R.log_mel_spectrogram(torch.from_numpy(clip), n_mels=n_mels)
        content = n // 160
        for b, cap in enumerate(caps):
            size = min(3000, content - seek, cap)
            ref = R.pad_or_trim(full[:, seek: seek + size], 3000)
            within(N_MEL, float((mel[b] - ref).abs().max()), 1e-4, (n_mels, cap))
            assert float(mel[b][:, size:].abs().max()) == 0.0 if size < 3000 else True      # literal zeros behind the cap
        # NULL is ccx_whisper_logmel; a cap the window never reaches changes nothing either
        plain = m.log_mel(dev, [n] * 3, seek=[seek] * 3, return_mel=True).cpu()
        out = torch.empty_like(plain, device="cuda")
        ns, sk = (C.c_int * 3)(n, n, n), (C.c_int * 3)(seek, seek, seek)
        m.ctx.check(m.lib.ccx_whisper_logmel_ex(m.handle, dev.data_ptr(), dev.shape[1], ns, sk, None, 3, out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "ccx_whisper_logmel_ex")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), plain) and torch.equal(plain[2], mel[2])
        with pytest.raises(Exception) as e:
            m.log_mel(dev, [n] * 3, seek=[seek] * 3, max_frames=[5, -1, 5])
        assert "max_frames[1] = -1" in str(e.value)
    finally:
        if n_mels != 80:
            m.close()


def _loud_inside(lo_s, hi_s, total_s, seed):
    """a clip whose global maximum lies inside [lo_s, hi_s): full level there, a tenth of it elsewhere"""
    clip = synthetic_clip(seed, 30.0)[: int(total_s * 16000)].copy()
    gain = np.full(len(clip), 0.1, dtype=np.float32)
    gain[int(lo_s * 16000): int(hi_s * 16000)] = 1.0
    return clip * gain


def test_transcribe_with_clips_replays_through_the_reference_loop(opt_model, monkeypatch):
    m = opt_model
    clip = _loud_inside(2.0, 9.0, 20.0, 7)
    calls, mels = [], []
    decode, log_mel = m.decode, m.log_mel
    monkeypatch.setattr(m, "decode", lambda prompts, **kw: calls.append((list(map(list, prompts)), decode(prompts, **kw))) or calls[-1][1])
    monkeypatch.setattr(m, "log_mel", lambda a, n, seek=None, **kw: mels.append((list(seek), kw.get("max_frames"))) or log_mel(a, n, seek, **kw))
    out = m.transcribe(clip, initial_prompt="<7000> <7001>", clip_timestamps=[2.0, 9.0, 14.0], no_speech_threshold=None)
    assert len(calls) >= 2 and all(len(p) == 1 for p, _ in calls)
    it = iter(calls)

    def replay(window):
        prompts, res = next(it)
        assert prompts[0] == window["prompt"], (prompts[0], window["prompt"])
        return dict(tokens=res[0]["tokens"], temperature=0.0, avg_logprob=res[0]["avg_logprob"], no_speech_prob=res[0]["no_speech_prob"])

    ref = DO.transcribe_loop(len(clip) // 160, ORULES, m.dims.n_text_ctx, replay, m.tokenizer.decode,
                             m.tokenizer.encode(" <7000> <7001>"), [2.0, 9.0, 14.0], no_speech_threshold=None)
    assert next(it, None) is None                                  # as many windows as the reference walks
    assert [w["seek"] for w in ref["windows"]] == [s for sk, _ in mels for s in sk]
    assert [w["segment_size"] for w in ref["windows"]] == [f for _, mf in mels for f in mf]
    assert ref["windows"][0]["seek"] == 200 and ref["windows"][0]["segment_size"] <= 700
    assert all(200 <= w["seek"] < 900 or 1400 <= w["seek"] < 2000 for w in ref["windows"])
    assert any(w["seek"] >= 1400 for w in ref["windows"])
    assert out["tokens"] == ref["tokens"] and out["segments"] == ref["segments"]
    assert len(out["segments"]) >= 2 and all(s["start"] >= 2.0 for s in out["segments"])


def test_clip_range_equals_the_cropped_audio(opt_model):
    m = opt_model
    clip = _loud_inside(2.0, 9.0, 20.0, 7)
    crop = clip[2 * 16000: 9 * 16000]
    a = m.log_mel(torch.from_numpy(clip[None]).cuda(), [len(clip)], seek=[200], return_mel=True, max_frames=[700]).cpu()[0]
    b = m.log_mel(torch.from_numpy(crop[None]).cuda(), [len(crop)], return_mel=True).cpu()[0]
    # frames 2 .. 697 of the range read the same 400 samples in both (the crop's first and last two frames see its reflected edge)
    within(N_CROP, float((a[:, 2:698] - b[:, 2:698]).abs().max()), 1e-4)
    assert float(a[:, 700:].abs().max()) == 0.0 and float(b[:, 700:].abs().max()) == 0.0


def test_without_timestamps_on_45_seconds(ccx_ctx):
    m = _model(ccx_ctx, quiet_timestamps=True, decoding_options=True)
    try:
        _without_timestamps_on_45_seconds(m)
    finally:
        m.close()


def _without_timestamps_on_45_seconds(m):
    clip = np.concatenate([synthetic_clip(8, 30.0), synthetic_clip(9, 30.0)[: 15 * 16000]])
    out = m.transcribe(clip, without_timestamps=True, no_speech_threshold=None)
    assert [(s["seek"], s["start"], s["end"]) for s in out["segments"]] == [(0, 0.0, 30.0), (3000, 30.0, 45.0)]
    assert len(out["tokens"]) >= 1 and all(t < RULES.timestamp_begin for t in out["tokens"])
    ruled = m.transcribe(clip, no_speech_threshold=None)
    assert any(t >= RULES.timestamp_begin for s in ruled["segments"] for t in s["tokens"])        # the default decode stamps
    assert m.sot_tail == 0 and m.graph_count(True) >= 1                                          # the call left the defaults behind
    with pytest.raises(Exception) as e:
        m.transcribe(clip, without_timestamps=True, hallucination_silence_threshold=2.0)
    assert "without_timestamps" in str(e.value) and "hallucination_silence_threshold" in str(e.value)


def test_an_instance_without_the_opt_in_ignores_the_arguments(ccx_ctx):
    m = _model(ccx_ctx)
    try:
        clip = _loud_inside(2.0, 9.0, 20.0, 7)
        want = m.transcribe(clip)
        got = m.transcribe(clip, without_timestamps=True, prefix="hello there", suppress_blank=False, suppress_tokens="5,6",
                           max_initial_timestamp=None, sample_len=3, clip_timestamps=[2.0, 9.0, 14.0], carry_initial_prompt=True)
        assert got == want and m.graph_count(True) == 0
    finally:
        m.close()
