"""CPU checks of the stressed Whisper weights (tests/stressed_whisper.py) and of the oracle's float64 mode they are judged with.

* The float64 oracle agrees with the float32 one on the plain synthetic weights (the float64 mode changes the arithmetic only).
* Offset stress leaves the model unchanged: float64 logits (decoder_logits and CachedDecoder) and the encoder output of the stressed
  weights equal those of the plain weights to 1e-9 -- so the GPU stress tests judge the stressed model against the same oracle.
* The stress reaches its intended level at EVERY cross_attn_ln input (the rows the X-stream query rounds to bf16 uncentred):
  |mean| / std >= 10 and >= 40 at the two offset levels, max|x| >= 50 x the bulk rms under outlier stress; at mini dims and, for the
  levels the full-size GPU tests use, at full small.en size.
"""
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import stressed_whisper as S
from tests.stressed_whisper import MU, OUTLIER_CHANNELS, OUTLIER_SCALE


def _dims(size):
    return WhisperDims.mini(n_layer=2, n_state=128) if size == "mini" else WhisperDims.small_en()


def _tokens(B=2, T=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(0, 50000, (B, T), generator=g)
    toks[:, 0] = 50257
    return toks


def _xa(dims, B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, dims.n_audio_ctx, dims.n_audio_state, generator=g, dtype=torch.float64)


def _orc(dims, sd, dtype=torch.float64):
    return R.WhisperRef(R.Dims(**dims.__dict__), sd, dtype=dtype)


def _mel(seconds=5.0):
    clip = synthetic_clip(0, 30.0)[: int(16000 * seconds)]
    return R.pad_or_trim(R.log_mel_spectrogram(torch.from_numpy(clip))[:, : len(clip) // 160], 3000)[None]


def test_float64_oracle_matches_float32_oracle():
    dims = _dims("mini")
    sd = synthetic_whisper_state_dict(dims, seed=3)
    toks, xa = _tokens(), _xa(dims)
    o32, o64 = _orc(dims, sd, torch.float32), _orc(dims, sd)
    a, b = o32.decoder_logits(toks, xa.float()), o64.decoder_logits(toks, xa)
    assert a.dtype == torch.float32 and b.dtype == torch.float64
    assert float((a.double() - b).norm() / b.norm()) < 1e-5
    c32, c64 = R.CachedDecoder(o32, xa.float()), R.CachedDecoder(o64, xa)
    s32, s64 = c32.step(toks[:, :5]), c64.step(toks[:, :5])
    s32 = torch.cat([s32, c32.step(toks[:, 5:])], 1); s64 = torch.cat([s64, c64.step(toks[:, 5:])], 1)
    assert s64.dtype == torch.float64
    assert float((s32.double() - s64).norm() / s64.norm()) < 1e-5
    assert float((s64 - b).abs().max()) < 1e-10                     # cached = full recompute, in float64
    mel = _mel()
    e32, e64 = o32.encode(mel), o64.encode(mel)
    assert e64.dtype == torch.float64
    assert float((e32.double() - e64).norm() / e64.norm()) < 1e-5


@pytest.mark.parametrize("level", [10, 40])
def test_offset_stress_leaves_the_model_unchanged(level):
    dims = _dims("mini")
    sd = synthetic_whisper_state_dict(dims, seed=3)
    st = S.offset_state_dict(sd, dims, MU[level], MU[level])
    assert not torch.equal(st["decoder.positional_embedding"], sd["decoder.positional_embedding"])
    assert torch.equal(sd["decoder.positional_embedding"], synthetic_whisper_state_dict(dims, seed=3)["decoder.positional_embedding"])
    toks, xa = _tokens(), _xa(dims)
    plain, stressed = _orc(dims, sd), _orc(dims, st)
    ref = plain.decoder_logits(toks, xa)
    scale = max(1.0, float(ref.abs().max()))
    assert float((stressed.decoder_logits(toks, xa) - ref).abs().max()) < 1e-9 * scale
    cached = R.CachedDecoder(stressed, xa)
    got = torch.cat([cached.step(toks[:, :4])] + [cached.step(toks[:, t:t + 1]) for t in range(4, toks.shape[1])], 1)
    assert float((got - ref).abs().max()) < 1e-9 * scale
    mel = _mel()
    e_ref = plain.encode(mel)
    assert float((stressed.encode(mel) - e_ref).abs().max()) < 1e-9 * max(1.0, float(e_ref.abs().max()))


@pytest.mark.parametrize("size,levels", [("mini", (10, 40)), ("full", (40,))])
def test_stress_levels_at_every_cross_attention_layernorm(size, levels):
    dims = _dims(size)
    sd = synthetic_whisper_state_dict(dims, seed=3 if size == "mini" else 0)
    toks, xa = _tokens(), _xa(dims)
    names = [f"decoder.blocks.{l}.cross_attn_ln" for l in range(dims.n_text_layer)]
    base = S.residual_stats(sd, dims, toks, xa)
    assert set(names) <= set(base) and "decoder.ln" in base
    assert max(float(base[n][0].max()) for n in names) < 0.5            # the plain weights: near-zero-mean rows
    for level in levels:
        st = S.residual_stats(S.offset_state_dict(sd, dims, MU[level], MU[level]), dims, toks, xa)
        for n in names:
            assert float(st[n][0].min()) >= level, (size, level, n, float(st[n][0].min()))
    st = S.residual_stats(S.outlier_state_dict(sd, dims, OUTLIER_CHANNELS, OUTLIER_SCALE[size]), dims, toks, xa)
    for n in names:
        assert float(st[n][1].min()) >= 50, (size, n, float(st[n][1].min()))
        assert float(st[n][1].max()) <= 150, (size, n, float(st[n][1].max()))
        assert float(st[n][0].max()) < 0.5, (size, n)                   # outliers alone: the row mean stays near 0


def test_stress_helpers_are_deterministic():
    dims = _dims("mini")
    sd = synthetic_whisper_state_dict(dims, seed=3)
    a, b = S.offset_state_dict(sd, dims, 10.0, 5.0), S.offset_state_dict(sd, dims, 10.0, 5.0)
    c, d = S.outlier_state_dict(sd, dims, OUTLIER_CHANNELS, 70.0), S.outlier_state_dict(sd, dims, OUTLIER_CHANNELS, 70.0)
    assert all(torch.equal(a[k], b[k]) and torch.equal(c[k], d[k]) for k in sd)
    assert float((a["encoder.positional_embedding"] - sd["encoder.positional_embedding"]).mean()) == pytest.approx(5.0)
    assert float((a["decoder.blocks.1.mlp.2.bias"] - sd["decoder.blocks.1.mlp.2.bias"]).mean()) == pytest.approx(2.5)
    assert float(c["decoder.positional_embedding"][0, 50] - sd["decoder.positional_embedding"][0, 50]) == pytest.approx(-70.0)
