"""Whisper's `large` family on the host side (no GPU): the three presets, the 128-bin filterbank, synthetic weights at 128 mels and a
checkpoint file with the large-v3-turbo dims through the loader."""
import numpy as np
import torch

from clearconverse_amd.audio import mel_filterbank
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, find_whisper_checkpoint, synthetic_whisper_state_dict
from oracle import whisper_ref as R


def test_large_presets():
    want = dict(large=(80, 51865, 32, 99), large_v3=(128, 51866, 32, 100), large_v3_turbo=(128, 51866, 4, 100))
    for name, (n_mels, n_vocab, n_text_layer, n_lang) in want.items():
        d = getattr(WhisperDims, name)()
        assert (d.n_mels, d.n_vocab, d.n_text_layer, d.n_audio_layer) == (n_mels, n_vocab, n_text_layer, 32), name
        assert d.n_audio_state == d.n_text_state == 1280 and d.n_audio_head == d.n_text_head == 20, name
        assert d.n_audio_state // d.n_audio_head == 64 and d.n_audio_ctx == 1500 and d.n_text_ctx == 448, name
        assert d.is_multilingual and d.num_languages == n_lang, name
        r = DecodeRules.for_dims(d)
        assert r.is_multilingual and r.num_languages == n_lang and len(r.languages) == n_lang, name
        assert r.timestamp_begin + 1501 == n_vocab, name
    # the ids of the 51866-token vocabulary: one more language token, everything behind it one higher than in 51865
    r3, r2 = DecodeRules.for_dims(WhisperDims.large_v3()), DecodeRules.for_dims(WhisperDims.large())
    assert (r3.eot, r3.sot, r3.language_begin) == (r2.eot, r2.sot, r2.language_begin) == (50257, 50258, 50259)
    assert (r3.translate, r3.transcribe, r3.sot_lm, r3.sot_prev, r3.no_speech, r3.no_timestamps, r3.timestamp_begin) == \
        (50359, 50360, 50361, 50362, 50363, 50364, 50365)
    assert r3.timestamp_begin == r2.timestamp_begin + 1 and r3.no_speech == r2.no_speech + 1
    assert r3.sot_sequence() == [50258, 50259, 50360]
    # the presets are fresh objects: changing one leaves the next call's alone
    d = WhisperDims.large_v3_turbo()
    d.n_text_layer = 2
    assert WhisperDims.large_v3_turbo().n_text_layer == 4 and WhisperDims.large_v3().n_text_layer == 32


def test_mini_takes_n_mels_and_keeps_its_positional_meaning():
    d = WhisperDims.mini(n_mels=128)
    assert d.n_mels == 128 and (d.n_audio_layer, d.n_audio_state, d.n_vocab) == (2, 128, 51864)
    assert WhisperDims.mini(2, 128) == WhisperDims.mini(n_layer=2, n_state=128, n_vocab=51864, n_mels=80)
    assert WhisperDims.mini(2, 128).n_mels == 80
    assert WhisperDims.mini(1, 256, 51866) == WhisperDims.mini(n_layer=1, n_state=256, n_vocab=51866)
    big = WhisperDims.mini(n_layer=2, n_state=1280, n_vocab=51866, n_mels=128)
    assert big.n_audio_head == big.n_text_head == 20 and big.n_mels == 128


def test_mel_filterbank_128_equals_the_oracle():
    ours = mel_filterbank(128)
    ref = R.mel_filters(128)
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert ours.shape == ref.shape == (128, 201)
    assert ours.dtype == np.float32
    assert np.array_equal(ours, ref.astype(np.float32))
    # narrower than the 80-bin filters: every row is populated, none spans more bins than the widest 80-bin row
    assert (ours > 0).sum(1).min() >= 1 and (ours > 0).sum(1).max() <= (mel_filterbank(80) > 0).sum(1).max()


def test_synthetic_state_dict_at_128_mels():
    dims = WhisperDims.mini(n_layer=1, n_state=128, n_vocab=51866, n_mels=128)
    sd = synthetic_whisper_state_dict(dims, seed=5)
    assert tuple(sd["encoder.conv1.weight"].shape) == (128, 128, 3)
    assert tuple(sd["encoder.conv2.weight"].shape) == (128, 128, 3)
    assert tuple(sd["decoder.token_embedding.weight"].shape) == (51866, 128)
    assert tuple(sd["encoder.positional_embedding"].shape) == (1500, 128)
    # asymmetric depths (turbo): encoder and decoder blocks are counted apart
    dims.n_audio_layer, dims.n_text_layer = 2, 1
    sd = synthetic_whisper_state_dict(dims, seed=5)
    assert "encoder.blocks.1.mlp.2.weight" in sd and "decoder.blocks.0.cross_attn.out.weight" in sd
    assert "decoder.blocks.1.attn.query.weight" not in sd and "encoder.blocks.2.attn.query.weight" not in sd
    # the oracle builds from it
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    mel = torch.zeros(1, 128, 3000)
    assert tuple(orc.encode(mel).shape) == (1, 1500, 128)


def test_large_v3_turbo_checkpoint_round_trips(tmp_path):
    """`<cache>/whisper/large-v3-turbo.pt` = {"dims", "model_state_dict"}: a file with the family's width, mel bins and vocabulary
    (layer counts shrunk to keep it small) comes back with exactly these dims and tensors"""
    dims = WhisperDims.large_v3_turbo()
    dims.n_audio_layer, dims.n_text_layer = 1, 1
    # the checkpoint's own tensors (shapes of the real file); the embedding is cut down by building it narrow and widening with zeros
    small = WhisperDims.mini(n_layer=1, n_state=128, n_vocab=51866, n_mels=128)
    sd = {k: v.to(torch.float16) for k, v in synthetic_whisper_state_dict(small, seed=9).items() if "embedding" not in k}
    sd["encoder.conv1.weight"] = torch.randn(1280, 128, 3, generator=torch.Generator().manual_seed(1)).to(torch.float16)
    sd["decoder.ln.weight"] = torch.ones(1280, dtype=torch.float16)
    (tmp_path / "whisper").mkdir()
    torch.save({"dims": dict(dims.__dict__), "model_state_dict": sd}, tmp_path / "whisper" / "large-v3-turbo.pt")
    got = find_whisper_checkpoint("large-v3-turbo", str(tmp_path))
    assert got is not None
    d, tensors = got
    assert d == dims and d.n_mels == 128 and d.n_audio_state == 1280 and d.n_vocab == 51866
    assert set(tensors) == set(sd)
    for k, v in sd.items():
        assert tensors[k].dtype == torch.float32 and torch.equal(tensors[k], v.float()), k
    assert find_whisper_checkpoint("large-v3", str(tmp_path)) is None
