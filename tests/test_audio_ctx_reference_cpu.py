"""CPU: the reduced audio context without a GPU -- its definition on the oracle (tests/audio_ctx_reference.py), the context policy
(clearconverse_amd/audio_ctx.py), the Python surface's refusals and defaults, and the ctypes mirrors of the new entry points."""
import re
from pathlib import Path

import pytest
import torch

from tests import audio_ctx_reference as A

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ref_and_mel():
    from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
    from oracle import whisper_ref as R
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=5)
    ref = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    g = torch.Generator().manual_seed(9)
    mel = torch.randn(3, dims.n_mels, 3000, generator=g) * 0.5
    mel[1, :, 900:] = -1.0          # a padded tail, as pad_or_trim on a normalised log-mel leaves it
    mel[2, :, 130:] = -1.0
    return ref, mel


# ---------------------------------------------------------------------------------------------------------------- the definition
def test_full_context_is_the_oracles_encode_op_for_op(ref_and_mel):
    ref, mel = ref_and_mel
    assert torch.equal(A.encode_ctx(ref, mel[:2], 1500), ref.encode(mel[:2]))


def test_reduced_context_is_not_the_truncated_full_encode(ref_and_mel):
    """the deviation from upstream is real: the first 512 rows of the full encode differ from the encode at 512 positions"""
    ref, mel = ref_and_mel
    full, red = ref.encode(mel[1:2])[0, :512], A.encode_ctx(ref, mel[1:2], 512)[0]
    assert red.shape == (512, ref.dims.n_audio_state)
    assert float((full - red).abs().max()) > 1e-3


def test_masked_in_a_batch_equals_truncated_alone(ref_and_mel):
    """what the library runs (one batch at max(n) rows, keys masked per window) against the definition (each window on its own):
    float32 on both sides, so equal to the rounding of a softmax over a few hundred keys"""
    ref, mel = ref_and_mel
    n = [200, 512, 65]
    alone, batch = A.encode_ctx(ref, mel, n), A.encode_ctx_masked(ref, mel, n)
    for b, k in enumerate(n):
        assert alone[b].shape == batch[b].shape == (k, ref.dims.n_audio_state)
        assert float((alone[b] - batch[b]).abs().max()) < 2e-5, b
    xa = A.padded_xa(alone, 1500)
    assert xa.shape == (3, 1500, ref.dims.n_audio_state) and not bool(xa[2, 65:].any()) and torch.equal(xa[2, :65], alone[2])


# ---------------------------------------------------------------------------------------------------------------- the policy
def test_positions_for_by_hand():
    from clearconverse_amd.audio_ctx import positions_for
    # ceil(F / 2) + 50 positions, rounded up to 64s, clamped to [64, 1500]
    assert positions_for(3000) == 1500          # 1550 -> 1600 -> clamp
    assert positions_for(900) == 512            # 500 -> 512
    assert positions_for(600) == 384            # 350 -> 384
    assert positions_for(10) == 64              # 55 -> 64
    assert positions_for(0) == 64
    assert positions_for(29) == 128             # ceil(29 / 2) = 15, + 50 = 65: one past a granule
    assert positions_for(28) == 64              # 14 + 50 = 64: exactly one
    assert positions_for(900, margin_s=0.0) == 512 and positions_for(900, margin_s=2.0) == 576
    assert positions_for(900, granule=1) == 500 and positions_for(10, floor=100) == 100
    assert positions_for(900, n_audio_ctx=400) == 400
    prev = 0
    for f in range(0, 3001):
        p = positions_for(f)
        assert 64 <= p <= 1500 and p >= prev and (p % 64 == 0 or p == 1500) and (p == 1500 or p >= (f + 1) // 2 + 50)
        prev = p
    for bad in (dict(content_frames=-1), dict(content_frames=5, margin_s=-0.5), dict(content_frames=5, granule=0),
                dict(content_frames=5, floor=2000)):
        with pytest.raises(ValueError):
            positions_for(**bad)
    assert "POLICY, not" in positions_for.__doc__


def test_settings(monkeypatch):
    from clearconverse_amd import audio_ctx as P
    assert P.parse_setting(None) is None and P.parse_setting("auto") == "auto" and P.parse_setting(" AUTO ") == "auto"
    assert P.parse_setting(64) == 64 and P.parse_setting(1500) == 1500 and P.parse_setting("256") == 256
    for bad in (63, 1501, 0, -5, 3.5, True, "full", "fast", [64]):
        with pytest.raises(ValueError):
            P.parse_setting(bad)
    assert P.context_of(None, 100) == 1500 and P.context_of("auto", 600) == 384 and P.context_of(200, 3000) == 200
    for env, want in ((None, None), ("", None), ("0", None), ("off", None), ("auto", "auto"), ("320", 320)):
        if env is None:
            monkeypatch.delenv("CCX_AUDIO_CTX", raising=False)
        else:
            monkeypatch.setenv("CCX_AUDIO_CTX", env)
        assert P.from_environment() == want, env
    monkeypatch.setenv("CCX_AUDIO_CTX", "7")
    with pytest.raises(ValueError):
        P.from_environment()


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_constructor_refuses_before_any_library_call(monkeypatch):
    from clearconverse_amd import _lib, whisper
    from clearconverse_amd.weights import WhisperDims

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "Context", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.delenv("CCX_AUDIO_CTX", raising=False)
    for dims, word in ((WhisperDims.large(), "1280"), (WhisperDims.large_v3_turbo(), "1280"), (WhisperDims.medium(), "1024")):
        for val in ("auto", 256):
            with pytest.raises(_lib.CcxError) as e:
                whisper.WhisperModel(dims, {}, audio_ctx=val)
            assert "audio_ctx" in str(e.value) and word in str(e.value), str(e.value)
    uneven = WhisperDims.mini()
    uneven.n_text_state, uneven.n_text_head = 256, 4
    with pytest.raises(_lib.CcxError) as e:
        whisper.WhisperModel(uneven, {}, audio_ctx="auto")
    assert "differs" in str(e.value)
    for bad in (63, 1501, "fast", 2.5):
        with pytest.raises(ValueError):
            whisper.WhisperModel(WhisperDims.mini(), {}, audio_ctx=bad)
    monkeypatch.setenv("CCX_CROSS_X", "0")
    with pytest.raises(_lib.CcxError) as e:
        whisper.WhisperModel(WhisperDims.mini(), {}, audio_ctx="auto")
    assert "CCX_CROSS_X=0" in str(e.value) and "key count per sequence" in str(e.value)


def test_refusal_rule_and_defaults():
    import inspect

    from clearconverse_amd import models, whisper
    from clearconverse_amd.weights import WhisperDims
    for dims in (WhisperDims.mini(), WhisperDims.mini(n_state=256), WhisperDims.tiny(), WhisperDims.base(), WhisperDims.small_en()):
        assert whisper.audio_ctx_refusal(dims) is None, dims
    assert whisper.audio_ctx_refusal(WhisperDims.large_v3()) is not None
    assert inspect.signature(whisper.WhisperModel.__init__).parameters["audio_ctx"].default is None
    assert inspect.signature(whisper.WhisperModel.encode).parameters["audio_ctx"].default is None
    assert inspect.signature(whisper.WhisperModel.transcribe).parameters["audio_ctx"].default is None
    assert inspect.signature(whisper.WhisperModel.transcribe_batch).parameters["audio_ctx"].default is None
    assert inspect.signature(models.load_models).parameters["whisper_audio_ctx"].default is None
    assert whisper.WhisperModel.audio_ctx is None
    doc = whisper.WhisperModel.__init__.__doc__
    assert "audio_ctx" in doc and "NOT upstream's arithmetic" in doc and "NOT measured" in doc


def test_ctypes_mirror_matches_the_header():
    import ctypes as C

    from clearconverse_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ccx.h").read_text(), flags=re.S)
    want = dict.fromkeys(["ccx_whisper_set_audio_ctx", "ccx_whisper_audio_ctx", "ccx_whisper_encode_ctx", "ccx_enc_attention_keys",
                          "ccx_cross_attention_xa_keys", "ccx_cross_attention_xa_fp8_keys"])
    for name in want:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"include/ccx.h does not declare {name}"
        want[name] = [a.strip() for a in m.group(1).split(",")]
    for name, args in want.items():
        res, proto = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(proto) == len(args), (name, args)
        for a, t in zip(args, proto):
            assert (t is C.c_void_p) == ("*" in a), (name, a)
            if "*" not in a:
                assert a.startswith("int ") and t is C.c_int, (name, a)
    # each sibling: its plain operator's arguments with the counts in front of the outputs / the stream
    base = _lib.PROTOTYPES["ccx_cross_attention_xa"][1]
    assert _lib.PROTOTYPES["ccx_cross_attention_xa_keys"][1] == base[:-2] + [C.c_void_p] + base[-2:]
    assert want["ccx_cross_attention_xa_keys"][-3].endswith("n_keys_host")
    base8 = _lib.PROTOTYPES["ccx_cross_attention_xa_fp8"][1]
    assert _lib.PROTOTYPES["ccx_cross_attention_xa_fp8_keys"][1] == base8[:-3] + [C.c_void_p] + base8[-3:]
    assert want["ccx_cross_attention_xa_fp8_keys"][-4].endswith("n_keys_host")
    enc = _lib.PROTOTYPES["ccx_enc_attention"][1]
    assert _lib.PROTOTYPES["ccx_enc_attention_keys"][1] == enc[:-1] + [C.c_void_p] + enc[-1:]
    assert want["ccx_enc_attention_keys"][-2].endswith("n_keys_host")
    assert _lib.PROTOTYPES["ccx_whisper_encode_ctx"][1] == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert want["ccx_whisper_encode_ctx"][2].endswith("n_ctx")
    # the deviation from upstream stands in the header
    head = (ROOT / "include" / "ccx.h").read_text()
    for phrase in ("NOT upstream's arithmetic", "[64, n_audio_ctx]", "resets", "slot stride of n_audio_ctx rows"):
        assert phrase in head, phrase
