"""CPU: the FP8 encoder-output format (include/ccx.h "FP8 encoder-output stream") as tests/xa_fp8_reference.py states it -- by hand on
integer and bit operations, and on torch.frexp with the torch.float8_e4m3fn cast -- the two compared on seeded data and against blocks
worked by hand; and the Python surface of the opt-in without a GPU: the constructor's refusal before any library call, and the ctypes
mirror against include/ccx.h."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import xa_fp8_reference as R

ROOT = Path(__file__).resolve().parent.parent


def _bits(t):
    return t.contiguous().view(torch.int32)


def _seeded(seed, shape, spread):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * torch.exp2(torch.randn(*shape[:-1], 1, generator=g) * spread)
    return x.to(torch.bfloat16).to(torch.float32)


@pytest.mark.parametrize("spread", [0.0, 3.0, 12.0])
def test_the_two_statements_agree_on_seeded_data(spread):
    x = _seeded(5 + int(spread), (40, 768), spread)
    x[3, 64:96] = 0.0                                   # an all-zero block among them
    x[7, 100] = x[7, 96:128].abs().max() * 1024.0       # and an outlier
    codes, e, xhat = R.quantise_bits(R.bf16_bits(x))
    codes_t, e_t, xhat_t = R.quantise_torch(x)
    assert np.array_equal(e, e_t.numpy())
    assert np.array_equal(codes, codes_t.numpy())
    assert torch.equal(_bits(R.bits_to_f32(xhat).reshape(x.shape)), _bits(xhat_t))


@pytest.mark.parametrize("name", list(R.HAND_BLOCKS))
def test_blocks_worked_by_hand(name):
    x, want, e_want = (torch.tensor(v, dtype=torch.float32) if isinstance(v, list) else v for v in R.HAND_BLOCKS[name])
    assert torch.equal(x.to(torch.bfloat16).to(torch.float32), x), "the hand block must hold bf16 values"
    codes, e, xhat = R.quantise_bits(R.bf16_bits(x[None]))
    assert int(e[0, 0]) == e_want
    got = R.bits_to_f32(xhat)[0]
    assert torch.equal(_bits(got), _bits(want)), (got, want)          # bit for bit: the sign of a flushed negative value stays
    _, e_t, xhat_t = R.quantise_torch(x[None])
    assert int(e_t[0, 0]) == e_want and torch.equal(_bits(xhat_t[0]), _bits(want))
    assert int(codes.astype(np.int32).__and__(0x7F).max()) <= 0x7E                      # never the NaN code


def test_rne_ties_by_name():
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1], x[0, 2] = 256.0, 1.0625, 1.1875
    xh = R.xhat_of(x)
    assert float(xh[0, 1]) == 1.0 and float(xh[0, 2]) == 1.25 and float(xh[0, 0]) == 256.0


def test_outlier_flushes_the_small_values():
    """expected, not a defect: one value 2^10 above the rest takes the block's scale with it"""
    x, want, _ = R.HAND_BLOCKS["outlier"]
    xh = R.xhat_of(torch.tensor(x)[None])[0]
    small = [i for i, v in enumerate(x) if 0 < abs(v) < 2.0 ** -8]
    assert len(small) >= 20 and all(float(xh[i]) == 0.0 for i in small)
    assert float(xh[3]) == 1024.0 and float(xh[4]) == 1.0


def test_scaled_values_stay_within_448_and_the_exponent_within_its_clamp():
    x = _seeded(21, (64, 512), 10.0)
    blk = x.reshape(64, 16, 32)
    _, e, _ = R.quantise_bits(R.bf16_bits(x))
    assert e.min() >= R.EMIN and e.max() <= R.EMAX
    scaled = torch.ldexp(blk, -torch.from_numpy(e.astype(np.int32))[..., None])
    free = torch.from_numpy((e > R.EMIN) & (e < R.EMAX))
    assert bool(free.any())
    assert float(scaled.abs().amax(dim=-1)[free].max()) <= 448.0
    # the smallest such e: one less would not hold amax
    assert float(scaled.abs().amax(dim=-1)[free].min()) > 224.0
    # clamped from below the bound holds a fortiori; clamped from above the CODE clamp takes over
    x = torch.tensor(R.HAND_BLOCKS["clamp_high"][0])[None]
    codes, e, _ = R.quantise_bits(R.bf16_bits(x))
    assert int(e[0, 0]) == R.EMAX and int(codes[0, 0]) == 0x7E and int(codes[0, 1]) == 0xFE


def test_xhat_is_bf16_and_a_fixed_point():
    x = _seeded(33, (32, 768), 6.0)
    for name, (blk, _, _) in R.HAND_BLOCKS.items():
        x[len(name) % 32, 0:32] = torch.tensor(blk)
    xh = R.xhat_of(x)
    assert torch.isfinite(xh).all()
    assert torch.equal(_bits(xh.to(torch.bfloat16).to(torch.float32)), _bits(xh))      # float -> bf16 -> float unchanged
    assert torch.equal(_bits(R.xhat_of(xh)), _bits(xh))                                # quantise(xhat) == xhat
    _, _, xh_t = R.quantise_torch(xh)
    assert torch.equal(_bits(xh_t), _bits(xh))


def test_hand_places_cover_the_tiles_and_do_not_overlap():
    for S, D in ((16, 128), (37, 256), (100, 384), (1499, 768), (1500, 768)):
        places = R.hand_places(S, D)
        assert len({p[:3] for p in places}) == len(places)
        keys = {p[1] for p in places}
        nt = (S + 15) // 16
        assert {0, min(15, S - 1), 16 * (nt - 1), S - 1} <= keys and max(keys) == S - 1
        assert {p[2] for p in places} == {0, D // 32 - 1} and {p[3] for p in places} == set(R.HAND_BLOCKS)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_constructor_refuses_before_any_library_call(monkeypatch):
    from clearconverse_amd import _lib, whisper
    from clearconverse_amd.weights import WhisperDims

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "Context", boom)
    monkeypatch.setattr(_lib, "load", boom)
    for dims, word in ((WhisperDims.large(), "1280"), (WhisperDims.large_v3_turbo(), "1280"), (WhisperDims.medium(), "1024")):
        with pytest.raises(_lib.CcxError) as e:
            whisper.WhisperModel(dims, {}, cross_fp8=True)
        assert "cross_fp8" in str(e.value) and word in str(e.value), str(e.value)
    uneven = WhisperDims.mini()
    uneven.n_text_state, uneven.n_text_head = 256, 4
    with pytest.raises(_lib.CcxError) as e:
        whisper.WhisperModel(uneven, {}, cross_fp8=True)
    assert "differs" in str(e.value)
    monkeypatch.setenv("CCX_CROSS_X", "0")
    with pytest.raises(_lib.CcxError) as e:
        whisper.WhisperModel(WhisperDims.mini(), {}, cross_fp8=True)
    assert "CCX_CROSS_X=0" in str(e.value)


def test_refusal_rule_and_defaults():
    import inspect

    from clearconverse_amd import models, whisper
    from clearconverse_amd.weights import WhisperDims
    for dims in (WhisperDims.mini(), WhisperDims.mini(n_state=256), WhisperDims.tiny(), WhisperDims.base(), WhisperDims.small_en()):
        assert whisper.cross_fp8_refusal(dims) is None, dims
    assert whisper.cross_fp8_refusal(WhisperDims.large_v3()) is not None
    assert inspect.signature(whisper.WhisperModel.__init__).parameters["cross_fp8"].default is False
    assert inspect.signature(models.load_models).parameters["whisper_cross_fp8"].default is False
    assert whisper.WhisperModel.cross_fp8 is False
    doc = whisper.WhisperModel.__init__.__doc__
    assert "cross_fp8" in doc and "NOT measured" in doc


def test_ctypes_mirror_matches_the_header():
    import ctypes as C

    from clearconverse_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ccx.h").read_text(), flags=re.S)
    want = {"ccx_whisper_set_cross_fp8": None, "ccx_whisper_cross_fp8": None, "ccx_cross_attention_xa_fp8": None}
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
    # the operator: ccx_cross_attention_xa's arguments, then xhat_out_dev, then the stream
    base = _lib.PROTOTYPES["ccx_cross_attention_xa"][1]
    assert _lib.PROTOTYPES["ccx_cross_attention_xa_fp8"][1] == base[:-1] + [C.c_void_p] + base[-1:]
    assert want["ccx_cross_attention_xa_fp8"][-2].endswith("xhat_out_dev")
    # the format rule stands in the header, word for word testable
    head = (ROOT / "include" / "ccx.h").read_text()
    for phrase in ("448 * 2^e", "[-64, 64]", "e + 127", "round to nearest even", "NaN and Inf are NOT handled"):
        assert phrase in head, phrase
