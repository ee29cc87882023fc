"""-m gpu: RE-SepFormer with 1, 3 and 4 sources (SepDims.n_spk: a mask head of 128 * n_spk rows, sep_decoder_kernel<NSPK>) through
the C ABI vs oracle/sepformer_ref.py (CPU fp32), which is generic in n_spk.  The transformer kernels are the two-source model's.

Tolerance: separated waveforms rel-L2 per utterance over all sources, as tests/test_sepformer_gpu.py measures it.  Bounds are 2.5 x
the worst value measured on an MI355X (profiles/sep_nspk_measured_deviations.json), and never above the 1e-2
SURVEY.md section 8c gives a bf16 stage:
  3 sources, 2 layers, ragged batch   measured 4.141e-3 -> 1e-2     (2.5 x would be 1.04e-2: held at the 1e-2 cap, 2.41 x)
  1 and 4 sources, 1 layer            measured 3.849e-3 -> 9.6e-3
  3 sources, full depth               measured 3.708e-3 -> 9.3e-3
The two-source model measures 3.9e-3 / 4.4e-3 on the same kernels: the mask head's width does not show in the error.
"""
import pytest
import torch

from clearconverse_amd.weights import SepDims, synthetic_sepformer_state_dict
from oracle import sepformer_ref as S
from tests.conftest import within
from tests.test_sepformer_gpu import _mix, _rel

pytestmark = pytest.mark.gpu

BOUND_RAGGED_3, BOUND_ONE_LAYER, BOUND_FULL_3 = 1e-2, 9.6e-3, 9.3e-3
RAGGED = [8000, 5213, 1216, 16 + 8 * 149]       # the lengths of the two-source test: L == 150 exactly and a short clip included


def _separator(ctx, dims, seed, max_tokens=20000, max_utts=8):
    from clearconverse_amd.separator import SepformerSeparator
    sd = synthetic_sepformer_state_dict(dims, seed=seed)
    return sd, SepformerSeparator(dims, sd, max_tokens=max_tokens, max_utts=max_utts, ctx=ctx)


@pytest.fixture(scope="module")
def three(ccx_ctx):
    dims = SepDims(n_layers=2, n_spk=3)
    sd, m = _separator(ccx_ctx, dims, seed=4)
    yield dims, sd, m
    m.close()


def test_three_sources_match_the_oracle_ragged(three):
    dims, sd, m = three
    assert m.n_spk == 3
    mix = _mix(RAGGED)
    got = m.separate_batch(mix, RAGGED).cpu()
    assert got.shape == (len(RAGGED), max(RAGGED), 3) and bool(torch.isfinite(got).all())
    orc = S.SepformerRef(S.SepDims(**dims.__dict__), sd)
    for i, n in enumerate(RAGGED):
        ref = orc.separate(mix[i:i + 1, :n])[0]
        assert ref.shape == (n, 3)
        within("sepformer n_spk=3, 2 layers: separated waveform rel-L2 (ragged batch)", _rel(got[i, :n], ref), BOUND_RAGGED_3, i)
        assert bool((got[i, n:] == 0).all()), i                              # zero past the length, for every source


def test_three_source_rows_are_independent(three):
    dims, sd, m = three
    mix = _mix([4000, 4000])
    both = m.separate_batch(mix).cpu()
    one = m.separate_batch(mix[1:2]).cpu()
    assert both.shape == (2, 4000, 3) and torch.equal(both[1], one[0])
    ragged = m.separate_batch(_mix(RAGGED), RAGGED).cpu()
    alone = m.separate_batch(_mix(RAGGED)[1:2, :RAGGED[1]].contiguous(), [RAGGED[1]]).cpu()      # odd length: an odd out stride alone
    assert torch.equal(ragged[1, :RAGGED[1]], alone[0])


@pytest.mark.parametrize("n_spk", [1, 4])
def test_one_and_four_sources(ccx_ctx, n_spk):
    dims = SepDims(n_layers=1, n_spk=n_spk)
    sd, m = _separator(ccx_ctx, dims, seed=6)
    try:
        lengths = [4000, 1216]
        mix = _mix(lengths)
        got = m.separate_batch(mix, lengths).cpu()
        assert got.shape == (2, 4000, n_spk) and bool(torch.isfinite(got).all())
        orc = S.SepformerRef(S.SepDims(**dims.__dict__), sd)
        for i, n in enumerate(lengths):
            ref = orc.separate(mix[i:i + 1, :n])[0]
            within("sepformer n_spk=1 / 4, 1 layer: separated waveform rel-L2", _rel(got[i, :n], ref), BOUND_ONE_LAYER, (n_spk, i))
            assert bool((got[i, n:] == 0).all())
    finally:
        m.close()


def test_three_sources_full_depth(ccx_ctx):
    dims = SepDims(n_spk=3)                     # the 3-mix sibling of the reference's checkpoint: 8 layers x (2 segment + 1 memory) blocks
    sd, m = _separator(ccx_ctx, dims, seed=9, max_tokens=4000, max_utts=2)
    try:
        mix = _mix([4000])
        got = m.separate_batch(mix).cpu()
        ref = S.SepformerRef(S.SepDims(**dims.__dict__), sd).separate(mix)
        assert got.shape == (1, 4000, 3)
        within("sepformer n_spk=3 FULL depth (8 layers x 3 blocks): separated waveform rel-L2", _rel(got, ref), BOUND_FULL_3)
    finally:
        m.close()


def test_five_sources_are_refused_at_construction(ccx_ctx):
    from clearconverse_amd._lib import CcxError
    from clearconverse_amd.separator import SepformerSeparator
    dims = SepDims(n_layers=1, n_spk=5)
    with pytest.raises(CcxError, match="n_spk"):
        SepformerSeparator(dims, synthetic_sepformer_state_dict(dims, seed=1), max_tokens=2000, max_utts=2, ctx=ccx_ctx)
    with pytest.raises(CcxError, match="n_spk"):
        SepformerSeparator(SepDims(n_layers=1, n_spk=0), {}, max_tokens=2000, max_utts=2, ctx=ccx_ctx)
