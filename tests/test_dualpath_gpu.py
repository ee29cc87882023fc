"""GPU: the dual-path SepFormer handle (csrc/dualpath.hip through clearconverse_amd.separator.DualPathSeparator) against the fp64
restatement of tests/dualpath_reference.py, bf16-mirrored, at d_model 256: relative L2 of every utterance's sources below
BOUND_MODEL (2.5 x the worst measured on an MI355X; every mutation of the reference moves the output by 4 x that bound or more,
tests/test_dualpath_reference_cpu.py)."""
import functools

import pytest
import torch

from tests import dualpath_reference as R
from tests.conftest import within

pytestmark = pytest.mark.gpu
N_MODEL = "dualpath model: rel-L2 of an utterance's sources vs the mirrored fp64 reference"


def _dims(K, n_spk, n_layers=1, d_ffn=64):
    return R.Dims(n_layers=n_layers, n_blocks=2, d_ffn=d_ffn, segment=K, n_spk=n_spk)


@functools.lru_cache(maxsize=None)
def _weights(K, n_spk, n_layers=1, d_ffn=64):
    return R.case_state_dict(_dims(K, n_spk, n_layers, d_ffn), 11)


def _separator(ctx, K, n_spk, n_layers=1, d_ffn=64, max_tokens=8000, max_utts=8):
    from clearconverse_amd.separator import DualPathSeparator
    from clearconverse_amd.weights import DualPathDims
    d = _dims(K, n_spk, n_layers, d_ffn)
    return DualPathSeparator(DualPathDims(**d.__dict__), _weights(K, n_spk, n_layers, d_ffn), max_tokens=max_tokens, max_utts=max_utts, ctx=ctx)


def _batch(K):
    """a ragged batch: T = 16 (one frame), a length whose frames leave gap = K, about 2000 samples, and the short utterances of the
    CPU mutation test (the same mixtures)"""
    ns = [16, R.samples_with_gap_K(K), 1995] + [R.samples_for_frames(L) for L in R.MUTATION_CASE_FRAMES]
    seeds = [100, 101, 102] + list(R.MUTATION_CASE_FRAMES)
    T = max(ns) + 5
    mix = torch.zeros(len(ns), T)
    for i, n in enumerate(ns):
        mix[i, :n] = R.synthetic_mix(n, seeds[i])
    return mix, ns


@functools.lru_cache(maxsize=None)
def _reference(K, n_spk):
    mix, ns = _batch(K)
    return R.DualPathRef(_dims(K, n_spk), _weights(K, n_spk), mirror=True).separate(mix, ns)


@pytest.mark.parametrize("K", [10, 250])
@pytest.mark.parametrize("n_spk", [1, 2, 3])
def test_ragged_batch_against_the_reference(ccx_ctx, K, n_spk):
    mix, ns = _batch(K)
    L = (ns[1] - 16) // 8 + 1
    assert R.geometry(L, K)[0] == K
    sep = _separator(ccx_ctx, K, n_spk)
    try:
        got = sep.separate_batch(mix, ns).cpu()
        assert got.shape == (len(ns), mix.shape[1], n_spk) and torch.isfinite(got).all()
        ref = _reference(K, n_spk)
        figures = [R.rel_l2(got[b, :n], ref[b, :n]) for b, n in enumerate(ns)]
        print(f"dualpath model K={K} n_spk={n_spk} samples {ns}: rel-L2 " + " ".join(f"{f:.3e}" for f in figures))
        for b, n in enumerate(ns):
            assert float(got[b, n:].abs().max()) == 0.0, "a source is not zero past n_samples"
            within(N_MODEL, figures[b], R.BOUND_MODEL, (K, n_spk, b))
        # a row alone equals the same row in the batch, bit for bit; the shorter call comes second: stale padding would show
        for b in (2, 0, 1):
            alone = sep.separate_batch(mix[b:b + 1, :ns[b]].contiguous()).cpu()
            assert torch.equal(alone[0], got[b, :ns[b]]), f"row {b} alone differs from the row in the batch"
        assert sep.tokens_for(ns[1]) == R.geometry(L, K)[1] * K
    finally:
        sep.close()


def test_capacity_and_geometry_refusals(ccx_ctx):
    from clearconverse_amd import _lib
    from clearconverse_amd.separator import DualPathSeparator
    from clearconverse_amd.weights import DualPathDims
    sep = _separator(ccx_ctx, 10, 2, max_tokens=400, max_utts=2)
    try:
        mix = torch.zeros(3, 400)
        with pytest.raises(_lib.CcxError, match="max 2"):
            sep.separate_batch(mix)
        with pytest.raises(_lib.CcxError, match="exceed capacity"):
            sep.separate_batch(torch.zeros(1, 16 + 8 * 400))
        with pytest.raises(_lib.CcxError, match="samples"):
            sep.separate_batch(torch.zeros(1, 15))
        assert torch.isfinite(sep.separate_batch(R.synthetic_mix(400, 0)[None])).all()       # the handle still works
    finally:
        sep.close()
    for field, val in (("n_filters", 128), ("d_model", 128), ("n_head", 4), ("kernel", 15), ("kernel", 34), ("stride", 4), ("segment", 9),
                       ("segment", 258), ("d_ffn", 96), ("d_ffn", 4096), ("n_layers", 9), ("n_blocks", 0), ("n_spk", 4)):
        d = DualPathDims(**dict(_dims(10, 2).__dict__, **{field: val}))
        with pytest.raises(_lib.CcxError, match=field):
            DualPathSeparator(d, {}, max_tokens=400, max_utts=2, ctx=ccx_ctx)
    sd = dict(_weights(10, 2))
    for bad in ("masknet.pos_enc.pe", "masknet.dual_mdl.0.intra_linear.weight"):
        with pytest.raises(_lib.CcxError, match="not built"):
            DualPathSeparator(DualPathDims(**_dims(10, 2).__dict__), dict(sd, **{bad: torch.zeros(4)}), max_tokens=400, max_utts=2, ctx=ccx_ctx)
    ok = DualPathSeparator(DualPathDims(**_dims(10, 2).__dict__), dict(sd, **{"masknet.dual_mdl.0.intra_mdl.pos_enc.pe": torch.zeros(1, 8, 256)}),
                           max_tokens=400, max_utts=2, ctx=ccx_ctx)
    ok.close()


def test_full_depth_three_sources_one_second(ccx_ctx):
    """8 layers, 2 blocks, K = 250, d_ffn 1024, three sources, 1 s at 8 kHz"""
    d = _dims(250, 3, n_layers=8, d_ffn=1024)
    sep = _separator(ccx_ctx, 250, 3, n_layers=8, d_ffn=1024, max_tokens=4000, max_utts=1)
    try:
        mix = R.synthetic_mix(8000, 3)[None]
        got = sep.separate_batch(mix).cpu()
        assert torch.isfinite(got).all() and float(got.abs().max()) > 0
        ref = R.DualPathRef(d, _weights(250, 3, 8, 1024), mirror=True).separate(mix)
        figure = R.rel_l2(got[0], ref[0])
        print(f"dualpath model full depth: rel-L2 {figure:.3e}")
        within("dualpath model, full depth (8 layers): rel-L2 vs the mirrored fp64 reference", figure, R.BOUND_MODEL_FULL)
    finally:
        sep.close()
