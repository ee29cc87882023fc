"""-m gpu: `load_models(sep_checkpoint="sepformer-wsj03mix")` on a savedir written here in SpeechBrain's layout builds the dual-path
separator, and `EnhancedAudioProcessor(speakers=3, all_overlap_sources=True)` carries its three sources through an overlap region
(scripted VAD / diarization / Whisper of tests/glue_stubs.py and tests/overlap_stubs.py, imported, not edited).  A default
`load_models()` beside it still returns the RE-SepFormer object, with the output bits of a separator built directly."""
import os

import numpy as np
import pytest
import torch

from clearconverse_amd.processor import Config, EnhancedAudioProcessor
from clearconverse_amd.weights import DualPathDims, SepDims, WhisperDims, synthetic_dualpath_state_dict, synthetic_sepformer_state_dict
from tests.overlap_stubs import Annotation, Scenario, StubWhisper, scenario_audio   # the scripted pipeline pieces (its builders pin the CPU)

pytestmark = pytest.mark.gpu

CLOSE = ("whisper_model", "separator", "embedding_model", "diarization_embedder", "segmentation_vad", "segmentation_diar", "denoiser")
SCENE = Scenario("three_at_once", 7.0, truth=[("A", 0, 5), ("B", 1, 6), ("C", 2, 7)],
                 diarization=[(0.0, 5.0, "SPEAKER_00"), (1.0, 6.0, "SPEAKER_01"), (2.0, 7.0, "SPEAKER_02")], vad=[(0.0, 7.0)])
SAVED = DualPathDims(n_layers=1, d_ffn=64, n_spk=3)


def _load(ccx_ctx, **kw):
    from clearconverse_amd.models import load_models
    return load_models(None, 0, whisper_batch=2, ctx=ccx_ctx, whisper_dims=WhisperDims.mini(2, 128), max_crops=32, gate_max_clips=2, **kw)


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("model_cache")
    base = root / "sepformer-wsj03mix"
    base.mkdir()
    sd = synthetic_dualpath_state_dict(SAVED, seed=21, pos_enc_buffers=True)
    for part in ("encoder", "masknet", "decoder"):
        torch.save({k[len(part) + 1:]: v for k, v in sd.items() if k.startswith(part + ".")}, str(base / f"{part}.ckpt"))
    (base / "hyperparams.yaml").write_text("num_spks: 3\nMaskNet: !new:speechbrain.lobes.models.dual_path.Dual_Path_Model\n    K: 250\n")
    old = os.environ.get("MODEL_CACHE_DIR")
    os.environ["MODEL_CACHE_DIR"] = str(root)
    yield root
    if old is None:
        os.environ.pop("MODEL_CACHE_DIR", None)
    else:
        os.environ["MODEL_CACHE_DIR"] = old


@pytest.fixture(scope="module")
def models(ccx_ctx, cache_dir):
    m = _load(ccx_ctx, sep_checkpoint="sepformer-wsj03mix", sep_tokens=48_000)
    yield m
    for k in CLOSE:
        m[k].close()


def test_load_models_builds_the_dual_path_separator(models):
    from clearconverse_amd.separator import DualPathSeparator
    sep = models["separator"]
    assert isinstance(sep, DualPathSeparator) and sep.n_spk == 3 and sep.dims == SAVED
    assert models["weights_sources"]["sepformer"] == "checkpoint"
    out = sep.separate_batch(torch.randn(1, 4000, generator=torch.Generator().manual_seed(0)))
    assert out.shape == (1, 4000, 3) and bool(torch.isfinite(out).all())
    assert float((out[..., 0] - out[..., 1]).abs().max()) > 0 and float((out[..., 1] - out[..., 2]).abs().max()) > 0


def test_three_named_sources_come_back_from_an_overlap_region(models):
    p = EnhancedAudioProcessor(Config(auth_token="x"), load_models_immediately=False, speakers=3, all_overlap_sources=True)
    audio = scenario_audio(SCENE).to(p.device)
    p.load_audio = lambda path: (audio.clone(), 16000)
    p.whisper_model, p.separator, p.embedding_model = StubWhisper(), models["separator"], models["embedding_model"]
    p.denoiser = lambda y, sr, prop_decrease: np.asarray(y)
    p.vad_pipeline = lambda path: Annotation([(s, e, "SPEECH") for s, e in SCENE.vad])
    p.diarization = lambda path, min_speakers=None, max_speakers=None: Annotation(list(SCENE.diarization))
    p.models_loaded = {k: True for k in p.models_loaded}
    shapes = []
    inner = p.separator.separate_batch

    class Spy:
        n_spk = models["separator"].n_spk

        def separate_batch(self, mix, *a, **kw):
            out = inner(mix, *a, **kw)
            shapes.append(tuple(out.shape))
            assert bool(torch.isfinite(out).all())
            return out
    p.separator = Spy()
    res = p.process_file("clip.wav")
    assert res is not None and res["metadata"]["speakers"] == ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"]
    assert shapes and all(s[-1] == 3 for s in shapes)
    emitted = [s for s in res["segments"] if s.is_overlap]
    assert len(emitted) >= 3 and len(emitted) % 3 == 0
    by_region = {}
    for s in emitted:
        by_region.setdefault((s.start, s.end), []).append(s)
    for region, segs in by_region.items():
        assert sorted(s.metadata["overlap_source"] for s in segs) == [0, 1, 2], region
        assert sorted(s.speaker_id for s in segs) == ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"], region


def test_the_default_is_still_the_resepformer_with_unchanged_bits(ccx_ctx, cache_dir):
    from clearconverse_amd.separator import SepformerSeparator
    dims = SepDims(n_layers=1)
    m = _load(ccx_ctx, sep_dims=dims, sep_tokens=20_000)          # no `resepformer` savedir in the cache: seeded weights, seed + 1
    direct = SepformerSeparator(dims, synthetic_sepformer_state_dict(dims, seed=1), max_tokens=20_000, max_utts=64, ctx=ccx_ctx)
    try:
        sep = m["separator"]
        assert type(sep) is SepformerSeparator and sep.n_spk == 2 and sep.dims == dims
        x = torch.randn(2, 6000, generator=torch.Generator().manual_seed(1))
        a, b = sep.separate_batch(x, [6000, 4321]).cpu(), direct.separate_batch(x, [6000, 4321]).cpu()
        assert a.shape == (2, 6000, 2) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        direct.close()
        for k in CLOSE:
            m[k].close()
