"""GPU: the ECAPA-TDNN embedder end to end (clearconverse_amd.speaker.ECAPAEmbedder over ccx_ecapa_embed) against the fp64
restatement of tests/ecapa_reference.py, and as `models["embedding_model"]` of the processor.

The inputs (four crops, seeded weights) are those of tests/ecapa_reference.py::gpu_test_crops / gpu_test_state_dict; the CPU suite
checks the conditions of non-degeneracy on exactly them (tests/test_ecapa_reference_cpu.py).
Bounds: 2.5 x the deviation measured on an MI355X (ECAPA-TDNN), asserted through tests.conftest.within."""
import numpy as np
import pytest
import torch

from tests import ecapa_reference as R
from tests.conftest import within

pytestmark = pytest.mark.gpu

# measured on an MI355X over the four crops: worst rel-L2 and worst 1 - cosine of the 192-d embedding against fp64
EMB_MEASURED = {"rel_l2": 4.992e-3, "one_minus_cos": 1.246e-5}
EMB_REL_L2_BOUND = 2.5 * EMB_MEASURED["rel_l2"]


@pytest.fixture(scope="module")
def setup(ccx_ctx):
    from clearconverse_amd.speaker import ECAPAEmbedder
    sd, crops = R.gpu_test_state_dict(), R.gpu_test_crops()
    emb = ECAPAEmbedder(sd, max_crops=8, max_samples=260000, ctx=ccx_ctx)
    ref = torch.stack([R.embed(c, sd) for c in crops])             # computed once, shared, left unchanged
    got = emb.embed_batch(crops)
    yield emb, crops, ref, got
    emb.close()


def test_embeddings_against_fp64(setup):
    emb, crops, ref, got = setup
    assert got.shape == (len(crops), 192) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    for i, c in enumerate(crops):
        e, cs = R.rel_l2(got[i].cpu(), ref[i]), R.cosine(got[i].cpu(), ref[i])
        print(f"ecapa embedding n={c.numel()}: rel-L2 {e:.3e}, 1 - cos {1 - cs:.3e}")
        within("ecapa embedding rel-L2", e, EMB_REL_L2_BOUND, c.numel())
        within("ecapa embedding 1 - cosine", 1 - cs, 2.5 * EMB_MEASURED["one_minus_cos"], c.numel())


def test_single_call_and_split_groups_equal_the_batch_bit_for_bit(setup, ccx_ctx):
    emb, crops, _, got = setup
    for i, c in enumerate(crops):
        one = emb({"waveform": c[None, :], "sample_rate": 16000})
        assert isinstance(one, np.ndarray) and one.shape == (192,)
        assert np.array_equal(one.view(np.int32), got[i].cpu().numpy().view(np.int32)), i
    # a capacity that forces two launch groups (the 144000-sample crop goes alone)
    from clearconverse_amd.speaker import ECAPAEmbedder
    small = ECAPAEmbedder(R.gpu_test_state_dict(), max_crops=3, max_samples=170000, ctx=ccx_ctx)
    try:
        assert len(list(small._groups(crops))) == 2
        two = small.embed_batch(crops)
    finally:
        small.close()
    assert torch.equal(two.view(torch.int32), got.view(torch.int32))


def test_refusals(setup):
    from clearconverse_amd import _lib
    emb, crops, _, _ = setup
    with pytest.raises(_lib.CcxError, match="too short"):
        emb.embed_batch([torch.zeros(700)])
    with pytest.raises(_lib.CcxError, match="weights"):
        emb.embed_batch(crops[:1], weights=[torch.ones(10)])
    with pytest.raises(_lib.CcxError, match="16 kHz"):
        emb({"waveform": crops[0][None, :], "sample_rate": 8000})


def test_process_file_with_the_ecapa_embedder(ccx_ctx, tmp_path):
    """load_models(embedding="ecapa") through EnhancedAudioProcessor.process_file on one synthetic clip: the embedder is the ECAPA one,
    no x-vector handle exists, and the segments carry SPEAKER_A / SPEAKER_B labels (scripted segmentation weights, as in
    tests/test_pipeline_gpu.py, guarantee speech and two diarization labels)."""
    from clearconverse_amd.audio import synthetic_clip, write_wav
    from clearconverse_amd.models import build_state_dicts, load_models
    from clearconverse_amd.processor import Config, EnhancedAudioProcessor
    from clearconverse_amd.speaker import ECAPAEmbedder
    from clearconverse_amd.weights import SepDims, WhisperDims
    from tests.scripted_nets import scripted_pyannet_state_dict
    sds = build_state_dicts(None, whisper_dims=WhisperDims.mini(2, 128), sep_dims=SepDims(n_layers=2), seed=0, embedding="ecapa")
    assert sds["weights_sources"]["ecapa"] in ("synthetic", "checkpoint")
    sds["pyannet_diar"], _ = scripted_pyannet_state_dict(1, 7, True)
    sds["pyannet_vad"], _ = scripted_pyannet_state_dict(1, 3, False, window_s=5.0, seed=4)
    m = load_models(None, 0, whisper_batch=16, ctx=ccx_ctx, state_dicts=sds, sep_tokens=60_000, max_crops=128, embedding="ecapa")
    try:
        assert isinstance(m["embedding_model"], ECAPAEmbedder) and m["embedding_model"].DIM == 192
        path = str(tmp_path / "clip.wav")
        write_wav(path, synthetic_clip(1, 30.0))
        p = EnhancedAudioProcessor(Config(temperature=0.0, min_speakers=2, max_speakers=2), load_models_immediately=True,
                                   model_loader=lambda cfg, dev: m)
        res = p.process_file(path)
        assert len(res["segments"]) >= 2
        labels = {s.speaker_id for s in res["segments"]}
        assert labels <= {"SPEAKER_A", "SPEAKER_B", "UNKNOWN"} and labels & {"SPEAKER_A", "SPEAKER_B"}, labels
    finally:
        for k in ("whisper_model", "separator", "embedding_model", "diarization_embedder", "segmentation_vad", "segmentation_diar", "denoiser"):
            m[k].close()


def test_state_dicts_without_ecapa_are_refused(ccx_ctx):
    from clearconverse_amd.models import load_models
    with pytest.raises(ValueError, match="ecapa"):
        load_models(None, 0, ctx=ccx_ctx, state_dicts={"whisper_dims": {}}, embedding="ecapa")
