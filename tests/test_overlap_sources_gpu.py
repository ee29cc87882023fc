"""-m gpu: `all_overlap_sources` with the libccx models -- a three-source separator (SepDims(n_layers=1, n_spk=3)) and the x-vector
embedder, both out of `load_models` -- and scripted VAD / diarization / Whisper objects: three speakers talk at once.  The (speaker,
source) pairs the processor emits must be the assignment recomputed here, region by region, from `separate_batch` and the embedder's
own outputs by a different enumeration (tests/overlap_stubs.brute_force_assignment); `run()` writes one transcript entry per kept
source."""
import itertools

import numpy as np
import pytest
import torch

from clearconverse_amd.processor import Config, EnhancedAudioProcessor
from clearconverse_amd.weights import SepDims, WhisperDims
from tests import overlap_stubs as OS
from tests.glue_stubs import Annotation, Scenario, StubWhisper, scenario_audio

pytestmark = pytest.mark.gpu

CLOSE = ("whisper_model", "separator", "embedding_model", "diarization_embedder", "segmentation_vad", "segmentation_diar", "denoiser")
# staggered starts and ends: the overlap detection (the reference's sweep) then reports one region with all three speakers involved,
# and every segment meets it first
SCENE = Scenario("three_at_once", 7.0, truth=[("A", 0, 5), ("B", 1, 6), ("C", 2, 7)],
                 diarization=[(0.0, 5.0, "SPEAKER_00"), (1.0, 6.0, "SPEAKER_01"), (2.0, 7.0, "SPEAKER_02")], vad=[(0.0, 7.0)])


@pytest.fixture(scope="module")
def models(ccx_ctx):
    from clearconverse_amd.models import load_models
    m = load_models(None, 0, whisper_batch=2, ctx=ccx_ctx, whisper_dims=WhisperDims.mini(2, 128), sep_dims=SepDims(n_layers=1, n_spk=3),
                    sep_tokens=20_000, max_crops=32, gate_max_clips=2)
    yield m
    for k in CLOSE:
        m[k].close()


def test_load_models_builds_a_three_source_separator(models):
    sep = models["separator"]
    assert sep.n_spk == 3 and sep.dims == SepDims(n_layers=1, n_spk=3)
    out = sep.separate_batch(torch.randn(1, 4000))
    assert out.shape == (1, 4000, 3) and bool(torch.isfinite(out).all())


def _processor(models, **kw):
    p = EnhancedAudioProcessor(Config(auth_token="x"), load_models_immediately=False, **kw)
    audio = scenario_audio(SCENE).to(p.device)
    p.load_audio = lambda path: (audio.clone(), 16000)
    p.whisper_model, p.separator, p.embedding_model = StubWhisper(), models["separator"], models["embedding_model"]
    p.denoiser = lambda y, sr, prop_decrease: np.asarray(y)
    p.vad_pipeline = lambda path: Annotation([(s, e, "SPEECH") for s, e in SCENE.vad])
    p.diarization = lambda path, min_speakers=None, max_speakers=None: Annotation(list(SCENE.diarization))
    p.models_loaded = {k: True for k in p.models_loaded}
    seen = []                       # one entry per _process_overlap_segment call: its arguments, its regions, its records
    inner_regions, inner_overlap = p._resegment_overlap, p._process_overlap_segment

    def regions(audio_segment, seg_start, seg_end, profiles):
        r = inner_regions(audio_segment, seg_start, seg_end, profiles)
        seen[-1]["regions"] = list(r)
        return r

    def overlap(audio_segment, profiles, involved, seg_start, seg_end, jobs=None):
        seen.append(dict(audio=audio_segment, profiles=profiles, involved=list(involved), seg_start=seg_start))
        seen[-1]["records"] = inner_overlap(audio_segment, profiles, involved, seg_start, seg_end, jobs)
        return seen[-1]["records"]
    p._resegment_overlap, p._process_overlap_segment = regions, overlap
    return p, seen


def _expected_pairs(p, call, region):
    """(speaker, source) pairs of one region from separate_batch and the embedder, `who` first"""
    ns, ne, who = region
    piece = p._extract_segment(call["audio"], ns - call["seg_start"], ne - call["seg_start"])
    sources = p.separator.separate_batch(piece)
    assert sources.shape[-1] == 3
    embs = []
    for k in range(3):
        src = sources[..., k]
        src = src / (torch.max(torch.abs(src)) + 1e-8)
        e = p.embedding_model({"waveform": src.detach().cpu(), "sample_rate": 16000}) if src.shape[-1] >= 8000 else None
        embs.append(None if e is None else torch.tensor(e, dtype=torch.float64))
    cands = [who] + [s for i, s in enumerate(call["involved"]) if s != who and s in call["profiles"] and s not in call["involved"][:i]]
    rows = [k for k in range(3) if embs[k] is not None]
    cos = lambda a, b: float(torch.dot(a, b) / (a.norm() * b.norm()))
    sim = [[cos(embs[k], call["profiles"][c].double().cpu()) for c in cands] for k in rows]
    total, pairs = OS.brute_force_assignment(sim)
    # the runner-up must lose by more than fp32 cosine rounding, or the comparison below would test the rounding
    totals = sorted((sum(sim[k][c] for c, k in enumerate(perm)) for perm in itertools.permutations(range(len(rows)), min(len(rows), len(cands)))), reverse=True)
    assert len(totals) < 2 or totals[0] - totals[1] > 1e-5, totals[:2]
    return [(cands[c], rows[k]) for k, c in pairs], sim, pairs


def test_every_source_of_a_three_speaker_overlap_is_emitted(models, tmp_path):
    p, seen = _processor(models, speakers=3, all_overlap_sources=True)
    res = p.process_file("clip.wav")
    assert res is not None and res["metadata"]["speakers"] == ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"]
    assert seen and all(sorted(c["involved"]) == ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"] and len(c["profiles"]) == 3 for c in seen)
    emitted = [s for s in res["segments"] if s.is_overlap]
    n_regions = n_records = 0
    for call in seen:
        assert len(call["regions"]) >= 1
        recs = iter(call["records"])
        for region in call["regions"]:
            want, sim, pairs = _expected_pairs(p, call, region)
            assert len(want) == 3 and want[0][0] == region[2]                        # three sources, three candidates, `who` first
            n_records += len(want)
            for (spk, k), (i, c) in zip(want, pairs):
                r = next(recs)
                assert (r["speaker_id"], r["overlap_source"]) == (spk, k), (region, want)
                assert r["confidence"] == pytest.approx(sim[i][c], abs=1e-5) and r["transcription"]
            n_regions += 1
        assert next(recs, None) is None
    assert len(emitted) == n_records == 3 * n_regions and n_regions >= 1 and all(s.metadata["overlap_source"] in (0, 1, 2) for s in emitted)
    # the default keeps one voice per region, from the same regions
    q, seen_q = _processor(models, speakers=3)
    ref = q.process_file("clip.wav")
    assert [c["regions"] for c in seen_q] == [c["regions"] for c in seen]
    assert len([s for s in ref["segments"] if s.is_overlap]) == n_regions and all("overlap_source" not in s.metadata for s in ref["segments"])
    # run() writes whatever segments it gets: one entry per kept source
    src, transcript, path = p.run("clip.wav", output_dir=str(tmp_path / "out"))
    blocks = [b for b in open(path, encoding="utf-8").read().split("\n\n") if b.strip()]
    assert len(blocks) == len(res["segments"]) and sum(b.startswith("[SPEAKER_") for b in blocks) >= 3 * n_regions
    assert len(list((tmp_path / "out" / "overlap_segments").glob("overlap_*.wav"))) >= 3
