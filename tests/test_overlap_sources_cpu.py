"""CPU: the two opt-in arguments of EnhancedAudioProcessor -- `speakers` (2 to 4 named speakers) and `all_overlap_sources` (every
separated source of an overlap region that can be paired with an involved speaker becomes a segment) -- with the scripted stubs of
tests/overlap_stubs.py.  With the defaults, and with the defaults spelled out, every scenario of tests/glue_stubs.py gives what the
committed fixtures of the reference's own code give (tests/golden/glue_process_file.json)."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from clearconverse_amd.processor import PROMPT_SINGLE, Config, EnhancedAudioProcessor
from tests import overlap_stubs as OS
from tests.glue_stubs import SCENARIOS, Scenario, result_to_json
from tests.test_processor_glue import _close

PROCESS = json.loads((Path(__file__).resolve().parent / "golden" / "glue_process_file.json").read_text())


# ---------------------------------------------------------------------------------------------------------------------------------
# defaults: nothing changes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [sc.name for sc in SCENARIOS])
def test_defaults_give_todays_results(name):
    assert name in PROCESS["scenarios"]
    entry = PROCESS["scenarios"][name]
    sc = Scenario.from_json(entry["scenario"])
    got = []
    for kw in ({}, dict(speakers=2, all_overlap_sources=False)):
        p, calls = OS.build(sc, **kw)
        res = p.process_file("clip.wav")
        got.append(json.loads(json.dumps(result_to_json(res, p.whisper_model.calls, p.separator.calls, [c["file"] for c in calls]))))
        for c in calls:     # what the diarization object is asked for is today's too
            assert (c["min_speakers"], c["max_speakers"]) == ((1, 2) if c["file"] == "temp_segment.wav" else (p.config.min_speakers, p.config.max_speakers))
        if res is not None:
            assert "speaker_segments" not in res["metadata"] and all("overlap_source" not in s.metadata for s in res["segments"])
    exp = dict(entry["expected"])
    exp.pop("transcript", None)
    _close(got[0], exp, name)
    assert got[0] == got[1]


def test_a_lower_config_cap_is_left_alone_at_the_default():
    sc = Scenario.from_json(PROCESS["scenarios"]["single_speaker"]["scenario"])
    sc.config = dict(sc.config, max_speakers=1)
    p, calls = OS.build(sc)
    assert p.process_file("clip.wav") is not None and calls[0]["max_speakers"] == 1


@pytest.mark.parametrize("bad", [1, 5, 0, -2, 2.0, "3", True, None])
def test_speakers_outside_the_range_are_refused(bad):
    with pytest.raises(ValueError, match="speakers"):
        EnhancedAudioProcessor(Config(auth_token="x"), speakers=bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# speakers = 3, 4
# ---------------------------------------------------------------------------------------------------------------------------------
def _five_labels():
    """five labels, none overlapping, with 5, 4, 3, 2 and 1 segments: SPEAKER_02 is the most frequent, SPEAKER_04 the least"""
    order = ["SPEAKER_02", "SPEAKER_00", "SPEAKER_03", "SPEAKER_01", "SPEAKER_04"]
    diar, truth, t = [], [], 0.0
    for i in range(15):
        lab = [l for n, l in zip((5, 4, 3, 2, 1), order) for _ in range(n)][(i * 7) % 15]      # interleaved, same counts
        diar.append((t, t + 1.2, lab))
        truth.append(("ABC"[order.index(lab) % 3], t, t + 1.2))
        t += 2.0                                                                               # gaps of 0.8 s: nothing merges
    return Scenario("five_labels", 30.0, truth=truth, diarization=diar, vad=[(0.0, 30.0)]), order


@pytest.mark.parametrize("speakers", [2, 3, 4])
def test_speakers_are_named_by_frequency(speakers):
    sc, order = _five_labels()
    p, calls = OS.build(sc, speakers=speakers)
    res = p.process_file("clip.wav")
    want = {lab: ("SPEAKER_" + "ABCD"[i] if i < speakers else "UNKNOWN") for i, lab in enumerate(order)}
    by_start = {round(s, 3): lab for s, _, lab in sc.diarization}
    assert len(res["segments"]) == 15
    for seg in res["segments"]:
        assert seg.speaker_id == want[by_start[round(seg.start, 3)]], (seg.start, seg.speaker_id)
    md = res["metadata"]
    assert md["speakers"] == ["SPEAKER_" + c for c in "ABCD"[:speakers]]
    assert (md["speaker_a_segments"], md["speaker_b_segments"], md["total_segments"]) == (5, 4, 15) and "duration" in md and "rapid_exchanges" in md
    if speakers == 2:
        assert "speaker_segments" not in md
    else:
        assert md["speaker_segments"] == {"SPEAKER_" + c: n for c, n in zip("ABCD"[:speakers], (5, 4, 3, 2))}
    main = [c for c in calls if c["file"] != "temp_segment.wav"]
    assert [(c["min_speakers"], c["max_speakers"]) for c in main] == [(1, speakers)]
    assert all((c["min_speakers"], c["max_speakers"]) == (1, speakers) for c in calls if c["file"] == "temp_segment.wav")


def test_the_config_cap_wins_when_it_is_higher():
    sc, _ = _five_labels()
    sc.config = dict(max_speakers=6)
    p, calls = OS.build(sc, speakers=3)
    p.process_file("clip.wav")
    assert calls[0]["max_speakers"] == 6


def test_secondary_diarization_takes_the_speaker_count():
    sc = Scenario.from_json(PROCESS["scenarios"]["low_similarity_secondary_diarization"]["scenario"])
    p, calls = OS.build(sc, speakers=4)
    assert p.process_file("clip.wav") is not None
    second = [c for c in calls if c["file"] == "temp_segment.wav"]
    assert second and all((c["min_speakers"], c["max_speakers"]) == (1, 4) for c in second)


# ---------------------------------------------------------------------------------------------------------------------------------
# the assignment
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (4, 4), (3, 2), (4, 2), (2, 3), (2, 4), (1, 3), (4, 1), (3, 4)])
def test_best_assignment_equals_brute_force(shape):
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    for _ in range(25):
        sim = rng.uniform(-1, 1, size=shape).tolist()
        got = EnhancedAudioProcessor._assign_sources(sim)
        total, want = OS.brute_force_assignment(sim)
        assert got == want, (sim, got, want)
        assert len(got) == min(shape) and len({k for k, _ in got}) == len(got) == len({c for _, c in got})
        assert [c for _, c in got] == sorted(c for _, c in got)                     # candidate order
        assert sum(sim[k][c] for k, c in got) == pytest.approx(total)


def test_ties_go_to_the_first_in_lexicographic_order():
    A = EnhancedAudioProcessor._assign_sources
    assert A([[0.5, 0.5], [0.5, 0.5]]) == [(0, 0), (1, 1)]
    assert A([[0.5] * 3] * 3) == [(0, 0), (1, 1), (2, 2)]
    assert A([[0.25, 0.75], [0.5, 1.0]]) == [(0, 0), (1, 1)]                        # 1.25 both ways (exact in binary)
    assert A([[0.5, 0.5], [0.5, 0.5], [0.5, 0.5]]) == [(0, 0), (1, 1)]              # three sources, two candidates
    assert A([[0.5, 0.5, 0.5]]) == [(0, 0)]                                         # one source: the first candidate
    assert A([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]) == [(0, 0), (1, 1)]
    assert A([]) == [] and A([[]]) == []


def _region(p, involved, profiles, regions=((0.0, 1.0, "SPEAKER_A"),), jobs=None):
    OS.scripted_regions(p, list(regions))
    piece = OS.scenario_audio(Scenario("x", 1.0, truth=[("A", 0, 1), ("B", 0, 1)], diarization=[], vad=[]))
    return p._process_overlap_segment(piece, profiles, list(involved), 0.0, 1.0, jobs), piece


def test_every_assigned_source_becomes_a_record_with_the_regions_speaker_first():
    # columns: similarity of sources 0, 1, 2 to the candidate.  Best: A <- source 2, B <- source 0, C <- source 1
    prof = OS.profiles_for({"SPEAKER_A": (0.1, 0.3, 0.9), "SPEAKER_B": (0.8, 0.1, 0.2), "SPEAKER_C": (0.3, 0.7, 0.1)})
    p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(), whisper=OS.TagFailingWhisper(), all_overlap_sources=True)
    jobs = []
    recs, piece = _region(p, ["SPEAKER_C", "SPEAKER_A", "SPEAKER_B"], prof, regions=[(0.0, 1.0, "SPEAKER_A")], jobs=jobs)
    assert [(r["speaker_id"], r["overlap_source"]) for r in recs] == [("SPEAKER_A", 2), ("SPEAKER_C", 1), ("SPEAKER_B", 0)]     # who, then `involved`
    for r in recs:
        col = prof[r["speaker_id"]]
        assert r["confidence"] == pytest.approx(float(col[r["overlap_source"]] / col.norm()), abs=1e-6)
        assert OS.tag_of(r["audio"]) == r["overlap_source"] and r["audio"].shape == piece.shape and r["transcription"] is None
        assert float(r["audio"].abs().max()) == pytest.approx(1.0, abs=1e-6)       # peak-normalised, as the single record's audio is
    assert len(jobs) == 3 and all(j.prompt == PROMPT_SINGLE and j.dep is None and j.wrap_errors and not j.word_timestamps for j in jobs)
    p._run_whisper_jobs(jobs)
    assert [r["transcription"] for r in recs] == [" source2.", " source1.", " source0."]
    assert [c["initial_prompt"] for c in p.whisper_model.calls] == [PROMPT_SINGLE] * 3
    # without the deferral list the calls are made at once, with the same result
    p2 = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(), whisper=OS.TagFailingWhisper(), all_overlap_sources=True)
    recs2, _ = _region(p2, ["SPEAKER_C", "SPEAKER_A", "SPEAKER_B"], prof)
    assert [(r["speaker_id"], r["overlap_source"], r["transcription"]) for r in recs2] == \
        [("SPEAKER_A", 2, " source2."), ("SPEAKER_C", 1, " source1."), ("SPEAKER_B", 0, " source0.")]


def test_default_keeps_one_voice():
    prof = OS.profiles_for({"SPEAKER_A": (0.1, 0.3, 0.9), "SPEAKER_B": (0.8, 0.1, 0.2)})
    p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding())
    recs, _ = _region(p, ["SPEAKER_A", "SPEAKER_B"], prof, jobs=[])
    assert len(recs) == 1 and recs[0]["speaker_id"] == "SPEAKER_A" and OS.tag_of(recs[0]["audio"]) == 2 and "overlap_source" not in recs[0]


def test_a_third_source_is_dropped_in_a_two_speaker_region():
    prof = OS.profiles_for({"SPEAKER_A": (0.2, 0.9, 0.3), "SPEAKER_B": (0.1, 0.2, 0.8), "SPEAKER_C": (0.9, 0.1, 0.1)})
    p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(), all_overlap_sources=True)
    recs, _ = _region(p, ["SPEAKER_A", "SPEAKER_B"], prof, regions=[(0.0, 1.0, "SPEAKER_B")], jobs=[])       # C has a profile but is not involved
    assert [(r["speaker_id"], r["overlap_source"]) for r in recs] == [("SPEAKER_B", 2), ("SPEAKER_A", 1)]


def test_two_sources_against_three_candidates():
    prof = OS.profiles_for({"SPEAKER_A": (0.6, 0.5), "SPEAKER_B": (0.9, 0.1), "SPEAKER_C": (0.2, 0.9)})
    p = OS.bare_processor(OS.TaggedSeparator(2), OS.ScriptedEmbedding(), all_overlap_sources=True)
    recs, _ = _region(p, ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"], prof, jobs=[])
    # B <- 0 and C <- 1 beat every pairing that serves A: the region's own speaker gets no record, nobody gets a source twice
    assert [(r["speaker_id"], r["overlap_source"]) for r in recs] == [("SPEAKER_B", 0), ("SPEAKER_C", 1)]
    # involved speakers without a profile are no candidates; repeats in `involved` count once
    recs, _ = _region(p, ["SPEAKER_B", "SPEAKER_D", "SPEAKER_B", "SPEAKER_A"], prof, jobs=[])
    assert [(r["speaker_id"], r["overlap_source"]) for r in recs] == [("SPEAKER_A", 1), ("SPEAKER_B", 0)]


def test_a_source_without_an_embedding_takes_no_part():
    prof = OS.profiles_for({"SPEAKER_A": (0.9, 0.2, 0.1), "SPEAKER_B": (0.1, 0.3, 0.8), "SPEAKER_C": (0.2, 0.9, 0.3)})
    emb = OS.ScriptedEmbedding(none_for=[0])                                       # A's best source cannot be embedded
    p = OS.bare_processor(OS.TaggedSeparator(3), emb, all_overlap_sources=True)
    recs, _ = _region(p, ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"], prof, jobs=[])
    assert emb.tags == [0, 1, 2]
    assert [(r["speaker_id"], r["overlap_source"]) for r in recs] == [("SPEAKER_B", 2), ("SPEAKER_C", 1)]      # A <- 1, B <- 2 totals less
    # no source embedded at all: today's record (the mixture itself, confidence -1)
    p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(none_for=[0, 1, 2]), all_overlap_sources=True)
    recs, piece = _region(p, ["SPEAKER_A", "SPEAKER_B"], prof, jobs=[])
    assert len(recs) == 1 and recs[0]["speaker_id"] == "SPEAKER_A" and recs[0]["confidence"] == -1.0 and torch.equal(recs[0]["audio"], piece)


def test_a_missing_profile_falls_back_to_todays_record():
    prof = OS.profiles_for({"SPEAKER_B": (0.1, 0.3, 0.8)})
    out = []
    for flag in (True, False):
        p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(), all_overlap_sources=flag)
        jobs = []
        recs, _ = _region(p, ["SPEAKER_A", "SPEAKER_B"], prof, jobs=jobs)
        assert len(recs) == 1 == len(jobs) and "overlap_source" not in recs[0]
        out.append((recs[0]["speaker_id"], recs[0]["confidence"], OS.tag_of(recs[0]["audio"])))
    assert out[0] == out[1] == ("SPEAKER_A", 1.0, 0)                                 # similarity with itself: the first source


def test_a_failing_transcription_marks_its_own_source_only():
    prof = OS.profiles_for({"SPEAKER_A": (0.9, 0.2, 0.1), "SPEAKER_B": (0.1, 0.9, 0.2), "SPEAKER_C": (0.2, 0.1, 0.9)})
    p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(), whisper=OS.TagFailingWhisper(bad=[1]), all_overlap_sources=True)
    jobs = []
    recs, piece = _region(p, ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"], prof, jobs=jobs)
    p._run_whisper_jobs(jobs)
    assert [r["transcription"] for r in recs] == [" source0.", "[Processing error]", " source2."]
    bad = recs[1]
    assert bad["speaker_id"] == "SPEAKER_B" and bad["confidence"] == 0.0 and torch.equal(bad["audio"], piece) and "scripted failure" in bad["error"]
    assert all("error" not in r and OS.tag_of(r["audio"]) == r["overlap_source"] for r in (recs[0], recs[2]))
    # the immediate path marks the same record
    p = OS.bare_processor(OS.TaggedSeparator(3), OS.ScriptedEmbedding(), whisper=OS.TagFailingWhisper(bad=[1]), all_overlap_sources=True)
    recs, _ = _region(p, ["SPEAKER_A", "SPEAKER_B", "SPEAKER_C"], prof)
    assert [r["transcription"] for r in recs] == [" source0.", "[Processing error]", " source2."]


# ---------------------------------------------------------------------------------------------------------------------------------
# through process_file and run
# ---------------------------------------------------------------------------------------------------------------------------------
def test_process_file_emits_one_segment_per_kept_source(tmp_path):
    sc = Scenario.from_json(PROCESS["scenarios"]["two_speakers_overlap_10s"]["scenario"])
    base, _ = OS.build(sc)
    ref = base.process_file("clip.wav")
    p, _ = OS.build(sc, all_overlap_sources=True)
    res = p.process_file("clip.wav")
    ref_ov, ov = [s for s in ref["segments"] if s.is_overlap], [s for s in res["segments"] if s.is_overlap]
    assert len(ref_ov) == 3 and len(ov) == 6                                        # both voices of each of the three regions
    assert [s.speaker_id for s in res["segments"] if not s.is_overlap] == [s.speaker_id for s in ref["segments"] if not s.is_overlap]
    for i, first in enumerate(ref_ov):
        a, b = ov[2 * i], ov[2 * i + 1]
        assert a.speaker_id == first.speaker_id and {a.speaker_id, b.speaker_id} == {"SPEAKER_A", "SPEAKER_B"}       # `who` first
        assert {a.metadata["overlap_source"], b.metadata["overlap_source"]} == {0, 1}
        assert a.metadata["overlap_speakers"] == first.metadata["overlap_speakers"] and (a.start, a.end) == (b.start, b.end) == (first.start, first.end)
        assert a.transcription and b.transcription and a.transcription != b.transcription
    assert p.separator.calls == base.separator.calls                                 # one separation per region, as before
    src, transcript, path = p.run("clip.wav", output_dir=str(tmp_path / "out"))
    blocks = [b for b in open(path, encoding="utf-8").read().split("\n\n") if b.strip()]
    assert len(blocks) == len(res["segments"]) == len(ref["segments"]) + 3


def test_batch_pipeline_refuses_a_separator_that_is_not_two_source():
    from clearconverse_amd.batch import BatchPipeline

    class W:
        class rules:
            is_multilingual = False

    class Sep:
        def __init__(self, n):
            self.n_spk = n
    for n in (1, 3, 4):
        with pytest.raises(ValueError, match="two-source"):
            BatchPipeline({"ctx": None, "whisper_model": W(), "separator": Sep(n)})
    BatchPipeline({"ctx": None, "whisper_model": W(), "separator": Sep(2)})
    BatchPipeline({"ctx": None, "whisper_model": W(), "separator": object()})        # a duck-typed two-source separator says nothing
