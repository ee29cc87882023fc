"""Scripted stand-ins for tests/test_overlap_sources_cpu.py (and the stub pipelines of tests/test_overlap_sources_gpu.py): an
N-source separator whose sources carry a tag, an embedder that answers with a scripted vector per tag, a Whisper that can fail on
one tag, and a processor builder that takes the new constructor arguments.  tests/glue_stubs.py is imported, never edited.

A tagged source k is a cosine of period TAG_PERIODS[k]: peak normalisation leaves the tag alone, `tag_of` reads it back.
"""
from __future__ import annotations

import itertools
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from clearconverse_amd.processor import Config, EnhancedAudioProcessor
from tests.glue_stubs import Annotation, Scenario, StubEmbedding, StubSeparator, StubWhisper, scenario_audio

SR = 16000
TAG_PERIODS = (4.0, 8.0, 16.0, 32.0)


def tagged(k: int, n: int) -> torch.Tensor:
    t = torch.arange(n, dtype=torch.float64)
    return (0.5 * torch.cos(2 * np.pi * t / TAG_PERIODS[k])).float()


def tag_of(x) -> int:
    x = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).reshape(-1).astype(np.float64)
    t = np.arange(x.size, dtype=np.float64)
    return int(np.argmax([abs(np.dot(x, np.exp(-2j * np.pi * t / p))) for p in TAG_PERIODS]))


class TaggedSeparator:
    """separate_batch([1, T]) -> [1, T, n_spk]: source k is tag k, whatever the mixture"""

    def __init__(self, n_spk: int):
        self.n_spk = n_spk
        self.calls: List[int] = []

    def separate_batch(self, mix: torch.Tensor) -> torch.Tensor:
        n = int(mix.shape[-1])
        self.calls.append(n)
        return torch.stack([tagged(k, n) for k in range(self.n_spk)], dim=-1)[None]


class ScriptedEmbedding:
    """tag k -> the unit vector e_k, so cosine(source k, profile c) = profile_c[k] / |profile_c|: a similarity matrix is scripted
    through the profiles.  Tags in `none_for` raise (the processor turns that into "no embedding")."""

    def __init__(self, none_for: Sequence[int] = ()):
        self.none_for = set(none_for)
        self.tags: List[int] = []

    def __call__(self, d):
        k = tag_of(d["waveform"])
        self.tags.append(k)
        if k in self.none_for:
            raise RuntimeError("scripted: no embedding for this source")
        e = np.zeros(len(TAG_PERIODS), dtype=np.float32)
        e[k] = 1.0
        return e


def profiles_for(sim_columns: Dict[str, Sequence[float]]) -> Dict[str, torch.Tensor]:
    """name -> profile vector whose cosine with e_k is column[k] / |column|"""
    out = {}
    for name, col in sim_columns.items():
        v = torch.zeros(len(TAG_PERIODS))
        v[:len(col)] = torch.tensor(list(col), dtype=torch.float32)
        out[name] = v
    return out


class TagFailingWhisper(StubWhisper):
    """fails on the sources whose tag is in `bad`; the text of the others names their tag"""

    def __init__(self, bad: Sequence[int] = ()):
        super().__init__()
        self.bad = set(bad)

    def transcribe(self, audio, initial_prompt=None, **kw):
        k = tag_of(audio)
        if k in self.bad:
            raise ValueError(f"scripted failure on source {k}")
        super().transcribe(audio, initial_prompt=initial_prompt, **kw)
        return {"text": f" source{k}."}


def brute_force_assignment(sim) -> Tuple[float, List[Tuple[int, int]]]:
    """the best one-to-one assignment by a different enumeration than the processor's: permutations of the longer side"""
    n_src, n_cand = len(sim), len(sim[0])
    best = (-np.inf, None)
    if n_src >= n_cand:
        for perm in itertools.permutations(range(n_src), n_cand):          # lexicographic in the source index per candidate
            tot = sum(float(sim[k][c]) for c, k in enumerate(perm))
            if tot > best[0]:
                best = (tot, [(k, c) for c, k in enumerate(perm)])
    else:
        for perm in itertools.permutations(range(n_cand), n_src):
            tot = sum(float(sim[k][c]) for k, c in enumerate(perm))
            if tot > best[0]:
                best = (tot, sorted([(k, c) for k, c in enumerate(perm)], key=lambda p: p[1]))
    return best


def bare_processor(separator, embedder, whisper=None, **kw) -> EnhancedAudioProcessor:
    p = EnhancedAudioProcessor(Config(auth_token="x"), load_models_immediately=False, **kw)
    p.device = torch.device("cpu")
    p.separator, p.embedding_model, p.whisper_model = separator, embedder, whisper or StubWhisper()
    p.denoiser = lambda y, sr, prop_decrease: np.asarray(y)
    p.models_loaded = {k: True for k in p.models_loaded}
    return p


def scripted_regions(p: EnhancedAudioProcessor, regions: List[Tuple[float, float, str]]) -> None:
    """replace the sliding-window attribution by its scripted answer"""
    p._resegment_overlap = lambda audio_segment, seg_start, seg_end, profiles: list(regions)


def build(sc: Scenario, separator=None, **kw):
    """tests/test_processor_glue._build with constructor arguments; the diarization stub keeps the arguments of every call"""
    p = EnhancedAudioProcessor(Config(auth_token="x", **sc.config), load_models_immediately=False, **kw)
    p.device = torch.device("cpu")
    audio = scenario_audio(sc)
    p.load_audio = lambda path: (audio.clone(), 16000)
    p.whisper_model, p.separator, p.embedding_model = StubWhisper(), separator or StubSeparator(), StubEmbedding()
    p.denoiser = lambda y, sr, prop_decrease: np.asarray(y)
    p.vad_pipeline = lambda path: Annotation([(s, e, "SPEECH") for s, e in sc.vad])
    calls: List[dict] = []

    def diar(path, min_speakers=None, max_speakers=None):
        name = os.path.basename(str(path))
        calls.append(dict(file=name, min_speakers=min_speakers, max_speakers=max_speakers))
        return Annotation(list(sc.secondary if name == "temp_segment.wav" else sc.diarization))
    p.diarization = diar
    p.models_loaded = {k: True for k in p.models_loaded}
    return p, calls
