"""Model set of the hot path: builds the five libccx-backed objects the processor drives
(reference: `_load_resepformer_model`, `_load_whisper_model`, `_initialize_pyannote_models`,
/root/reference/back/api.py:657-797).  Real checkpoints are used when present under MODEL_CACHE_DIR;
there is no network in the build/bench environment, so otherwise seeded synthetic weights of the same
architectures are generated.  No CPU fallback: every object needs the HIP
library and a GPU."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import _lib
from .denoise import SpectralGate
from .pipelines import SpeakerDiarization, VoiceActivityDetection
from .separator import DualPathSeparator, SepformerSeparator
from .speaker import ECAPAEmbedder, ResNetEmbedder, SegmentationNet, XVectorEmbedder
from .weights import (DualPathDims, SepDims, WhisperDims, find_separator_checkpoint, synthetic_dualpath_state_dict, find_ecapa_checkpoint, find_pipeline_config, find_pyannote_checkpoint, find_sepformer_checkpoint,
                      find_whisper_checkpoint, sep_dims_from_state_dict, synthetic_pyannet_state_dict, synthetic_resnet34_state_dict,
                      synthetic_ecapa_state_dict, synthetic_sepformer_state_dict, synthetic_whisper_state_dict,
                      synthetic_xvector_state_dict)
from .whisper import WhisperModel


EMBEDDINGS = ("xvector", "ecapa")


def _check_embedding(embedding: str) -> str:
    if embedding not in EMBEDDINGS:
        raise ValueError(f"embedding={embedding!r}: must be one of {EMBEDDINGS}")
    return embedding


DENOISE_MODES = ("stationary", "nonstationary")


def _check_denoise(denoise: str) -> str:
    if denoise not in DENOISE_MODES:
        raise ValueError(f"denoise={denoise!r}: must be one of {DENOISE_MODES}")
    return denoise


def build_state_dicts(config=None, whisper_dims: Optional[WhisperDims] = None, sep_dims: Optional[SepDims] = None,
                      seed: int = 0, embedding: str = "xvector", sep_checkpoint: str = "resepformer",
                      sep_family: Optional[str] = None) -> Dict[str, object]:
    """Every weight of the path as host tensors: the real Whisper checkpoint when MODEL_CACHE_DIR holds one, seeded
    synthetic weights of the same architectures otherwise.  In a multi-GPU job rank 0 calls this and the result
    travels by ONE broadcast (batch.broadcast_weights).
    sep_checkpoint: the separator's savedir under MODEL_CACHE_DIR (default: the reference's `resepformer`); a checkpoint found there
    brings its own geometry (weights.sep_dims_from_state_dict: a 3-mix savedir gives n_spk = 3) and its own family: a savedir of
    the dual-path SepFormer (`masknet.dual_mdl.0....` keys, e.g. "sepformer-wsj03mix") yields `sep_family: "dualpath"` and DualPathDims.
    sep_family: None (default: RE-SepFormer unless the savedir says otherwise) or "dualpath" for seeded synthetic weights of the
    dual-path model when no checkpoint is found (sep_dims then is a DualPathDims or None)."""
    _check_embedding(embedding)
    if sep_family not in (None, "resepformer", "dualpath"):
        raise ValueError(f"sep_family={sep_family!r}: must be None, 'resepformer' or 'dualpath'")
    size = getattr(config, "whisper_model_size", "small.en") if config is not None else "small.en"
    ck = find_whisper_checkpoint(size) if whisper_dims is None else None
    if ck is not None:
        wd, wsd = ck
    else:
        wd = whisper_dims or WhisperDims.small_en()
        wsd = synthetic_whisper_state_dict(wd, seed=seed)
    sep_ck = find_sepformer_checkpoint(subdir=sep_checkpoint) if sep_dims is None else None
    found = find_separator_checkpoint(subdir=sep_checkpoint) if sep_ck is not None else None
    if found is not None and found[0] == "dualpath":
        if sep_family == "resepformer":
            raise ValueError(f"sep_family='resepformer' but the savedir '{sep_checkpoint}' holds a dual-path SepFormer")
        sep_family, sd_ = "dualpath", found[2]
    elif sep_family == "dualpath":
        if found is not None:
            raise ValueError(f"sep_family='dualpath' but the savedir '{sep_checkpoint}' holds a RE-SepFormer")
        if sep_dims is not None and not isinstance(sep_dims, DualPathDims):
            raise ValueError("sep_family='dualpath' needs sep_dims of type DualPathDims")
        sd_ = sep_dims or DualPathDims()
    else:
        sd_ = sep_dims or (sep_dims_from_state_dict(sep_ck) if sep_ck is not None else SepDims())
    dual = sep_family == "dualpath"
    # pyannote-side networks (reference back/api.py:776-792): real checkpoints when the hub cache holds them, seeded otherwise
    synth = {"xvector": lambda: synthetic_xvector_state_dict(seed=seed + 2), "pyannet_diar": lambda: synthetic_pyannet_state_dict(7, seed=seed + 3),
             "pyannet_vad": lambda: synthetic_pyannet_state_dict(3, seed=seed + 4), "resnet34": lambda: synthetic_resnet34_state_dict(seed=seed + 5)}
    nets, sources = {}, {"whisper": "checkpoint" if ck is not None else f"synthetic-seed{seed}",
                         "sepformer": "checkpoint" if sep_ck is not None else f"synthetic-seed{seed + 1}"}
    for kind, make in synth.items():
        real = find_pyannote_checkpoint(kind)
        nets[kind] = real if real is not None else make()
        sources[kind] = "checkpoint" if real is not None else "synthetic"
    if embedding == "ecapa":            # built only when asked: 80 MB of host tensors the default path never reads
        real = find_ecapa_checkpoint()
        nets["ecapa"] = real if real is not None else synthetic_ecapa_state_dict(seed=seed + 6)
        sources["ecapa"] = "checkpoint" if real is not None else "synthetic"
    return {
        "whisper_dims": dict(wd.__dict__), "whisper": wsd, "whisper_source": sources["whisper"],
        "sep_dims": dict(sd_.__dict__),
        "sepformer": sep_ck or (synthetic_dualpath_state_dict(sd_, seed=seed + 1) if dual else synthetic_sepformer_state_dict(sd_, seed=seed + 1)),
        **({"sep_family": "dualpath"} if dual else {}),
        **nets,
        "weights_sources": sources,
        # pipeline hyper-parameters: the pipelines' own config.yaml when on disk, the published values otherwise
        "vad_params": find_pipeline_config("vad"), "diarization_params": find_pipeline_config("diarization"),
    }


def load_models(config=None, device=None, whisper_batch: int = 8, ctx: Optional[_lib.Context] = None, max_audio_seconds: float = 600.0,
                whisper_dims: Optional[WhisperDims] = None, sep_dims: Optional[SepDims] = None, seed: int = 0,
                sep_tokens: int = 160_000, max_crops: int = 256, state_dicts: Optional[Dict[str, object]] = None,
                seg_max_crops: Optional[int] = None, seg_max_seconds: float = 1200.0, emb_max_crops: Optional[int] = None,
                resnet_max_chunks: int = 96, whisper_instances: int = 1, share_encoder_scratch: bool = True,
                gate_max_clips: int = 32, gate_max_seconds: float = 30.0, word_alignment: bool = False,
                word_probabilities: bool = False, embedding: str = "xvector", denoise: str = "stationary",
                decoding_options: bool = False, whisper_cross_fp8: bool = False, whisper_audio_ctx=None,
                whisper_token_logprobs: bool = False, sep_checkpoint: str = "resepformer",
                sep_family: Optional[str] = None) -> Dict[str, object]:
    """embedding: "xvector" (default: `pyannote/embedding`, what the reference loads) or "ecapa" (ECAPA-TDNN, 192-d) for
    `models["embedding_model"]`; the diarization pipeline keeps its ResNet-34 either way.
    denoise: the mode of `models["denoiser"]` -- "stationary" (default: what the reference asks noisereduce for) or "nonstationary"
    (noisereduce's own default mode, SpectralGate(stationary=False)).
    whisper_cross_fp8 (default off): every Whisper instance keeps the FP8 image of its encoder output and streams it in the decode's
    cross attention (WhisperModel.__init__ `cross_fp8`; transcript quality on real checkpoints unmeasured).
    whisper_audio_ctx (default None: off): "auto" or an integer builds every Whisper instance for the reduced audio context
    (WhisperModel.__init__ `audio_ctx`; not upstream's arithmetic, transcript quality on real checkpoints unmeasured).
    whisper_token_logprobs (default off): every Whisper instance holds the buffers of the per-token log-probabilities, and its
    `transcribe` / `decode` take `logprobs=n` (WhisperModel.__init__ `token_logprobs`; parity unpinned).
    sep_checkpoint (default "resepformer", the reference's savedir): the separator's savedir under MODEL_CACHE_DIR, handed to
    build_state_dicts when no state_dicts are given; `models["separator"].n_spk` says how many sources it returns.  A savedir of the
    dual-path SepFormer (e.g. "sepformer-wsj03mix"), or sep_family="dualpath" without one (synthetic weights), makes
    `models["separator"]` a DualPathSeparator (state_dicts["sep_family"] == "dualpath"); the default stays the RE-SepFormer.  Its
    capacity is min(sep_tokens, 64000) chunk rows (about 1 GB of workspaces at three sources: 30 s of 8 kHz audio per call)."""
    _check_embedding(embedding)
    _check_denoise(denoise)
    if not torch.cuda.is_available():
        raise _lib.CcxError("load_models needs a ROCm GPU: the HIP path has no CPU fallback")
    dev_index = device.index if isinstance(device, torch.device) and device.index is not None else (device if isinstance(device, int) else 0)
    ctx = ctx or _lib.Context(dev_index)
    W = state_dicts if state_dicts is not None else build_state_dicts(config, whisper_dims, sep_dims, seed, embedding=embedding,
                                                                                  sep_checkpoint=sep_checkpoint,
                                                                                  **({"sep_family": sep_family} if sep_family else {}))
    dual = W.get("sep_family") == "dualpath"
    sep_dims_t = DualPathDims if dual else SepDims
    if embedding == "ecapa" and "ecapa" not in W:
        raise ValueError("load_models(embedding='ecapa'): state_dicts has no 'ecapa' entry (build_state_dicts(embedding='ecapa'))")
    wd, wsd = WhisperDims(**W["whisper_dims"]), W["whisper"]
    if state_dicts is not None:         # the geometry travels WITH the weights: a contradicting argument is an error, not ignored
        if whisper_dims is not None and whisper_dims != wd:
            raise ValueError(f"load_models: whisper_dims {whisper_dims} contradicts state_dicts['whisper_dims'] {wd}")
        if sep_dims is not None and sep_dims != sep_dims_t(**W["sep_dims"]):
            raise ValueError(f"load_models: sep_dims {sep_dims} contradicts state_dicts['sep_dims'] {W['sep_dims']}")
    vp, dp = W.get("vad_params") or {}, W.get("diarization_params") or {}
    sd_ = sep_dims_t(**W["sep_dims"])   # the geometry the separator weights were built with (broadcast manifest included)
    # whisper_instances = 2: the software-pipelined batch driver (batch.py) encodes batch i + 1 into one instance while batch i
    # is still decoding out of the other (each holds its own cross-KV, workspaces and step graphs; the weights are 0.5 GB)
    # The further instances take the first one's log-mel / encoder workspaces (share_encoder_scratch; 32 GB at 768 windows): those
    # are only live inside log_mel / encode, and the pipelined driver orders every instance's log_mel / encode on one stream.
    # word_alignment (default off): transcribe(word_timestamps=True) then aligns words on the GPU (WhisperModel.__init__)
    # word_probabilities (default off, needs word_alignment): the words carry `probability` and transcribe() honours
    # hallucination_silence_threshold; handed on only when set
    # decoding_options (default off): transcribe() then honours without_timestamps, prefix, clip_timestamps and the rest of upstream's
    # per-call decoding options (WhisperModel.__init__); handed on only when set
    wp = {"word_probabilities": True} if word_probabilities else {}
    if decoding_options:
        wp["decoding_options"] = True
    if whisper_cross_fp8:
        wp["cross_fp8"] = True
    if whisper_audio_ctx is not None:
        wp["audio_ctx"] = whisper_audio_ctx
    if whisper_token_logprobs:
        wp["token_logprobs"] = True
    whispers = [WhisperModel(wd, wsd, max_batch=whisper_batch, device=dev_index, ctx=ctx, max_audio_seconds=max_audio_seconds,
                             word_alignment=word_alignment, **wp)]
    for _ in range(1, max(1, int(whisper_instances))):
        whispers.append(WhisperModel(wd, wsd, max_batch=whisper_batch, device=dev_index, ctx=ctx, max_audio_seconds=max_audio_seconds,
                                     share_encoder_scratch_with=whispers[0] if share_encoder_scratch else None,
                                     word_alignment=word_alignment, **wp))
    whisper = whispers[0]
    if dual:                            # opt-in: the published dual-path checkpoints (weights.DualPathDims)
        separator = DualPathSeparator(sd_, W["sepformer"], max_tokens=min(int(sep_tokens), 64_000), max_utts=64, device=dev_index, ctx=ctx)
    else:
        separator = SepformerSeparator(sd_, W["sepformer"], max_tokens=sep_tokens, max_utts=64,
                                       device=dev_index, ctx=ctx)
    if embedding == "ecapa":            # the x-vector handle is then not created
        embedder = ECAPAEmbedder(W["ecapa"], max_crops=int(emb_max_crops or max_crops), max_samples=16000 * 600, device=dev_index, ctx=ctx)
    else:
        embedder = XVectorEmbedder(W["xvector"], max_crops=int(emb_max_crops or max_crops), max_samples=16000 * 1200,
                                   device=dev_index, ctx=ctx)
    # embedding model of the diarization pipeline (speaker-diarization-3.1 uses WeSpeaker ResNet-34, not pyannote/embedding)
    diar_embedder = ResNetEmbedder(W["resnet34"], max_chunks=int(resnet_max_chunks), max_samples=160000, max_masks=max(512, 3 * int(resnet_max_chunks)),
                                   device=dev_index, ctx=ctx)
    # one launch group of the segmentation nets holds seg_max_crops windows / seg_max_seconds of audio (≈60 B of device
    # buffers per sample): the batched pipeline raises both so that every window of a step shares one LSTM launch
    seg_crops = int(seg_max_crops or max_crops)
    seg_diar = SegmentationNet(W["pyannet_diar"], n_classes=7, powerset=True, max_crops=seg_crops,
                               max_samples=int(16000 * seg_max_seconds), device=dev_index, ctx=ctx)
    seg_vad = SegmentationNet(W["pyannet_vad"], n_classes=3, powerset=False, max_crops=seg_crops,
                              max_samples=int(16000 * seg_max_seconds), device=dev_index, ctx=ctx)
    # one launch of the spectral gate holds gate_max_clips rows of gate_max_seconds (longer inputs take the chunked path)
    gate = SpectralGate(max_samples=int(16000 * gate_max_seconds), max_clips=int(gate_max_clips), device=dev_index, ctx=ctx,
                        stationary=denoise == "stationary")
    return {
        "ctx": ctx,
        "weights_source": W.get("whisper_source", "given"),
        "whisper_model": whisper,
        "whisper_models": whispers,
        "separator": separator,
        "embedding_model": embedder,
        "vad_pipeline": VoiceActivityDetection(seg_vad, batch=seg_crops, **{k: vp[k] for k in ("onset", "offset", "min_duration_on", "min_duration_off") if k in vp}),
        "diarization": SpeakerDiarization(seg_diar, diar_embedder, batch=seg_crops,
                                          **{k: dp[k] for k in ("threshold", "min_cluster_size", "min_duration_off") if k in dp}),
        "weights_sources": W.get("weights_sources", {}),
        "diarization_embedder": diar_embedder,
        "denoiser": gate,
        "segmentation_vad": seg_vad,
        "segmentation_diar": seg_diar,
    }
