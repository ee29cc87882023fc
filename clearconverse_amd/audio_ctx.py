"""Reduced audio context: how many of Whisper's 1500 encoder positions a window keeps (`WhisperModel(audio_ctx=...)`,
include/ccx.h ccx_whisper_set_audio_ctx / ccx_whisper_encode_ctx).  GPU-free.

The encoder then runs positions [0, n) of a window only and the decoder's cross attention reads those n rows: a 5 s window costs a
fifth of the encoder's rows and of the bytes every decode step streams.  This is NOT upstream's arithmetic -- Whisper was trained on
zero-padded 30 s windows -- and what it costs in transcript quality on real checkpoints is not measured here: off by default."""
from __future__ import annotations

import math
import os
from typing import Optional, Union

N_AUDIO_CTX = 1500
FLOOR = 64              # the library's smallest context (ccx_whisper_encode_ctx)
FRAMES_PER_POSITION = 2  # conv2's stride: two log-mel frames (20 ms) per encoder position
POSITIONS_PER_SECOND = 50

Setting = Union[None, str, int]


def positions_for(content_frames: int, margin_s: float = 1.0, granule: int = 64, floor: int = FLOOR, n_audio_ctx: int = N_AUDIO_CTX) -> int:
    """Encoder positions for a window with `content_frames` log-mel frames of audio (the rest of its 3000 frames is padding):
        clamp(granule * ceil((ceil(content_frames / 2) + 50 * margin_s) / granule), floor, n_audio_ctx)
    -- the positions the audio covers, a margin of silence behind it (the decoder was trained to see the padding begin), rounded up to
    whole 64-key tiles of the encoder attention.  The defaults (1 s of margin, granules of 64, a floor of 64) are POLICY, not
    measurements: nobody has measured which margin real checkpoints need."""
    if content_frames < 0 or margin_s < 0 or granule < 1 or not 1 <= floor <= n_audio_ctx:
        raise ValueError(f"positions_for: content_frames={content_frames}, margin_s={margin_s}, granule={granule}, floor={floor}, "
                         f"n_audio_ctx={n_audio_ctx} out of range")
    need = math.ceil(content_frames / FRAMES_PER_POSITION) + POSITIONS_PER_SECOND * margin_s
    n = granule * math.ceil(need / granule)
    return int(min(max(n, floor), n_audio_ctx))


def parse_setting(value, n_audio_ctx: int = N_AUDIO_CTX, what: str = "audio_ctx") -> Setting:
    """A constructor / per-call value -> None (off: the whole window), "auto" (positions_for per window) or an int in
    [FLOOR, n_audio_ctx] (that many positions for every window).  Anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, str):
        v = value.strip().lower()
        if v == "auto":
            return "auto"
        if v.lstrip("+").isdigit():
            value = int(v)
        else:
            raise ValueError(f"{what}={value!r}: expected None, 'auto' or an integer in [{FLOOR}, {n_audio_ctx}]")
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"{what}={value!r}: expected None, 'auto' or an integer in [{FLOOR}, {n_audio_ctx}]")
    if not FLOOR <= value <= n_audio_ctx:
        raise ValueError(f"{what}={value}: out of range [{FLOOR}, {n_audio_ctx}]")
    return int(value)


def from_environment(n_audio_ctx: int = N_AUDIO_CTX) -> Setting:
    """CCX_AUDIO_CTX (`auto` or an integer; unset, empty, `0` or `off`: nothing) -- for A/B runs of an unmodified bench.py only; code
    passes `audio_ctx=`."""
    e: Optional[str] = os.environ.get("CCX_AUDIO_CTX")
    if e is None or e.strip().lower() in ("", "0", "off"):
        return None
    return parse_setting(e, n_audio_ctx, "CCX_AUDIO_CTX")


def context_of(setting: Setting, content_frames: int, n_audio_ctx: int = N_AUDIO_CTX) -> int:
    """the context of one window under a setting"""
    if setting is None:
        return n_audio_ctx
    if setting == "auto":
        return positions_for(content_frames, n_audio_ctx=n_audio_ctx)
    return int(setting)
