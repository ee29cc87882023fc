"""Host half of openai-whisper's per-call decoding options [UPSTREAM-RECALL: whisper/decoding.py::DecodingOptions, whisper/transcribe.py;
parity unpinned]: what `WhisperModel(decoding_options=True)` does with `without_timestamps`, `prefix`, `suppress_blank`,
`suppress_tokens`, `max_initial_timestamp`, `sample_len`, `clip_timestamps` and `carry_initial_prompt` before anything reaches the
library.  No GPU state; tests/decoding_options_reference.py restates the same rules independently.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

FRAMES_PER_SECOND = 100
TIME_PRECISION = 0.02


def always_suppressed(rules) -> List[int]:
    """decoding.py::_get_suppress_tokens: the specials it adds to every non-empty list"""
    return [rules.transcribe, rules.translate, rules.sot, rules.sot_prev, rules.sot_lm, rules.no_speech]


def non_speech_tokens(rules) -> List[int]:
    """Tokenizer.non_speech_tokens as the rules carry it: their list without the specials"""
    special = set(always_suppressed(rules))
    return [int(t) for t in rules.suppress if int(t) not in special]


def parse_suppress_tokens(spec: Union[None, str, Sequence[int]], rules) -> Optional[List[int]]:
    """`suppress_tokens` -> the ids SuppressTokens bans, sorted; None: the filter is off altogether (upstream skips it when the option
    is falsy: an empty string, an empty list or None -- the specials are then not suppressed either).  A string holds comma-separated
    ids; -1 stands for the non-speech list."""
    if spec is None:
        return None
    if isinstance(spec, str):
        ids = [int(t) for t in spec.split(",") if t.strip()]
    else:
        ids = [int(t) for t in spec]
    if not ids:
        return None
    if -1 in ids:
        ids = [t for t in ids if t >= 0] + non_speech_tokens(rules)
    return sorted(set(ids + always_suppressed(rules)))


def max_initial_timestamp_index(seconds: Optional[float]) -> int:
    """decoding.py: round(max_initial_timestamp / precision); None disables the rule (-1 for the library)"""
    return -1 if seconds is None else int(round(float(seconds) / TIME_PRECISION))


def prefix_tokens(tokenizer, prefix: Union[None, str, Sequence[int]], n_text_ctx: int, sample_len: Optional[int]) -> List[int]:
    """decoding.py::_get_initial_tokens: encode(" " + prefix.strip()) (or the ids as given); with a sample_len, the last
    n_ctx // 2 - sample_len of them."""
    if prefix is None or (isinstance(prefix, str) and not prefix.strip()):
        return []
    toks = list(tokenizer.encode(" " + prefix.strip())) if isinstance(prefix, str) else [int(t) for t in prefix]
    if sample_len is not None:
        keep = n_text_ctx // 2 - int(sample_len)
        toks = toks[-keep:] if keep > 0 else []
    return toks


def parse_clip_timestamps(spec: Union[None, str, Sequence[float]], content_frames: int) -> List[Tuple[int, int]]:
    """transcribe.py: `clip_timestamps` -> the (start, end) frame pairs the window loop walks.  A string holds comma-separated
    seconds; seek points are round(t * 100); no point at all means [0]; an odd count is closed by the content's end."""
    if spec is None:
        pts: List[float] = []
    elif isinstance(spec, str):
        pts = [float(t) for t in spec.split(",") if t.strip()]
    else:
        pts = [float(t) for t in spec]
    seeks = [int(round(t * FRAMES_PER_SECOND)) for t in pts]
    if not seeks:
        seeks = [0]
    if len(seeks) % 2 == 1:
        seeks.append(int(content_frames))
    return list(zip(seeks[::2], seeks[1::2]))


@dataclass
class CallOptions:
    """One call's options as `WhisperModel.transcribe_batch` resolved them (the device part goes to ccx_whisper_set_decode_options)."""
    without_timestamps: bool = False
    suppress_blank: bool = True
    suppress: Optional[List[int]] = None          # the list that replaces the rules'; [] = SuppressTokens off
    suppress_default: bool = True                 # the option was left at "-1": the rules' own list, nothing to replace
    max_initial_timestamp_index: int = -2         # -2: the rules' own
    sample_len: Optional[int] = None
    carry_initial_prompt: bool = False

    def device_default(self, rules) -> bool:
        """nothing for the library to do: the decode the rules alone give"""
        mi = self.max_initial_timestamp_index
        return not self.without_timestamps and self.suppress_default and mi in (-2, rules.max_initial_timestamp_index)


def resolve(rules, without_timestamps=False, suppress_blank=True, suppress_tokens="-1", max_initial_timestamp=1.0, sample_len=None,
            carry_initial_prompt=False) -> CallOptions:
    sup = parse_suppress_tokens(suppress_tokens, rules)
    default = sup is not None and sup == sorted(set(int(t) for t in rules.suppress))
    if sample_len is not None and int(sample_len) < 1:
        raise ValueError("sample_len must be at least 1")
    return CallOptions(bool(without_timestamps), bool(suppress_blank), [] if sup is None else sup, default,
                       max_initial_timestamp_index(max_initial_timestamp), None if sample_len is None else int(sample_len),
                       bool(carry_initial_prompt))
