"""Reference for the multilingual Whisper tests (TEST INFRASTRUCTURE ONLY; imported by tests/test_multilingual_cpu.py,
tests/test_token_probs_gpu.py and tests/test_multilingual_gpu.py).

* `ranged_softmax`: what dec_token_probs_kernel (csrc/dec_probs.hip) computes, in fp64 on the same fp32 logits: the softmax over
  the ids [lo, hi) only, argmax by LOWEST id on equal values, the probability of a picked id.
* model level, on oracle/whisper_ref.py (imported, not edited; its id fields take the multilingual values):
  no-speech = softmax of the RAW logits at prompt position len(prompt) - 1 - n_tail (decoding.py `logits[:, self.sot_index]`),
  language = softmax over the language ids of the logits of [sot] (decoding.py::detect_language) [UPSTREAM-RECALL].
"""
import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from clearconverse_amd.tokenizer import DecodeRules
from oracle import whisper_ref as R


def ranged_softmax(row: np.ndarray, lo: int, hi: int, pick: int) -> Tuple[int, float, np.ndarray]:
    """row: fp32 logits (ids [0, len)), read as fp64.  -> (argmax id, log-probability of `pick`, log-probabilities [hi - lo]);
    -inf entries have log-probability -inf; everything outside [lo, hi) is never looked at."""
    assert 0 <= lo < hi <= len(row) and lo <= pick < hi
    x = np.asarray(row[lo:hi], dtype=np.float64)
    mx = x.max()
    am = lo + int(np.flatnonzero(x == mx)[0])        # lowest id on equal values
    with np.errstate(divide="ignore"):
        logp = (x - mx) - math.log(np.exp(x - mx).sum())
    return am, float(logp[pick - lo]), logp


def oracle_rules(rules: DecodeRules) -> R.Rules:
    """oracle/whisper_ref.Rules with the ids of `rules` (the oracle's defaults are the English-only ones)."""
    return R.Rules(eot=rules.eot, sot=rules.sot, sot_prev=rules.sot_prev, no_speech=rules.no_speech, no_timestamps=rules.no_timestamps,
                   timestamp_begin=rules.timestamp_begin, blank=rules.blank, max_initial_timestamp_index=rules.max_initial_timestamp_index,
                   suppress=tuple(rules.suppress))


def no_speech_logprob(logits: torch.Tensor, prompt_len: int, n_tail: int, no_speech: int) -> float:
    """logits [T, V] of the initial tokens (T >= prompt_len): log softmax(logits[prompt_len - 1 - n_tail])[no_speech], fp64."""
    row = logits[prompt_len - 1 - n_tail].double()
    return float(torch.log_softmax(row, dim=-1)[no_speech])


def language_logprobs(orc: R.WhisperRef, xa: torch.Tensor, rules: DecodeRules) -> torch.Tensor:
    """xa [B, 1500, D] -> fp64 log-probabilities [B, num_languages] over the language ids of the logits of [sot]."""
    B = xa.shape[0]
    lg = orc.decoder_logits(torch.full((B, 1), rules.sot, dtype=torch.long), xa)[:, 0].double()
    return torch.log_softmax(lg[:, rules.language_begin:rules.language_begin + rules.num_languages], dim=-1)


def self_check() -> None:
    """hand-worked rows"""
    ln = math.log
    # two ids: logits (0, ln 3) -> probabilities (1/4, 3/4)
    am, lp, all_ = ranged_softmax(np.array([0.0, ln(3.0)], dtype=np.float32), 0, 2, 0)
    assert am == 1 and abs(lp - ln(0.25)) < 1e-7 and abs(all_[1] - ln(0.75)) < 1e-7
    # the range hides everything else: a huge value and a NaN outside do not count
    row = np.array([1e30, 5.0, 5.0, -np.inf, 4.0, np.nan], dtype=np.float32)
    am, lp, all_ = ranged_softmax(row, 1, 5, 4)
    z = 2.0 + math.exp(-1.0)
    assert am == 1                                            # equal maxima: the lower id
    assert abs(lp - (-1.0 - ln(z))) < 1e-12 and all_[2] == -np.inf and abs(all_[0] + ln(z)) < 1e-12
    # a single-id range is certain, whatever the value; a common offset changes nothing
    assert ranged_softmax(np.array([3.0, -7.0], dtype=np.float32), 1, 2, 1)[:2] == (1, 0.0)
    a = ranged_softmax(np.array([1.0, 2.0, 4.0], dtype=np.float32), 0, 3, 1)
    b = ranged_softmax(np.array([81.0, 82.0, 84.0], dtype=np.float32), 0, 3, 1)
    assert a[0] == b[0] == 2 and abs(a[1] - b[1]) < 1e-12
    # the no-speech position: two tokens behind the last one with a three-token SOT sequence
    lg = torch.zeros(5, 4, dtype=torch.float64)
    lg[2, 3] = ln(3.0)                                        # row 2 = position 5 - 1 - 2: p = 3 / 6
    lg[4, 3] = 9.0
    assert abs(no_speech_logprob(lg, 5, 2, 3) - ln(0.5)) < 1e-12
    assert abs(no_speech_logprob(lg, 5, 0, 3) - (9.0 - ln(3.0 + math.exp(9.0)))) < 1e-12
