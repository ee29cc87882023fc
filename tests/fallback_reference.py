"""Plain restatements of the temperature-fallback and best_of rules (tests/test_fallback_reference_cpu.py, tests/test_fallback_gpu.py).
Written from the rules' statement, not from clearconverse_amd/fallback.py:
[UPSTREAM-RECALL: whisper/transcribe.py::decode_with_fallback, decoding.py::MaximumLikelihoodRanker, DecodingResult]; parity unpinned.

* a window walks the temperature schedule in order and is accepted at the first temperature at which it needs no fallback; at the
  last one it is accepted whatever it scores;
* it needs a fallback when compression_ratio > compression_ratio_threshold or avg_logprob < logprob_threshold (a threshold that is
  None tests nothing) -- unless no_speech_prob > no_speech_threshold and avg_logprob < logprob_threshold with both thresholds set;
* avg_logprob = sum_logprob / (n_tokens + 1); compression_ratio = len(b) / len(zlib.compress(b)), b the stripped text in UTF-8;
* temperature 0: one row per window; above 0 with best_of = n: n rows, tokens cut at the first eot, score sum_logprob / len(tokens),
  empty = -inf, first maximum; no_speech_prob from the first row;
* the noise stream of candidate c of the group's window w is w * n + c.
"""
import math
import zlib


def compression_ratio_ref(text):
    b = text.strip().encode("utf-8")
    return len(b) / len(zlib.compress(b))


def needs_fallback_ref(cr, avg_logprob, no_speech_prob, cr_thr, lp_thr, ns_thr):
    repetitive = cr_thr is not None and cr > cr_thr
    improbable = lp_thr is not None and avg_logprob < lp_thr
    silent = ns_thr is not None and lp_thr is not None and no_speech_prob > ns_thr and avg_logprob < lp_thr
    return (repetitive or improbable) and not silent


def n_rows_ref(temperature, best_of):
    return best_of if (temperature > 0 and best_of is not None) else 1


def rank_ref(cands, eot):
    """cands: [(tokens, sum_logprob)] -> index of the kept one"""
    scores = []
    for toks, slp in cands:
        cut = []
        for t in toks:
            if t == eot:
                break
            cut.append(t)
        scores.append(slp / len(cut) if cut else -math.inf)
    return scores.index(max(scores))


def walk_ref(rounds, cr_thr, lp_thr, ns_thr):
    """One window.  rounds[k] = (temperature, compression_ratio, avg_logprob, no_speech_prob) of what the window kept at schedule
    entry k, for every k the walk may reach -> index of the accepted entry."""
    for k, (_, cr, lp, ns) in enumerate(rounds):
        if k == len(rounds) - 1 or not needs_fallback_ref(cr, lp, ns, cr_thr, lp_thr, ns_thr):
            return k
    raise AssertionError("empty schedule")


def plan_ref(table, schedule, best_of, max_batch):
    """A group's rounds from a pass/fail table: table[w][k] True = window w needs a fallback after schedule entry k (ignored at the
    last entry).  -> per round: list of calls, each a list of (window, candidate, stream id), at most max_batch rows, window-major."""
    live = list(range(len(table)))
    out = []
    for k, t in enumerate(schedule):
        if not live:
            break
        n = n_rows_ref(t, best_of)
        rows = []
        for w in live:
            for c in range(n):
                rows.append((w, c, w * n + c))
        out.append([rows[i:i + max_batch] for i in range(0, len(rows), max_batch)])
        live = [w for w in live if table[w][k]] if k + 1 < len(schedule) else []
    return out


def avg_logprob_ref(sum_logprob, n_tokens):
    return sum_logprob / (n_tokens + 1)


# Stream ids of the select kernel's stream_ids test (tests/test_dec_mapped_gpu.py): a permutation of the 24 sampling rows with gaps
# (row b -> 3 * ((7 b + 5) mod 24) + 1).  tests/test_fallback_reference_cpu.py checks that with these ids the reference's draws stay
# inside the 2 % leave-out cap at the temperatures and seeds the GPU test uses.
SELECT_STREAM_IDS = [3 * ((7 * b + 5) % 24) + 1 for b in range(24)]
SELECT_TEMPERATURES = (0.1, 0.7, 5.0)
SELECT_SEEDS = (99, 2 ** 40 + 5, 7)
