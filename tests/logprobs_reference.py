"""Per-token log-probabilities and top-N alternatives restated: the rule of include/ccx.h ccx_decode_logprob_options in fp64 numpy, the
fp32 sequential sum that ties the per-token values to sum_logprob, and a generator of kernel rows whose every rank decision has a
margin, so that ids, order and fill can be compared EXACTLY with the fp32 kernel.

THE RULE.  Take a row that samples at this step (not in its prompt phase, not done).  x = its logit row as the step draws from it: after
the bias kernel, the history kernel, the suppress mask of the rules or the call's options, SuppressBlank, ApplyTimestampRules on ruled
plans, and the removal of the text ids when the summed timestamp mass beats the best text token.  x is not divided by the
temperature, not truncated by top_k / top_p / min_p, and has no noise.  A = {v : x_v > -inf}; lp_v = (x_v - max_A x) - log sum_A
exp(x - max_A x).  token_logprob[step] is the float the kernel adds to sum_logprob at that step; top[step][k], k < n, is (id, lp_id)
of the n largest x_v over A in descending order, the lower id first among equal values; where |A| < n the rest is (-1, -inf).
n lies in [0, 8].

The generated rows:
  * the n + 1 = 9 best allowed values (fewer where fewer are allowed) are at least LOGIT_MARGIN = TR.LOGIT_MARGIN = 0.5 apart and
    within SPAN = 16 of the row's maximum -- except the built exact ties (equal fp32 values: exact on every side) at adjacent ranks,
    whose id pairs sit in one thread but different 4096-groups, in neighbouring threads, and in different waves of the kernel's
    layout (thread t holds ids 4 t + j + 4096 g);
  * forced-timestamp rows carry text ids inside the top that the force rule removes; first-step rows under the rules have
    TR.MAX_INITIAL_TS + 1 = 5 allowed ids, fewer than 8; banned decoys sit above everything;
  * a no-rules launch whose call list suppresses every id (`all_suppressed`) has nothing allowed at all.

MISREADINGS names wrong readings of the rule; tests/test_logprobs_reference_cpu.py shows that every one of them changes some generated
case, so a kernel that implemented it would fail the GPU tests built on these rows.
"""
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from tests import dec_reference as DR
from tests import decoding_options_reference as DO
from tests import truncation_reference as TR

MAX_TOP = 8                          # CCX_LOGPROB_MAX_TOP
LOGIT_MARGIN = TR.LOGIT_MARGIN
SPAN = 16.0
TOP, TAIL, DECOY = TR.TOP, TR.TAIL, TR.DECOY
HEAD = MAX_TOP + 2                   # built values of a row: the 9 that are compared and one more
NS = (0, 1, 5, 8)

MISREADINGS = ("temperature_scaled", "truncated_row", "text_kept_on_force", "tie_high_id", "normaliser_unfiltered")

RULE_SETS = {"rules": DO.Options(), "no rules": DO.Options(True, True)}
VOCABS = dict(DR.VOCABS)
VOCABS["1024"] = 1024


def rules_for(V):
    return TR.rules_for(V)


def all_suppressed(V) -> DO.Options:
    """a no-rules call whose list suppresses every id: nothing is allowed"""
    return DO.Options(True, True, tuple(range(V)))


def seq_sum_f32(values: Sequence[float]) -> np.float32:
    """the fp32 sum in step order from 0.0f: what sum_logprob holds after those steps"""
    s = np.float32(0.0)
    for v in values:
        s = np.float32(s + np.float32(v))
    return s


def row_logprobs(x: np.ndarray) -> np.ndarray:
    """fp64 log-softmax over A of a filtered row (-inf outside A; all -inf for an empty A)"""
    x = np.asarray(x, dtype=np.float64)
    fin = x > -np.inf
    if not fin.any():
        return np.full(len(x), -np.inf)
    m = x[fin].max()
    return np.where(fin, (x - m) - math.log(np.exp(x[fin] - m).sum()), -np.inf)


def top_of_row(x: np.ndarray, n: int, lp: Optional[np.ndarray] = None, high_id_first: bool = False) -> List[Tuple[int, float]]:
    """the rule on a filtered row x: n (id, lp) pairs, descending x, the lower id first among equals, (-1, -inf) once A is used up"""
    x = np.asarray(x, dtype=np.float64)
    lp = row_logprobs(x) if lp is None else lp
    ids = np.arange(len(x))
    order = np.lexsort((-ids if high_id_first else ids, -x))
    out = []
    for k in range(n):
        v = int(order[k]) if k < len(x) else -1
        out.append((v, float(lp[v])) if v >= 0 and x[v] > -np.inf else (-1, -math.inf))
    return out


def rule(logits: torch.Tensor, sampled: Sequence[int], rules, opts: DO.Options, n: int, temperature: float = 0.0,
         trunc: Optional[TR.Params] = None, misreading: Optional[str] = None):
    """-> (lp [V] fp64 over the row the step draws from, top: n (id, lp) pairs).  temperature and trunc enter only through the
    misreadings that would use them."""
    assert misreading is None or misreading in MISREADINGS
    flt = TR.filtered_row(logits, list(sampled), rules, opts, force=misreading != "text_kept_on_force")
    x = flt.numpy().astype(np.float64)
    if misreading == "temperature_scaled" and temperature > 0.0:
        x = x / float(np.float32(temperature))
    lp = row_logprobs(x)
    if misreading == "normaliser_unfiltered":        # the normaliser over the raw row, banned ids included
        raw = logits.double().numpy()
        lp = np.where(x > -np.inf, x - (raw.max() + math.log(np.exp(raw - raw.max()).sum())), -np.inf)
    if misreading == "truncated_row" and trunc is not None:
        keep = TR.keep_set(flt.numpy(), trunc).mask
        x = np.where(keep, x, -np.inf)
    return lp, top_of_row(x, n, lp=np.where(x > -np.inf, lp, -np.inf), high_id_first=misreading == "tie_high_id")


# ---------------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------------
def _thread(v):
    return (v % 4096) // 4


TIE_KINDS = ("one thread, two groups", "neighbouring threads", "different waves")


def tie_pair_ok(kind, a, b) -> bool:
    """a < b, placed as `kind` says in the kernel's layout"""
    if kind == "one thread, two groups":
        return _thread(a) == _thread(b) and a // 4096 != b // 4096
    if kind == "neighbouring threads":
        return a // 4096 == b // 4096 and _thread(b) == _thread(a) + 1
    return _thread(a) // 64 != _thread(b) // 64


def _tie_pair(kind, pool: np.ndarray, g) -> Optional[Tuple[int, int]]:
    have = set(int(v) for v in pool)
    for a in g.permutation(pool):
        a = int(a)
        cand = {"one thread, two groups": [a + 4096, a + 8192], "neighbouring threads": [a + 4 - a % 4], "different waves": [a + 256, a + 1024]}[kind]
        for b in cand:
            if b in have and tie_pair_ok(kind, a, b):
                return a, b
    return None


def _head_values(g, tie_rank: Optional[int]) -> np.ndarray:
    gaps = g.uniform(LOGIT_MARGIN + 0.02, 1.4, HEAD)
    gaps[0] = 0.0
    if tie_rank is not None:
        gaps[tie_rank + 1] = 0.0
    return (TOP - np.cumsum(gaps)).astype(np.float32)


def _row(V, rules, opts, kind, g, tie: Optional[str] = None) -> DR.SelectCase:
    tsb = rules.timestamp_begin
    sup = set(DO.suppress_list(rules, opts)) | {rules.no_timestamps, rules.blank, rules.eot, rules.sot, rules.sot_prev, rules.no_speech}
    text_ids = np.array([v for v in range(rules.eot) if v not in sup and not DR.TEXT <= v < DR.TEXT + 8])
    lg = (TAIL + 0.5 * g.standard_normal(V)).astype(np.float32)
    banned = [int(v) for v in list(DO.suppress_list(rules, opts))[:3]]
    tie_rank = None if tie is None else int(g.integers(1, 4))
    if kind == "first step":
        sampled = []
        if opts.without_timestamps:
            ids = g.choice(text_ids, HEAD, replace=False)
            banned += [rules.blank, rules.eot]
        else:
            ids = tsb + g.permutation(min(TR.MAX_INITIAL_TS + 1, V - tsb))     # all that is allowed: 5 ids (4 where the vocabulary ends)
            banned += [int(v) for v in g.choice(text_ids, 3, replace=False)] + [v for v in [tsb + TR.MAX_INITIAL_TS + 1] if v < V]
    elif kind == "forced timestamp":
        sampled = [tsb + 3, DR.TEXT]
        pool = np.arange(tsb + 4, V)
        ids = g.choice(pool, HEAD, replace=False)
        banned += [tsb, tsb + 2]
    else:                            # mid text
        sampled = [tsb + 3, DR.TEXT, DR.TEXT + 1]
        pool = text_ids
        ids = g.choice(pool, HEAD, replace=False)
        if not opts.without_timestamps:
            banned += [tsb + 1]
    ids = [int(v) for v in ids]
    if tie is not None:
        pair = _tie_pair(tie, pool, g)
        assert pair is not None, (tie, V, kind)
        rest = [v for v in ids if v not in pair][:HEAD - 2]
        ids = rest[:tie_rank] + list(pair) + rest[tie_rank:]
    vals = _head_values(g, tie_rank)
    lg[ids] = vals[:len(ids)]
    if kind == "forced timestamp":   # text inside the top that the force rule removes: between ranks, half a margin from both
        lg[g.choice(text_ids, 3, replace=False)] = np.float32(TOP - 0.3)
    lg[banned] = np.float32(DECOY)
    lg[rules.no_speech] = np.float32(1.0)
    name = kind if tie is None else f"{kind}, tie at ranks {tie_rank}, {tie_rank + 1} ({tie})"
    return DR.SelectCase(name, torch.from_numpy(lg), sampled, prompt=[rules.sot], tie=tie is not None)


def logprob_cases(V, rules, opts: DO.Options, seed=0) -> List[DR.SelectCase]:
    """The rows of ONE launch: a finished row, a row in its prompt phase, a first-step row, mid-text rows, under the rules a
    forced-timestamp row, and a row per tie placement the vocabulary has room for."""
    g = np.random.default_rng(seed * 1000003 + V + (7 if opts.without_timestamps else 0))
    tsb = rules.timestamp_begin
    bg = torch.full((V,), TAIL)
    bg[DR.TEXT + 2] = TOP
    cases = [DR.SelectCase("finished row", bg.clone(), [tsb, DR.TEXT], prompt=[rules.sot], done=1, sum_logprob=-1.5),
             DR.SelectCase("prompt phase", bg.clone(), [], prompt=[rules.sot_prev, 11, rules.sot], pos=0)]
    forced = not opts.without_timestamps and V - (tsb + 4) >= 2 * HEAD       # room for a head of timestamps behind tsb + 3
    kinds = ["first step", "mid text", "mid text"] + (["forced timestamp"] if forced else [])
    cases += [_row(V, rules, opts, k, g) for k in kinds]
    for tie in TIE_KINDS:
        if tie == "one thread, two groups" and rules.eot <= 4096 + 500:
            continue                 # a vocabulary without a second 4096-group of text ids
        cases.append(_row(V, rules, opts, "mid text", g, tie))
    if forced:
        cases.append(_row(V, rules, opts, "forced timestamp", g, "neighbouring threads"))
    return cases


def samples(case: DR.SelectCase) -> bool:
    return not case.done and case.pos is None


def case_margins(case, rules, opts, n=MAX_TOP):
    """-> (smallest gap between unequal neighbours among the n + 1 best allowed values, the span of those values, the number of exact
    ties among them, how many ids are allowed)"""
    x = TR.filtered_row(case.logits, case.sampled, rules, opts).double().numpy()
    best = np.sort(x[x > -np.inf])[::-1][:n + 1]
    d = -np.diff(best)
    gaps = d[d > 0]
    return (float(gaps.min()) if len(gaps) else math.inf, float(best[0] - best[-1]) if len(best) else 0.0, int((d == 0).sum()),
            int((x > -np.inf).sum()))
