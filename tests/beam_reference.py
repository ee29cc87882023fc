"""Beam search as the product implements it, restated in plain Python with fp64 scores, and the generator of the beam kernels' test cases.
CPU only.  [UPSTREAM-RECALL: decoding.py::BeamSearchDecoder, MaximumLikelihoodRanker, DecodingTask._main_loop]; parity unpinned.

The rule, per window of `beam` rows and step:
  candidates  every row filters its logits as the select kernel does (oracle.whisper_ref.apply_filters: suppress mask, timestamp rules
              from the row's own tokens, text banned when the timestamps' mass beats the best text logit -- the filtered row whose
              arg-max tests/dec_reference.py::folded_select restates), takes log_softmax and proposes its top beam + 1 ids; cumulative
              score = the row's sum_logprob + logprob.  On the first sampled step only row 0 proposes (equal prefixes collapse).
  survivors   walk the candidates by descending score: one that ends in eot is finished in this step, any other becomes the next live
              row until `beam` are taken, then the walk stops (eot candidates below the last survivor are dropped).  Newly finished
              ones join the window's finished list, best first, while it holds fewer than max_candidates = round(beam * patience).
  completion  a window whose finished list holds max_candidates is complete and freezes; the loop also ends at sample_len.
  finalize    a window with fewer than `beam` finished hypotheses takes its live rows by descending sum_logprob, eot appended.
  ranker      tokens cut at the first eot; sum_logprob / len, or sum_logprob / ((5 + len) / 6) ** length_penalty; empty: -inf; the
              first maximum wins.
Ties (equal cumulative scores) go to the lower source row, then the lower id; the generated cases have none.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import whisper_ref as R

ROW_GAP = 0.5        # filtered logits ranked beam + 1 and beam + 2 of a generated row are at least this far apart
SCORE_GAP = 0.05     # ... and a window's candidate cumulative scores pairwise at least this


def max_candidates(beam: int, patience: Optional[float] = None) -> int:
    return round(beam * (1.0 if patience is None else patience))


def filtered_logprobs(logits: torch.Tensor, sampled: Sequence[int], rules) -> torch.Tensor:
    """fp64 log_softmax of the row after the select kernel's filters"""
    return torch.log_softmax(R.apply_filters(logits.float(), list(sampled), rules).double(), dim=-1)


def propose(logits: torch.Tensor, sampled: Sequence[int], rules, k: int) -> List[Tuple[int, float]]:
    """the row's top k (id, logprob), best first, equal values by ascending id; ids without mass are not proposed"""
    lp = filtered_logprobs(logits, sampled, rules).numpy()
    order = np.lexsort((np.arange(len(lp)), -lp))[:k]
    return [(int(i), float(lp[i])) for i in order if np.isfinite(lp[i])]


def sorted_filtered(logits, sampled, rules):
    """the filtered logits of a row in descending order (the generator's gap condition reads ranks beam + 1 and beam + 2)"""
    x = R.apply_filters(logits.float(), list(sampled), rules).double().numpy()
    return np.sort(x[np.isfinite(x)])[::-1]


@dataclass
class Row:
    tokens: List[int]
    sum_logprob: float


@dataclass
class Window:
    rows: List[Row]
    finished: List[Tuple[List[int], float]] = field(default_factory=list)   # (tokens before the eot, score), insertion order
    complete: bool = False


def walk(cands: Sequence[Tuple[float, int, int]], beam: int, eot: int):
    """cands: (cumulative score, source row, id).  -> (survivors, finished) as lists of candidates, in walk order."""
    order = sorted(cands, key=lambda c: (-c[0], c[1], c[2]))
    survivors, finished = [], []
    for c in order:
        if c[2] == eot:
            finished.append(c)
        else:
            survivors.append(c)
            if len(survivors) == beam:
                break
    return survivors, finished


def apply_walk(win: Window, cands, beam: int, max_cand: int, eot: int, sample_len: int):
    """One step of a live window from its candidates.  Returns dict(tokens, parents, scores, appended) and updates the window."""
    survivors, finished = walk(cands, beam, eot)
    assert len(survivors) == beam, "the generated cases always leave `beam` continuations"
    appended = []
    for c in finished:                      # already in descending score
        if len(win.finished) >= max_cand:
            break
        win.finished.append((list(win.rows[c[1]].tokens), c[0]))
        appended.append(c)
    win.rows = [Row(win.rows[c[1]].tokens + [c[2]], c[0]) for c in survivors]
    if len(win.finished) >= max_cand or len(win.rows[0].tokens) >= sample_len:
        win.complete = True
    return dict(tokens=[c[2] for c in survivors], parents=[c[1] for c in survivors], scores=[c[0] for c in survivors],
                appended=appended, finished=finished)


def step(win: Window, logits_rows, rules, beam: int, max_cand: int, sample_len: int):
    """One step from the rows' logits.  -> (proposals per row, apply_walk's record)"""
    first = len(win.rows[0].tokens) == 0
    props, cands = [], []
    for j, row in enumerate(win.rows):
        pr = [] if (first and j > 0) else propose(logits_rows[j], row.tokens, rules, beam + 1)
        props.append(pr)
        cands += [(row.sum_logprob + lp, j, i) for i, lp in pr]
    return props, apply_walk(win, cands, beam, max_cand, rules.eot, sample_len)


def finalize(win: Window, beam: int) -> List[Tuple[List[int], float]]:
    """(tokens before the eot, sum_logprob) of the window's hypotheses in insertion order"""
    out = list(win.finished)
    if len(out) < beam:
        for j in sorted(range(len(win.rows)), key=lambda j: (-win.rows[j].sum_logprob, j)):
            out.append((list(win.rows[j].tokens), win.rows[j].sum_logprob))
            if len(out) >= beam:
                break
    return out


def rank(hyps: Sequence[Tuple[Sequence[int], float]], eot: int, length_penalty: Optional[float] = None) -> int:
    best, best_score = 0, None
    for k, (toks, slp) in enumerate(hyps):
        toks = list(toks)
        if eot in toks:
            toks = toks[:toks.index(eot)]
        n = len(toks)
        if n == 0:
            score = -math.inf
        elif length_penalty is None:
            score = slp / n
        else:
            score = slp / (((5 + n) / 6) ** length_penalty)
        if best_score is None or score > best_score:
            best, best_score = k, score
    return best


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel cases: three windows per launch
# ---------------------------------------------------------------------------------------------------------------------------------
SAMPLE_LEN, N_POS, D, TEXT = 8, 64, 64, 400
BACKGROUND = -20.0


@dataclass
class BeamCase:
    """One launch: G = 3 windows of `beam` rows.  Window 0 is complete (must stay untouched), window 1 takes its first step, window
    2 is three tokens in.  variant "eot": eot tops row 0 (and row 1), closes the last row's proposals, and the finished list of window
    2 is one short of max_cand, so it fills mid-step and the window completes; "force": one row's timestamp mass beats its best
    text token, nothing finishes, the window goes on."""
    beam: int
    max_cand: int
    variant: str
    logits: torch.Tensor                 # [R][V]
    sampled: List[List[int]]             # per row
    sum_logprob: List[float]
    done: List[int]
    prompt_len: int
    fin_count: List[int]


def rules_for(V):
    """51864: the English tokenizer's ids with the product's suppress list; a small vocabulary: the same roles packed below V"""
    if V >= 51864:
        from tests import dec_reference as DR
        return DR.rules_for(V)
    return R.Rules(eot=V - 24, sot=V - 23, sot_prev=V - 22, no_speech=V - 21, no_timestamps=V - 20, timestamp_begin=V - 16, blank=220,
                   max_initial_timestamp_index=50, suppress=(1, 2, 7, 11, V - 23, V - 22, V - 21))


def _tops(g, K):
    """the proposals' logits: 0.8 apart, the same in every row, so that all rows share one log-normaliser (the background's mass is
    e^-11 of it) and cumulative scores differ by the rows' sum_logprob lattice below"""
    return 6.0 - 0.8 * torch.arange(K, dtype=torch.float32)


def beam_case(V: int, rules, beam: int, variant: str, seed: int = 0, patience: Optional[float] = None) -> BeamCase:
    tsb, eot = rules.timestamp_begin, rules.eot
    K = beam + 1
    mc = max_candidates(beam, patience)
    nts = V - tsb
    a = 3 if nts > 1000 else 0
    banned = set(rules.suppress) | {rules.no_timestamps, rules.blank, eot}
    pool = torch.tensor([i for i in range(10, min(eot, tsb)) if i not in banned and not (TEXT <= i < TEXT + 32)])
    for attempt in range(200):
        g = torch.Generator().manual_seed(90000 + 1000 * seed + 17 * beam + (0 if variant == "eot" else 7) + V % 101 + 100003 * attempt)
        R_ = 3 * beam
        logits = BACKGROUND + 0.5 * torch.randn(R_, V, generator=g)
        sampled, slp, done = [], [], []
        # window 0: complete
        for j in range(beam):
            sampled.append([tsb + a, TEXT, TEXT + 1 + j, eot][:3]); slp.append(-2.0 - 0.3 * j); done.append(1)
            logits[j, pool[torch.randperm(len(pool), generator=g)[:K]]] = _tops(g, K)
        # window 1: first step -- timestamps [tsb, tsb + max_initial] only; every row holds logits, row 0's decide
        for j in range(beam):
            r = beam + j
            sampled.append([]); slp.append(0.0); done.append(0)
            mit = rules.max_initial_timestamp_index
            span = min(nts, (mit + 1) if mit is not None and mit >= 0 else nts)
            ids = tsb + torch.randperm(span, generator=g)[:min(K, span)]
            logits[r, ids] = _tops(g, len(ids)) + (0.0 if j == 0 else 3.0)      # other rows would outbid row 0 if they proposed
            logits[r, TEXT] = 9.0                                                 # banned decoys
            logits[r, rules.no_speech] = 2.0
        # window 2: three tokens in, all rows mid text after one timestamp
        for j in range(beam):
            r = 2 * beam + j
            # sum_logprob = -(1 + 0.1 res + 0.8 m), res a permutation of the residues and m in {0, 1, 2}: every pair of cumulative
            # scores -(1 + 0.1 res + 0.8 (m + k)) is >= 0.1 apart, some rows get several children and some none
            if j == 0:
                res = torch.randperm(8, generator=g)[:beam].tolist()
                ms = torch.randint(0, 3, (beam,), generator=g).tolist()
                if variant == "eot":          # the rows whose best proposal is eot stand high, the row that ends in eot low
                    ms[0] = 0
                    if beam > 2:
                        ms[1] = 0
                    if beam > 1:
                        ms[beam - 1] = 2
            sampled.append([tsb + a, TEXT + j, TEXT + 10 + j]); slp.append(-(1.0 + 0.1 * res[j] + 0.8 * ms[j])); done.append(0)
            ids = pool[torch.randperm(len(pool), generator=g)[:K]].clone()        # allowed text ids
            vals = _tops(g, K)
            if variant == "eot":
                if j == 0 or (j == 1 and beam > 2):
                    ids[0] = eot                                                  # eot tops rows 0 and 1: above every survivor
                if j == beam - 1 and beam > 1:
                    ids[K - 1] = eot                                              # ... and closes the last row: below the last survivor
                logits[r, ids] = vals
            elif j == (1 if beam > 1 else 0):
                # force rule: the timestamps' mass beats the best text token -> text banned, the proposals are timestamps
                ts = tsb + a + 1 + torch.randperm(min(nts - a - 1, 500), generator=g)[:K]
                if len(ts) < K:
                    break
                logits[r, ts] = vals
                logits[r, ids[0]] = float(vals[0]) + 0.2      # best text: above every timestamp, >= 0.17 below their summed mass
            else:
                if j == beam - 1 and beam > 1:
                    ids[K - 1] = eot
                logits[r, ids] = vals
            logits[r, tsb + a] = 9.0                                              # banned decoy: a timestamp not above the last one
        else:
            case = BeamCase(beam, mc, variant, logits, sampled, slp, done, 1, [mc, 0, mc - 1 if variant == "eot" else 0])
            if case_gaps_ok(case, rules):
                return case
    raise AssertionError("no decided case found")


def case_candidates(case: BeamCase, rules, window: int):
    """(cumulative score, local source row, id) of a window's proposals, and the proposals per row"""
    beam = case.beam
    rows = range(window * beam, (window + 1) * beam)
    first = len(case.sampled[window * beam]) == 0
    props, cands = [], []
    for j, r in enumerate(rows):
        pr = [] if (first and j > 0) else propose(case.logits[r], case.sampled[r], rules, beam + 1)
        props.append(pr)
        cands += [(case.sum_logprob[r] + lp, j, i) for i, lp in pr]
    return cands, props


def case_gaps_ok(case: BeamCase, rules) -> bool:
    beam = case.beam
    for w in (1, 2):
        for j in range(beam):
            r = w * beam + j
            if w == 1 and j > 0:
                continue
            x = sorted_filtered(case.logits[r], case.sampled[r], rules)
            if len(x) < beam + 1:
                return False
            if len(x) > beam + 1 and x[beam] - x[beam + 1] < ROW_GAP:
                return False
        sc = sorted(c[0] for c in case_candidates(case, rules, w)[0])
        if any(b - a_ < SCORE_GAP for a_, b in zip(sc, sc[1:])):
            return False
    return True


def case_window(case: BeamCase, window: int) -> Window:
    beam = case.beam
    return Window([Row(list(case.sampled[r]), case.sum_logprob[r]) for r in range(window * beam, (window + 1) * beam)])


KERNEL_CASES = [(beam, variant) for beam in (1, 2, 5, 8) for variant in ("eot", "force")]
KERNEL_VOCABS = (1024, 51864)
