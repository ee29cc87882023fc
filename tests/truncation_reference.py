"""Truncated sampling (top_k, top_p, min_p) restated: the rule of include/ccx.h ccx_decode_sampling_options in fp64 numpy, the truncated
Gumbel draw on top of oracle/whisper_ref's Philox noise, one step of the select kernel's state machine with it, and a generator of
kernel rows whose every decision has a margin, so that kept sets, cuts and tokens can be compared EXACTLY with the fp32 kernel:

  * every row has a head of ids with probability >= 1e-2 under softmax(x / T), then a tail far below it;
  * the top_p boundary lies in the head, at least MASS_MARGIN = 2e-3 of (renormalised) mass from both neighbouring cumulative values;
  * the top_k boundary (k-th against (k+1)-th value) and the min_p threshold are at least LOGIT_MARGIN = 0.5 from the nearest value;
  * ties are built on purpose (equal fp32 values: exact on every side) at the k-th value and at the top_p boundary.

MUTATIONS names wrong readings of the rule; tests/test_truncation_reference_cpu.py shows that every one of them changes some generated
case, so a kernel that implemented it would fail the GPU tests built on these rows.
"""
import math
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle import whisper_ref as R
from tests import dec_reference as DR
from tests import decoding_options_reference as DO

MASS_MARGIN = 2e-3
LOGIT_MARGIN = 0.5
HEAD_PROB = 1e-2

MUTATIONS = ("top_p_non_strict", "top_k_strict", "top_p_before_top_k", "min_p_before_top_p", "no_renormalisation", "min_p_without_T",
             "before_force_ts", "truncated_logprob", "ties_split")


@dataclass(frozen=True)
class Params:
    temperature: float
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0


@dataclass
class Kept:
    mask: np.ndarray                 # [V] bool: K
    cut: float                       # the smallest kept logit (-inf: nothing allowed)
    n: int                           # |K|
    mass: float                      # mass of K under softmax(x / T) over A (fp64)
    mass_margin: float               # distance of top_p from the nearest cumulative value it is compared with (inf: step off)
    logit_margin: float              # distance of the top_k / min_p boundaries from the nearest value (inf: steps off)


def _top_k(xs, k, strict=False):
    if k <= 0:
        return np.ones(len(xs), bool), math.inf
    order = np.sort(xs)[::-1]
    c1 = order[k - 1] if len(xs) >= k else order[-1]
    keep = xs > c1 if strict else xs >= c1
    below = order[order < c1]
    margin = float(c1 - below[0]) if len(below) else math.inf     # ties at c1 stay: only the next smaller value can be confused
    return keep, margin


def _top_p(xs, alive, T, p, strict=True, renorm=True, split_ties=False):
    """keep v (alive) iff the alive mass strictly above x_v, over the alive total, is < p"""
    if p >= 1.0:
        return alive.copy(), math.inf
    w = np.where(alive, np.exp((xs - xs.max()) / T), 0.0)
    total = w.sum() if renorm else np.exp((xs - xs.max()) / T).sum()
    order = np.argsort(-xs, kind="stable")
    above = np.empty(len(xs))
    if split_ties:                   # HF's sort: equal values get different cumulative sums
        above[order] = np.cumsum(w[order]) - w[order]
    else:
        vals, inv = np.unique(-xs, return_inverse=True)            # ascending in -x: descending in x
        per_val = np.bincount(inv, weights=w, minlength=len(vals))
        cum = np.cumsum(per_val)
        above = (cum - per_val)[inv] if strict else cum[inv]
    above = above / total
    keep = alive & (above < p)
    margin = float(np.abs(above[alive] - p).min())
    return keep, margin


def _min_p(xs, T, m, with_T=True):
    if m <= 0.0:
        return np.ones(len(xs), bool), math.inf
    mx = np.float32(xs.max())
    lnm = np.log(np.float32(m))
    c3 = mx + (np.float32(T) * lnm if with_T else lnm)             # fp32, product and sum rounded separately
    return xs >= np.float64(c3), float(np.abs(xs - np.float64(c3)).min())


def keep_set(x, prm: Params, mutation: Optional[str] = None) -> Kept:
    """x [V]: the row after EVERY filter (-inf: banned), any float dtype; evaluated in fp64 on the row's fp32 values."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    V, T = len(x), float(np.float32(prm.temperature))
    A = np.nonzero(x > -np.inf)[0]
    if len(A) == 0:
        return Kept(np.zeros(V, bool), -math.inf, 0, 0.0, math.inf, math.inf)
    xs = x[A]
    p, m = float(np.float32(prm.top_p)), float(np.float32(prm.min_p))
    if mutation == "top_p_before_top_k":
        k2, mm = _top_p(xs, np.ones(len(xs), bool), T, p)
        k1, lm1 = _top_k(np.where(k2, xs, -np.inf), prm.top_k)
        k1 &= k2
    else:
        k1, lm1 = _top_k(xs, prm.top_k, strict=mutation == "top_k_strict")
        alive = k1
        if mutation == "min_p_before_top_p":
            alive = k1 & _min_p(xs, T, m)[0]
        k2, mm = _top_p(xs, alive, T, p, strict=mutation != "top_p_non_strict", renorm=mutation != "no_renormalisation",
                        split_ties=mutation == "ties_split")
    k3, lm3 = _min_p(xs, T, m, with_T=mutation != "min_p_without_T")
    keep = k1 & k2 & k3
    keep[np.argmax(xs)] = True       # the maximum always survives (every step keeps it; stated for the mutations that would not)
    w = np.exp((xs - xs.max()) / T)
    mask = np.zeros(V, bool)
    mask[A[keep]] = True
    return Kept(mask, float(xs[keep].min()), int(keep.sum()), float(w[keep].sum() / w.sum()), mm, min(lm1, lm3))


def filtered_row(logits, sampled, rules, opts: DO.Options = DO.Options(), force: bool = True) -> torch.Tensor:
    """the row the kernel truncates: every filter, the forced-timestamp ban included (force=False: without that ban, for the mutation)"""
    lg32 = logits.float()
    if force:
        return DO.apply_filters(lg32, sampled, rules, opts)
    z = torch.zeros_like(lg32)
    z[:rules.timestamp_begin] = 1e4                       # text far above the timestamp mass: the ban stays out, the filters remain
    allowed = torch.isfinite(DO.apply_filters(z, sampled, rules, opts))
    return torch.where(allowed, lg32, torch.full_like(lg32, -math.inf))


def truncated_draw(flt: torch.Tensor, prm: Params, seed: int, row: int, step: int, keep: np.ndarray):
    """Gumbel-max over the kept ids with the noise of the untruncated sampler -> (token, scores [V] with -inf outside K)"""
    _, _, score = R.sample_token(flt, float(prm.temperature), seed, row, step)
    score = torch.where(torch.from_numpy(keep), score, torch.full_like(score, -math.inf))
    return int(score.argmax()), score


@dataclass
class TruncStep:
    res: DR.StepResult
    kept: Optional[Kept] = None      # None: the row did not sample


def select_step_ref(logits, st: DR.SeqState, prompt, gen, rules, opts: DO.Options, sample_len, tok_emb, pos_emb, prm: Params, seed=0,
                    row=0, mutation: Optional[str] = None) -> TruncStep:
    """tests/decoding_options_reference.select_step_ref with the truncation between the filters and the draw"""
    st = replace(st)
    gen = list(gen)
    if st.pos < st.prompt_len - 1 or st.done:
        return TruncStep(DO.select_step_ref(logits, st, prompt, gen, rules, opts, sample_len, tok_emb, pos_emb))
    i_gen = st.n_gen
    lg32 = logits.float()
    if i_gen == 0:
        st.no_speech_prob = float(torch.softmax(lg32.double(), dim=-1)[rules.no_speech])
    flt = filtered_row(lg32, gen[:i_gen], rules, opts)
    seen = filtered_row(lg32, gen[:i_gen], rules, opts, force=False) if mutation == "before_force_ts" else flt
    kept = keep_set(seen.numpy(), prm, mutation)
    keep = kept.mask & torch.isfinite(flt).numpy()
    if not keep.any():                                    # (only a mutation gets here)
        keep = torch.isfinite(flt).numpy()
    nxt, score = truncated_draw(flt, prm, seed, row, i_gen, keep)
    top2 = torch.topk(score.double(), 2).values
    norm_over = torch.where(torch.from_numpy(keep), flt, torch.full_like(flt, -math.inf)) if mutation == "truncated_logprob" else flt
    logprob = float(torch.log_softmax(norm_over.double(), dim=-1)[nxt])
    st.sum_logprob = st.sum_logprob + logprob
    gen[i_gen] = nxt
    st.n_gen = i_gen + 1
    st.pen_tok, st.last_tok = st.last_tok, nxt
    if nxt >= rules.timestamp_begin:
        st.last_ts_tok = nxt
    res = DR.StepResult(st, gen, None, None, None, 0, token=nxt, logprob=logprob, margin=float(top2[0] - top2[1]), scores=score)
    if nxt == rules.eot:
        st.done, st.n_tokens, res.finished = 1, i_gen, 1
    elif st.n_gen >= sample_len:
        st.done, st.n_tokens, res.finished = 1, st.n_gen, 1
    else:
        st.pos += 1
        res.cur_tok, res.pos, res.x = nxt, st.pos, tok_emb[nxt] + pos_emb[st.pos]
    return TruncStep(res, kept)


# ---------------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------------
VOCABS = {"1024": 1024, "small.en / mini": 51864}
TOP, TAIL, DECOY = 6.0, -40.0, 9.0
MAX_INITIAL_TS = 4                   # the first-step row has 5 allowed ids: fewer than PARAM_SETS["all three"].top_k

PARAM_SETS = {
    "top_p": Params(1.0, 0, 0.6, 0.0),
    "top_k": Params(0.7, 4, 1.0, 0.0),
    "min_p": Params(0.5, 0, 1.0, 0.1),
    "k then p": Params(1.0, 3, 0.7, 0.0),
    "p and min_p": Params(1.0, 0, 0.8, 0.3),
    "all three": Params(0.5, 6, 0.8, 0.05),
    "cold": Params(0.2, 0, 0.9, 0.001),
}


def rules_for(V):
    if V == 1024:                    # a small vocabulary of its own: 600 text ids, a few specials, 416 timestamps
        return R.Rules(eot=600, sot=601, sot_prev=602, no_speech=603, no_timestamps=604, timestamp_begin=608, blank=220,
                       max_initial_timestamp_index=MAX_INITIAL_TS, suppress=(1, 2, 7, 50, 300, 601, 602, 603, 605))
    return DR.rules_for(V, MAX_INITIAL_TS)


def _head(g: np.random.Generator, n: int, prm: Params, tie_at: Optional[int] = None) -> np.ndarray:
    """n descending fp32 logits from TOP down, the first four at least with probability >= HEAD_PROB at the row's temperature, gaps
    random; tie_at = i: values i and i + 1 are EQUAL"""
    T = prm.temperature
    for _ in range(10000):
        gaps = g.uniform(0.05, 0.7, n) * T
        gaps[0] = 0.0
        if 0 < prm.top_k < n:
            gaps[prm.top_k] += LOGIT_MARGIN              # the k-th value stands clear of the next one
        if tie_at is not None:
            gaps[tie_at + 1] = 0.0
            if tie_at + 1 == prm.top_k and prm.top_k + 1 < n:
                gaps[prm.top_k + 1] += LOGIT_MARGIN      # the tie straddles the k-th place: the gap goes behind it
        x = TOP - np.cumsum(gaps)
        if prm.min_p > 0.0:                              # a clear band around the min_p threshold
            c3 = TOP + T * math.log(prm.min_p)
            near = np.nonzero(x < c3 + LOGIT_MARGIN + 0.01)[0]
            if len(near) and x[near[0]] > c3 - LOGIT_MARGIN - 0.01:
                x[near[0]:] -= x[near[0]] - (c3 - LOGIT_MARGIN - 0.01)
        x = x.astype(np.float32)
        w = np.exp((x.astype(np.float64) - x[0]) / T)
        if ((w / w.sum()) >= 1.5 * HEAD_PROB).sum() >= min(n, 4):        # (a value pushed below a boundary may leave the head)
            return x
    raise AssertionError("no head found")


def _row(V, rules, opts, kind, g, prm, tie_at=None):
    """-> DR.SelectCase of one kind, or None when this draw misses a margin (the caller draws again)"""
    tsb, nts = rules.timestamp_begin, V - rules.timestamp_begin
    sup = set(DO.suppress_list(rules, opts)) | {rules.no_timestamps, rules.blank, rules.eot, rules.sot, rules.sot_prev, rules.no_speech}
    text_ids = np.array([v for v in range(min(rules.eot, 5000)) if v not in sup and not DR.TEXT <= v < DR.TEXT + 8])
    lg = (TAIL + 0.5 * g.standard_normal(V)).astype(np.float32)
    banned_decoys = [v for v in list(DO.suppress_list(rules, opts))[:3]]
    if kind == "first step":
        sampled = []
        n = MAX_INITIAL_TS + 1 if not opts.without_timestamps else 7
        ids = tsb + g.permutation(n) if not opts.without_timestamps else g.choice(text_ids, n, replace=False)
        if not opts.without_timestamps:
            banned_decoys += [int(v) for v in g.choice(text_ids, 3, replace=False)] + [tsb + MAX_INITIAL_TS + 1]
        else:
            banned_decoys += [rules.blank, rules.eot]
        lg[ids] = _head(g, n, prm, tie_at)
    elif kind == "forced timestamp":
        sampled = [tsb + 3, DR.TEXT]
        n = int(g.integers(7, 11))
        ids = tsb + 4 + g.permutation(min(nts - 4, 300))[:n]
        lg[ids] = _head(g, n, prm, tie_at)
        lg[g.choice(text_ids, 3, replace=False)] = np.float32(TOP - 0.3)     # text that the ban removes: it would sit in every top_k
        banned_decoys += [tsb, tsb + 2]
    else:                            # mid text
        sampled = [tsb + 3, DR.TEXT, DR.TEXT + 1]
        n = int(g.integers(7, 11))
        ids = g.choice(text_ids, n, replace=False)
        lg[ids] = _head(g, n, prm, tie_at)
        if not opts.without_timestamps:
            banned_decoys += [tsb + 1]
    lg[banned_decoys] = np.float32(DECOY)
    lg[rules.no_speech] = np.float32(1.0)                 # (suppressed; read by the first step's no-speech probability only)
    case = DR.SelectCase(f"{kind}{'' if tie_at is None else f' (tie at {tie_at})'}", torch.from_numpy(lg), sampled, prompt=[rules.sot])
    return case if margins_ok(case, rules, opts, prm) else None


def case_kept(case, rules, opts, prm, mutation=None) -> Kept:
    seen = filtered_row(case.logits, case.sampled, rules, opts, force=mutation != "before_force_ts")
    return keep_set(seen.numpy(), prm, mutation)


def head_of(case, rules, opts, prm) -> np.ndarray:
    """ids with probability >= HEAD_PROB under softmax(x / T) of the filtered row"""
    x = filtered_row(case.logits, case.sampled, rules, opts).double().numpy()
    w = np.exp((x - x.max()) / prm.temperature)
    return np.nonzero(w / w.sum() >= HEAD_PROB)[0]


def margins_ok(case, rules, opts, prm) -> bool:
    k = case_kept(case, rules, opts, prm)
    x = filtered_row(case.logits, case.sampled, rules, opts).numpy()
    head = head_of(case, rules, opts, prm)
    # the top_p boundary in the head: the smallest kept value is a head value (the tail is then dropped as a whole or kept by top_p = 1)
    in_head = prm.top_p >= 1.0 or bool(np.isin(np.nonzero(x == np.float32(k.cut))[0], head).all())
    if not opts.without_timestamps:
        gap = DR._force_gap(case.logits.float(), case.sampled, rules)
        if abs(gap) < 0.05:
            return False
    return k.mass_margin >= MASS_MARGIN and k.logit_margin >= LOGIT_MARGIN and in_head and len(head) >= 2


def trunc_cases(V, rules, opts: DO.Options, prm: Params, seed=0) -> List[DR.SelectCase]:
    """The rows of ONE launch: a finished row, a row in its prompt phase, a first-step row (under the rules: MAX_INITIAL_TS + 1 allowed
    ids), a forced-timestamp row (under the rules), mid-text rows, and rows with a tie at the boundary."""
    g = np.random.default_rng(seed * 1000003 + V + int(1000 * prm.temperature) + 17 * prm.top_k)
    tsb = rules.timestamp_begin
    bg = torch.full((V,), TAIL)
    bg[DR.TEXT + 2] = TOP
    cases = [DR.SelectCase("finished row", bg.clone(), [tsb, DR.TEXT], prompt=[rules.sot], done=1, sum_logprob=-1.5),
             DR.SelectCase("prompt phase", bg.clone(), [], prompt=[rules.sot_prev, 11, rules.sot], pos=0)]
    kinds = ["first step", "mid text", "mid text"] + ([] if opts.without_timestamps else ["forced timestamp"])
    wanted = [(kind, None) for kind in kinds]
    # ties: at the k-th value (values k - 1 and k equal), else two values in the middle of the head
    wanted.append(("mid text", prm.top_k - 1 if prm.top_k >= 2 else 2))
    if not opts.without_timestamps:
        wanted.append(("forced timestamp", 1))
    for kind, tie in wanted:
        for _ in range(4000):
            c = _row(V, rules, opts, kind, g, prm, tie)
            if c is not None:
                break
        else:
            raise AssertionError(f"no row with margins for {kind} (tie {tie}) under {prm}")
        cases.append(c)
    return cases
