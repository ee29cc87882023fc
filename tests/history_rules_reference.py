"""Plain numpy / torch statement of the two decoding rules over a row's own sampled history -- repetition_penalty and
no_repeat_ngram_size (include/ccx.h: ccx_decode_history_options; csrc/dec_history.hip) -- for the tests of
`WhisperModel(repetition_control=True)`.  The rule is this project's, in the form of Hugging Face's RepetitionPenaltyLogitsProcessor
and NoRepeatNGramLogitsProcessor (tests/test_history_rules_reference_cpu.py runs the installed ones beside it on histories of text
ids, where the two agree exactly); parity with CTranslate2 / faster-whisper is unpinned.

For one row in the sampling phase, H = the m tokens this decode has sampled so far (no prompt, SOT sequence or prefix), E = rules.eot
(ids >= E are never edited):
  1. penalty p != 1: every distinct v in H with v < E: x = logits[v]; logits[v] = x / p if x > 0 else x * p, in fp32, once per id
  2. n-gram ban n >= 1, only when m >= n: every i in [0, m - n] with H[i : i+n-1] == H[m-n+1 : m] and H[i+n-1] < E:
     logits[H[i+n-1]] = -inf (the matched context may hold ids >= E)
  1 before 2, both before SuppressBlank / SuppressTokens / ApplyTimestampRules (decoding_options_reference.apply_filters).

Also: the case generator of the kernel test (tests/test_dec_history_gpu.py) and the eps-argmax oracle walk under the rule.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from tests import dec_reference as DR
from tests.decoding_options_reference import WALK_EPS, Options, apply_filters

SETTINGS = ((1.3, 0), (1.0, 1), (1.0, 2), (1.0, 5), (1.5, 3))      # the five the kernel test launches
WALK_SETTINGS = ((1.3, 0), (1.0, 2), (1.5, 3))                       # the three the walks run
WALK_FREE_LEN = 24


def edited_ids(history: Sequence[int], text_end: int, penalty: float = 1.0, ngram: int = 0) -> Tuple[Set[int], Set[int]]:
    """(ids the penalty edits, ids the ban sets to -inf) for one row"""
    H = [int(t) for t in history]
    m = len(H)
    pen = {v for v in H if v < text_end} if penalty != 1.0 else set()
    ban: Set[int] = set()
    n = int(ngram)
    if n >= 1 and m >= n:
        tail = H[m - n + 1:m]
        for i in range(0, m - n + 1):
            if H[i:i + n - 1] == tail and H[i + n - 1] < text_end:
                ban.add(H[i + n - 1])
    return pen, ban


def apply_history_rules_np(logits: np.ndarray, history: Sequence[int], text_end: int, penalty: float = 1.0, ngram: int = 0) -> np.ndarray:
    """the rule on one fp32 row; returns a new array"""
    x = np.array(logits, dtype=np.float32, copy=True)
    pen, ban = edited_ids(history, text_end, penalty, ngram)
    p = np.float32(penalty)
    for v in sorted(pen):
        x[v] = x[v] / p if x[v] > 0 else x[v] * p
    for v in sorted(ban):
        x[v] = -np.inf
    return x


def apply_history_rules(logits: torch.Tensor, history: Sequence[int], text_end: int, penalty: float = 1.0, ngram: int = 0) -> torch.Tensor:
    """the torch face of apply_history_rules_np (fp32 in, fp32 out)"""
    return torch.from_numpy(apply_history_rules_np(logits.detach().float().cpu().numpy(), history, text_end, penalty, ngram))


def ngram_invariant_violations(tokens: Sequence[int], text_end: int, ngram: int) -> List[Tuple[int, int]]:
    """What a decode under no_repeat_ngram_size = n must never hold: two occurrences of an n-gram that ends in an id < text_end.
    -> [(first start, second start), ...] (empty: the invariant holds).  n = 1: no text id twice."""
    n = int(ngram)
    if n < 1:
        return []
    seen, bad = {}, []
    toks = [int(t) for t in tokens]
    for i in range(0, len(toks) - n + 1):
        g = tuple(toks[i:i + n])
        if g[-1] >= text_end:
            continue
        if g in seen:
            bad.append((seen[g], i))
        else:
            seen[g] = i
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel test's rows
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class HistoryRow:
    name: str
    history: List[int]
    logits: np.ndarray                       # [V] f32
    done: int = 0
    prompt_len: int = 1
    pos: Optional[int] = None                # None: the sampling phase at its natural position
    live: bool = field(init=False, default=True)

    def __post_init__(self):
        if self.pos is None:
            self.pos = self.prompt_len - 1 + len(self.history)
        self.live = not self.done and self.pos >= self.prompt_len - 1


def history_rows(V: int, text_end: int, timestamp_begin: int, sample_len: int, ngram: int, n_rows: int, seed: int = 0) -> List[HistoryRow]:
    """Rows of one launch.  Histories of every length the kernel treats differently -- 0, 1, n - 1, n, sample_len, 447 (where they fit)
    and a few in between -- in three styles: loops of period 1 .. 3 (n-gram hits), random text ids with duplicates, and mixes that hold
    the ids 0, eot - 1, eot, timestamp_begin and V - 1 (as a would-be ban and inside the matched context).  The logits of the ids a
    history holds cycle through a positive value, a negative one, 0.0 and -inf; the rest is N(0, 3).  Two rows are not in the sampling
    phase (a finished one and one in the prompt phase): whatever their history, nothing of them may change."""
    g = np.random.default_rng(9000 + 31 * seed + 7 * ngram + sample_len)
    E, tsb = text_end, timestamp_begin
    n = max(ngram, 1)
    lens = [0, 1, n - 1, n, n + 1, 2 * n + 1, sample_len, min(447, sample_len), sample_len - 1, 7, 33, 257]
    lens = [m for m in lens if 0 <= m <= sample_len]
    specials = [0, E - 1, E, tsb, V - 1]
    rows: List[HistoryRow] = []

    def logits_for(hist):
        lg = (3.0 * g.standard_normal(V)).astype(np.float32)
        vals = [2.5, -1.75, 0.0, -np.inf, 7.0, -0.001]
        for k, v in enumerate(sorted(set(hist))):
            lg[v] = vals[k % len(vals)]
        lg[int(g.integers(0, V))] = -np.inf          # an id outside the history: stays what it is
        return lg

    def hist_of(style, m):
        if m == 0:
            return []
        if style == 0:                               # a loop: every n-gram of the tail was seen before
            q = int(g.integers(1, 4))
            base = [int(t) for t in g.integers(10, 20000, size=q)]
            return [base[i % q] for i in range(m)]
        if style == 1:                               # text ids from a small pool: duplicates, some n-gram hits
            pool = g.integers(0, E, size=max(2, m // 3))
            return [int(t) for t in g.choice(pool, size=m)]
        h = [int(t) for t in g.choice(np.array(specials + [400, 401]), size=m)]      # style 2: specials as banned id and as context
        return h

    if n_rows < 3:                                   # a launch of one row: a loop of period 2 long enough for every n of the tests
        loop = [int(t) for t in g.integers(10, 20000, size=2)] * (min(sample_len, 2 * n + 2) // 2)
        return [HistoryRow(f"row {k}: a loop of {len(loop)}", loop, logits_for(loop)) for k in range(n_rows)]
    i = 0
    while len(rows) < n_rows - 2:
        m, style = lens[i % len(lens)], (i // len(lens) + i) % 3
        h = hist_of(style, m)
        rows.append(HistoryRow(f"row {len(rows)}: m = {m}, style {style}", h, logits_for(h), prompt_len=1 + (i % 3)))
        i += 1
    loop = [77, 78] * (min(sample_len, 12) // 2)
    rows.append(HistoryRow("a finished row", loop, logits_for(loop), done=1))
    rows.append(HistoryRow("a row in the prompt phase", loop, logits_for(loop), prompt_len=4, pos=1))
    return rows


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in fp32 representable values between equal-shaped arrays (the same non-finite value or the same zero: 0; one side
    non-finite, or the signs differ: a huge number)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    d = np.abs(ia - ib)
    same = (ia == ib) | ((a == 0) & (b == 0))
    bad = ~same & (~np.isfinite(a) | ~np.isfinite(b) | (np.signbit(a) != np.signbit(b)))
    return np.where(same, 0, np.where(bad, 2 ** 40, d))


# ---------------------------------------------------------------------------------------------------------------------------------
# composition with the select kernel: the 6 / 5 / 9 winner, rival and decoy convention of dec_reference.select_cases
# ---------------------------------------------------------------------------------------------------------------------------------
def composition_cases(V: int, rules, penalty: float, ngram: int, seed: int = 0) -> List[DR.SelectCase]:
    """Rows whose greedy token the history rule decides (or must leave alone): background -20 +- 0.5, the winner at 6, a legal rival
    at 5, banned decoys at 9.  `expect` is the id the row was built to produce under (penalty, ngram)."""
    g = torch.Generator().manual_seed(6000 + seed + V + 13 * ngram)
    tsb, eot = rules.timestamp_begin, rules.eot
    WIN, RIVAL, DECOY, TEXT = DR.WIN, DR.RIVAL, DR.DECOY, DR.TEXT
    cases: List[DR.SelectCase] = []

    def add(name, sampled, winner, rival, decoys=(), expect=None):
        assert winner not in rules.suppress and rival not in rules.suppress, name
        lg = DR.BACKGROUND + 0.5 * torch.randn(V, generator=g)
        lg[rival] = RIVAL
        for d_ in decoys:
            lg[d_] = DECOY
        lg[winner] = WIN
        cases.append(DR.SelectCase(name, lg, list(sampled), prompt=[rules.sot], sum_logprob=-1.5, expect=expect))

    n = ngram
    pen_on = penalty != 1.0
    assert not pen_on or WIN / penalty < RIVAL - 0.25, "the penalty must decide the 6 / 5 rows"
    # the winner is a text id of the history: the penalty drops it below the rival (6 / p < 5); n = 1 bans it
    hit = pen_on or n == 1
    add("winner in the history", [tsb + 1, TEXT, TEXT + 1], TEXT, 900, expect=900 if hit else TEXT)
    add("winner twice in the history", [tsb + 1, TEXT, TEXT, TEXT + 2], TEXT, 901, expect=901 if hit else TEXT)
    add("winner not in the history", [tsb + 1, TEXT, TEXT + 1], 902, 903, expect=902)
    # a decoy at a suppressed id stays banned by SuppressTokens behind the rule
    add("decoy at a suppressed id", [tsb + 1, TEXT, TEXT + 1], 904, 905, decoys=(rules.suppress[0],), expect=904)
    # the winner would complete an n-gram the history holds
    if n >= 2:
        ctx = [TEXT + 10 + k for k in range(n - 1)]
        add("winner completes a seen n-gram", [tsb + 1] + ctx + [906] + ctx, 906, 907, expect=907)
        add("winner behind another context", [tsb + 1] + ctx + [908] + [c + 50 for c in ctx], 908, 909, expect=909 if pen_on else 908)
    if n >= 3:
        # timestamps inside the matched context still match: the context ends in a closed pair <|t|><|t|>, behind which text is legal
        tctx = [TEXT + 20 + k for k in range(n - 3)] + [tsb + 1, tsb + 1]
        add("timestamps inside the matched context", tctx + [911] + tctx, 911, 912, expect=912)
    # ids >= eot are never edited: a timestamp that the history holds wins again where the timestamp rules allow it
    add("a timestamp of the history is exempt", [tsb + 3, TEXT, tsb + 5], tsb + 5, tsb + 9, expect=tsb + 5)
    add("eot is exempt", [tsb + 1, TEXT, TEXT + 1], eot, 910, expect=eot)
    # the first sampled step: an empty history, the rule does nothing
    lg0 = len(cases)
    add("step 0: empty history", [], tsb + 2, tsb + 4, expect=tsb + 2)
    cases[lg0].sum_logprob = 0.0
    cases[lg0].logits[rules.no_speech] = 2.0
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk of a decode through oracle/whisper_ref.WhisperRef under the rule and then the options' filters
# ---------------------------------------------------------------------------------------------------------------------------------
def walk_prompts(rules) -> dict:
    """name -> (prompt, Options) of the two decodes the walks run"""
    return {"default": ([rules.sot], Options()), "without_timestamps": ([rules.sot, rules.no_timestamps], Options(True))}


def oracle_walk(orc, xa_row, prompt: Sequence[int], rules, opts: Options, sample_len: int, penalty: float = 1.0, ngram: int = 0,
                forced: Optional[Sequence[int]] = None, eps: float = WALK_EPS) -> dict:
    """decoding_options_reference.oracle_walk with the history rule applied to the raw logits before the filters: free-running
    (forced None) or teacher-forced with a decode's tokens.  Every forced token must lie within eps of the oracle's edited and
    filtered maximum and equal its argmax where the margin exceeds 2 eps (`decisive` counts those steps).  sum_logprob (fp64) is
    taken from the edited logits; no_speech_prob from the raw ones at <|startoftranscript|>."""
    seq, sampled, decisive, violations, slp = list(prompt), [], 0, [], 0.0
    sot_index = list(prompt).index(rules.sot)
    no_speech = None
    n = sample_len if forced is None else len(forced)
    for i in range(n):
        logits = orc.decoder_logits(torch.tensor([seq]), xa_row)[0]
        if no_speech is None:
            no_speech = float(torch.softmax(logits[sot_index].double(), dim=-1)[rules.no_speech])
        lg = apply_filters(apply_history_rules(logits[-1].float(), sampled, rules.eot, penalty, ngram), sampled, rules, opts)
        top = torch.topk(lg.double(), 2).values
        margin = float(top[0] - top[1])
        t = int(lg.argmax()) if forced is None else int(forced[i])
        if float(lg[t]) < float(lg.max()) - eps:
            violations.append((i, t, int(lg.argmax()), float(lg.max()) - float(lg[t])))
        if margin > 2 * eps:
            decisive += 1
            if t != int(lg.argmax()):
                violations.append((i, t, int(lg.argmax()), "decisive"))
        slp += float(torch.log_softmax(lg.double(), dim=-1)[t])
        seq.append(t); sampled.append(t)
        if t == rules.eot:
            break
    return dict(tokens=sampled, steps=len(sampled), decisive=decisive, violations=violations, sum_logprob=slp, no_speech_prob=no_speech)
