"""Plain numpy / torch statement of the sequence bias -- sequence_bias, bad_words_ids and hotwords (include/ccx.h:
ccx_decode_bias_options; csrc/dec_bias.hip) -- for the tests of `WhisperModel(contextual_bias=True)`.  The rule is this project's, in
the form of Hugging Face's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (tests/test_bias_reference_cpu.py runs the
installed ones beside it with input_ids = H, where the two agree exactly but for entries whose context is the whole history, which HF
skips and this rule fires); parity is unpinned.

A table is an ordered list of entries (ids[0 .. L), bias): 1 <= L <= 32, every id in [0, n_vocab), the target ids[L - 1] < E =
rules.eot (ids >= E are never edited; context ids may be any id), bias finite or -inf.  For one row in the sampling phase, H = the m
tokens this decode has sampled so far (no prompt, SOT sequence or prefix):
  b1[v] = the fp32 sum, in table order, of the length-1 entries with target v
  S[v]  = the fp32 sum, in table order, of the entries with L >= 2, target v, L - 1 <= m and H[m - L + 1 : m] == ids[0 : L - 1]
  logits[v] = (logits[v] + b1[v]) + S[v]; a term that does not exist is skipped, not added as zero; each term lands once per id
before the history rules (history_rules_reference.apply_history_rules) and the filters (decoding_options_reference.apply_filters).

Also: a Python mirror of the library's table compile and of the kernel's walk over it, the rows of the kernel test
(tests/test_dec_bias_gpu.py), and the eps-argmax oracle walk under bias, history rules and filters in that order.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from tests.decoding_options_reference import WALK_EPS, Options, apply_filters
from tests.history_rules_reference import apply_history_rules

MAX_ENTRIES, MAX_IDS, MAX_LEN = 8192, 65536, 32
WALK_FREE_LEN = 24
Entry = Tuple[Tuple[int, ...], float]
NINF = float("-inf")


def to_arrays(entries: Sequence[Entry]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """entries -> (offsets, ids, bias): the three arrays of ccx_decode_bias_options"""
    offsets = np.zeros(len(entries) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(e[0]) for e in entries], dtype=np.int64)
    ids = np.array([t for e in entries for t in e[0]], dtype=np.int32)
    return offsets, ids, np.array([e[1] for e in entries], dtype=np.float32)


def from_arrays(offsets, ids, bias) -> List[Entry]:
    return [(tuple(int(t) for t in ids[offsets[e]:offsets[e + 1]]), float(bias[e])) for e in range(len(bias))]


def terms(entries: Sequence[Entry], history: Sequence[int]) -> Tuple[Dict[int, np.float32], Dict[int, np.float32]]:
    """(b1, S) of one row: only the terms that exist"""
    H = [int(t) for t in history]
    m = len(H)
    b1: Dict[int, np.float32] = {}
    S: Dict[int, np.float32] = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for ids, b in entries:
            L, v, b = len(ids), int(ids[-1]), np.float32(b)
            if L == 1:
                b1[v] = b if v not in b1 else np.float32(b1[v] + b)
            elif L - 1 <= m and H[m - L + 1:m] == [int(t) for t in ids[:-1]]:
                S[v] = b if v not in S else np.float32(S[v] + b)
    return b1, S


def apply_bias_np(logits: np.ndarray, history: Sequence[int], entries: Sequence[Entry], text_end: int) -> np.ndarray:
    """the rule on one fp32 row, float32 arithmetic in exactly the order of the rule; returns a new array"""
    x = np.array(logits, dtype=np.float32, copy=True)
    for ids, _ in entries:
        assert 1 <= len(ids) <= MAX_LEN and 0 <= ids[-1] < text_end, ids
    b1, S = terms(entries, history)
    with np.errstate(invalid="ignore", over="ignore"):
        for v, b in b1.items():
            x[v] = np.float32(x[v] + b)
        for v, s in S.items():
            x[v] = np.float32(x[v] + s)
    return x


def apply_bias(logits: torch.Tensor, history: Sequence[int], entries: Sequence[Entry], text_end: int) -> torch.Tensor:
    """the torch face of apply_bias_np (fp32 in, fp32 out)"""
    return torch.from_numpy(apply_bias_np(logits.detach().float().cpu().numpy(), history, entries, text_end))


def banned_occurrences(tokens: Sequence[int], bad_words: Sequence[Sequence[int]]) -> List[Tuple[int, Tuple[int, ...]]]:
    """What a decode under bad_words_ids must never hold: [(start, sequence), ...] of every occurrence (empty: none).  A sequence of
    L ids is banned from the position L - 1 of the row's own tokens on, which is every place it can occur in them."""
    toks = [int(t) for t in tokens]
    out = []
    for w in bad_words:
        w = tuple(int(t) for t in w)
        for i in range(0, len(toks) - len(w) + 1):
            if tuple(toks[i:i + len(w)]) == w:
                out.append((i, w))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's table compile (csrc/dec_bias.hip: ccx_compile_bias_table) and the kernel's walk over it, mirrored
# ---------------------------------------------------------------------------------------------------------------------------------
def compile_table(entries: Sequence[Entry], n_vocab: int, text_end: int) -> dict:
    """The checks and the layout of the host compile: length-1 entries stable by target with their sums; the others stable by (last
    context id, target): sorted distinct keys, per key its groups (one per target), per group its entries in the caller's order.
    ValueError naming the field for what the library refuses."""
    n = len(entries)
    if n > MAX_ENTRIES:
        raise ValueError(f"n_entries = {n} out of range")
    total = 0
    for e, (ids, b) in enumerate(entries):
        if not 1 <= len(ids) <= MAX_LEN:
            raise ValueError(f"offsets: entry {e} has {len(ids)} ids")
        total += len(ids)
        if total > MAX_IDS:
            raise ValueError("offsets: more than 65536 ids in total")
    for e, (ids, b) in enumerate(entries):
        for t in ids:
            if not 0 <= t < n_vocab:
                raise ValueError(f"ids: {t} out of range")
        if ids[-1] >= text_end:
            raise ValueError(f"ids: the target of entry {e} must be < eot")
        if np.isnan(b) or b == np.inf or (np.isfinite(b) and abs(b) > 3.4028234e38):
            raise ValueError(f"bias[{e}] must be finite or -inf")
    one = sorted((e for e in range(n) if len(entries[e][0]) == 1), key=lambda e: entries[e][0][-1])           # sorted() is stable
    multi = sorted((e for e in range(n) if len(entries[e][0]) > 1), key=lambda e: (entries[e][0][-2], entries[e][0][-1]))
    t = dict(l1_tgt=[], l1_bias=[], key=[], key_off=[], grp_tgt=[], grp_off=[], ent_len=[], ent_ctx=[], ent_bias=[], ctx=[], ent_src=[])
    with np.errstate(invalid="ignore", over="ignore"):
        for e in one:
            v, b = entries[e][0][-1], np.float32(entries[e][1])
            if t["l1_tgt"] and t["l1_tgt"][-1] == v:
                t["l1_bias"][-1] = np.float32(t["l1_bias"][-1] + b)
            else:
                t["l1_tgt"].append(v); t["l1_bias"].append(b)
    for v, s in zip(t["l1_tgt"], t["l1_bias"]):
        if np.isnan(s) or s == np.inf:
            raise ValueError(f"bias: the length-1 entries of target {v} sum to {s}")
    for i, e in enumerate(multi):
        ids, b = entries[e]
        k, v = ids[-2], ids[-1]
        new_key = i == 0 or entries[multi[i - 1]][0][-2] != k
        if new_key:
            t["key"].append(k); t["key_off"].append(len(t["grp_tgt"]))
        if new_key or entries[multi[i - 1]][0][-1] != v:
            t["grp_tgt"].append(v); t["grp_off"].append(i)
        t["ent_len"].append(len(ids) - 1); t["ent_ctx"].append(len(t["ctx"])); t["ent_bias"].append(np.float32(b)); t["ent_src"].append(e)
        t["ctx"].extend(ids[:-1])
    t["key_off"].append(len(t["grp_tgt"]))
    t["grp_off"].append(len(multi))
    return t


def apply_compiled_np(logits: np.ndarray, history: Sequence[int], t: dict, text_end: int) -> Tuple[np.ndarray, int]:
    """the kernel's walk over a compiled table: the staged tail of at most 31 ids, phase 1, the binary search for H[m - 1], one
    read-modify-write per group.  -> (edited row, groups visited)"""
    import bisect
    x = np.array(logits, dtype=np.float32, copy=True)
    H = [int(v) for v in history]
    tail = H[max(0, len(H) - (MAX_LEN - 1)):]
    k = len(tail)
    with np.errstate(invalid="ignore", over="ignore"):
        for v, b in zip(t["l1_tgt"], t["l1_bias"]):
            x[v] = np.float32(x[v] + b)
        if k == 0 or not t["key"]:
            return x, 0
        i = bisect.bisect_left(t["key"], tail[-1])
        if i >= len(t["key"]) or t["key"][i] != tail[-1]:
            return x, 0
        for g in range(t["key_off"][i], t["key_off"][i + 1]):
            s = None
            for e in range(t["grp_off"][g], t["grp_off"][g + 1]):
                c, co = t["ent_len"][e], t["ent_ctx"][e]
                if c <= k and t["ctx"][co:co + c] == tail[k - c:]:
                    s = t["ent_bias"][e] if s is None else np.float32(s + t["ent_bias"][e])
            if s is not None:
                v = t["grp_tgt"][g]
                x[v] = np.float32(x[v] + s)
        return x, t["key_off"][i + 1] - t["key_off"][i]


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel test's table and rows
# ---------------------------------------------------------------------------------------------------------------------------------
BIG = 1.0e8                 # (BIG + 1) - BIG = 0 in fp32, 1 in any other order: the sum's order shows in the bits
LONG = tuple(range(100, 131))                  # the 31-id context of the L = 32 entry


def kernel_table(V: int, E: int, many: int) -> List[Entry]:
    """The table of the kernel test, in an order that interleaves lengths and groups so that the compile has something to sort.
    `many`: groups under the key 70 (more than 256: the block's threads loop)."""
    assert E >= 200 and V > E + 3 and many <= E
    t: List[Entry] = [
        ((40, 41, 50), BIG),                   # [a, b, v] ...
        ((7,), 0.5),                           # length 1
        ((20, 30), 1.0),                       # length 2
        ((41, 50), 1.0),                       # ... and [b, v] on one target: summed in table order with the 4-gram below
        ((9,), NINF),                          # a length-1 bad word
        ((20, 31), NINF),                      # a bad bigram
        ((7,), 0.25),                          # the second length-1 entry of target 7: b1[7] = 0.75
        ((20, 7), 2.0),                        # a length-1 term and a multi-token term on one id
        ((39, 40, 41, 50), -BIG),              # L - 1 == 3
        ((37, 39, 40, 41, 51), 64.0),          # L - 1 == 4: one more than a history of 3 holds
        (LONG + (60,), 4.0),                   # L = 32
        ((E - 1,), 1.5),                       # a target at text_end - 1, length 1 ...
        ((20, E - 1), -0.5),                   # ... and behind a context
        ((0,), -2.0),                          # id 0
        ((E + 3, 25), 1.0),                    # a context id >= text_end is matched like any other
        ((1, 26), 3.0),                        # the first key
        ((V - 1, 27), 3.0),                    # the last key
        ((20, 33), 0.375),                     # a finite bias for a logit of -inf
        ((41, 52), -0.0),                      # a term of -0.0 exists and is added: +0.0 stays, -0.0 stays
    ]
    t += [((70, v), 0.125 * (1 + v % 5)) for v in range(many)]         # one key, `many` groups
    t += [((70, 3), NINF), ((5, 70, 4), 0.5)]                          # two of those groups with a second entry
    return t


@dataclass
class BiasRow:
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


def bias_rows(V: int, E: int, sample_len: int, n_rows: int, seed: int = 0) -> List[BiasRow]:
    """Rows of one launch under kernel_table: every history the kernel treats differently, as far as sample_len holds it, then
    random ones; with 3 rows and more the last two are a finished row and a row in the prompt phase.  Logits are N(0, 3) with -inf,
    0.0 and -0.0 planted at targets."""
    g = np.random.default_rng(4000 + 17 * seed + sample_len + n_rows)
    named = [
        ("m = 0", []),
        ("the key 20: four groups", [20]),
        ("[a, b]: two of three entries of one group", [40, 41]),
        ("L - 1 == m: all three, and L - 1 == m + 1 must not fire", [39, 40, 41]),
        ("the key 70: every group", [70]),
        ("[5, 70]: a second entry in one group", [5, 70]),
        ("the 5-gram", [37, 39, 40, 41]),
        ("a 4-gram that differs in its first id", [38, 40, 41]),
        ("a special as the key", [3, E + 3]),
        ("the first key", [1]),
        ("the last key", [V - 1]),
        ("an absent key between keys", [45]),
        ("an absent key below the first", [0]),
        ("an absent key above the last but one", [V - 2]),
        ("L = 32 with m = 31", list(LONG)),
        ("L = 32 behind two more ids", [8, 9] + list(LONG)),
        ("L = 32 with another first id", [99] + list(LONG[1:])),
        ("30 ids of the long context", list(LONG[1:])),
        ("a full history that ends in 20", [int(t) for t in g.integers(0, V, size=sample_len - 1)] + [20]),
    ]
    cases = [(n, h) for n, h in named if len(h) <= sample_len]

    def logits_for():
        lg = (3.0 * g.standard_normal(V)).astype(np.float32)
        lg[33] = -np.inf                         # gets a finite bias behind 20
        lg[31] = -np.inf                         # -inf + -inf
        lg[52] = -0.0 if g.integers(0, 2) else 0.0
        lg[490] = -0.0                           # no term ever (with up to 480 groups): the sign must stay
        lg[int(g.integers(200, E))] = -np.inf
        return lg

    rows: List[BiasRow] = []
    n_live = n_rows - 2 if n_rows >= 3 else n_rows
    i = 0
    while len(rows) < n_live:
        if i < len(cases):
            name, h = cases[i]
        else:
            m = int(g.integers(0, sample_len + 1))
            pool = np.array([20, 41, 70, 40, 39, 5, 1, V - 1, E + 3, 45, 7, 9])
            name, h = f"random, m = {m}", [int(t) for t in g.choice(pool, size=m)]
        rows.append(BiasRow(f"row {len(rows)}: {name}", h, logits_for(), prompt_len=1 + (i % 3)))
        i += 1
    if n_rows >= 3:
        rows.append(BiasRow("a finished row", [20], logits_for(), done=1))
        rows.append(BiasRow("a row in the prompt phase", [20], logits_for(), prompt_len=4, pos=1))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk of a decode through oracle/whisper_ref.WhisperRef under bias, history rules and filters
# ---------------------------------------------------------------------------------------------------------------------------------
def walk_prompts(rules) -> dict:
    """name -> (prompt, Options) of the two decodes the walks run"""
    return {"default": ([rules.sot], Options()), "without_timestamps": ([rules.sot, rules.no_timestamps], Options(True))}


def walk_tables(free_walks: Sequence[Sequence[int]], rules) -> Dict[str, List[Entry]]:
    """The walk tables of one prompt, built from the oracle's own free walks of every window the decode holds (one table serves every
    row of a call):
      ban   -- bad words only: of each walk the first three distinct bigrams it emits that end in a text id, and a trigram behind them
      boost -- a finite boost that redirects it: of each walk +6 on its second most frequent text id (a length-1 entry: the row at the
               SOT position is edited too), -4 on the most frequent one behind itself, -8 on the boosted one behind itself, and the
               walk's first ban"""
    E = rules.eot
    ban: List[Entry] = []
    boost: List[Entry] = []

    def add(table, entry):
        if entry[0] not in [e[0] for e in table]:
            table.append(entry)

    for walk in free_walks:
        toks = [int(t) for t in walk]
        bigrams: List[Tuple[int, int]] = []
        for a, b in zip(toks, toks[1:]):
            if b < E and (a, b) not in bigrams:
                bigrams.append((a, b))
        for bg in bigrams[:3]:
            add(ban, (bg, NINF))
        tri = next((tuple(toks[i:i + 3]) for i in range(3, len(toks) - 2) if toks[i + 2] < E), None)
        if tri is not None:
            add(ban, (tri, NINF))
        text = [t for t in toks if t < E]
        by_count = sorted(set(text), key=lambda t: (-text.count(t), text.index(t)))
        top, second = by_count[0], by_count[1 % len(by_count)]
        for entry in (((second,), 6.0), ((top, top), -4.0), ((second, second), -8.0), (bigrams[0], NINF)):
            add(boost, entry)
    return {"ban": ban, "boost": boost}


def bad_words_of(entries: Sequence[Entry]) -> List[Tuple[int, ...]]:
    return [ids for ids, b in entries if b == NINF]


def oracle_walk(orc, xa_row, prompt: Sequence[int], rules, opts: Options, sample_len: int, entries: Sequence[Entry] = (),
                penalty: float = 1.0, ngram: int = 0, forced: Optional[Sequence[int]] = None, eps: float = WALK_EPS) -> dict:
    """history_rules_reference.oracle_walk with the bias applied to the raw logits first: bias, then the history rules, then the
    options' filters; free-running (forced None) or teacher-forced with a decode's tokens.  Every forced token must lie within eps of
    the oracle's edited and filtered maximum and equal its argmax where the margin exceeds 2 eps (`decisive` counts those steps).
    sum_logprob (fp64) is taken from the edited logits.  no_speech_prob: from the row at <|startoftranscript|> -- the EDITED row where
    that is the row of the first sampled step (the prompt ends in it; only length-1 entries can fire there), the raw row otherwise."""
    seq, sampled, decisive, violations, slp = list(prompt), [], 0, [], 0.0
    sot_index = list(prompt).index(rules.sot)
    no_speech = None
    n = sample_len if forced is None else len(forced)
    for i in range(n):
        logits = orc.decoder_logits(torch.tensor([seq]), xa_row)[0]
        if no_speech is None:
            at_sot = logits[sot_index].float()
            if sot_index == len(prompt) - 1:
                at_sot = apply_bias(at_sot, [], entries, rules.eot)
            no_speech = float(torch.softmax(at_sot.double(), dim=-1)[rules.no_speech])
        lg = apply_bias(logits[-1].float(), sampled, entries, rules.eot)
        lg = apply_filters(apply_history_rules(lg, sampled, rules.eot, penalty, ngram), sampled, rules, opts)
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
