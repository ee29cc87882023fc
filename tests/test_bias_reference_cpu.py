"""CPU: tests/bias_reference.py -- the plain statement of the sequence bias (include/ccx.h: ccx_decode_bias_options) the GPU tests
compare the kernel and the model against --, clearconverse_amd/decode_bias.py, and the C ABI of the two new structs.

  * every branch of the rule by hand
  * a second statement: the installed transformers' SequenceBiasLogitsProcessor (dict form) and NoBadWordsLogitsProcessor with
    input_ids = H agree with the rule bit for bit on seeded cases whose logits are multiples of 2^-6 and whose biases are multiples of
    2^-3, all small: (x + b1) + S and x + (b1 + S) are then both exact
  * the table compile: grouping, stable order, limits; the kernel's walk over the compiled table equals the rule
  * compile_bias_table: every error, prefix expansion and dedup of hotwords with IdTokenizer and with a scripted encode, merging
  * the order against repetition_penalty: (x + b) / p
  * the oracle alone walks the decodes of tests/test_decode_bias_gpu.py free for 24 steps under tables built from its own free walk:
    at least half of the steps are decisive, each table changes at least 3 steps (conditions, not measurements)
  * the ctypes mirrors against sizeof / offsetof from a compiled C snippet; the defaults and the NULL-handle answers
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.decode_bias import compile_bias_table
from clearconverse_amd.tokenizer import DecodeRules, IdTokenizer
from oracle import whisper_ref as R
from tests import bias_reference as BR
from tests import decoding_options_reference as DO
from tests import history_rules_reference as HR

ROOT = Path(__file__).resolve().parent.parent
RULES = DecodeRules()
TSB, EOT = RULES.timestamp_begin, RULES.eot
ORULES = R.Rules(suppress=tuple(RULES.suppress))
NINF = -np.inf


def _row(V=60000, fill=1.0):
    return np.full(V, fill, dtype=np.float32)


def _changed(x, y):
    return sorted(np.flatnonzero(x.view(np.int32) != y.view(np.int32)).tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rule_by_hand():
    x = _row()
    T = [((5,), 0.5), ((7, 8), 2.0), ((6, 7, 8), 0.25), ((7, 9), NINF), ((5,), 1.0), ((4, 5), -3.0)]
    y = BR.apply_bias_np(x, [], T, EOT)                       # m = 0: the length-1 entries only, summed in table order
    assert _changed(x, y) == [5] and y[5] == 2.5
    y = BR.apply_bias_np(x, [7], T, EOT)                      # L - 1 == m for the bigrams, L - 1 == m + 1 for the trigram
    assert _changed(x, y) == [5, 8, 9] and y[8] == 3.0 and y[9] == NINF
    y = BR.apply_bias_np(x, [6, 7], T, EOT)                   # [a, b, v] and [b, v] on one target
    assert y[8] == 3.25 and y[9] == NINF and y[5] == 2.5
    y = BR.apply_bias_np(x, [7, 6], T, EOT)                   # the last id decides
    assert _changed(x, y) == [5]
    y = BR.apply_bias_np(x, [3, 4], T, EOT)                   # a length-1 term and a multi-token term on one id: (1 + 1.5) + -3
    assert _changed(x, y) == [5] and y[5] == -0.5
    assert _changed(x, BR.apply_bias_np(x, [7, 7, 7], [], EOT)) == []
    assert y.dtype == np.float32
    t = BR.apply_bias(torch.from_numpy(x), [3, 4], T, EOT)
    assert t.dtype == torch.float32 and torch.equal(t, torch.from_numpy(y))


def test_order_of_the_sum_and_terms_that_do_not_exist():
    x = _row(fill=0.0)
    big = BR.BIG
    T = [((1, 2, 3), big), ((2, 3), 1.0), ((0, 1, 2, 3), -big)]
    assert BR.apply_bias_np(x, [0, 1, 2], T, EOT)[3] == 0.0                 # (big + 1) - big in table order
    assert BR.apply_bias_np(x, [0, 1, 2], [T[0], T[2], T[1]], EOT)[3] == 1.0  # another order, another number
    assert BR.apply_bias_np(x, [1, 2], T, EOT)[3] == np.float32(big)
    # a term that does not exist is not added as zero: -0.0 keeps its sign unless a term lands on it
    x[10] = x[11] = -0.0
    y = BR.apply_bias_np(x, [2], [((2, 10), -0.0), ((9, 11), 5.0), ((12,), 0.0)], EOT)
    assert np.signbit(y[10]) and np.signbit(y[11]) and y[12] == 0.0
    x[12] = -0.0
    assert not np.signbit(BR.apply_bias_np(x, [], [((12,), 0.0)], EOT)[12])  # -0.0 + 0.0 = +0.0: the term was added
    # -inf: stays under a finite bias, and a -inf bias wins over a finite logit
    x[20], x[21] = NINF, 3.0
    y = BR.apply_bias_np(x, [2], [((2, 20), 9.0), ((21,), NINF), ((2, 21), 4.0)], EOT)
    assert y[20] == NINF and y[21] == NINF


def test_targets_and_contexts_around_eot():
    x = _row()
    y = BR.apply_bias_np(x, [TSB + 3], [((TSB + 3, EOT - 1), 1.0), ((EOT, 4), 1.0)], EOT)        # a timestamp as the context matches
    assert _changed(x, y) == [EOT - 1]
    assert _changed(x, BR.apply_bias_np(x, [EOT], [((EOT, 4), 1.0)], EOT)) == [4]
    for bad in ([((EOT,), 1.0)], [((4, TSB), NINF)]):
        with pytest.raises(AssertionError):
            BR.apply_bias_np(x, [], bad, EOT)
    assert BR.banned_occurrences([1, 2, 3, 2, 3], [(2, 3), (9,)]) == [(1, (2, 3)), (3, (2, 3))]
    assert BR.banned_occurrences([1, 2, 3], [(3, 2)]) == []


# ---------------------------------------------------------------------------------------------------------------------------------
# the installed transformers' processors with input_ids = H
# ---------------------------------------------------------------------------------------------------------------------------------
def _without_whole_history_matches(entries, hist):
    """HF's processor skips an entry whose L ids outnumber input_ids (`len(sequence_ids) > input_ids.shape[1]`), so an entry whose
    context is the WHOLE history (L - 1 == m) never fires there; here it does (L - 1 <= m: a bad bigram holds from the second sampled
    token on).  The one place the two statements differ with input_ids = H: those entries are taken out for the comparison, which
    shows HF's result is ours without exactly them.  -> (entries HF honours, how many were taken out)"""
    m = len(hist)
    keep = [(ids, b) for ids, b in entries if not (len(ids) >= 2 and len(ids) - 1 == m and list(ids[:-1]) == list(hist))]
    return keep, len(entries) - len(keep)


def _seeded_case(g, V):
    m = int(g.integers(0, 12))
    pool = g.integers(0, V, size=6)
    hist = [int(t) for t in g.choice(pool, size=m)]
    x = (g.integers(-512, 512, size=V) / 64.0).astype(np.float32)
    return pool, hist, x


def test_hf_sequence_bias_agrees_bit_for_bit():
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    V = 300
    g = np.random.default_rng(77)
    hits = multi_hits = edge = 0
    for trial in range(60):
        pool, hist, x = _seeded_case(g, V)
        table = {}
        for _ in range(int(g.integers(1, 12))):
            L = int(g.integers(1, 5))
            seq = tuple(int(t) for t in g.choice(pool, size=L)) if g.integers(0, 3) else tuple(int(t) for t in g.integers(0, V, size=L))
            if hist and L >= 2 and g.integers(0, 2):                       # a context that is the history's tail
                seq = tuple(hist[-(L - 1):][-(L - 1):]) + (seq[-1],) if len(hist) >= L - 1 else seq
            table[seq] = float(g.integers(-40, 40)) / 8.0
        entries, dropped = _without_whole_history_matches(list(table.items()), hist)
        edge += dropped
        ours = BR.apply_bias_np(x, hist, entries, V)                       # text_end = V: every id may be a target
        ids = torch.tensor([hist], dtype=torch.long).reshape(1, len(hist))
        theirs = SequenceBiasLogitsProcessor(sequence_bias=dict(table))(ids, torch.from_numpy(x.copy())[None])[0].numpy()
        assert np.array_equal(ours.view(np.int32), theirs.view(np.int32)), (trial, hist, entries)
        hits += int(not np.array_equal(ours, x))
        multi_hits += int(bool(BR.terms(entries, hist)[1]))
    assert hits >= 40 and multi_hits >= 15 and edge >= 3, (hits, multi_hits, edge)


def test_hf_no_bad_words_agrees_bit_for_bit():
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor
    V = 300
    g = np.random.default_rng(78)
    multi_hits = 0
    for trial in range(60):
        pool, hist, x = _seeded_case(g, V)
        words = []
        for _ in range(int(g.integers(1, 8))):
            L = int(g.integers(1, 4))
            seq = [int(t) for t in g.choice(pool, size=L)]
            if seq not in words:
                words.append(seq)
        entries, _ = _without_whole_history_matches([(tuple(w), NINF) for w in words], hist)
        ours = BR.apply_bias_np(x, hist, entries, V)
        ids = torch.tensor([hist], dtype=torch.long).reshape(1, len(hist))
        theirs = NoBadWordsLogitsProcessor(words, eos_token_id=V - 1)(ids, torch.from_numpy(x.copy())[None])[0].numpy()
        if [V - 1] in words:
            continue                                                       # HF drops [eos]; here such a table is refused
        assert np.array_equal(ours.view(np.int32), theirs.view(np.int32)), (trial, hist, words)
        multi_hits += int(bool(BR.terms(entries, hist)[1]))
    assert multi_hits >= 10, multi_hits


# ---------------------------------------------------------------------------------------------------------------------------------
# the table compile
# ---------------------------------------------------------------------------------------------------------------------------------
def test_compile_groups_and_keeps_the_callers_order():
    T = [((4, 9), 1.0), ((3,), 1.0), ((2, 9), 2.0), ((1, 4, 9), 3.0), ((4, 8), 4.0), ((3,), 0.5), ((1,), NINF), ((4, 9), 5.0), ((7, 2, 9), 6.0)]
    t = BR.compile_table(T, 100, 50)
    assert t["l1_tgt"] == [1, 3] and t["l1_bias"] == [NINF, 1.5]
    assert t["key"] == [2, 4] and t["key_off"] == [0, 1, 3]
    assert t["grp_tgt"] == [9, 8, 9] and t["grp_off"] == [0, 2, 3, 6]
    assert t["ent_src"] == [2, 8, 4, 0, 3, 7]                              # inside a group: the caller's order
    assert t["ent_len"] == [1, 2, 1, 1, 2, 1] and t["ctx"] == [2, 7, 2, 4, 4, 1, 4, 4]
    assert [t["ctx"][c:c + n] for c, n in zip(t["ent_ctx"], t["ent_len"])] == [[2], [7, 2], [4], [4], [1, 4], [4]]
    empty = BR.compile_table([], 100, 50)
    assert empty["key"] == [] and empty["l1_tgt"] == [] and empty["key_off"] == [0] and empty["grp_off"] == [0]


def test_compile_limits_and_checks():
    ok = [((1, 2), 1.0)]
    BR.compile_table(ok * BR.MAX_ENTRIES, 100, 50)
    BR.compile_table([(tuple(range(32)), 1.0)] * 2048, 100, 50)            # 65536 ids
    for bad, frag in (([((1, 2), 1.0)] * (BR.MAX_ENTRIES + 1), "n_entries"), ([(tuple(range(32)), 1.0)] * 2048 + ok, "65536"),
                      ([(tuple(range(33)), 1.0)], "33 ids"), ([((), 1.0)], "0 ids"), ([((1, 100), 1.0)], "out of range"),
                      ([((-1, 2), 1.0)], "out of range"), ([((1, 50), 1.0)], "target"), ([((50,), NINF)], "target"),
                      ([((1,), np.inf)], "bias[0]"), ([((1,), np.nan)], "bias[0]"), ([((1,), 3e38), ((1,), 3e38)], "sum to")):
        with pytest.raises(ValueError, match=frag.replace("[", r"\[").replace("]", r"\]")):
            BR.compile_table(bad, 100, 50)
    BR.compile_table([((99, 49), NINF)], 100, 50)                          # a context id >= text_end is legal


@pytest.mark.parametrize("sample_len,n_rows", [(8, 1), (8, 3), (8, 70), (64, 1), (64, 3), (64, 70)])
def test_kernel_rows_cover_what_they_claim_and_the_compiled_walk_is_the_rule(sample_len, n_rows):
    V, E = 515, 500
    T = BR.kernel_table(V, E, 480)
    t = BR.compile_table(T, V, E)
    rows = BR.bias_rows(V, E, sample_len, n_rows)
    assert len(rows) == n_rows and all(len(r.history) <= sample_len for r in rows)
    visited, fired = 0, set()
    for r in rows:
        want = BR.apply_bias_np(r.logits, r.history, T, E)
        got, n = BR.apply_compiled_np(r.logits, r.history, t, E)
        assert np.array_equal(want.view(np.int32), got.view(np.int32)), r.name
        visited = max(visited, n)
        assert n <= 482                                                    # a row never walks the whole table
        H, m = r.history, len(r.history)
        fired |= {i for i, (ids, b) in enumerate(T) if len(ids) > 1 and len(ids) - 1 <= m and list(ids[:-1]) == H[m - len(ids) + 1:]}
        assert want[490] == 0 and np.signbit(want[490])
    if n_rows >= 70:
        assert visited > 256                                               # the key of 480 groups was looked up
        assert sum(1 for r in rows if not r.live) == 2
        lens = {len(T[i][0]) for i in fired}
        assert {2, 3, 4} <= lens and (sample_len < 31 or {5, 32} <= lens), lens
        assert {0, 1, 2, 3} <= {len(r.history) for r in rows}


# ---------------------------------------------------------------------------------------------------------------------------------
# compile_bias_table
# ---------------------------------------------------------------------------------------------------------------------------------
def _entries(*a, **k):
    k.setdefault("eot", EOT)
    return BR.from_arrays(*compile_bias_table(*a, **k))


def test_compile_bias_table_forms_order_and_merging():
    o, i, b = compile_bias_table(eot=EOT)
    assert o.tolist() == [0] and len(i) == 0 and len(b) == 0 and (o.dtype, i.dtype, b.dtype) == (np.int32, np.int32, np.float32)
    assert _entries({(5,): 1.5, (7, 8): -2.0}) == [((5,), 1.5), ((7, 8), -2.0)]
    assert _entries([[[5], 1.5], [[7, 8], -2.0]]) == [((5,), 1.5), ((7, 8), -2.0)]
    assert _entries(None, [[9], [7, 8]]) == [((9,), NINF), ((7, 8), NINF)]
    enc = IdTokenizer(EOT).encode
    # hotwords first, then sequence_bias, then bad_words_ids; every prefix of every encoding; identical expansions once
    got = _entries({(30,): 1.0}, [[40, 41]], "<10> <11>", 2.0, enc)
    assert got == [((10,), 2.0), ((10, 11), 2.0), ((30,), 1.0), ((40, 41), NINF)]     # IdTokenizer: " x" encodes as "x" does
    assert _entries(None, None, ["<10> <11>", "<10> <12>"], 0.5, enc) == [((10,), 0.5), ((10, 11), 0.5), ((10, 12), 0.5)]
    # as written and with a leading space, through a scripted encode
    script = {"ab": [1, 2], " ab": [3], "c": [4], " c": [4]}
    assert _entries(None, None, ["ab", "c"], 1.0, script.__getitem__) == [((1,), 1.0), ((1, 2), 1.0), ((3,), 1.0), ((4,), 1.0)]
    # a sequence in more than one source: the float32 sum, at its first place
    got = _entries({(10,): 0.1, (10, 11): 1.0}, [[10, 11]], "<10> <11>", 0.2, enc)
    assert got == [((10,), float(np.float32(0.2) + np.float32(0.1))), ((10, 11), NINF)]
    assert _entries([[[5], 1.0]], [[5]]) == [((5,), NINF)]


def test_compile_bias_table_errors():
    enc = IdTokenizer(EOT).encode
    E = lambda *a, **k: compile_bias_table(*a, eot=EOT, **k)
    with pytest.raises(ValueError, match="twice"):
        E([[[5, 6], 1.0], [[5, 6], 2.0]])
    with pytest.raises(ValueError, match="eot"):
        E(None, [[EOT]])
    with pytest.raises(ValueError, match="never edited"):
        E(None, [[5, TSB + 1]])
    with pytest.raises(ValueError, match="eot"):
        E({(5, EOT + 1): 1.0})
    E({(EOT, 5): 1.0})                                                     # as a context any id is fine
    for bad in (np.inf, np.nan, "x", None, 1e39):
        with pytest.raises(ValueError, match="sequence_bias"):
            E({(5,): bad})
    with pytest.raises(ValueError, match="1 to 32"):
        E({tuple(range(33)): 1.0})
    with pytest.raises(ValueError, match="1 to 32"):
        E(None, [[]])
    with pytest.raises(ValueError, match="outside the vocabulary"):
        E({(-1, 5): 1.0})
    with pytest.raises(ValueError, match="outside the vocabulary"):
        E({(70000, 5): 1.0}, n_vocab=51864)
    with pytest.raises(ValueError, match="no token id"):
        E({(1.5, 5): 1.0})
    with pytest.raises(ValueError, match=r"\[ids, bias\]"):
        E([[5, 6, 7]])
    with pytest.raises(ValueError, match="hotword_boost"):
        E(None, None, "<10>", None, enc)                                   # no default
    for boost in (0.0, -1.0, np.inf, np.nan, "x"):
        with pytest.raises(ValueError, match="hotword_boost"):
            E(None, None, "<10>", boost, enc)
    with pytest.raises(ValueError, match="encode"):
        E(None, None, "<10>", 1.0)
    with pytest.raises(ValueError, match="at most 32"):
        E(None, None, " ".join(f"<{k}>" for k in range(33)), 1.0, enc)
    with pytest.raises(ValueError, match="no phrase"):
        E(None, None, ["  "], 1.0, enc)
    with pytest.raises(ValueError, match="eot"):
        E(None, None, f"<{EOT + 2}>", 1.0, enc)
    with pytest.raises(ValueError, match="limits"):
        E({(k // 50000, k % 50000): 1.0 for k in range(8193)})
    assert len(E({(k, 5): 1.0 for k in range(8192)})[2]) == 8192


def test_the_order_against_repetition_penalty_matters():
    x = _row(fill=0.0)
    x[5] = 2.0
    T, H, p = [((4, 5), 4.0)], [5, 4], 2.0
    ours = HR.apply_history_rules_np(BR.apply_bias_np(x, H, T, EOT), H, EOT, p, 0)
    assert ours[5] == (2.0 + 4.0) / 2.0
    other = BR.apply_bias_np(HR.apply_history_rules_np(x, H, EOT, p, 0), H, T, EOT)
    assert other[5] == 2.0 / 2.0 + 4.0 and other[5] != ours[5]
    # a -inf commutes with both history rules
    T = [((4, 5), NINF)]
    a = HR.apply_history_rules_np(BR.apply_bias_np(x, H, T, EOT), H, EOT, p, 2)
    b = BR.apply_bias_np(HR.apply_history_rules_np(x, H, EOT, p, 2), H, T, EOT)
    assert np.array_equal(a, b) and a[5] == NINF


# ---------------------------------------------------------------------------------------------------------------------------------
# the model walks of tests/test_decode_bias_gpu.py, by the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------
def test_oracle_walks_are_decisive_and_every_table_changes_them():
    from clearconverse_amd.audio import synthetic_clip
    from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    xas = []
    for seed, seconds in zip(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS):
        clip = torch.from_numpy(synthetic_clip(seed, 30.0)[: int(seconds * 16000)])
        mel = R.pad_or_trim(R.log_mel_spectrogram(clip)[:, : len(clip) // 160], 3000)
        xas.append(orc.encode(mel[None]))
    for name, (prompt, opts) in BR.walk_prompts(ORULES).items():
        plains = [BR.oracle_walk(orc, xa, prompt, ORULES, opts, BR.WALK_FREE_LEN) for xa in xas]
        tables = BR.walk_tables([p["tokens"] for p in plains], ORULES)      # one table per prompt serves both windows
        for b, (xa, plain) in enumerate(zip(xas, plains)):
            same = HR.oracle_walk(orc, xa, prompt, ORULES, opts, BR.WALK_FREE_LEN)
            assert plain["tokens"] == same["tokens"] and plain["sum_logprob"] == same["sum_logprob"]      # no table: the walk without the rule
            assert plain["no_speech_prob"] == same["no_speech_prob"]
            assert BR.banned_occurrences(plain["tokens"], BR.bad_words_of(tables["ban"]))                 # the free walk emits what is banned
            for tname, T in tables.items():
                BR.compile_table(T, dims.n_vocab, EOT)
                w = BR.oracle_walk(orc, xa, prompt, ORULES, opts, BR.WALK_FREE_LEN, T)
                what = (b, name, tname)
                assert not w["violations"] and w["steps"] == BR.WALK_FREE_LEN, (what, w)
                assert 2 * w["decisive"] >= w["steps"], (what, w["decisive"], w["steps"])
                assert not BR.banned_occurrences(w["tokens"], BR.bad_words_of(T)), what
                assert sum(x != y for x, y in zip(w["tokens"], plain["tokens"])) >= 3, (what, w["tokens"], plain["tokens"])
                # no_speech_prob: the edited row only where a length-1 entry exists and the prompt ends in <|startoftranscript|>
                edited = any(len(ids) == 1 for ids, _ in T) and name == "default"
                assert (w["no_speech_prob"] != plain["no_speech_prob"]) == edited, what
            # with the history rules behind the bias: still a walk without violations
            w = BR.oracle_walk(orc, xa, prompt, ORULES, opts, BR.WALK_FREE_LEN, tables["boost"], 1.3, 2)
            assert not w["violations"] and not HR.ngram_invariant_violations(w["tokens"], EOT, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "ccx.h"
int main() {
  printf("ccx_decode_bias_options %zu\n", sizeof(ccx_decode_bias_options));
  printf("ccx_decode_bias_options.n_entries %zu\n", offsetof(ccx_decode_bias_options, n_entries));
  printf("ccx_decode_bias_options.offsets %zu\n", offsetof(ccx_decode_bias_options, offsets));
  printf("ccx_decode_bias_options.ids %zu\n", offsetof(ccx_decode_bias_options, ids));
  printf("ccx_decode_bias_options.bias %zu\n", offsetof(ccx_decode_bias_options, bias));
  printf("ccx_dec_bias_desc %zu\n", sizeof(ccx_dec_bias_desc));
  printf("ccx_dec_bias_desc.logits %zu\n", offsetof(ccx_dec_bias_desc, logits));
  printf("ccx_dec_bias_desc.logits_elems %zu\n", offsetof(ccx_dec_bias_desc, logits_elems));
  printf("ccx_dec_bias_desc.ld %zu\n", offsetof(ccx_dec_bias_desc, ld));
  printf("ccx_dec_bias_desc.n_vocab %zu\n", offsetof(ccx_dec_bias_desc, n_vocab));
  printf("ccx_dec_bias_desc.rows %zu\n", offsetof(ccx_dec_bias_desc, rows));
  printf("ccx_dec_bias_desc.state %zu\n", offsetof(ccx_dec_bias_desc, state));
  printf("ccx_dec_bias_desc.hist %zu\n", offsetof(ccx_dec_bias_desc, hist));
  printf("ccx_dec_bias_desc.sample_len %zu\n", offsetof(ccx_dec_bias_desc, sample_len));
  printf("ccx_dec_bias_desc.text_end %zu\n", offsetof(ccx_dec_bias_desc, text_end));
  printf("ccx_dec_bias_desc.table %zu\n", offsetof(ccx_dec_bias_desc, table));
  printf("limits %d\n", CCX_BIAS_MAX_ENTRIES + CCX_BIAS_MAX_IDS + CCX_BIAS_MAX_LEN);
  return 0;
}
"""


def test_ctypes_mirrors_have_the_c_structs_layout(tmp_path):
    from clearconverse_amd.build import _hipcc
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert c.pop("limits") == BR.MAX_ENTRIES + BR.MAX_IDS + BR.MAX_LEN == 8192 + 65536 + 32
    mirrors = {"ccx_decode_bias_options": _lib.DecodeBiasOptions, "ccx_dec_bias_desc": _lib.DecBiasDesc}
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == c[name], (name, C.sizeof(cls), c[name])
    n_fields = 0
    for key, want in c.items():
        if "." in key:
            name, fld = key.split(".")
            assert getattr(mirrors[name], fld).offset == want, (key, getattr(mirrors[name], fld).offset, want)
            n_fields += 1
    assert n_fields == sum(len(m._fields_) for m in mirrors.values())           # every field of both mirrors was compared


def test_defaults_and_null_handles_need_no_device():
    lib = _lib.load()
    arr = (C.c_int * 2)(0, 1)
    o = _lib.DecodeBiasOptions(9, arr, arr, None)
    lib.ccx_decode_bias_options_default(C.byref(o))
    assert o.n_entries == 0 and not o.offsets and not o.ids and not o.bias
    lib.ccx_decode_bias_options_default(None)                       # a NULL pointer is left alone
    assert lib.ccx_whisper_set_bias_options(None, C.byref(o)) == 1          # CCX_ERR_ARG
    assert lib.ccx_whisper_set_bias_options(None, None) == 1
    assert lib.ccx_whisper_bias_graph_count(None) == -1
    assert lib.ccx_dec_bias_step(None, None, None) == 1
