"""CPU: tests/history_rules_reference.py -- the plain statement of repetition_penalty and no_repeat_ngram_size (include/ccx.h:
ccx_decode_history_options) the GPU tests compare the kernel and the model against -- and the C ABI of the two new structs.

  * every branch of the rule by hand
  * a second statement on seeded histories of text ids: the installed transformers' RepetitionPenaltyLogitsProcessor and
    NoRepeatNGramLogitsProcessor agree with the rule exactly when every id is below eot
  * the kernel test's rows hold what they are meant to hold; the composition cases are decided by a margin of at least 0.25
  * the oracle alone walks the decodes of tests/test_decode_history_gpu.py free for 24 steps: at least half of the steps are decisive,
    and the rule changes at least 3 steps where it is stated to (conditions, not measurements)
  * the ctypes mirrors against sizeof / offsetof from a compiled C snippet; the defaults and the NULL-handle answers
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.tokenizer import DecodeRules
from oracle import whisper_ref as R
from tests import dec_reference as DR
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
    return sorted(np.flatnonzero(~((x == y) | (np.isnan(x) & np.isnan(y)))).tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ngram_ban_by_hand():
    x = _row()
    y = HR.apply_history_rules_np(x, [5, 7, 5, 7, 5], EOT, 1.0, 2)          # the tail [5] was followed by 7, twice
    assert _changed(x, y) == [7] and y[7] == NINF
    y = HR.apply_history_rules_np(x, [5, 7, 5, 7, 5], EOT, 1.0, 1)          # n = 1: every text id sampled so far
    assert _changed(x, y) == [5, 7] and y[5] == NINF and y[7] == NINF
    y = HR.apply_history_rules_np(x, [5, 7, 5, 7, 5], EOT, 1.0, 3)          # the tail [7, 5] was followed by 7
    assert _changed(x, y) == [7]
    y = HR.apply_history_rules_np(x, [5, 7, 5, 7, 5], EOT, 1.0, 5)          # m = n: the one window [5, 7, 5, 7] is not the tail [7, 5, 7, 5]
    assert _changed(x, y) == []
    assert _changed(x, HR.apply_history_rules_np(x, [9, 9, 9, 9], EOT, 1.0, 4)) == [9]     # m = n and it matches (overlapping)
    assert _changed(x, HR.apply_history_rules_np(x, [9, 9, 9], EOT, 1.0, 4)) == []         # m = n - 1: nothing
    assert _changed(x, HR.apply_history_rules_np(x, [], EOT, 1.0, 1)) == []
    assert _changed(x, HR.apply_history_rules_np(x, [5, 7, 5], EOT, 1.0, 0)) == []         # off
    assert _changed(x, HR.apply_history_rules_np(x, [5, 7, 5], EOT, 1.0, 7)) == []         # n > m: legal, never fires


def test_ids_from_eot_up_are_never_edited_but_match_as_context():
    x = _row()
    # the would-be ban is eot / a timestamp: nothing
    assert _changed(x, HR.apply_history_rules_np(x, [5, EOT, 5], EOT, 1.0, 2)) == []
    assert _changed(x, HR.apply_history_rules_np(x, [5, TSB + 3, 5], EOT, 1.0, 2)) == []
    assert _changed(x, HR.apply_history_rules_np(x, [TSB + 3, TSB + 3, EOT + 1], EOT, 2.0, 1)) == []
    # eot - 1 is the last id that is edited
    assert _changed(x, HR.apply_history_rules_np(x, [EOT - 1, EOT], EOT, 2.0, 1)) == [EOT - 1]
    # a timestamp inside the matched context still matches: [<t>, <t>] was followed by 11
    y = HR.apply_history_rules_np(x, [TSB + 3, TSB + 3, 11, 12, TSB + 3, TSB + 3], EOT, 1.0, 3)
    assert _changed(x, y) == [11] and y[11] == NINF


def test_penalty_by_hand():
    x = _row(fill=0.5)
    x[10], x[11], x[12], x[13] = 3.0, -3.0, 0.0, NINF
    y = HR.apply_history_rules_np(x, [10, 11, 12, 13, 10, 10], EOT, 1.5, 0)
    assert _changed(x, y) == [10, 11]
    assert y[10] == np.float32(3.0) / np.float32(1.5) and y[11] == np.float32(-3.0) * np.float32(1.5)     # a duplicate id: once
    assert y[12] == 0.0 and y[13] == NINF
    assert y.dtype == np.float32
    # below 1 the rule rewards: both directions are the same expression
    y = HR.apply_history_rules_np(x, [10, 11], EOT, 0.5, 0)
    assert y[10] == 6.0 and y[11] == -1.5
    # penalised and banned: -inf
    y = HR.apply_history_rules_np(x, [10, 11, 10], EOT, 1.5, 2)
    assert y[11] == NINF and y[10] == np.float32(2.0)
    assert _changed(x, HR.apply_history_rules_np(x, [10, 11], EOT, 1.0, 0)) == []
    # different penalties give different numbers
    assert HR.apply_history_rules_np(x, [10], EOT, 1.3, 0)[10] != HR.apply_history_rules_np(x, [10], EOT, 2.0, 0)[10]
    t = HR.apply_history_rules(torch.from_numpy(x), [10, 11, 10], EOT, 1.5, 2)
    assert t.dtype == torch.float32 and torch.equal(t, torch.from_numpy(y))


def test_invariant_checker():
    assert HR.ngram_invariant_violations([5, 7, 5, 7], EOT, 2) == [(0, 2)]
    assert HR.ngram_invariant_violations([5, 7, 5, 8], EOT, 2) == []
    assert HR.ngram_invariant_violations([5, TSB, 5, TSB], EOT, 2) == []           # ends in a timestamp: exempt
    assert HR.ngram_invariant_violations([TSB, 5, TSB, 5], EOT, 2) == [(0, 2)]
    assert HR.ngram_invariant_violations([5, 6, 5], EOT, 1) == [(0, 2)]
    assert HR.ngram_invariant_violations([5, 5, 5], EOT, 0) == []


# ---------------------------------------------------------------------------------------------------------------------------------
# the installed transformers' processors on histories of text ids
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("penalty,ngram", list(HR.SETTINGS) + [(2.0, 0), (0.7, 2)])
def test_hf_processors_agree_on_text_histories(penalty, ngram):
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    V = 2000
    g = np.random.default_rng(int(1000 * penalty) + ngram)
    hits = 0
    for trial in range(60):
        m = int(g.integers(0, 40))
        pool = g.integers(0, V, size=int(g.integers(1, 8)))
        hist = [int(t) for t in g.choice(pool, size=m)]
        if trial % 2:                                                         # a loop of period 1 .. 3: n-gram hits at every n
            hist = [int(pool[i % min(len(pool), 1 + trial % 3)]) for i in range(m)]
        x = (3.0 * g.standard_normal(V)).astype(np.float32)
        x[int(g.integers(0, V))] = 0.0
        ours = HR.apply_history_rules_np(x, hist, V, penalty, ngram)          # text_end = V: every id is "text"
        sc = torch.from_numpy(x.copy())[None]
        ids = torch.tensor([hist], dtype=torch.long).reshape(1, m)
        if penalty != 1.0 and m > 0:
            sc = RepetitionPenaltyLogitsProcessor(penalty)(ids, sc)
        if ngram > 0:
            sc = NoRepeatNGramLogitsProcessor(ngram)(ids, sc)
        assert np.array_equal(ours, sc[0].numpy()), (trial, hist)
        hits += int(not np.array_equal(ours, x))
    assert hits >= 20, hits


# ---------------------------------------------------------------------------------------------------------------------------------
# the generators of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("penalty,ngram", HR.SETTINGS)
@pytest.mark.parametrize("sample_len,n_rows", [(16, 70), (447, 14), (16, 1)])
def test_kernel_rows_cover_what_they_claim(penalty, ngram, sample_len, n_rows):
    V = DR.VOCABS["small.en / mini"]
    rows = HR.history_rows(V, EOT, TSB, sample_len, ngram, n_rows)
    assert len(rows) == n_rows
    lens = {len(r.history) for r in rows}
    n = max(ngram, 1)
    if n_rows >= 14:
        assert {0, 1, n - 1, n, sample_len} <= lens and (min(447, sample_len) in lens)
        ids = {t for r in rows for t in r.history}
        assert {0, EOT - 1, EOT, TSB, V - 1} <= ids
        assert sum(1 for r in rows if not r.live) == 2
    pen_n = ban_n = 0
    kinds = set()
    for r in rows:
        assert len(r.history) <= sample_len and all(0 <= t < V for t in r.history)
        if not r.live:
            continue
        pen, ban = HR.edited_ids(r.history, EOT, penalty, ngram)
        pen_n, ban_n = pen_n + len(pen), ban_n + len(ban)
        for v in pen:
            x = r.logits[v]
            kinds.add("pos" if x > 0 else "zero" if x == 0 else "ninf" if x == NINF else "neg")
    assert (pen_n > 0) == (penalty != 1.0) and (ban_n > 0) == (ngram > 0), (pen_n, ban_n)
    if n_rows >= 70:
        assert pen_n >= 20 * (penalty != 1.0) and ban_n >= 10 * (ngram > 0), (pen_n, ban_n)
    if n_rows >= 14 and penalty != 1.0:
        assert kinds == {"pos", "neg", "zero", "ninf"}


@pytest.mark.parametrize("penalty,ngram", HR.SETTINGS)
def test_composition_cases_are_decided(penalty, ngram):
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = HR.composition_cases(V, rules, penalty, ngram)
    moved = 0
    for c in cases:
        assert len(c.sampled) < 16
        edited = HR.apply_history_rules(c.logits, c.sampled, rules.eot, penalty, ngram)
        flt = R.apply_filters(edited, c.sampled, rules).double()
        top = torch.topk(flt, 2).values
        assert float(top[0] - top[1]) >= 0.25, (c.name, float(top[0] - top[1]))
        assert int(flt.argmax()) == c.expect, (c.name, int(flt.argmax()), c.expect)
        plain = int(R.apply_filters(c.logits, c.sampled, rules).argmax())
        moved += plain != c.expect
    assert moved >= 1, moved                                   # the rule decides some rows ...
    assert moved <= len(cases) - 4                             # ... and leaves others alone


# ---------------------------------------------------------------------------------------------------------------------------------
# the model walks of tests/test_decode_history_gpu.py, by the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------
def test_oracle_walks_are_decisive_and_the_rule_changes_them():
    from clearconverse_amd.audio import synthetic_clip
    from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    for seed, seconds in zip(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS):
        clip = torch.from_numpy(synthetic_clip(seed, 30.0)[: int(seconds * 16000)])
        mel = R.pad_or_trim(R.log_mel_spectrogram(clip)[:, : len(clip) // 160], 3000)
        xa = orc.encode(mel[None])
        for name, (prompt, opts) in HR.walk_prompts(ORULES).items():
            plain = HR.oracle_walk(orc, xa, prompt, ORULES, opts, HR.WALK_FREE_LEN)
            same = DO.oracle_walk(orc, xa, prompt, ORULES, opts, HR.WALK_FREE_LEN)
            assert plain["tokens"] == same["tokens"] and plain["sum_logprob"] == same["sum_logprob"]      # (1.0, 0) is the walk without the rule
            for p, n in HR.WALK_SETTINGS:
                w = HR.oracle_walk(orc, xa, prompt, ORULES, opts, HR.WALK_FREE_LEN, p, n)
                what = (seed, name, p, n)
                assert not w["violations"] and w["steps"] == HR.WALK_FREE_LEN, (what, w)
                assert 2 * w["decisive"] >= w["steps"], (what, w["decisive"], w["steps"])
                assert not HR.ngram_invariant_violations(w["tokens"], EOT, n), what
                differ = sum(a != b for a, b in zip(w["tokens"], plain["tokens"]))
                if p != 1.0 or name == "without_timestamps":
                    assert differ >= 3, (what, differ)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "ccx.h"
int main() {
  printf("ccx_decode_history_options %zu\n", sizeof(ccx_decode_history_options));
  printf("ccx_decode_history_options.repetition_penalty %zu\n", offsetof(ccx_decode_history_options, repetition_penalty));
  printf("ccx_decode_history_options.no_repeat_ngram_size %zu\n", offsetof(ccx_decode_history_options, no_repeat_ngram_size));
  printf("ccx_dec_history_desc %zu\n", sizeof(ccx_dec_history_desc));
  printf("ccx_dec_history_desc.logits %zu\n", offsetof(ccx_dec_history_desc, logits));
  printf("ccx_dec_history_desc.logits_elems %zu\n", offsetof(ccx_dec_history_desc, logits_elems));
  printf("ccx_dec_history_desc.ld %zu\n", offsetof(ccx_dec_history_desc, ld));
  printf("ccx_dec_history_desc.n_vocab %zu\n", offsetof(ccx_dec_history_desc, n_vocab));
  printf("ccx_dec_history_desc.rows %zu\n", offsetof(ccx_dec_history_desc, rows));
  printf("ccx_dec_history_desc.state %zu\n", offsetof(ccx_dec_history_desc, state));
  printf("ccx_dec_history_desc.hist %zu\n", offsetof(ccx_dec_history_desc, hist));
  printf("ccx_dec_history_desc.sample_len %zu\n", offsetof(ccx_dec_history_desc, sample_len));
  printf("ccx_dec_history_desc.text_end %zu\n", offsetof(ccx_dec_history_desc, text_end));
  printf("ccx_dec_history_desc.repetition_penalty %zu\n", offsetof(ccx_dec_history_desc, repetition_penalty));
  printf("ccx_dec_history_desc.no_repeat_ngram_size %zu\n", offsetof(ccx_dec_history_desc, no_repeat_ngram_size));
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
    mirrors = {"ccx_decode_history_options": _lib.DecodeHistoryOptions, "ccx_dec_history_desc": _lib.DecHistoryDesc}
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
    o = _lib.DecodeHistoryOptions(9.0, 9)
    lib.ccx_decode_history_options_default(C.byref(o))
    assert (o.repetition_penalty, o.no_repeat_ngram_size) == (1.0, 0)
    lib.ccx_decode_history_options_default(None)                     # a NULL pointer is left alone
    assert lib.ccx_whisper_set_history_options(None, C.byref(o)) == 1        # CCX_ERR_ARG
    assert lib.ccx_whisper_set_history_options(None, None) == 1
    assert lib.ccx_whisper_history_graph_count(None) == -1
    assert lib.ccx_dec_history_step(None, None, None) == 1


def test_python_range_check():
    from clearconverse_amd.whisper import WhisperModel
    assert WhisperModel.check_history_options(1.3, 2) == (1.3, 2)
    assert WhisperModel.check_history_options(1, 0) == (1.0, 0)
    for p in (0.0, -1.0, float("inf"), float("nan"), 1e39, None, "x"):
        with pytest.raises(ValueError, match="repetition_penalty"):
            WhisperModel.check_history_options(p, 0)
    for n in (-1, 1.5, True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            WhisperModel.check_history_options(1.0, n)
