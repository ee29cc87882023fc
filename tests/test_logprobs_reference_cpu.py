"""CPU: the per-token log-probability rule restated in tests/logprobs_reference.py -- by hand, against torch.topk(torch.log_softmax) on
the tie-free rows, the generator's margins on the reference alone, every listed misreading caught by some generated case -- the C
structs of include/ccx.h against their ctypes mirrors, and the opt-in's defaults."""
import ctypes as C
import inspect
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.build import _hipcc
from tests import logprobs_reference as LR
from tests import truncation_reference as TR

ROOT = Path(__file__).resolve().parent.parent
NINF = -math.inf
TRUNC = TR.Params(0.7, 3, 0.9, 0.0)


@pytest.fixture(scope="module")
def generated():
    """every generated launch, made once and never changed: (vocab, rule set) -> (V, rules, opts, cases)"""
    out = {}
    for vocab, V in LR.VOCABS.items():
        rules = LR.rules_for(V)
        for rs, opts in LR.RULE_SETS.items():
            out[(vocab, rs)] = (V, rules, opts, LR.logprob_cases(V, rules, opts))
    return out


# ---------------------------------------------------------------------------------------------- the rule by hand
def test_the_rule_by_hand():
    x = np.array([NINF, 1.0, 3.0, NINF, 2.0, 3.0, 0.0])
    z = math.log(math.exp(-2) + 1 + math.exp(-1) + 1 + math.exp(-3))
    top = LR.top_of_row(x, 4)
    assert [i for i, _ in top] == [2, 5, 4, 1]                        # equal values: the lower id first
    assert [round(v, 12) for _, v in top] == [round(v, 12) for v in (-z, -z, -1 - z, -2 - z)]
    assert [i for i, _ in LR.top_of_row(x, 4, high_id_first=True)] == [5, 2, 4, 1]
    # |A| = 5 < 8: the rest is (-1, -inf)
    top8 = LR.top_of_row(x, 8)
    assert [i for i, _ in top8] == [2, 5, 4, 1, 6, -1, -1, -1] and all(v == NINF for _, v in top8[5:])
    assert LR.top_of_row(x, 0) == []
    # nothing allowed
    assert LR.top_of_row(np.full(8, NINF), 3) == [(-1, NINF)] * 3
    # the probabilities of A sum to 1
    assert abs(np.exp(LR.row_logprobs(x)[x > NINF]).sum() - 1.0) < 1e-12


def test_the_sequential_sum_is_fp32_in_step_order():
    vals = [np.float32(-1e-8), np.float32(-3.0), np.float32(-1e-8), np.float32(-7.25)]
    s = np.float32(0.0)
    for v in vals:
        s = np.float32(s + v)
    assert LR.seq_sum_f32(vals) == s and LR.seq_sum_f32(vals).dtype == np.float32
    assert LR.seq_sum_f32([]) == np.float32(0.0)
    # the order matters in fp32: this is not the fp64 sum rounded once
    big = [np.float32(-16777216.0), np.float32(-1.0), np.float32(-1.0)]
    assert LR.seq_sum_f32(big) == np.float32(-16777216.0) and LR.seq_sum_f32(big[::-1]) == np.float32(-16777218.0)


def test_tie_free_rows_against_torch_topk(generated):
    seen = 0
    for (vocab, rs), (V, rules, opts, cases) in generated.items():
        for c in cases:
            if not LR.samples(c) or c.tie:
                continue
            flt = TR.filtered_row(c.logits, c.sampled, rules, opts)
            lsm = torch.log_softmax(flt.double(), dim=-1)
            allowed = int(torch.isfinite(flt).sum())
            for n in LR.NS:
                lp, top = LR.rule(c.logits, c.sampled, rules, opts, n)
                k = min(n, allowed)
                vals, idx = torch.topk(lsm, k) if k else (torch.zeros(0), torch.zeros(0))
                assert [i for i, _ in top[:k]] == idx.tolist(), (vocab, rs, c.name, n)
                assert all(abs(a - float(b)) < 1e-12 for (_, a), b in zip(top[:k], vals)), (vocab, rs, c.name, n)
                assert top[k:] == [(-1, NINF)] * (n - k)
                seen += 1
    assert seen >= 4 * 4 * len(LR.VOCABS)


def test_generated_rows_have_their_margins_and_their_kinds(generated):
    for (vocab, rs), (V, rules, opts, cases) in generated.items():
        names = [c.name for c in cases]
        assert names[0] == "finished row" and names[1] == "prompt phase" and "first step" in names and "mid text" in names
        ties = [c for c in cases if c.tie]
        assert any("neighbouring threads" in c.name for c in ties) and any("different waves" in c.name for c in ties)
        if V > 8192:
            assert any("one thread, two groups" in c.name for c in ties)
        if rs == "rules" and V - rules.timestamp_begin > 64:
            assert any(c.name == "forced timestamp" for c in cases)
        for c in cases:
            if not LR.samples(c):
                continue
            gap, span, n_ties, allowed = LR.case_margins(c, rules, opts)
            assert gap >= LR.LOGIT_MARGIN and span <= LR.SPAN and n_ties == (1 if c.tie else 0), (vocab, rs, c.name, gap, span, n_ties)
            if c.name == "first step" and rs == "rules":
                assert allowed == min(TR.MAX_INITIAL_TS + 1, V - rules.timestamp_begin) < LR.MAX_TOP
            else:
                assert allowed > LR.MAX_TOP
            if c.tie:                # the equal pair is placed as its name says
                _, top = LR.rule(c.logits, c.sampled, rules, opts, LR.MAX_TOP)
                x = TR.filtered_row(c.logits, c.sampled, rules, opts)
                pair = [(top[k][0], top[k + 1][0]) for k in range(LR.MAX_TOP - 1) if x[top[k][0]] == x[top[k + 1][0]]]
                assert len(pair) == 1 and pair[0][0] < pair[0][1]
                kind = c.name[c.name.rindex("(") + 1:-1]
                assert LR.tie_pair_ok(kind, *pair[0]), (c.name, pair)
            if c.name.startswith("forced timestamp"):      # the force rule holds, and removes text that would be listed
                _, top = LR.rule(c.logits, c.sampled, rules, opts, LR.MAX_TOP)
                assert all(i >= rules.timestamp_begin for i, _ in top)


def test_a_row_with_every_id_suppressed_has_nothing_allowed():
    V = 1024
    rules, opts = LR.rules_for(V), LR.all_suppressed(V)
    c = LR.logprob_cases(V, rules, LR.RULE_SETS["no rules"])[3]
    lp, top = LR.rule(c.logits, c.sampled, rules, opts, LR.MAX_TOP)
    assert top == [(-1, NINF)] * LR.MAX_TOP and not np.isfinite(lp).any()


@pytest.mark.parametrize("misreading", LR.MISREADINGS)
def test_every_misreading_changes_a_generated_case(generated, misreading):
    changed = 0
    for (vocab, rs), (V, rules, opts, cases) in generated.items():
        for c in cases:
            if not LR.samples(c):
                continue
            lp, top = LR.rule(c.logits, c.sampled, rules, opts, 5, temperature=TRUNC.temperature, trunc=TRUNC)
            lp2, top2 = LR.rule(c.logits, c.sampled, rules, opts, 5, temperature=TRUNC.temperature, trunc=TRUNC, misreading=misreading)
            ids, ids2 = [i for i, _ in top], [i for i, _ in top2]
            # a change the GPU tests see: other ids (compared exactly), or a value off by more than their bound allows (2e-5)
            if ids != ids2 or any(abs(a - b) > 1e-3 for (_, a), (_, b) in zip(top, top2) if a > NINF and b > NINF):
                changed += 1
    assert changed >= 1, misreading


# ---------------------------------------------------------------------------------------------- the C ABI
PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "ccx.h"
int main() {
  printf("CCX_LOGPROB_MAX_TOP %d\n", CCX_LOGPROB_MAX_TOP);
  printf("ccx_decode_logprob_options %zu\n", sizeof(ccx_decode_logprob_options));
  printf("ccx_decode_logprob_options.top_n %zu\n", offsetof(ccx_decode_logprob_options, top_n));
  printf("ccx_dec_select_desc %zu\n", sizeof(ccx_dec_select_desc));
  printf("ccx_dec_select_desc.kept_mass_out %zu\n", offsetof(ccx_dec_select_desc, kept_mass_out));
  printf("ccx_dec_select_desc.logprobs %zu\n", offsetof(ccx_dec_select_desc, logprobs));
  printf("ccx_dec_select_desc.tok_logprob_out %zu\n", offsetof(ccx_dec_select_desc, tok_logprob_out));
  printf("ccx_dec_select_desc.top_id_out %zu\n", offsetof(ccx_dec_select_desc, top_id_out));
  printf("ccx_dec_select_desc.top_lp_out %zu\n", offsetof(ccx_dec_select_desc, top_lp_out));
  return 0;
}
"""


def test_ctypes_mirrors_have_the_c_structs_layout(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert c.pop("CCX_LOGPROB_MAX_TOP") == _lib.LOGPROB_MAX_TOP == LR.MAX_TOP == 8
    mirrors = {"ccx_decode_logprob_options": _lib.DecodeLogprobOptions, "ccx_dec_select_desc": _lib.DecSelectDesc}
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == c[name], (name, C.sizeof(cls), c[name])
    for key, want in c.items():
        if "." in key:
            name, field = key.split(".")
            assert getattr(mirrors[name], field).offset == want, (key, getattr(mirrors[name], field).offset, want)
    # appended: nothing before the new fields moved
    assert _lib.DecSelectDesc.logprobs.offset == _lib.DecSelectDesc.kept_mass_out.offset + 8


def test_null_handles_need_no_device():
    lib = _lib.load()
    o = _lib.DecodeLogprobOptions(3)
    assert lib.ccx_whisper_set_token_logprobs(None, 1) == 1            # CCX_ERR_ARG
    assert lib.ccx_whisper_set_logprob_options(None, C.byref(o)) == 1
    assert lib.ccx_whisper_set_logprob_options(None, None) == 1
    assert lib.ccx_whisper_token_logprobs(None, 1, 1, None, 0, None, None, None) == 1
    assert lib.ccx_whisper_logprob_graph_count(None) == -1
    d = _lib.DecSelectDesc()
    assert not d.logprobs and not d.tok_logprob_out and not d.top_id_out and not d.top_lp_out


def test_the_opt_in_is_off_by_default():
    from clearconverse_amd import models
    from clearconverse_amd.whisper import CallSettings, WhisperModel
    assert inspect.signature(WhisperModel.__init__).parameters["token_logprobs"].default is False
    assert inspect.signature(models.load_models).parameters["whisper_token_logprobs"].default is False
    assert WhisperModel.token_logprobs is False
    assert CallSettings().logprobs is None and CallSettings._fields[-1] == "logprobs"
    for fn in (WhisperModel.decode, WhisperModel.decode_rows, WhisperModel.transcribe, WhisperModel.transcribe_batch):
        assert inspect.signature(fn).parameters["logprobs"].default is None
    assert "logprobs" not in inspect.signature(WhisperModel.decode_beam).parameters
