"""GPU: the LOGP instantiations of the select kernel (dec_select_kernel<SAMPLE, RULES, TRUNC, true>, csrc/dec_logprobs.h) through
ccx_dec_select_step, against the rule in fp64 (tests/logprobs_reference.py, which restates it).  Every row comes from the generator
there, whose margins tests/test_logprobs_reference_cpu.py asserts (0.5 between the 9 best allowed values, built exact ties excepted)
and whose cases it proves sensitive to every listed misreading -- so ids, order and fill are compared EXACTLY.  All cases of a
vocabulary go through one launch per instantiation and top_n: a finished row, a row in its prompt phase, a first-step row (under the
rules: 5 allowed ids, fewer than 8), mid-text rows, a forced-timestamp row, rows with ties.  The output arrays go in under a sentinel
and rows that do not sample must leave it.

Exact: the ids and the fill; the tie order; tok_logprob_out[b] == state.sum_logprob after a launch from sum_logprob = 0, bit for bit;
the chosen id's entry == tok_logprob_out[b], bit for bit; the sentinel of rows that do not sample and of the top arrays at n = 0; and
every other output of the launch (state, gen, cur_tok, pos, n_done, x -- at T > 0 the token drawn) against the same launch without
the new fields.
Bounded: every returned log-probability against fp64, under the bound and by the expression of tests/test_dec_select_gpu.py's
TOL_LOGPROB (derived there: 2e-5 a priori), lowered to 2.5 x the worst value measured on an MI355X where that is smaller: see
TOL_LP below, profiles/token_logprobs_measured_deviations.json and DESIGN.md section 3.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests import decoding_options_reference as DO
from tests import logprobs_reference as LR
from tests import test_dec_select_gpu as TS
from tests import test_dec_truncate_gpu as TT
from tests import truncation_reference as TR
from tests.conftest import within

pytestmark = pytest.mark.gpu

# 2.5 x the worst value an MI355X run of this file recorded (5.851e-07 over 2766 checks: DESIGN.md section 3,
# profiles/token_logprobs_measured_deviations.json), far inside the a-priori bound of tests/test_dec_select_gpu.py
TOL_LP = 1.46e-6
assert TOL_LP <= TS.TOL_LOGPROB
N_LP = "dec logprobs: returned log-probability, |err| against fp64"
LP_FILL, ID_FILL, TLP_FILL = 777.0, -9, 555.0
TRUNC = (3, 0.9, 0.0)
T_WARM = 0.7
# name -> (rule set, sample, temperature, truncation)
INSTANTIATIONS = {
    "greedy ruled": ("rules", 0, 0.0, None),
    "sampling ruled": ("rules", 1, T_WARM, None),
    "greedy no-rules": ("no rules", 0, 0.0, None),
    "sampling no-rules": ("no rules", 1, T_WARM, None),
    "truncated ruled": ("rules", 1, T_WARM, TRUNC),
    "truncated no-rules": ("no rules", 1, T_WARM, TRUNC),
}


@pytest.fixture(scope="module")
def embeddings():
    cache = {}

    def get(V):
        if V not in cache:
            g = torch.Generator().manual_seed(V)
            tok, pos = torch.randn(V, TS.D, generator=g), torch.randn(DR.N_POS, TS.D, generator=g)
            cache[V] = (tok, pos, tok.cuda(), pos.cuda())
        return cache[V]
    return get


@pytest.fixture(scope="module")
def case_sets():
    """every generated launch and its fp64 reference, made once and never changed: (vocab, rule set) -> (V, rules, opts, cases, refs);
    refs[b] = (lp [V] fp64, the 8 best (id, lp)) or None for a row that does not sample"""
    cache = {}

    def get(vocab, rule_set):
        key = (vocab, rule_set)
        if key not in cache:
            V = LR.VOCABS[vocab]
            rules, opts = LR.rules_for(V), LR.RULE_SETS[rule_set]
            cases = LR.logprob_cases(V, rules, opts)
            refs = [LR.rule(c.logits, c.sampled, rules, opts, LR.MAX_TOP) if LR.samples(c) else None for c in cases]
            cache[key] = (V, rules, opts, cases, refs)
        return cache[key]
    return get


def _launch(ctx, V, rules, cases, emb, opts, sample, temperature, trunc, n=None, seed=11, override=None, top_arrays=True):
    """n None: the launch without the new fields -> (inp, out); out gains tok_lp [B], top_id / top_lp [B][n] (as the caller's arrays
    come back)"""
    from clearconverse_amd import _lib
    B = len(cases)
    ov, keep = {}, []
    tok_lp = (C.c_float * B)(*[LP_FILL] * B)
    m = max(n or 0, 1)
    top_id = (C.c_int * (B * m))(*[ID_FILL] * (B * m))
    top_lp = (C.c_float * (B * m))(*[TLP_FILL] * (B * m))
    if n is not None:
        lo = _lib.DecodeLogprobOptions(n)
        keep.append(lo)
        ov.update(logprobs=C.pointer(lo), tok_logprob_out=tok_lp)
        if top_arrays:
            ov.update(top_id_out=top_id, top_lp_out=top_lp)
    ov.update(override or {})
    inp, out = TT._launch(ctx, V, rules, cases, emb, opts, temperature, seed, trunc=trunc, outs=False, sample=sample, override=ov)
    out.update(tok_lp=list(tok_lp), top_id=np.array(top_id[:]).reshape(B, m), top_lp=np.array(top_lp[:], dtype=np.float64).reshape(B, m))
    return inp, out


def _bits(x):
    return struct.pack("<d", x)          # of a Python float that came out of a c_float: one to one with its 32 bits


def _same_launch(a, b):
    """every output the two launches share, bit for bit"""
    assert a["n_done"] == b["n_done"]
    for r in range(len(a["gen"])):
        sa, sb = a["state"][r], b["state"][r]
        assert all(_bits(float(sa[k])) == _bits(float(sb[k])) for k in sa), (r, sa, sb)
        assert a["gen"][r] == b["gen"][r] and a["cur_tok"][r] == b["cur_tok"][r] and a["pos"][r] == b["pos"][r], r
        assert a["x"][r].view(torch.int32).equal(b["x"][r].view(torch.int32)), r


@pytest.mark.parametrize("inst", list(INSTANTIATIONS))
@pytest.mark.parametrize("vocab", list(LR.VOCABS))
def test_rows_against_the_rule(ccx_ctx, embeddings, case_sets, vocab, inst):
    rule_set, sample, temperature, trunc = INSTANTIATIONS[inst]
    V, rules, opts, cases, refs = case_sets(vocab, rule_set)
    emb = embeddings(V)
    _, base = _launch(ccx_ctx, V, rules, cases, emb, opts, sample, temperature, trunc)
    for n in LR.NS:
        inp, out = _launch(ccx_ctx, V, rules, cases, emb, opts, sample, temperature, trunc, n=n)
        _same_launch(out, base)
        m = max(n, 1)
        for b, (c, ref) in enumerate(zip(cases, refs)):
            what = (vocab, inst, n, c.name)
            if ref is None:              # prompt phase / finished: the sentinel stands
                assert out["tok_lp"][b] == LP_FILL and (out["top_id"][b] == ID_FILL).all() and (out["top_lp"][b] == TLP_FILL).all(), what
                continue
            lp64, top = ref
            i_gen = inp["states"][b].n_gen
            tok = out["gen"][b][i_gen]
            # the step's increment IS the recorded value (a launch from sum_logprob = 0)
            assert inp["states"][b].sum_logprob == 0.0
            assert _bits(out["tok_lp"][b]) == _bits(out["state"][b]["sum_logprob"]), what
            within(N_LP, abs(out["tok_lp"][b] - lp64[tok]), TOL_LP, what)
            if n == 0:
                assert (out["top_id"][b] == ID_FILL).all() and (out["top_lp"][b] == TLP_FILL).all(), what
                continue
            ids = out["top_id"][b].tolist()
            assert ids == [i for i, _ in top[:n]], (what, ids, top[:n])          # ids, order (ties: the lower id first), fill
            for k, (i, want) in enumerate(top[:n]):
                got = float(out["top_lp"][b][k])
                if i < 0:
                    assert got == -math.inf, what
                else:
                    within(N_LP, abs(got - want), TOL_LP, what + (k,))
            if temperature == 0.0:
                assert ids[0] == tok, what
            if tok in ids:
                assert _bits(float(out["top_lp"][b][ids.index(tok)])) == _bits(out["tok_lp"][b]), what
        print(f"{vocab} / {inst} / n = {n}: ok")


@pytest.mark.parametrize("sample,temperature", [(0, 0.0), (1, T_WARM)], ids=["greedy", "sampling"])
def test_a_launch_with_every_id_suppressed(ccx_ctx, embeddings, case_sets, sample, temperature):
    """nothing allowed: the row ends with eot, the list is all fill, and the recorded value is whatever the step adds"""
    V, rules, _, cases, _ = case_sets("1024", "no rules")
    rows = [c for c in cases if LR.samples(c)][:3] + cases[:2]
    opts = LR.all_suppressed(V)
    emb = embeddings(V)
    _, base = _launch(ccx_ctx, V, rules, rows, emb, opts, sample, temperature, None)
    inp, out = _launch(ccx_ctx, V, rules, rows, emb, opts, sample, temperature, None, n=LR.MAX_TOP)
    _same_launch(out, base)
    for b, c in enumerate(rows):
        if not LR.samples(c):
            assert out["tok_lp"][b] == LP_FILL and (out["top_id"][b] == ID_FILL).all()
            continue
        assert out["gen"][b][inp["states"][b].n_gen] == rules.eot and out["state"][b]["done"] == 1
        assert (out["top_id"][b] == -1).all() and (out["top_lp"][b] == -math.inf).all()
        assert _bits(out["tok_lp"][b]) == _bits(out["state"][b]["sum_logprob"])


def _opts(n):
    from clearconverse_amd import _lib
    return C.pointer(_lib.DecodeLogprobOptions(n))


REJECTIONS = [
    ("top_n -1", dict(logprobs=lambda _: _opts(-1)), "opts.top_n = -1 out of range [0, 8]"),
    ("top_n 9", dict(logprobs=lambda _: _opts(9)), "opts.top_n = 9 out of range [0, 8]"),
    ("tok_logprob_out NULL", dict(tok_logprob_out=None), "tok_logprob_out NULL"),
    ("top_id_out NULL", dict(top_id_out=None), "top_id_out or top_lp_out NULL"),
    ("top_lp_out NULL", dict(top_lp_out=None), "top_id_out or top_lp_out NULL"),
    ("outputs without logprobs", dict(logprobs=None), "need logprobs"),
    ("tables too large", dict(sample_len=1 << 20), "B * sample_len"),
]


@pytest.mark.parametrize("name,override,fragment", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(ccx_ctx, embeddings, case_sets, name, override, fragment):
    from clearconverse_amd import _lib
    V, rules, opts, cases, _ = case_sets("1024", "rules")
    with pytest.raises(_lib.CcxError) as e:
        _launch(ccx_ctx, V, rules, cases, embeddings(V), opts, 0, 0.0, None, n=2, override=override)
    assert "ccx_dec_select_step" in str(e.value) and fragment in str(e.value), str(e.value)


def test_top_arrays_are_not_needed_at_zero(ccx_ctx, embeddings, case_sets):
    V, rules, opts, cases, refs = case_sets("1024", "rules")
    _, out = _launch(ccx_ctx, V, rules, cases, embeddings(V), opts, 0, 0.0, None, n=0, top_arrays=False)
    assert all((out["tok_lp"][b] == LP_FILL) == (refs[b] is None) for b in range(len(cases)))
