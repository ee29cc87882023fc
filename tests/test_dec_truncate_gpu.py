"""GPU: the truncating instantiations of the select kernel (dec_select_kernel<true, RULES, true>, csrc/dec_truncate.h) through
ccx_dec_select_step, against the rule in fp64 (tests/truncation_reference.py).  Every row comes from the generator there, whose margins
tests/test_truncation_reference_cpu.py asserts (top_p: 2e-3 of mass; top_k, min_p: 0.5 in logit units) and whose cases it proves
sensitive to every listed misreading of the rule -- so |K|, the cut, the token, the state machine and the next embedding are compared
EXACTLY.  One launch holds a finished row, a row in its prompt phase, a first-step row (under the rules with fewer allowed ids than
top_k of the "all three" set), a forced-timestamp row, mid-text rows and rows with ties.  The logit rows have NaN behind the
vocabulary; the three output arrays go in as NaN / a sentinel and rows that do not sample must leave them so.

kept_mass_out against fp64 -- the bound, from the kernel's own arithmetic (u = 2^-24):
  * a term is exp2((x - max) * (log2(e) * (1 / T))): the scale carries 2 roundings, the difference and the product one each, so the
    argument is off by <= 4 u relative; a term that matters (>= 1e-7 of the largest) has |argument| <= 23.3, so its value is off by
    <= 23.3 * ln 2 * 4 u = 3.9e-6 relative, plus v_exp_f32's 1 ulp (1.2e-7);
  * a sum is a chain of 52 (registers) + 6 (wave butterfly) + 16 (wave totals) = 74 additions of non-negative terms: <= 74 u = 4.4e-6;
  * the quotient of two such sums, one more rounding: <= 2 * (3.9e-6 + 1.2e-7 + 4.4e-6) + u = 1.7e-5 relative, of a mass <= 1.
  1.7e-5 is 1/29 of a quarter of the generator's 2e-3 margin (5e-4): the top_p decisions of these rows cannot flip.
  Measured on an MI355X over this file: see TOL_MASS below and DESIGN.md.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests import decoding_options_reference as DO
from tests import test_dec_select_gpu as TS
from tests import truncation_reference as TR
from tests.conftest import within

pytestmark = pytest.mark.gpu

MASS_BOUND_A_PRIORI = 1.7e-5
assert MASS_BOUND_A_PRIORI <= TR.MASS_MARGIN / 4
# at most 2.5 x the worst value an MI355X run of this file recorded (1.52e-7: DESIGN.md section 3), far inside the a-priori bound
TOL_MASS = 3.8e-7
assert TOL_MASS <= MASS_BOUND_A_PRIORI
N_MASS = "dec truncate: kept_mass_out, |err| against fp64"
N_DRAW = "dec truncate: reference margin of a draw the kernel decides otherwise"
KEPT_FILL = -12345
RULE_SETS = {"rules": DO.Options(), "no rules": DO.Options(True, True)}


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
    """every generated launch, made once and never changed: (vocab, rule set, param set) -> (V, rules, opts, prm, cases)"""
    cache = {}

    def get(vocab, rule_set, param_set):
        key = (vocab, rule_set, param_set)
        if key not in cache:
            V = TR.VOCABS[vocab]
            rules, opts, prm = TR.rules_for(V), RULE_SETS[rule_set], TR.PARAM_SETS[param_set]
            cache[key] = (V, rules, opts, prm, TR.trunc_cases(V, rules, opts, prm))
        return cache[key]
    return get


def _launch(ctx, V, rules, cases, emb, opts, temperature, seed, trunc=None, outs=True, sample=1, row0=0, override=None):
    """trunc: (top_k, top_p, min_p) or None (no sampling options: the plain kernels) -> (inp, out); out gains cut / kept / mass"""
    from clearconverse_amd import _lib
    B = len(cases)
    keep = []
    ov = {}
    if opts is not None and opts != DO.Options():
        sup = None if opts.suppress is None else (C.c_int * max(len(opts.suppress), 1))(*opts.suppress)
        mit = opts.max_initial_timestamp_index
        oc = _lib.DecodeOptions(int(opts.without_timestamps), int(opts.suppress_blank), -1 if mit is None else mit,
                                0 if opts.suppress is None else len(opts.suppress), sup)
        keep += [sup, oc]
        ov["opts"] = C.pointer(oc)
    cut = (C.c_float * B)(*[math.nan] * B)
    kept = (C.c_int * B)(*[KEPT_FILL] * B)
    mass = (C.c_float * B)(*[math.nan] * B)
    if trunc is not None:
        so = _lib.DecodeSamplingOptions(*trunc)
        keep.append(so)
        ov["sampling"] = C.pointer(so)
        if outs:
            ov.update(cut_out=cut, kept_out=kept, kept_mass_out=mass)
    ov.update(override or {})
    inp, out = TS._launch(ctx, V, rules, cases, emb, sample=sample, temperature=temperature, seed=seed, row0=row0, override=ov)
    out.update(cut=list(cut), kept=list(kept), mass=list(mass))
    return inp, out


def _same(a, b, rows=None):
    """two launches left the same bits (for the rows given)"""
    rows = range(len(a["gen"])) if rows is None else rows
    for r in rows:
        assert a["state"][r] == b["state"][r] and a["gen"][r] == b["gen"][r], r
        assert a["cur_tok"][r] == b["cur_tok"][r] and a["pos"][r] == b["pos"][r] and torch.equal(a["x"][r], b["x"][r]), r


def _f32(x):
    return float(np.float32(x))


def _reference(V, rules, opts, prm, cases, inp, emb, seed, row0=0):
    return [TR.select_step_ref(c.logits, inp["states"][b], inp["prompts"][b], inp["gens"][b], rules, opts, DR.SAMPLE_LEN, emb[0], emb[1],
                               prm, seed=seed, row=row0 + b) for b, c in enumerate(cases)]


@pytest.mark.parametrize("param_set", list(TR.PARAM_SETS))
@pytest.mark.parametrize("rule_set", list(RULE_SETS))
@pytest.mark.parametrize("vocab", list(TR.VOCABS))
def test_rows_against_the_rule(ccx_ctx, embeddings, case_sets, vocab, rule_set, param_set):
    V, rules, opts, prm, cases = case_sets(vocab, rule_set, param_set)
    emb = embeddings(V)
    trunc = (prm.top_k, prm.top_p, prm.min_p)
    eps = DR.sampling_eps(prm.temperature)
    draws = close = 0
    for seed in (5, 2 ** 41 + 9):
        inp, out = _launch(ccx_ctx, V, rules, cases, emb, opts, prm.temperature, seed, trunc)
        refs = _reference(V, rules, opts, prm, cases, inp, emb, seed)
        _, plain = _launch(ccx_ctx, V, rules, cases, emb, opts, prm.temperature, seed)
        finished, worst_draw, worst_mass = 0, 0.0, 0.0
        for b, (c, ref) in enumerate(zip(cases, refs)):
            what = (vocab, rule_set, param_set, seed, c.name)
            if ref.kept is None:                         # a finished row, a row in its prompt phase: nothing written
                assert math.isnan(out["cut"][b]) and out["kept"][b] == KEPT_FILL and math.isnan(out["mass"][b]), what
                TS._check_row(b, c, inp, out, ref.res, what)
                continue
            assert out["kept"][b] == ref.kept.n, (what, out["kept"][b], ref.kept.n)
            assert out["cut"][b] == _f32(ref.kept.cut), (what, out["cut"][b], ref.kept.cut)
            dev = abs(out["mass"][b] - ref.kept.mass)
            print(f"kept_mass {what}: kernel {out['mass'][b]:.9f} fp64 {ref.kept.mass:.9f} |err| {dev:.3e}")
            worst_mass = max(worst_mass, dev)
            got = out["gen"][b][len(c.sampled)]
            assert ref.kept.mask[got], (what, got)       # never an id outside K
            # coupling: where the untruncated draw lands in K, it is the truncated draw
            plain_tok = plain["gen"][b][len(c.sampled)]
            if ref.kept.mask[plain_tok]:
                assert got == plain_tok, (what, got, plain_tok)
            draws += 1
            close += ref.res.margin <= eps
            if got != ref.res.token:
                worst_draw = max(worst_draw, float(ref.res.scores[ref.res.token] - ref.res.scores[got]))
                continue
            finished += TS._check_row(b, c, inp, out, ref.res, what)
        within(N_DRAW, worst_draw, eps, (vocab, rule_set, param_set, seed))
        within(N_MASS, worst_mass, TOL_MASS, (vocab, rule_set, param_set, seed))
    assert close <= 0.02 * draws + 1, (close, draws)


@pytest.mark.parametrize("rule_set", list(RULE_SETS))
@pytest.mark.parametrize("vocab", list(TR.VOCABS))
def test_top_k_of_the_whole_vocabulary_is_the_plain_sampler(ccx_ctx, embeddings, case_sets, vocab, rule_set):
    """identity: top_k = n_vocab takes the truncating instantiation (it writes |K| = |A|) and leaves the plain launch's bits"""
    V, rules, opts, prm, cases = case_sets(vocab, rule_set, "top_p")
    emb = embeddings(V)
    for seed, T in ((1, 0.3), (2, 1.0)):
        inp, out = _launch(ccx_ctx, V, rules, cases, emb, opts, T, seed, (V, 1.0, 0.0))
        _, plain = _launch(ccx_ctx, V, rules, cases, emb, opts, T, seed)
        _same(out, plain)
        assert out["n_done"] == plain["n_done"]
        for b, c in enumerate(cases[2:], start=2):
            n_allowed = int(torch.isfinite(TR.filtered_row(c.logits, c.sampled, rules, opts)).sum())
            assert out["kept"][b] == n_allowed and abs(out["mass"][b] - 1.0) < 1e-6, (c.name, out["kept"][b], n_allowed, out["mass"][b])
        # ... and so do the default values, which still launch it
        _, dflt = _launch(ccx_ctx, V, rules, cases, emb, opts, T, seed, (0, 1.0, 0.0))
        _same(dflt, plain)
        assert dflt["kept"] == out["kept"]


@pytest.mark.parametrize("trunc", [(1, 1.0, 0.0), (0, 1e-9, 0.0), (0, 1.0, 1.0)], ids=["top_k 1", "top_p 1e-9", "min_p 1"])
def test_a_cut_to_one_id_is_the_greedy_kernel(ccx_ctx, embeddings, trunc):
    """collapse: the token and the bits of sum_logprob of the greedy launch, whatever the seed and the temperature"""
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.sampling_cases(V, rules, n_rows=8)
    emb = embeddings(V)
    _, greedy = _launch(ccx_ctx, V, rules, cases, emb, None, 0.0, 0, sample=0)
    for seed, T in ((3, 0.1), (4, 0.7), (2 ** 35, 2.0)):
        _, out = _launch(ccx_ctx, V, rules, cases, emb, None, T, seed, trunc)
        _same(out, greedy)
        assert out["kept"] == [1] * len(cases)
        assert out["cut"] == [_f32(TR.filtered_row(c.logits, c.sampled, rules).max()) for c in cases]


def test_a_row_alone_is_the_row_in_a_batch(ccx_ctx, embeddings, case_sets):
    V, rules, opts, prm, cases = case_sets("small.en / mini", "rules", "all three")
    emb = embeddings(V)
    trunc = (prm.top_k, prm.top_p, prm.min_p)
    _, out = _launch(ccx_ctx, V, rules, cases, emb, opts, prm.temperature, 11, trunc)
    for b in range(2, len(cases)):
        inp1, one = _launch(ccx_ctx, V, rules, cases[b:b + 1], emb, opts, prm.temperature, 11, trunc, row0=b)
        assert one["state"][0] == out["state"][b] and one["gen"][0] == out["gen"][b] and one["cur_tok"][0] == out["cur_tok"][b]
        assert (one["cut"][0], one["kept"][0], one["mass"][0]) == (out["cut"][b], out["kept"][b], out["mass"][b])
        if not torch.equal(one["x"][0], inp1["x"][0]):           # (a launch fills x from the same sentinel rows: only rows that moved on)
            assert torch.equal(one["x"][0], out["x"][b])
    # the same rows in another order and with the outputs off: the same tokens and states
    order = [4, 2, 6, 3, 5]
    sid = (C.c_int * len(order))(*order)
    _, perm = _launch(ccx_ctx, V, rules, [cases[i] for i in order], emb, opts, prm.temperature, 11, trunc, outs=False,
                      override={"stream_ids": sid})
    for j, i in enumerate(order):
        assert perm["state"][j] == out["state"][i] and perm["gen"][j] == out["gen"][i], (j, i)
    assert all(math.isnan(v) for v in perm["cut"])


def test_temperature_zero_ignores_the_three_values(ccx_ctx, embeddings, case_sets):
    V, rules, opts, prm, cases = case_sets("1024", "rules", "all three")
    emb = embeddings(V)
    _, greedy = _launch(ccx_ctx, V, rules, cases, emb, opts, 0.0, 0, sample=0)
    _, out = _launch(ccx_ctx, V, rules, cases, emb, opts, 0.0, 9, (2, 0.5, 0.5))
    _same(out, greedy)
    assert out["kept"] == [KEPT_FILL] * len(cases)      # no row sampled


REJECTIONS = [
    ("negative top_k", (-1, 1.0, 0.0), {}, "ccx_dec_select_step: opts.top_k = -1"),
    ("top_p zero", (0, 0.0, 0.0), {}, "ccx_dec_select_step: opts.top_p = 0"),
    ("top_p above one", (0, 1.5, 0.0), {}, "ccx_dec_select_step: opts.top_p = 1.5"),
    ("top_p NaN", (0, math.nan, 0.0), {}, "ccx_dec_select_step: opts.top_p"),
    ("min_p negative", (0, 1.0, -0.25), {}, "ccx_dec_select_step: opts.min_p = -0.25"),
    ("min_p above one", (0, 1.0, 1.25), {}, "ccx_dec_select_step: opts.min_p = 1.25"),
    ("min_p NaN", (0, 1.0, math.nan), {}, "ccx_dec_select_step: opts.min_p"),
    ("the greedy kernel", (3, 1.0, 0.0), {"sample": 0, "temperature": 0.0}, "sampling options need sample = 1"),
    ("outputs without options", None, {"kept_out": "arr"}, "need sampling options"),
]


@pytest.mark.parametrize("name,trunc,override,fragment", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(ccx_ctx, embeddings, name, trunc, override, fragment):
    from clearconverse_amd import _lib
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.select_cases(V, rules)[:2]
    override = dict(override)
    if override.get("kept_out") == "arr":
        override["kept_out"] = (C.c_int * 2)()
    with pytest.raises(_lib.CcxError) as e:
        _launch(ccx_ctx, V, rules, cases, embeddings(V), None, 0.5, 1, trunc, outs=False, override=override)
    assert fragment in str(e.value) and "(1)" in str(e.value), str(e.value)
