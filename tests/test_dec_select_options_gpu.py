"""GPU: the select kernel under a call's decoding options (ccx_dec_select_desc.opts) through ccx_dec_select_step.

  * without_timestamps: the instantiations without ApplyTimestampRules (dec_select_kernel<SAMPLE, false>, csrc/decoder.hip) against
    one step of the state machine in plain Python (tests/decoding_options_reference.py).  The cases come from the generator there,
    which tests/test_decoding_options_reference_cpu.py proves decided (margins >= 0.5) and sensitive to a mutation of every rule they
    probe -- so tokens, tables, states, n_done and the next embedding are compared EXACTLY.  All cases of a vocabulary and option set
    go through ONE launch.  Vocabularies 1024 and 51864; the row stride is the vocabulary rounded up to 128, NaN behind it.
  * opts == NULL, default options and suppress_blank = 0 under the rules leave the bits of the ruled kernel on the existing cases.

Bounds: TOL_LOGPROB and TOL_NO_SPEECH of tests/test_dec_select_gpu.py -- the single softmax adds the same chains (52 terms per thread,
a wave tree, 16 waves) those were derived for; recorded under names of their own.
"""
import ctypes as C

import pytest
import torch

from tests import beam_reference as BR
from tests import dec_reference as DR
from tests import decoding_options_reference as DO
from tests import test_dec_select_gpu as TS
from tests.conftest import within

pytestmark = pytest.mark.gpu

N_LOGPROB = "dec select, no rules: sum_logprob increment, |err|"
N_NO_SPEECH = "dec select, no rules: no_speech_prob, relative error"
N_SAMPLING = "dec select, no rules: sampling, reference margin of a draw the kernel decides otherwise"
VOCABS = (1024, 51864)


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


def _opts(o: DO.Options, keep):
    from clearconverse_amd import _lib
    sup = None if o.suppress is None else (C.c_int * max(len(o.suppress), 1))(*o.suppress)
    mit = o.max_initial_timestamp_index
    oc = _lib.DecodeOptions(int(o.without_timestamps), int(o.suppress_blank), -1 if mit is None else mit,
                            0 if o.suppress is None else len(o.suppress), sup)
    keep += [sup, oc]
    return {"opts": C.pointer(oc)}


def _launch(ctx, V, rules, cases, emb, opts, **kw):
    keep = []
    override = dict(kw.pop("override", {}))
    if opts is not None:
        override.update(_opts(opts, keep))
    return TS._launch(ctx, V, rules, cases, emb, override=override, **kw)


def _reference(rules, opts, cases, inp, emb, temperature=0.0, seed=0):
    return [DO.select_step_ref(c.logits, inp["states"][b], inp["prompts"][b], inp["gens"][b], rules, opts, DR.SAMPLE_LEN, emb[0], emb[1],
                               temperature=temperature, seed=seed, row=b) for b, c in enumerate(cases)]


def _check_row(b, inp, out, res, what):
    """TS._check_row, with the deviations under this file's names"""
    st_in, got = inp["states"][b], out["state"][b]
    for n in TS._STATE_INTS:
        assert got[n] == getattr(res.state, n), (what, n, got[n], getattr(res.state, n))
    assert out["gen"][b] == res.gen, (what, out["gen"][b], res.gen)
    assert out["cur_tok"][b] == (inp["cur_tok"][b] if res.cur_tok is None else res.cur_tok), what
    assert out["pos"][b] == (inp["pos"][b] if res.pos is None else res.pos), what
    assert torch.equal(out["x"][b], inp["x"][b] if res.x is None else res.x), what
    if res.token is None:
        assert got["sum_logprob"] == TS._f32(st_in.sum_logprob) and got["no_speech_prob"] == TS._f32(st_in.no_speech_prob), what
        return 0
    within(N_LOGPROB, abs((got["sum_logprob"] - TS._f32(st_in.sum_logprob)) - res.logprob), TS.TOL_LOGPROB, what)
    if st_in.n_gen == 0:
        within(N_NO_SPEECH, abs(got["no_speech_prob"] / res.state.no_speech_prob - 1.0), TS.TOL_NO_SPEECH, what)
    else:
        assert got["no_speech_prob"] == TS._f32(st_in.no_speech_prob), what
    return res.finished


def _same(a, b):
    assert a["state"] == b["state"] and a["gen"] == b["gen"] and a["cur_tok"] == b["cur_tok"] and a["pos"] == b["pos"]
    assert a["n_done"] == b["n_done"] and torch.equal(a["x"], b["x"])


@pytest.mark.parametrize("option_set", ["rules' list", "call list", "no SuppressTokens", "suppress_blank off"])
@pytest.mark.parametrize("V", VOCABS)
def test_no_rules_cases_exactly(ccx_ctx, embeddings, V, option_set):
    rules = BR.rules_for(V)
    opts = DO.option_sets(rules)[option_set]
    cases = DO.select_cases(V, rules, opts)
    emb = embeddings(V)
    inp, out = _launch(ccx_ctx, V, rules, cases, emb, opts)
    refs = _reference(rules, opts, cases, inp, emb)
    finished = 0
    for b, c in enumerate(cases):
        if c.expect is not None:
            assert out["gen"][b][len(c.sampled)] == c.expect, (c.name, out["gen"][b], c.expect)
        finished += _check_row(b, inp, out, refs[b], (V, option_set, c.name))
    assert out["n_done"] == TS.N_DONE_IN + finished and finished >= 3
    # the sampling instantiation at temperature 0 leaves the greedy one's bits
    _, out2 = _launch(ccx_ctx, V, rules, cases, emb, opts, sample=1, temperature=0.0, seed=77)
    _same(out2, out)
    # ... and what max_initial_timestamp_index holds is not read without the rules
    _, out3 = _launch(ccx_ctx, V, rules, cases, emb, DO.Options(True, opts.suppress_blank, opts.suppress, 0))
    _same(out3, out)


@pytest.mark.parametrize("temperature", [0.1, 0.7, 5.0])
def test_no_rules_sampling_equals_the_reference_draw(ccx_ctx, embeddings, temperature):
    V = 51864
    rules = BR.rules_for(V)
    opts = DO.option_sets(rules)["call list"]
    cases = DO.sampling_cases(V, rules, n_rows=24)
    emb = embeddings(V)
    eps = DR.sampling_eps(temperature)
    draws = close = 0
    for seed in (99, 2 ** 40 + 5):
        inp, out = _launch(ccx_ctx, V, rules, cases, emb, opts, sample=1, temperature=temperature, seed=seed)
        refs = _reference(rules, opts, cases, inp, emb, temperature=temperature, seed=seed)
        worst = 0.0
        for b, c in enumerate(cases):
            got_tok = out["gen"][b][len(c.sampled)]
            draws += 1
            close += refs[b].margin <= eps
            if got_tok != refs[b].token:
                assert 0 <= got_tok < V
                worst = max(worst, float(refs[b].scores[refs[b].token] - refs[b].scores[got_tok]))
                continue
            _check_row(b, inp, out, refs[b], (temperature, seed, c.name))
        within(N_SAMPLING, worst, eps, (temperature, seed))
    assert close <= 0.04 * draws, (close, draws)


@pytest.mark.parametrize("max_initial_ts", [50, -1])
def test_null_default_and_suppress_blank_off_under_the_rules_are_one_kernel(ccx_ctx, embeddings, max_initial_ts):
    """the existing generator's cases: opts == NULL, the default options and suppress_blank = 0 (the first step bans every text id and
    eot anyway) give bit-identical outputs; so does the call's max_initial_timestamp_index where it names the rules' value"""
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V, max_initial_ts)
    cases = DR.select_cases(V, rules, seed=max_initial_ts + 1)
    emb = embeddings(V)
    _, base = _launch(ccx_ctx, V, rules, cases, emb, None)
    for what, opts in (("defaults", DO.Options()), ("suppress_blank = 0", DO.Options(False, False)),
                       ("the rules' index by the call", DO.Options(False, True, None, max_initial_ts)),
                       ("the rules' list by the call", DO.Options(False, True, tuple(rules.suppress)))):
        _, out = _launch(ccx_ctx, V, rules, cases, emb, opts)
        _same(out, base)
    # the call's index is honoured: another value moves the first-step rows
    _, other = _launch(ccx_ctx, V, rules, cases, emb, DO.Options(False, True, None, 0 if max_initial_ts else 3))
    assert other["gen"] != base["gen"]


@pytest.mark.parametrize("name,opts,fragment", [
    ("suppress id out of range", DO.Options(True, True, (51864,)), "ccx_dec_select_step: opts.suppress[0] = 51864"),
    ("negative suppress id", DO.Options(True, True, (5, -1)), "ccx_dec_select_step: opts.suppress[1] = -1"),
    ("max_initial_timestamp_index behind the vocabulary", DO.Options(False, True, None, 51864 - 50363), "opts.max_initial_timestamp_index"),
    ("max_initial_timestamp_index below -2", DO.Options(False, True, None, -3), "opts.max_initial_timestamp_index = -3"),
])
def test_rejections(ccx_ctx, embeddings, name, opts, fragment):
    from clearconverse_amd import _lib
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    with pytest.raises(_lib.CcxError) as e:
        _launch(ccx_ctx, V, rules, DR.select_cases(V, rules)[:2], embeddings(V), opts)
    assert fragment in str(e.value) and "(1)" in str(e.value), str(e.value)
