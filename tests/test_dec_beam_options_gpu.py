"""GPU: one beam-search step without ApplyTimestampRules (dec_beam_topk_kernel<false> + dec_beam_update_kernel, csrc/dec_beam.hip)
through ccx_dec_beam_step with `opts` set, against tests/decoding_options_reference.py (proposals) and tests/beam_reference.py (the
walk).  One launch = three windows: one on its first sampled step -- blank and eot stand above every proposal and are banned, or lead
the proposals with suppress_blank off -- and two mid-decode (a hypothesis finishes; blank, <|notimestamps|> and a timestamp below the
last one are proposed like any other id).  The generator's gaps (tests/test_decoding_options_reference_cpu.py) make proposals, tokens,
parents and finished sets exact; scores are held to tests/test_dec_beam_gpu.py's TOL_SCORE.  Vocabulary 1024; beam sizes 1, 2, 5.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import beam_reference as BR
from tests import decoding_options_reference as DO
from tests import test_dec_beam_gpu as TB
from tests.conftest import within

pytestmark = pytest.mark.gpu

N_SCORE = "dec beam, no rules: proposal log-probability / cumulative score, |err| against fp64"
N_NO_SPEECH = "dec beam, no rules: no_speech_prob, relative error"
V = 1024


@pytest.fixture(scope="module")
def emb():
    g = torch.Generator().manual_seed(V)
    tok, pos = torch.randn(V, BR.D, generator=g), torch.randn(BR.N_POS, BR.D, generator=g)
    return tok, pos, tok.cuda(), pos.cuda()


def _opts(o: DO.Options, keep):
    from clearconverse_amd import _lib
    sup = None if o.suppress is None else (C.c_int * max(len(o.suppress), 1))(*o.suppress)
    oc = _lib.DecodeOptions(int(o.without_timestamps), int(o.suppress_blank), -2, 0 if o.suppress is None else len(o.suppress), sup)
    keep += [sup, oc]
    return {"opts": C.pointer(oc)}


@pytest.mark.parametrize("option_set", ["call list", "suppress_blank off"])
@pytest.mark.parametrize("beam", [1, 2, 5])
def test_step_without_the_rules_exactly(ccx_ctx, emb, beam, option_set):
    rules = BR.rules_for(V)
    opts = DO.option_sets(rules)[option_set]
    case = DO.beam_case(V, rules, opts, beam)
    inp = TB._inputs(case, rules, V)
    keep = []
    out = TB._launch(ccx_ctx, V, rules, case, emb, inp, override=_opts(opts, keep))
    K, mc, tsb = beam + 1, case.max_cand, rules.timestamp_begin
    n_done = TB.N_DONE_IN
    for w in range(3):
        r0 = w * beam
        cands, props = DO.beam_candidates(case, rules, opts, w)
        for j in range(beam):
            got_ids = [int(i) for i in out["cand_id"][r0 + j]]
            want = props[j]
            assert got_ids == [i for i, _ in want] + [-1] * (K - len(want)), (w, j, got_ids, want)
            for k, (_, lp) in enumerate(want):
                within(N_SCORE, abs(float(out["cand_lp"][r0 + j][k]) - lp), TB.TOL_SCORE, (w, j, k))
        win = BR.case_window(case, w)
        rec = BR.apply_walk(win, cands, beam, mc, rules.eot, BR.SAMPLE_LEN)
        stop = win.complete
        n_gen, pos_old = inp["state"][r0]["n_gen"], inp["state"][r0]["pos"]
        n_done += beam if stop else 0
        assert out["fin_count"][w] == len(rec["appended"])
        if w == 1:
            assert len(rec["appended"]) == 1                  # row 0's eot finishes a hypothesis
        want_tok, want_n, want_sc = inp["fin_tok"][w].copy(), inp["fin_n"][w].copy(), inp["fin_score"][w].copy()
        for k, c in enumerate(rec["appended"]):
            want_tok[k, :n_gen] = inp["hist"][r0 + c[1], :n_gen]; want_n[k] = n_gen
            within(N_SCORE, abs(float(out["fin_score"][w][k]) - c[0]), TB.TOL_SCORE, (w, "finished", k))
            want_sc[k] = out["fin_score"][w][k]
        assert np.array_equal(out["fin_tok"][w], want_tok) and np.array_equal(out["fin_n"][w], want_n)
        assert np.array_equal(out["fin_score"][w], want_sc)
        nsp = float(torch.softmax(case.logits[r0].double(), dim=-1)[rules.no_speech]) if w == 0 else None
        for jj in range(beam):
            r, pj, tok = r0 + jj, rec["parents"][jj], rec["tokens"][jj]
            par = inp["state"][r0 + pj]
            assert out["tok"][r] == tok and out["parent"][r] == r0 + pj, (w, jj)
            got = out["state"][r]
            want = dict(pos=pos_old + (0 if stop else 1), prompt_len=par["prompt_len"], n_gen=n_gen + 1, done=int(stop), last_tok=tok,
                        pen_tok=par["last_tok"], last_ts_tok=tok if tok >= tsb else par["last_ts_tok"], n_tokens=n_gen + 1 if stop else 0)
            assert {n: got[n] for n in TB._INTS} == want, (w, jj, got, want)
            within(N_SCORE, abs(got["sum_logprob"] - rec["scores"][jj]), TB.TOL_SCORE, (w, jj))
            if nsp is not None:
                within(N_NO_SPEECH, abs(got["no_speech_prob"] / nsp - 1.0), TB.TOL_NO_SPEECH, (w, jj))
            else:
                assert got["no_speech_prob"] == par["no_speech_prob"]
            want_hist = inp["hist"][r].copy()
            want_hist[:n_gen] = inp["hist"][r0 + pj, :n_gen]; want_hist[n_gen] = tok
            assert np.array_equal(out["hist"][r], want_hist), (w, jj)
            want_ind, want_x, want_cur, want_pos = inp["ind"][r].copy(), inp["x"][r], inp["cur"][r], inp["pos"][r]
            if not stop:
                want_ind[:pos_old + 1] = inp["ind"][r0 + pj, :pos_old + 1]; want_ind[pos_old + 1] = r
                want_x, want_cur, want_pos = emb[0][tok] + emb[1][pos_old + 1], tok, pos_old + 1
            assert np.array_equal(out["ind"][r], want_ind), (w, jj)
            assert torch.equal(out["x"][r], want_x), (w, jj)
            assert out["cur"][r] == want_cur and out["pos"][r] == want_pos, (w, jj)
    assert out["n_done"] == n_done
    # the first-step ban, seen from the outside
    first = [int(i) for i in out["cand_id"][0]]
    if opts.suppress_blank:
        assert rules.blank not in first and rules.eot not in first
    else:
        assert first[:2] == [rules.blank, rules.eot][:K]


def test_default_options_and_null_are_one_kernel(ccx_ctx, emb):
    """the ruled top-k kernel: opts == NULL, the defaults and suppress_blank = 0 leave the same bits on an existing case"""
    rules = BR.rules_for(V)
    case = BR.beam_case(V, rules, 2, "force")
    inp = TB._inputs(case, rules, V)
    base = TB._launch(ccx_ctx, V, rules, case, emb, inp)
    for o in (DO.Options(), DO.Options(False, False)):
        keep = []
        out = TB._launch(ccx_ctx, V, rules, case, emb, inp, override=_opts(o, keep))
        for key in ("cand_id", "cand_lp", "tok", "parent", "hist", "ind", "fin_tok", "fin_score", "fin_n", "fin_count"):
            assert np.array_equal(out[key], base[key], equal_nan=True), key
        assert out["state"] == base["state"] and out["n_done"] == base["n_done"] and torch.equal(out["x"], base["x"])


def test_rejects_a_suppress_id_behind_the_vocabulary(ccx_ctx, emb):
    from clearconverse_amd import _lib
    rules = BR.rules_for(V)
    case = BR.beam_case(V, rules, 2, "force")
    keep = []
    with pytest.raises(_lib.CcxError) as e:
        TB._launch(ccx_ctx, V, rules, case, emb, TB._inputs(case, rules, V), override=_opts(DO.Options(True, True, (V,)), keep))
    assert f"ccx_dec_beam_step: opts.suppress[0] = {V}" in str(e.value)
