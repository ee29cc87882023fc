"""GPU: the two beam-search kernels (dec_beam_topk_kernel, dec_beam_update_kernel, csrc/dec_beam.hip) on logits, states and tables the
test chooses, through ccx_dec_beam_step, against tests/beam_reference.py.  Every case comes from the generator there, whose gaps
(filtered logits ranked beam + 1 / beam + 2 at least 0.5 apart, cumulative scores at least 0.05 apart) tests/test_beam_reference_cpu.py
asserts -- so proposals, tokens, parents, finished sets and their order, cache-indirection rows, states, n_done and the next embedding
are compared EXACTLY, and nothing is left out.  One launch = three windows: one complete (must stay untouched), one on its first sampled
step, one three tokens in.

Scores (log-probabilities of the proposals, cumulative scores of rows and finished hypotheses) against fp64: TOL_SCORE is 2.5 x the
worst deviation measured on an MI355X over this file ("Beam search"): 4.42e-7 measured.  The a-priori figure is the select
kernel's (tests/test_dec_select_gpu.py: 1.1e-5 for the increment) plus half an ulp of the sum.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import beam_reference as BR
from tests.conftest import within

pytestmark = pytest.mark.gpu

TOL_SCORE = 1.1e-6
TOL_NO_SPEECH = 2e-5              # relative, as tests/test_dec_select_gpu.py
N_SCORE = "dec beam: proposal log-probability / cumulative score, |err| against fp64"
N_NO_SPEECH = "dec beam: no_speech_prob, relative error"
FILL, N_DONE_IN, IND_FILL = -7, 5, 9999
_INTS = ("pos", "prompt_len", "n_gen", "done", "last_tok", "pen_tok", "last_ts_tok", "n_tokens")


@pytest.fixture(scope="module")
def embeddings():
    cache = {}

    def get(V):
        if V not in cache:
            g = torch.Generator().manual_seed(V)
            tok, pos = torch.randn(V, BR.D, generator=g), torch.randn(BR.N_POS, BR.D, generator=g)
            cache[V] = (tok, pos, tok.cuda(), pos.cuda())
        return cache[V]
    return get


def _rules_struct(rules, keep):
    from clearconverse_amd import _lib
    sup = (C.c_int * len(rules.suppress))(*rules.suppress)
    keep.append(sup)
    mit = rules.max_initial_timestamp_index
    return _lib.DecodeRules(rules.eot, rules.sot, rules.sot_prev, rules.no_speech, rules.no_timestamps, rules.timestamp_begin, rules.blank,
                            -1 if mit is None else mit, len(rules.suppress), sup)


def _inputs(case, rules, V):
    """the launch's host tables as numpy arrays / lists"""
    beam, mc = case.beam, case.max_cand
    R_ = 3 * beam
    g = np.random.default_rng(5 + beam)
    tsb = rules.timestamp_begin
    st = []
    for r in range(R_):
        s = case.sampled[r]
        ts = [t for t in s if t >= tsb]
        st.append(dict(pos=case.prompt_len - 1 + len(s), prompt_len=case.prompt_len, n_gen=len(s), done=case.done[r],
                       last_tok=s[-1] if s else -1, pen_tok=s[-2] if len(s) >= 2 else -1, last_ts_tok=ts[-1] if ts else -1,
                       n_tokens=len(s) if case.done[r] else 0, sum_logprob=float(np.float32(case.sum_logprob[r])),
                       no_speech_prob=0.25 if s else 0.0))
    hist = np.full((R_, BR.SAMPLE_LEN), FILL, dtype=np.int32)
    for r in range(R_):
        hist[r, :len(case.sampled[r])] = case.sampled[r]
    ind = np.full((R_, BR.N_POS), IND_FILL, dtype=np.uint16)
    for r in range(R_):
        w = r // beam
        ind[r, :st[r]["pos"] + 1] = g.integers(w * beam, (w + 1) * beam, st[r]["pos"] + 1)
    fin_tok = np.full((3, mc, BR.SAMPLE_LEN), FILL, dtype=np.int32)
    fin_score = np.full((3, mc), -99.0, dtype=np.float32)
    fin_n = np.full((3, mc), FILL, dtype=np.int32)
    fin_count = np.array(case.fin_count, dtype=np.int32)
    for w in range(3):
        for k in range(fin_count[w]):
            fin_tok[w, k, :2] = (tsb, BR.TEXT + k); fin_n[w, k] = 2; fin_score[w, k] = -0.5 - k
    cur = np.array([s[-1] if s else rules.sot for s in case.sampled], dtype=np.int32)
    pos = np.array([s["pos"] for s in st], dtype=np.int32)
    x = torch.randn(R_, BR.D, generator=torch.Generator().manual_seed(3))
    return dict(state=st, hist=hist, ind=ind, fin_tok=fin_tok, fin_score=fin_score, fin_n=fin_n, fin_count=fin_count, cur=cur, pos=pos, x=x)


def _launch(ctx, V, rules, case, emb, inp, override=None, state_override=None):
    from clearconverse_amd import _lib
    lib = _lib.load()
    beam, mc = case.beam, case.max_cand
    R_, K, ld = 3 * beam, beam + 1, (V + 127) // 128 * 128
    logits = torch.full((R_, ld), math.nan)
    logits[:, :V] = case.logits
    logits_d = logits.cuda()
    states = [dict(s) for s in inp["state"]]
    for b, (name, val) in (state_override or {}).items():
        states[b][name] = val
    st_c = (_lib.DecSeqState * R_)(*[_lib.DecSeqState(*[s[n] for n in _INTS], s["sum_logprob"], s["no_speech_prob"]) for s in states])
    out = {k: inp[k].copy() for k in ("hist", "ind", "fin_tok", "fin_score", "fin_n", "fin_count", "cur", "pos")}
    nd = (C.c_int * 1)(N_DONE_IN)
    x_d = inp["x"].cuda()
    cand_id, cand_lp = np.zeros((R_, K), dtype=np.int32), np.zeros((R_, K), dtype=np.float32)
    tok_out, par_out = np.zeros(R_, dtype=np.int32), np.zeros(R_, dtype=np.int32)
    keep = []
    r_c = _rules_struct(rules, keep)
    ip, fp, u16 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    d = _lib.DecBeamDesc()
    d.logits, d.ld, d.n_vocab = logits_d.data_ptr(), ld, V
    d.G, d.beam_size, d.max_candidates = 3, beam, mc
    d.rules, d.state, d.sample_len = C.pointer(r_c), st_c, BR.SAMPLE_LEN
    d.hist, d.cur_tok, d.pos, d.n_done = out["hist"].ctypes.data_as(ip), out["cur"].ctypes.data_as(ip), out["pos"].ctypes.data_as(ip), nd
    tok_dev, pos_dev = emb[2], emb[3]
    d.tok_emb, d.pos_emb, d.x, d.D = tok_dev.data_ptr(), pos_dev.data_ptr(), x_d.data_ptr(), BR.D
    d.ind, d.ind_ld = out["ind"].ctypes.data_as(u16), BR.N_POS
    d.fin_tok, d.fin_score = out["fin_tok"].ctypes.data_as(ip), out["fin_score"].ctypes.data_as(fp)
    d.fin_n, d.fin_count = out["fin_n"].ctypes.data_as(ip), out["fin_count"].ctypes.data_as(ip)
    d.cand_id, d.cand_lp = cand_id.ctypes.data_as(ip), cand_lp.ctypes.data_as(fp)
    d.tok_out, d.parent_out = tok_out.ctypes.data_as(ip), par_out.ctypes.data_as(ip)
    d.logits_elems, d.tok_emb_elems, d.pos_emb_elems, d.x_elems = logits_d.numel(), tok_dev.numel(), pos_dev.numel(), x_d.numel()
    for name, val in (override or {}).items():
        setattr(d, name, val(getattr(d, name)) if callable(val) else val)
    rc = lib.ccx_dec_beam_step(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_beam_step")
    out.update(state=[{n: getattr(st_c[b], n) for n in _INTS + ("sum_logprob", "no_speech_prob")} for b in range(R_)],
               n_done=nd[0], x=x_d.cpu(), cand_id=cand_id, cand_lp=cand_lp, tok=tok_out, parent=par_out)
    return out


@pytest.mark.parametrize("beam,variant", BR.KERNEL_CASES)
@pytest.mark.parametrize("V", BR.KERNEL_VOCABS)
def test_step_exactly(ccx_ctx, embeddings, V, beam, variant):
    rules = BR.rules_for(V)
    case = BR.beam_case(V, rules, beam, variant)
    emb = embeddings(V)
    inp = _inputs(case, rules, V)
    out = _launch(ccx_ctx, V, rules, case, emb, inp)
    K, mc, tsb = beam + 1, case.max_cand, rules.timestamp_begin
    n_done = N_DONE_IN
    # ---- window 0: complete, nothing of it moves ----
    for r in range(beam):
        assert out["state"][r] == inp["state"][r], r
        assert out["tok"][r] == -1 and out["parent"][r] == -1
        assert (out["cand_id"][r] == -1).all()                       # the operator's fill: the top-k kernel left the row alone
    for key in ("hist", "ind", "cur", "pos"):
        assert np.array_equal(out[key][:beam], inp[key][:beam]), key
    for key in ("fin_tok", "fin_score", "fin_n", "fin_count"):
        assert np.array_equal(out[key][0], inp[key][0]), key
    assert torch.equal(out["x"][:beam], inp["x"][:beam])
    # ---- windows 1 and 2 against the reference ----
    for w in (1, 2):
        r0 = w * beam
        cands, props = BR.case_candidates(case, rules, w)
        for j in range(beam):                                        # the proposals, in order
            got_ids = [int(i) for i in out["cand_id"][r0 + j]]
            want = props[j]
            assert got_ids == [i for i, _ in want] + [-1] * (K - len(want)), (w, j, got_ids, want)
            for k, (_, lp) in enumerate(want):
                within(N_SCORE, abs(float(out["cand_lp"][r0 + j][k]) - lp), TOL_SCORE, (w, j, k))
        win = BR.case_window(case, w)
        n_fin0 = int(inp["fin_count"][w])
        win.finished = [(None, None)] * n_fin0
        rec = BR.apply_walk(win, cands, beam, mc, rules.eot, BR.SAMPLE_LEN)
        stop = win.complete
        n_gen, pos_old = inp["state"][r0]["n_gen"], inp["state"][r0]["pos"]
        if w == 2 and variant == "eot":
            assert stop and len(rec["appended"]) == 1 and len(rec["finished"]) >= 1      # the list fills mid-step
        if w == 1 or variant == "force":
            assert not stop
        n_done += beam if stop else 0
        # finished tables: appended in order behind what was there, everything else untouched
        assert out["fin_count"][w] == n_fin0 + len(rec["appended"])
        want_tok, want_n, want_sc = inp["fin_tok"][w].copy(), inp["fin_n"][w].copy(), inp["fin_score"][w].copy()
        for k, c in enumerate(rec["appended"]):
            slot = n_fin0 + k
            want_tok[slot, :n_gen] = inp["hist"][r0 + c[1], :n_gen]; want_n[slot] = n_gen
            within(N_SCORE, abs(float(out["fin_score"][w][slot]) - c[0]), TOL_SCORE, (w, "finished", k))
            want_sc[slot] = out["fin_score"][w][slot]
        assert np.array_equal(out["fin_tok"][w], want_tok) and np.array_equal(out["fin_n"][w], want_n)
        assert np.array_equal(out["fin_score"][w], want_sc)
        nsp = float(torch.softmax(case.logits[r0].double(), dim=-1)[rules.no_speech]) if w == 1 else None
        for jj in range(beam):
            r, pj, tok = r0 + jj, rec["parents"][jj], rec["tokens"][jj]
            par = inp["state"][r0 + pj]
            assert out["tok"][r] == tok and out["parent"][r] == r0 + pj, (w, jj)
            got = out["state"][r]
            want = dict(pos=pos_old + (0 if stop else 1), prompt_len=par["prompt_len"], n_gen=n_gen + 1, done=int(stop), last_tok=tok,
                        pen_tok=par["last_tok"], last_ts_tok=tok if tok >= tsb else par["last_ts_tok"], n_tokens=n_gen + 1 if stop else 0)
            assert {n: got[n] for n in _INTS} == want, (w, jj, got, want)
            within(N_SCORE, abs(got["sum_logprob"] - rec["scores"][jj]), TOL_SCORE, (w, jj))
            if nsp is not None:
                within(N_NO_SPEECH, abs(got["no_speech_prob"] / nsp - 1.0), TOL_NO_SPEECH, (w, jj))
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
            assert torch.equal(out["x"][r], want_x), (w, jj)                            # the next embedding, bit for bit
            assert out["cur"][r] == want_cur and out["pos"][r] == want_pos, (w, jj)
    assert out["n_done"] == n_done


def test_first_step_ignores_the_other_rows(ccx_ctx, embeddings):
    """the first sampled step collapses a window's equal prefixes: rows 1.. hold logits that would outbid row 0's, and propose nothing"""
    V, beam = 1024, 5
    rules = BR.rules_for(V)
    case = BR.beam_case(V, rules, beam, "force")
    out = _launch(ccx_ctx, V, rules, case, embeddings(V), _inputs(case, rules, V))
    assert (out["cand_id"][beam + 1:2 * beam] == -1).all() and (out["parent"][beam:2 * beam] == beam).all()


@pytest.mark.parametrize("what,override,state_override", [
    ("beam_size", dict(beam_size=0), None),
    ("beam_size", dict(beam_size=9), None),
    ("max_candidates", dict(max_candidates=17), None),
    ("max_candidates", dict(max_candidates=0), None),
    ("n_vocab", dict(n_vocab=1022), None),
    ("logits", dict(logits=lambda p: p + 4), None),
    ("ld", dict(ld=1000), None),
    ("logits_elems", dict(logits_elems=lambda n: n - 200), None),
    ("x_elems", dict(x_elems=lambda n: n - 1), None),
    ("ind_ld", dict(ind_ld=4), None),
    ("sample_len", dict(sample_len=0), None),
    ("sampling phase", None, {4: ("prompt_len", 3)}),
    ("differs from its window", None, {5: ("n_gen", 2)}),
    ("done", None, {4: ("done", 2)}),
    ("fin_count", dict(fin_count="bad"), None),
])
def test_rejections(ccx_ctx, embeddings, what, override, state_override):
    from clearconverse_amd import _lib
    V, beam = 1024, 2
    rules = BR.rules_for(V)
    case = BR.beam_case(V, rules, beam, "force")
    inp = _inputs(case, rules, V)
    if override and override.get("fin_count") == "bad":
        inp["fin_count"][1] = case.max_cand + 1
        override = None
    so = {b: kv for b, kv in (state_override or {}).items()}
    with pytest.raises(_lib.CcxError) as e:
        _launch(ccx_ctx, V, rules, case, embeddings(V), inp, override=override, state_override=so)
    assert "ccx_dec_beam_step" in str(e.value) and what in str(e.value), str(e.value)
