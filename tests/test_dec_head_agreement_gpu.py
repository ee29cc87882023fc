"""GPU: the greedy select kernel (dec_select_kernel<false, RULES>, csrc/decoder.hip) and the beam top-k kernel at beam_size = 1
(dec_beam_topk_kernel<RULES>, csrc/dec_beam.hip) on the SAME logits and the SAME states, through ccx_dec_select_step and
ccx_dec_beam_step.  Both kernels run the filter of csrc/dec_head_row.h, so what they leave is compared as bits, against each other
and against no reference:

  * beam candidate 0's id is the token the select kernel wrote to gen;
  * beam candidate 0's log-probability and the select row's sum_logprob (0 going in: 0 + lp is lp) are the same 32 bits -- greedy
    forms -lnorm or (bs - mx_all) - lnorm, the first arg-max round forms (mx_all - mx_all) - lnorm or (bs - mx_all) - lnorm;
  * no_speech_prob of the first-step rows is the same 32 bits.

Rows: tests/dec_reference.select_cases at its smallest vocabulary and at the one whose last 4096-id round is ragged, every row that
is past its prompt (the beam operator takes no prompt-phase rows).  At beam_size = 1 every row is a window of its own, so the
first-step rows propose.  A row with no allowed id would end in the select kernel and propose -1 in the beam kernel: the Python
filters count such rows, and the count is asserted to be 0.
"""
import ctypes as C
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests import decoding_options_reference as DO
from tests import test_dec_select_gpu as TS
from tests import test_dec_select_options_gpu as TSO

pytestmark = pytest.mark.gpu

VOCABS = (DR.VOCABS["timestamp_begin + 4"], DR.VOCABS["small.en / mini"])
FILL = -7


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


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _beam1_launch(ctx, V, rules, cases, emb, override):
    """ccx_dec_beam_step with beam_size = 1: one window per row.  Returns candidate 0 (id, log-probability) and no_speech_prob per row."""
    from clearconverse_amd import _lib
    lib = _lib.load()
    R_, ld, SL, mc = len(cases), (V + 127) // 128 * 128, DR.SAMPLE_LEN, 1
    logits = torch.full((R_, ld), math.nan)
    for b, c in enumerate(cases):
        logits[b, :V] = c.logits
    logits_d = logits.cuda()
    states = [c.state(rules) for c in cases]
    st_c = (_lib.DecSeqState * R_)(*[_lib.DecSeqState(*[getattr(s, n) for n in TS._STATE_INTS], s.sum_logprob, s.no_speech_prob) for s in states])
    hist = np.array([(c.sampled + [FILL] * SL)[:SL] for c in cases], dtype=np.int32)
    cur = np.array([c.sampled[-1] if c.sampled else c.prompt[-1] for c in cases], dtype=np.int32)
    pos = np.array([s.pos for s in states], dtype=np.int32)
    ind = np.zeros((R_, DR.N_POS), dtype=np.uint16)
    fin_tok, fin_score = np.full((R_, mc, SL), FILL, dtype=np.int32), np.zeros((R_, mc), dtype=np.float32)
    fin_n, fin_count = np.zeros((R_, mc), dtype=np.int32), np.zeros(R_, dtype=np.int32)
    cand_id, cand_lp = np.zeros((R_, 2), dtype=np.int32), np.zeros((R_, 2), dtype=np.float32)
    tok_out, par_out = np.zeros(R_, dtype=np.int32), np.zeros(R_, dtype=np.int32)
    nd = (C.c_int * 1)(0)
    x_d = torch.zeros(R_, TS.D).cuda()
    keep = []
    r_c = TS._rules_struct(rules, keep)
    ip, fp, u16 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    d = _lib.DecBeamDesc()
    d.logits, d.ld, d.n_vocab = logits_d.data_ptr(), ld, V
    d.G, d.beam_size, d.max_candidates = R_, 1, mc
    d.rules, d.state, d.sample_len = C.pointer(r_c), st_c, SL
    d.hist, d.cur_tok, d.pos, d.n_done = hist.ctypes.data_as(ip), cur.ctypes.data_as(ip), pos.ctypes.data_as(ip), nd
    d.tok_emb, d.pos_emb, d.x, d.D = emb[2].data_ptr(), emb[3].data_ptr(), x_d.data_ptr(), TS.D
    d.ind, d.ind_ld = ind.ctypes.data_as(u16), DR.N_POS
    d.fin_tok, d.fin_score = fin_tok.ctypes.data_as(ip), fin_score.ctypes.data_as(fp)
    d.fin_n, d.fin_count = fin_n.ctypes.data_as(ip), fin_count.ctypes.data_as(ip)
    d.cand_id, d.cand_lp = cand_id.ctypes.data_as(ip), cand_lp.ctypes.data_as(fp)
    d.tok_out, d.parent_out = tok_out.ctypes.data_as(ip), par_out.ctypes.data_as(ip)
    d.logits_elems, d.tok_emb_elems, d.pos_emb_elems, d.x_elems = logits_d.numel(), emb[2].numel(), emb[3].numel(), x_d.numel()
    for name, val in override.items():
        setattr(d, name, val)
    rc = lib.ccx_dec_beam_step(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_beam_step")
    return [(int(cand_id[b][0]), float(cand_lp[b][0]), float(st_c[b].no_speech_prob)) for b in range(R_)]


def _agree(ctx, emb, V, rules, opts, seed, what):
    cases = [replace(c, sum_logprob=0.0) for c in DR.select_cases(V, rules, seed=seed)]
    cases = [c for c in cases if c.state(rules).pos >= len(c.prompt) - 1]            # past the prompt; finished rows stay in
    keep = []
    override = {} if opts is None else TSO._opts(opts, keep)
    o = DO.Options() if opts is None else opts
    _, sel = TS._launch(ctx, V, rules, cases, emb, override=override)
    beam = _beam1_launch(ctx, V, rules, cases, emb, override)
    compared = first = empty = 0
    for b, c in enumerate(cases):
        if c.done:
            continue
        empty += not bool(torch.isfinite(DO.apply_filters(c.logits.float(), c.sampled, rules, o)).any())
        n, st = len(c.sampled), sel["state"][b]
        cid, clp, nsp = beam[b]
        print(f"{what} | {c.name}: select {sel['gen'][b][n]} {st['sum_logprob']!r} | beam {cid} {clp!r}")
        assert cid == sel["gen"][b][n], (what, c.name, cid, sel["gen"][b][n])
        assert _bits(clp) == _bits(st["sum_logprob"]), (what, c.name, clp, st["sum_logprob"])
        if n == 0:
            assert _bits(nsp) == _bits(st["no_speech_prob"]) and nsp > 0.0, (what, c.name, nsp, st["no_speech_prob"])
            first += 1
        compared += 1
    assert empty == 0, (what, empty)
    assert compared >= 20 and first >= 3, (what, compared, first)


@pytest.mark.parametrize("max_initial_ts", [50, -1])
@pytest.mark.parametrize("V", VOCABS)
def test_select_and_beam1_agree_under_the_rules(ccx_ctx, embeddings, V, max_initial_ts):
    rules = DR.rules_for(V, max_initial_ts)
    _agree(ccx_ctx, embeddings(V), V, rules, None, max_initial_ts + 1, (V, "rules", max_initial_ts))


@pytest.mark.parametrize("option_set", ["call list", "suppress_blank off"])
@pytest.mark.parametrize("V", VOCABS)
def test_select_and_beam1_agree_without_the_rules(ccx_ctx, embeddings, V, option_set):
    rules = DR.rules_for(V)
    _agree(ccx_ctx, embeddings(V), V, rules, DO.option_sets(rules)[option_set], 0, (V, option_set))

