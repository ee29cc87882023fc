"""GPU: the two kernel-level pieces of a decode over a row -> window map (ccx_whisper_decode_rows), each on its own.

* form 7 of ccx_dec_attention_desc (CCX_DEC_ATTN_STREAM_MAPPED): dec_cross_stream_kernel<true, NP, false, true>, the lean streaming
  kernel reading the K/V of sequence row_seq[row].  Against the fp64 reference under the streaming form's own bound (the arithmetic is
  that of form 2: tests/test_dec_attention_gpu.py), and bit for bit against form 2 on K/V gathered physically into row order.
* the select kernel with a stream-id table: the Philox counter of row b is keyed by stream_ids[b] instead of row0 + b.  Against
  DR.select_step_ref(row=id) under DR.sampling_eps and the 2 % cap, as test_dec_select_gpu.py::test_sampling_equals_the_reference_draw
  (tests/test_fallback_reference_cpu.py shows the cap holds for these ids on the reference alone).
"""
import ctypes as C
import math

import pytest
import torch

from tests import dec_reference as DR
from tests import fallback_reference as FR
from tests import test_dec_attention_gpu as TA
from tests import test_dec_select_gpu as TS
from tests.conftest import within

pytestmark = pytest.mark.gpu

STREAM_MAPPED = 7
MAPPED_LABEL = {4: "dec_cross_stream_kernel<true,4,false,true>", 6: "dec_cross_stream_kernel<true,6,false,true>",
                12: "dec_cross_stream_kernel<true,12,false,true>"}
embeddings = TS.embeddings


@pytest.mark.parametrize("row_map", [[2, 0, 2, 1, 0], [2, 0, 2, 2, 0]], ids=["repeated, non-monotone", "sequence 1 unused"])
@pytest.mark.parametrize("T,kv_T", [(1500, 1536), (37, 128)])
def test_mapped_form_reads_the_mapped_sequence(ccx_ctx, T, kv_T, row_map):
    from clearconverse_amd import _lib
    assert _lib.DEC_ATTN_STREAM_MAPPED == STREAM_MAPPED
    H, n_seq, rows = 2, 3, 5
    q, k, v = TA._operands(300 + T, rows, n_seq, H, kv_T, gain=2.0)
    TA._pad_nan(k, v, [T] * n_seq)
    for s in set(range(n_seq)) - set(row_map):            # a sequence no row names is never read
        k[s], v[s] = math.nan, math.nan
    res = TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=T, row_seq=row_map, labels=True)
    assert res["labels"] == [MAPPED_LABEL[DR.np_pieces(T)]], res["labels"]
    ref, vmax = DR.attention_ref(q, k, v, [T] * rows, row_seq=row_map)
    TA._check_out(res, ref, vmax, ("stream mapped", T, row_map))
    # the unmapped kernel on K/V gathered into row order: the two runs differ in addresses only
    idx = torch.tensor(row_map)
    gathered = TA._run(ccx_ctx, TA.STREAM, k[idx].contiguous(), v[idx].contiguous(), q=q, T=T, labels=True)
    assert gathered["labels"] == [TA.STREAM_LABEL[DR.np_pieces(T)]]
    assert torch.equal(gathered["out"], res["out"])
    # the LDS claim of the lanes changes nothing, as for form 2
    padded = TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=T, row_seq=row_map, lds_pad=98304)
    assert torch.equal(padded["out"], res["out"])


def test_mapped_form_identity_map_and_null_map_equal_form2(ccx_ctx):
    T, kv_T, H = 500, 512, 2
    q, k, v = TA._operands(77, 3, 3, H, kv_T, gain=2.0)
    TA._pad_nan(k, v, [T] * 3)
    plain = TA._run(ccx_ctx, TA.STREAM, k, v, q=q, T=T)
    ident = TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=T, row_seq=[0, 1, 2])
    null = TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=T, labels=True)
    assert torch.equal(ident["out"], plain["out"]) and torch.equal(null["out"], plain["out"])
    assert null["labels"] == [TA.STREAM_LABEL[4]]          # no map: the instantiation of form 2


@pytest.mark.parametrize("row_map,fragment", [([0, 1, 3, 2], "row_seq[2] = 3"), ([0, -1, 1, 2], "row_seq[1] = -1")])
def test_mapped_form_rejects_a_map_entry_out_of_range(ccx_ctx, row_map, fragment):
    from clearconverse_amd import _lib
    q, k, v = TA._operands(78, 4, 3, 2, 32)
    ccx_ctx.prof_enable(True)
    try:
        with pytest.raises(_lib.CcxError) as e:
            TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=16, row_seq=row_map)
        assert ccx_ctx.prof_records() == []                 # nothing was launched
    finally:
        ccx_ctx.prof_enable(False)
    assert fragment in str(e.value) and "(1)" in str(e.value), str(e.value)
    # more rows than sequences is fine with a map, refused without one
    TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=16, row_seq=[0, 1, 2, 2])
    with pytest.raises(_lib.CcxError) as e:
        TA._run(ccx_ctx, STREAM_MAPPED, k, v, q=q, T=16)
    assert "row_seq is NULL" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# select kernel: stream ids
# ---------------------------------------------------------------------------------------------------------------------------------
def _ids(vals):
    return (C.c_int * len(vals))(*[int(x) for x in vals])


@pytest.mark.parametrize("temperature", FR.SELECT_TEMPERATURES)
def test_select_stream_ids_equal_the_reference_draw(ccx_ctx, embeddings, temperature):
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.sampling_cases(V, rules)
    ids = FR.SELECT_STREAM_IDS
    emb = embeddings(V)
    eps = DR.sampling_eps(temperature)
    draws = close = moved = 0
    for seed in FR.SELECT_SEEDS:
        inp, out = TS._launch(ccx_ctx, V, rules, cases, emb, sample=1, temperature=temperature, seed=seed, override={"stream_ids": _ids(ids)})
        refs = [DR.select_step_ref(c.logits, inp["states"][b], inp["prompts"][b], inp["gens"][b], rules, DR.SAMPLE_LEN, emb[0], emb[1],
                                   temperature=temperature, seed=seed, row=ids[b]) for b, c in enumerate(cases)]
        worst = 0.0
        for b, c in enumerate(cases):
            got_tok = out["gen"][b][len(c.sampled)]
            draws += 1
            close += refs[b].margin <= eps
            if got_tok != refs[b].token:
                assert 0 <= got_tok < V
                worst = max(worst, float(refs[b].scores[refs[b].token] - refs[b].scores[got_tok]))
                continue
            TS._check_row(b, c, inp, out, refs[b], (temperature, seed, c.name))
        within(TS.N_SAMPLING, worst, eps, (temperature, seed, "stream ids"))
        # the table is what keys the noise: the same rows under their batch rows draw otherwise somewhere
        _, plain = TS._launch(ccx_ctx, V, rules, cases, emb, sample=1, temperature=temperature, seed=seed)
        moved += plain["gen"] != out["gen"]
    assert close <= 0.02 * draws, (close, draws)
    assert moved >= 1


@pytest.mark.parametrize("row0", [0, 11])
def test_select_stream_ids_of_the_batch_rows_equal_the_null_table(ccx_ctx, embeddings, row0):
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.sampling_cases(V, rules)
    emb = embeddings(V)
    _, null = TS._launch(ccx_ctx, V, rules, cases, emb, sample=1, temperature=0.7, seed=99, row0=row0)
    _, tab = TS._launch(ccx_ctx, V, rules, cases, emb, sample=1, temperature=0.7, seed=99, row0=row0,
                        override={"stream_ids": _ids([row0 + b for b in range(len(cases))])})
    assert tab["state"] == null["state"] and tab["gen"] == null["gen"] and tab["cur_tok"] == null["cur_tok"]
    assert tab["pos"] == null["pos"] and tab["n_done"] == null["n_done"] and torch.equal(tab["x"], null["x"])
    # the greedy kernel does not look at the table
    _, g0 = TS._launch(ccx_ctx, V, rules, cases, emb)
    _, g1 = TS._launch(ccx_ctx, V, rules, cases, emb, override={"stream_ids": _ids(FR.SELECT_STREAM_IDS)})
    assert g0["state"] == g1["state"] and g0["gen"] == g1["gen"] and torch.equal(g0["x"], g1["x"])


def test_select_rejects_a_negative_stream_id(ccx_ctx, embeddings):
    from clearconverse_amd import _lib
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.select_cases(V, rules)[:2]
    with pytest.raises(_lib.CcxError) as e:
        TS._launch(ccx_ctx, V, rules, cases, embeddings(V), sample=1, temperature=0.5, override={"stream_ids": _ids([3, -2])})
    assert "stream_ids[1] = -2" in str(e.value) and "(1)" in str(e.value), str(e.value)
