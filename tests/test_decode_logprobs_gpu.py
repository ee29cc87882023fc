"""GPU: per-token log-probabilities and top-N alternatives through the model handle (ccx_whisper_set_token_logprobs,
ccx_whisper_set_logprob_options, ccx_whisper_token_logprobs; the LOGP select kernels in dec_head), on the model of
tests/test_decode_truncate_gpu.py: mini dims, 2 layers, 128 wide, max_batch 20, SL = 24, its three cross-attention paths.

  * Setting off: an opted-in instance with logprobs=None against a default instance on the same weights -- tokens, sum_logprob and
    no_speech_prob bit for bit, equal graph counts, no log-probability plan.
  * Setting on: logprobs=5 leaves tokens, sum_logprob and no_speech_prob bit-identical to logprobs=None -- greedy, at T = 0.7, with
    top_k = 12, with repetition_penalty and a small bias table; on each path.  For every row of every such case the fp32 sum of
    token_logprobs in step order IS sum_logprob, and the lists are len(tokens) + 1 long when the row ended by eot, else len(tokens).
  * Walk: per step the instance's OWN ccx_whisper_decoder_logits row under the filters of tests/decoding_options_reference.py, fp64
    log-softmax.  Every returned (id, lp) lies within the kernel bound (tests/test_dec_logprobs_gpu.py TOL_LP) + 2 * DELTA_LOGIT of it
    (DELTA_LOGIT = 1e-6: tests/test_decode_truncate_gpu.py's stated and measured agreement of step logits and teacher-forced logits);
    no unreturned allowed id has a reference logit above the smallest returned one by more than 2 * DELTA_LOGIT; the ids of a step are
    distinct, allowed and in non-increasing lp; at T = 0 the first id is the token.  Value-based on purpose, no excused steps: this
    model's logits are nearly flat, a check of ranks would decide nothing.
  * decode_rows: a row alone is the row in a batch; CCX_NO_GRAPH=1 gives the graph run's lists; plans side by side; a second top_n
    captures exactly ONE more graph (include/ccx.h: top_n sits in the step plan); lanes; sticky, reset, refusals.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import decoding_options_reference as DO
from tests import logprobs_reference as LR
from tests.test_dec_logprobs_gpu import TOL_LP
from tests.test_decode_truncate_gpu import DELTA_LOGIT, PATHS, ROWS, SL

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
ORULES = R.Rules(suppress=tuple(RULES.suppress))
EOT, SOT = RULES.eot, RULES.sot
OPT_INS = dict(truncated_sampling=True, repetition_control=True, contextual_bias=True, beam_search=True, temperature_fallback=True,
               decoding_options=True)
CASES = {"greedy": dict(), "T = 0.7": dict(temperature=0.7, seed=5), "top_k": dict(temperature=0.7, seed=5, top_k=12),
         "penalty and bias": dict(repetition_penalty=1.3, sequence_bias={(1000,): 1.5, (2000,): -1.0})}
N = 5


def _encoded(m, dims, rows):
    clips = [synthetic_clip(s, 30.0)[: int(t * 16000)] for s, t in zip(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS)]
    ns = [len(c) for c in clips]
    host = np.zeros((len(clips), max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    mel = m.log_mel(torch.from_numpy(host).cuda(), ns, return_mel=True).clone()
    m.set_mel(mel[torch.arange(rows, device=mel.device) % 2].contiguous())
    m.encode(rows)


@pytest.fixture(scope="module")
def models(ccx_ctx):
    """(the opted-in instance, a default instance on the same weights), both with the two test windows encoded ROWS times"""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    m = WhisperModel(dims, sd, max_batch=20, ctx=ccx_ctx, token_logprobs=True, **OPT_INS)
    d = WhisperModel(dims, sd, max_batch=20, ctx=ccx_ctx, **OPT_INS)
    for x in (m, d):
        _encoded(x, dims, ROWS)
    yield m, d
    m.close()
    d.close()


def _flat(res):
    return [(r["tokens"], r["sum_logprob"], r["no_speech_prob"]) for r in res]


def _lists(res):
    return [(r["token_logprobs"], r.get("top_logprobs")) for r in res]


def _path(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS", raising=False)
    else:
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", env)


def _f32bits(x):
    return np.float32(x).view(np.uint32)


def test_setting_off_is_the_default_instance(models, monkeypatch):
    """first in the file: both instances have run the same calls, so their graph caches must match"""
    m, d = models
    for path, rows, env in PATHS:
        _path(monkeypatch, env)
        for name, kw in CASES.items():
            a = _flat(m.decode([[SOT]] * rows, sample_len=SL, logprobs=None, **kw))
            assert m.last_cross_path == path
            assert a == _flat(d.decode([[SOT]] * rows, sample_len=SL, **kw)), (path, name)
    assert m.graph_count() == d.graph_count() >= 3 and m.logprob_graph_count() == 0 == d.logprob_graph_count()
    assert m.token_logprobs is True and d.token_logprobs is False
    with pytest.raises(ValueError, match="token_logprobs=True"):
        d.decode([[SOT]], sample_len=SL, logprobs=0)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("path,rows,env", PATHS)
def test_setting_on_keeps_the_bits_and_sums_to_sum_logprob(models, monkeypatch, path, rows, env, case):
    m, _ = models
    _path(monkeypatch, env)
    kw = CASES[case]
    off = m.decode([[SOT]] * rows, sample_len=SL, **kw)
    on = m.decode([[SOT]] * rows, sample_len=SL, logprobs=N, **kw)
    assert m.last_cross_path == path and _flat(on) == _flat(off)
    assert all("token_logprobs" not in r and "top_logprobs" not in r for r in off)
    ended = 0
    for b, r in enumerate(on):
        lp, top = r["token_logprobs"], r["top_logprobs"]
        by_eot = len(r["tokens"]) < SL
        ended += by_eot
        assert len(lp) == len(top) == len(r["tokens"]) + (1 if by_eot else 0), (path, case, b)
        assert _f32bits(LR.seq_sum_f32(lp)) == _f32bits(r["sum_logprob"]), (path, case, b, LR.seq_sum_f32(lp), r["sum_logprob"])
        toks = r["tokens"] + ([EOT] if by_eot else [])
        for i, (tok, step) in enumerate(zip(toks, top)):
            assert 1 <= len(step) <= N
            ids = [v for v, _ in step]
            if tok in ids:           # the chosen id's entry is the recorded value
                assert _f32bits(step[ids.index(tok)][1]) == _f32bits(lp[i]), (path, case, b, i)
            if kw.get("temperature", 0.0) == 0.0:
                assert ids[0] == tok, (path, case, b, i)
    zero = m.decode([[SOT]] * rows, sample_len=SL, logprobs=0, **kw)
    assert _flat(zero) == _flat(off) and [r["token_logprobs"] for r in zero] == [r["token_logprobs"] for r in on]
    assert all("top_logprobs" not in r for r in zero)
    print(f"{path} / {case}: {rows} rows, {ended} ended by eot")


@pytest.mark.parametrize("case", ["greedy", "T = 0.7", "top_k"])
@pytest.mark.parametrize("path,rows,env", PATHS)
def test_returned_values_walk_through_the_rule(models, monkeypatch, path, rows, env, case):
    m, _ = models
    _path(monkeypatch, env)
    kw = CASES[case]
    res = m.decode([[SOT]] * rows, sample_len=SL, logprobs=N, **kw)
    assert m.last_cross_path == path
    bound = TOL_LP + 2 * DELTA_LOGIT
    worst = 0.0
    for b in range(2):
        toks = res[b]["tokens"] + ([EOT] if len(res[b]["tokens"]) < SL else [])
        seq = np.array([[SOT] + toks[:-1]] * 2, dtype=np.int32)
        lg = m.decoder_logits(seq)[b].cpu()                               # row i predicts toks[i]; window b
        assert len(res[b]["token_logprobs"]) == len(toks)
        for i, tok in enumerate(toks):
            flt = DO.apply_filters(lg[i], toks[:i], ORULES).double()
            ref = torch.log_softmax(flt, -1).numpy()
            x = flt.numpy()
            step = res[b]["top_logprobs"][i]
            ids, lps = [v for v, _ in step], [v for _, v in step]
            what = (path, case, b, i)
            assert len(set(ids)) == len(ids) and all(np.isfinite(x[v]) for v in ids), what
            assert all(lps[k] >= lps[k + 1] for k in range(len(lps) - 1)), what
            assert len(ids) == min(N, int(np.isfinite(x).sum())), what
            for v, lp in step:
                worst = max(worst, abs(lp - ref[v]))
                assert abs(lp - ref[v]) < bound, (what, v, lp, ref[v])
            rest = x.copy()
            rest[ids] = -np.inf
            assert rest.max() <= min(x[v] for v in ids) + 2 * DELTA_LOGIT, what
            assert abs(res[b]["token_logprobs"][i] - ref[tok]) < bound, what
            if kw.get("temperature", 0.0) == 0.0:
                assert ids[0] == tok, what
    print(f"logprob walk {path} / {case}: worst |lp - fp64| {worst:.3e} (bound {bound:.1e})")


def test_the_step_that_samples_eot_has_an_entry(models, monkeypatch):
    """this model never ends a row by itself inside SL steps; a call list that leaves <|0.00|> and eot alone does: the first step may
    only take the timestamp, the second (a timestamp pair cannot be closed by an equal one, every text id is suppressed) only eot.
    Each step has ONE allowed id: log-probability exactly 0, one pair, the rest trimmed."""
    m, _ = models
    _path(monkeypatch, None)
    tsb = RULES.timestamp_begin
    keep = {EOT, tsb}
    res = m.decode([[SOT]] * 2, sample_len=SL, logprobs=N, suppress_tokens=[v for v in range(m.dims.n_vocab) if v not in keep])
    off = m.decode([[SOT]] * 2, sample_len=SL, suppress_tokens=[v for v in range(m.dims.n_vocab) if v not in keep])
    assert _flat(res) == _flat(off)
    for r in res:
        assert r["tokens"] == [tsb] and r["sum_logprob"] == 0.0
        assert r["token_logprobs"] == [0.0, 0.0] and r["top_logprobs"] == [[(tsb, 0.0)], [(EOT, 0.0)]]


def test_a_row_alone_is_the_row_in_a_batch(models, monkeypatch):
    m, _ = models
    _path(monkeypatch, None)
    kw = dict(sample_len=SL, temperature=0.7, seed=11, n_windows=2, logprobs=N)
    a = m.decode_rows([[SOT]] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw)
    assert _lists(a) == _lists(m.decode_rows([[SOT]] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw))      # reproducible
    assert _lists(m.decode_rows([[SOT]] * 2, [0, 1], [1, 2], **kw)) == _lists([a[1], a[2]])
    assert _lists(m.decode_rows([[SOT]], [1], [3], **kw)) == _lists([a[3]])
    assert a[0]["tokens"] != a[1]["tokens"] or a[2]["tokens"] != a[3]["tokens"]                  # two draws per window
    d = m.decode([[SOT]] * 2, **{k: v for k, v in kw.items() if k != "n_windows"})
    assert _lists(d) == _lists(m.decode_rows([[SOT]] * 2, [0, 1], [0, 1], **kw))


def test_graphs_side_by_side_and_one_graph_per_top_n(models, monkeypatch):
    m, _ = models
    _path(monkeypatch, None)
    prompts = [[SOT], [RULES.sot_prev, 5000, SOT]]
    greedy = _flat(m.decode(prompts, sample_len=SL))
    total, lg = m.graph_count(), m.logprob_graph_count()
    a = m.decode(prompts, sample_len=SL, logprobs=7)
    assert (m.graph_count(), m.logprob_graph_count()) == (total + 1, lg + 1)        # its own plan, beside the default one
    assert _lists(m.decode(prompts, sample_len=SL, logprobs=7)) == _lists(a)
    assert (m.graph_count(), m.logprob_graph_count()) == (total + 1, lg + 1)        # the same top_n: nothing captured
    b = m.decode(prompts, sample_len=SL, logprobs=6)
    assert (m.graph_count(), m.logprob_graph_count()) == (total + 2, lg + 2)        # a second top_n: exactly one graph
    assert [r["token_logprobs"] for r in b] == [r["token_logprobs"] for r in a]
    assert [[s[:6] for s in r["top_logprobs"]] for r in a] == [r["top_logprobs"] for r in b]
    assert _flat(a) == greedy == _flat(b) == _flat(m.decode(prompts, sample_len=SL))
    assert (m.graph_count(), m.logprob_graph_count()) == (total + 2, lg + 2)
    # graph against eager, bit for bit
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    assert _lists(m.decode(prompts, sample_len=SL, logprobs=7)) == _lists(a)
    s = m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, logprobs=N)
    monkeypatch.delenv("CCX_NO_GRAPH")
    assert _lists(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, logprobs=N)) == _lists(s)


def test_lanes_return_the_lists_of_one_lane(ccx_ctx, monkeypatch):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    rows = 64        # two lanes of 32 rows: each above 16 rows, so both runs step through the kernels of one path ("kv_stream")
    m = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED), max_batch=rows, ctx=ccx_ctx, token_logprobs=True)
    try:
        _encoded(m, dims, rows)
        monkeypatch.setenv("CCX_DEC_LANES", "1")
        one = m.decode([[SOT]] * rows, sample_len=SL, temperature=0.7, seed=2, logprobs=N)
        g1 = m.logprob_graph_count()
        assert m.last_cross_path == "kv_stream"
        monkeypatch.setenv("CCX_DEC_LANES", "2")      # the second lane offsets the buffers by its first row
        m.prepare_lanes()
        two = m.decode([[SOT]] * rows, sample_len=SL, temperature=0.7, seed=2, logprobs=N)
        assert m.last_cross_path == "kv_stream"
        print(f"log-probability plans: one lane {g1}, then {m.logprob_graph_count()} (two more: the decode ran in two lanes)")
        assert _flat(two) == _flat(one) and _lists(two) == _lists(one)
        assert len({tuple(r["tokens"]) for r in one}) > 2       # the rows are not copies of each other at T = 0.7
    finally:
        m.close()


def test_sticky_reset_and_refusals(models, monkeypatch):
    """last in the file: ccx_whisper_set_rules drops every graph"""
    from clearconverse_amd import _lib
    m, d = models
    _path(monkeypatch, None)
    prompts = [[SOT], [SOT]]
    want = m.decode(prompts, sample_len=SL, logprobs=3)
    m.set_logprob_options(3)
    try:
        for _ in range(2):           # sticky: a plain decode records, the fetch follows
            got = m._with_logprobs(m.decode(prompts, sample_len=SL), 3, SL)
            assert _lists(got) == _lists(want)
        got = m._with_logprobs(m.decode(prompts, sample_len=SL), 2, SL)       # fewer than recorded: a prefix of every step
        assert [[s[:2] for s in r["top_logprobs"]] for r in want] == [r["top_logprobs"] for r in got]
        with pytest.raises(_lib.CcxError, match="top_n = 4"):
            m._with_logprobs(m.decode(prompts, sample_len=SL), 4, SL)
        with pytest.raises(_lib.CcxError, match="the last decode had 2 rows of 24"):
            m._with_logprobs(m.decode(prompts, sample_len=SL)[:1], 3, SL)
    finally:
        m.reset_logprob_options()
    plain = m.decode(prompts, sample_len=SL)
    with pytest.raises(_lib.CcxError, match="did not record"):
        m._with_logprobs(plain, 0, SL)
    # the setter's checks name it and the field; an instance without the buffers is refused whatever the value
    for model, n in ((m, -1), (m, 9), (d, 3)):
        o = _lib.DecodeLogprobOptions(n)
        rc = model.lib.ccx_whisper_set_logprob_options(model.handle, C.byref(o))
        assert rc == 1
        with pytest.raises(_lib.CcxError) as e:
            model.ctx.check(rc, "set")
        assert "ccx_whisper_set_logprob_options" in str(e.value) and "top_n" in str(e.value), str(e.value)
    assert _flat(m.decode(prompts, sample_len=SL)) == _flat(plain)                # a refused setting changes nothing
    with pytest.raises(_lib.CcxError, match="did not record"):
        m._with_logprobs(plain, 0, SL)
    # beam search has no log-probabilities
    with pytest.raises(ValueError, match="beam"):
        m.decode(prompts, sample_len=SL, beam_size=2, logprobs=2)
    with pytest.raises(ValueError, match="beam"):
        m.transcribe(np.zeros(16000, dtype=np.float32), beam_size=2, logprobs=2)
    hyps = m.decode_beam(prompts, 2, sample_len=SL)
    assert all("token_logprobs" not in h for g in hyps for h in g)
    # the library's beam decode ignores a setting that is on, and records nothing
    m.set_logprob_options(2)
    assert [[h["tokens"] for h in g] for g in m.decode_beam(prompts, 2, sample_len=SL)] == [[h["tokens"] for h in g] for g in hyps]
    with pytest.raises(_lib.CcxError, match="did not record"):
        m._with_logprobs(plain, 0, SL)
    # ccx_whisper_set_rules resets the setting and drops every graph
    m.set_rules(m.rules)
    assert _flat(m.decode(prompts, sample_len=SL)) == _flat(plain)
    with pytest.raises(_lib.CcxError, match="did not record"):
        m._with_logprobs(plain, 0, SL)
    assert m.logprob_graph_count() == 0
