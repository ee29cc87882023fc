"""GPU: top_k / top_p / min_p through the model handle (ccx_whisper_set_sampling_options; the truncating select kernel in dec_head), at
the mini dims of tests/test_decode_history_gpu.py, on the two K / V paths (2 rows: split-KV kernels; 18 rows: the lean streaming kernel)
and on the X-stream path (CCX_CROSS_X_MIN_ROWS=1).

  * top_k = 1 at T = 0.7 is the greedy decode, top_k = n_vocab the plain sampling decode: tokens, sum_logprob, no_speech_prob bit for bit.
  * A truncated decode is walked teacher-forced: every step's kept set is computed in fp64 (tests/truncation_reference.py) from the
    instance's OWN ccx_whisper_decoder_logits row under the filters of tests/decoding_options_reference.py.  The step's logits and the
    teacher-forced row come from different kernels, so they agree to DELTA_LOGIT only (reasoned below); a
    logit shift of d moves a probability by at most a factor exp(2 d / T), which `_delta_mass` adds to the kernel's own
    mass bound (tests/test_dec_truncate_gpu.py).  Every token must lie in the kept set ENLARGED by those deltas; on every step whose
    boundary margins and draw margin exceed them it must equal the reference draw.  The share of steps excused is capped at 5 % and
    printed.
  * decode_rows: a row alone is the row in a batch, with repeated windows and explicit stream ids.
  * Graphs: default, plain sampling and truncation plans side by side; new values between two graph decodes capture nothing.
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
from tests import truncation_reference as TR
from tests.test_dec_truncate_gpu import MASS_BOUND_A_PRIORI

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
ORULES = R.Rules(suppress=tuple(RULES.suppress))
EOT, SOT = RULES.eot, RULES.sot
SL = 24
ROWS = 18
PATHS = [("kv16", 2, None), ("kv_stream", ROWS, None), ("xa_stream", 2, "1")]
T_WALK = 0.7
# the walk reads the instance's OWN logits, so the delta is the kernel's mass bound; on top of it one ulp of a logit of order 10
# (1e-6) for the last bits in which the step's row and the teacher-forced row may differ.  On an MI355X no step of this file decided
# otherwise than the reference at it, not even among the excused ones (printed as DISAGREE when one does).
DELTA_LOGIT = 1e-6
# (temperature, arguments).  top_p ALONE has no margin on this model at 0.7: its 51864 probabilities are ~2e-5 each, so consecutive
# cumulative values lie closer than any delta (an MI355X run: 38 of 48 steps within 1.7e-5, none of them decided otherwise) -- it is
# walked behind a top_k, which leaves it 25 values to cut among
WALKS = {"top_k": (T_WALK, dict(top_k=12)), "top_k top_p": (T_WALK, dict(top_k=25, top_p=0.6)),
         "min_p": (T_WALK, dict(min_p=0.05)), "all three": (T_WALK, dict(top_k=40, top_p=0.9, min_p=0.02))}


def _delta_mass(T):
    """the kernel's own mass bound plus what a logit shift of DELTA_LOGIT moves a probability by: a factor exp(2 d / T)"""
    return MASS_BOUND_A_PRIORI + math.expm1(2 * DELTA_LOGIT / T)


@pytest.fixture(scope="module")
def model(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    m = WhisperModel(dims, sd, max_batch=20, ctx=ccx_ctx, truncated_sampling=True)
    clips = [synthetic_clip(s, 30.0)[: int(t * 16000)] for s, t in zip(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS)]
    ns = [len(c) for c in clips]
    host = np.zeros((len(clips), max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    mel = m.log_mel(torch.from_numpy(host).cuda(), ns, return_mel=True).clone()
    m.set_mel(mel[torch.arange(ROWS, device=mel.device) % 2].contiguous())
    m.encode(ROWS)
    yield m
    m.close()


def _flat(res):
    return [(r["tokens"], r["sum_logprob"], r["no_speech_prob"]) for r in res]


def _path(monkeypatch, env):
    if env is not None:
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", env)


@pytest.mark.parametrize("path,rows,env", PATHS)
def test_top_k_1_is_greedy_and_top_k_n_vocab_is_plain_sampling(model, monkeypatch, path, rows, env):
    m = model
    _path(monkeypatch, env)
    prompts = [[SOT]] * rows
    greedy = _flat(m.decode(prompts, sample_len=SL))
    assert m.last_cross_path == path and len(greedy[0][0]) >= 4
    for trunc in (dict(top_k=1), dict(top_p=1e-9), dict(min_p=1.0)):
        assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=5, **trunc)) == greedy, trunc
    plain = _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=5))
    assert [t for t, _, _ in plain] != [t for t, _, _ in greedy]                 # the draw is a real choice on this model
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=5, top_k=m.dims.n_vocab)) == plain
    assert m.last_cross_path == path
    # temperature 0: the three values have no effect
    assert _flat(m.decode(prompts, sample_len=SL, top_k=3, top_p=0.5, min_p=0.2)) == greedy


def _enlarged(x, prm):
    """K under the rule with every boundary moved outward by the deltas: what a step whose logits differ by DELTA_LOGIT may keep"""
    A = np.isfinite(x)
    xs = np.sort(x[A].astype(np.float64))[::-1]
    keep = A.copy()
    if prm.top_k > 0 and len(xs) > prm.top_k:
        keep &= x >= xs[prm.top_k - 1] - 2 * DELTA_LOGIT
    big = TR.keep_set(x, TR.Params(prm.temperature, 0, min(1.0, prm.top_p + _delta_mass(prm.temperature)),
                                   prm.min_p * math.exp(-2 * DELTA_LOGIT / prm.temperature)))
    return keep & big.mask


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("path,rows,env", PATHS)
def test_truncated_decodes_walk_through_the_rule(model, monkeypatch, path, rows, env, walk):
    m = model
    _path(monkeypatch, env)
    T, kw = WALKS[walk]
    prm = TR.Params(T, kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("min_p", 0.0))
    seed = 1234
    res = m.decode([[SOT]] * rows, sample_len=SL, temperature=T, seed=seed, **kw)
    assert m.last_cross_path == path
    plain = m.decode([[SOT]] * rows, sample_len=SL, temperature=T, seed=seed)
    steps = excused = cut_steps = 0
    for b in range(2):
        toks = res[b]["tokens"] + ([EOT] if len(res[b]["tokens"]) < SL else [])
        seq = np.array([[SOT] + toks[:-1]] * 2, dtype=np.int32)
        lg = m.decoder_logits(seq)[b].cpu()                               # row i predicts toks[i]; window b
        slp = 0.0
        for i, tok in enumerate(toks):
            flt = DO.apply_filters(lg[i], toks[:i], ORULES)
            x = flt.numpy()
            k = TR.keep_set(x, prm)
            assert _enlarged(x, prm)[tok], (path, walk, b, i, tok)
            slp += float(torch.log_softmax(flt.double(), -1)[tok])
            steps += 1
            cut_steps += k.n < int(np.isfinite(x).sum())
            ref_tok, score = TR.truncated_draw(flt, prm, seed, b, i, k.mask)
            top2 = torch.topk(score.double(), 2).values
            gap = abs(TR.DR._force_gap(lg[i].float(), toks[:i], ORULES))      # the force-timestamp comparison of the filters
            decided = (k.mass_margin > _delta_mass(T) and k.logit_margin > 2 * DELTA_LOGIT and gap > 2 * DELTA_LOGIT
                       and float(top2[0] - top2[1]) > 2 * DELTA_LOGIT / T)
            if tok != ref_tok:
                print(f"  DISAGREE {path} {walk} row {b} step {i}: mass_margin {k.mass_margin:.3e} logit_margin {k.logit_margin:.3e} gap {gap:.3e} draw {float(top2[0] - top2[1]):.3e} in_K {bool(k.mask[tok])}")
            if decided:
                assert tok == ref_tok, (path, walk, b, i, tok, ref_tok)
            else:
                excused += 1
        # sum_logprob is the log-probability under the UNTRUNCATED filtered rows
        assert abs(slp - res[b]["sum_logprob"]) <= 1.5e-3 * max(1.0, abs(slp)), (path, walk, b, slp, res[b]["sum_logprob"])
    print(f"truncated walk {path} / {walk}: {steps} steps, {excused} excused ({100.0 * excused / steps:.1f} %), {cut_steps} really cut")
    assert excused <= 0.05 * steps, (path, walk, excused, steps)
    assert cut_steps >= steps // 2                                          # the truncation is not idle on this model
    # coupling, end to end: up to the first step at which the plain decode's draw leaves K the two decodes are one
    for b in range(2):
        t, p0 = res[b]["tokens"], plain[b]["tokens"]
        first = next((i for i, (x, y) in enumerate(zip(t, p0)) if x != y), None)
        print(f"  row {b}: first token that differs from the plain sampling decode: {first}")


def test_a_row_alone_is_the_row_in_a_batch(model):
    m = model
    kw = dict(sample_len=SL, temperature=0.7, seed=11, n_windows=2, top_k=30, top_p=0.85, min_p=0.01)
    a = m.decode_rows([[SOT]] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw)
    assert _flat(a) == _flat(m.decode_rows([[SOT]] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw))      # reproducible
    assert _flat(m.decode_rows([[SOT]] * 2, [0, 1], [1, 2], **kw)) == _flat([a[1], a[2]])
    assert _flat(m.decode_rows([[SOT]], [1], [3], **kw)) == _flat([a[3]])
    assert a[0]["tokens"] != a[1]["tokens"] or a[2]["tokens"] != a[3]["tokens"]                  # two draws per window
    # the row of a plain `decode` is stream id = row: the same numbers
    d = m.decode([[SOT]] * 2, **{k: v for k, v in kw.items() if k != "n_windows"})
    assert _flat(d) == _flat(m.decode_rows([[SOT]] * 2, [0, 1], [0, 1], **kw))


def test_graphs_side_by_side_and_values_without_a_capture(model, monkeypatch):
    m = model
    prompts = [[SOT], [RULES.sot_prev, 5000, SOT]]
    greedy = _flat(m.decode(prompts, sample_len=SL))
    plain = _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3))
    n_other = m.graph_count() - m.sampling_graph_count()
    assert n_other >= 2                                                     # the default plan and the plain sampling plan
    a = _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, top_k=8))
    n_trunc = m.sampling_graph_count()
    assert n_trunc >= 1 and m.graph_count() - n_trunc == n_other
    # new values: the same graphs, tokens that follow the values
    b = _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, top_k=1))
    c = _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, top_p=0.5, min_p=0.1))
    assert m.sampling_graph_count() == n_trunc and m.graph_count() - n_trunc == n_other
    assert b == greedy and a != greedy and c != a
    for r in a + c:
        assert len(r[0]) >= 1
    # the other plans kept their graphs and their bits
    assert _flat(m.decode(prompts, sample_len=SL)) == greedy
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3)) == plain
    assert m.sampling_graph_count() == n_trunc and m.graph_count() - n_trunc == n_other
    # (0, 1.0, 0.0) set explicitly: the plain sampling plan
    total = m.graph_count()
    m.set_sampling_options(0, 1.0, 0.0)
    try:
        assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3)) == plain
    finally:
        m.reset_sampling_options()
    assert m.graph_count() == total
    # graph against eager, bit for bit
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, top_k=8)) == a
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=3, top_p=0.5, min_p=0.1)) == c


def test_setting_is_sticky_checked_and_reset_by_set_rules(model):
    from clearconverse_amd import _lib
    m = model
    prompts = [[SOT], [SOT]]
    plain = _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=9))
    greedy = _flat(m.decode(prompts, sample_len=SL))
    m.set_sampling_options(top_k=1)
    try:
        assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=9)) == greedy       # sticky
        assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=9)) == greedy
    finally:
        m.reset_sampling_options()
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=9)) == plain
    for k, p, mp, frag in ((-1, 1.0, 0.0, "top_k"), (0, 0.0, 0.0, "top_p"), (0, 1.5, 0.0, "top_p"), (0, math.nan, 0.0, "top_p"),
                           (0, 1.0, -0.1, "min_p"), (0, 1.0, 1.1, "min_p"), (0, 1.0, math.nan, "min_p")):
        o = _lib.DecodeSamplingOptions(k, p, mp)
        rc = m.lib.ccx_whisper_set_sampling_options(m.handle, C.byref(o))
        assert rc == 1
        with pytest.raises(_lib.CcxError) as e:
            m.ctx.check(rc, "set")
        assert "ccx_whisper_set_sampling_options" in str(e.value) and frag in str(e.value), str(e.value)
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=9)) == plain              # a refused setting changes nothing
    with pytest.raises(ValueError):
        m.decode(prompts, sample_len=SL, top_p=0.0)
    # ccx_whisper_set_rules resets the setting (and drops every graph: last in this module)
    m.set_sampling_options(top_k=1)
    m.set_rules(m.rules)
    assert _flat(m.decode(prompts, sample_len=SL, temperature=0.7, seed=9)) == plain
    assert m.sampling_graph_count() == 0
