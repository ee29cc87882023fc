"""GPU: the decode step's token-select kernel (dec_select_kernel, csrc/decoder.hip) on logits the test chooses, through
ccx_dec_select_step, against one step of the state machine in plain Python (tests/dec_reference.py).  Every case comes from the
generator there, which tests/test_dec_reference_cpu.py proves decided (margins >= 0.5, force-timestamp comparison >= 0.05) and
sensitive to one-unit mutations of the kernel's folded ranges -- so tokens, tables and states are compared EXACTLY.  All cases of a
vocabulary and rule set go through ONE launch: rows in different states side by side.  The row stride is the vocabulary rounded up to
128, with NaN behind it.

Bounds (profiles/dec_kernels_measured_deviations.json): to be 2x the worst value measured on an MI355X over this
file; until a GPU session has measured them, the a-priori figures derived below.
  sum_logprob     absolute error of the step's increment against fp64; one bound, the rows whose logits are offset by +-3e4 included
                  (the kernel forms (x - max) - log(sum), which a common offset leaves alone)
  no_speech_prob  relative error against fp64
  sampling        the reference's margin between its own token and the kernel's where they differ (eps of the perturbed margin)
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests.conftest import within

pytestmark = pytest.mark.gpu

# A-PRIORI figures (DESIGN.md section 3 marks them as placeholders, to become 2 x measured),
# u = 2^-24: the <= 53248 probabilities are added in chains of ~75 terms (52 per thread, a wave tree, 16 waves): 75 u = 4.5e-6 relative in
# the sum, 1e-6 from the exponents' arguments, one ulp of logf; the difference (best - max) - log(sum) and the sum_logprob update each round at
# ulp(32) = 1.9e-6: 1.1e-5 in all.
TOL_LOGPROB = 2e-5
# expf, the same sum and a division: ~7e-6 relative
TOL_NO_SPEECH = 2e-5
N_LOGPROB = "dec select: sum_logprob increment, |err|"
N_NO_SPEECH = "dec select: no_speech_prob, relative error"
N_SAMPLING = "dec select: sampling, reference margin of a draw the kernel decides otherwise"
D = 64
GEN_FILL, N_DONE_IN = -7, 5
_STATE_INTS = ("pos", "prompt_len", "n_gen", "done", "last_tok", "pen_tok", "last_ts_tok", "n_tokens")


@pytest.fixture(scope="module")
def embeddings():
    cache = {}

    def get(V):
        if V not in cache:
            g = torch.Generator().manual_seed(V)
            tok, pos = torch.randn(V, D, generator=g), torch.randn(DR.N_POS, D, generator=g)
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


def _launch(ctx, V, rules, cases, emb, sample=0, temperature=0.0, seed=0, row0=0, override=None, state_override=None):
    """one launch for the rows `cases`; returns (inputs, outputs) as plain Python / CPU tensors"""
    from clearconverse_amd import _lib
    lib = _lib.load()
    B, ld = len(cases), (V + 127) // 128 * 128
    tok_cpu, pos_cpu, tok_dev, pos_dev = emb
    logits = torch.full((B, ld), math.nan)
    for b, c in enumerate(cases):
        logits[b, :V] = c.logits
    logits_d = logits.cuda()
    states = [c.state(rules) for c in cases]
    for b, (name, val) in (state_override or {}).items():
        setattr(states[b], name, val)
    st_c = (_lib.DecSeqState * B)(*[_lib.DecSeqState(*[getattr(s, n) for n in _STATE_INTS], s.sum_logprob, s.no_speech_prob) for s in states])
    prompts = [(c.prompt + [0] * DR.MAX_PROMPT)[:DR.MAX_PROMPT] for c in cases]
    gens = [(c.sampled + [GEN_FILL] * DR.SAMPLE_LEN)[:DR.SAMPLE_LEN] for c in cases]
    cur_in = [c.sampled[-1] if c.sampled else c.prompt[min(max(s.pos, 0), len(c.prompt) - 1)] for c, s in zip(cases, states)]
    pos_in = [s.pos for s in states]
    flat = lambda rows: (C.c_int * sum(len(r) for r in rows))(*[x for r in rows for x in r])
    prompt_c, gen_c, cur_c, pos_c, nd_c = flat(prompts), flat(gens), flat([cur_in]), flat([pos_in]), (C.c_int * 1)(N_DONE_IN)
    x_in = torch.randn(B, D, generator=torch.Generator().manual_seed(3))
    x_d = x_in.cuda()
    keep = []
    r_c = _rules_struct(rules, keep)
    d = _lib.DecSelectDesc()
    d.logits, d.ld, d.n_vocab, d.B = logits_d.data_ptr(), ld, V, B
    d.rules, d.state = C.pointer(r_c), st_c
    d.prompt, d.max_prompt, d.sample_len = prompt_c, DR.MAX_PROMPT, DR.SAMPLE_LEN
    d.gen, d.cur_tok, d.pos, d.n_done = gen_c, cur_c, pos_c, nd_c
    d.tok_emb, d.pos_emb, d.x, d.D = tok_dev.data_ptr(), pos_dev.data_ptr(), x_d.data_ptr(), D
    d.sample, d.temperature, d.seed, d.row0 = sample, temperature, seed, row0
    d.logits_elems, d.tok_emb_elems, d.pos_emb_elems, d.x_elems = logits_d.numel(), tok_dev.numel(), pos_dev.numel(), x_d.numel()
    for name, val in (override or {}).items():
        if name.startswith("rules."):
            setattr(r_c, name[6:], val)
        else:
            setattr(d, name, val(getattr(d, name)) if callable(val) else val)
    rc = lib.ccx_dec_select_step(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_select_step")
    out = {"state": [{n: getattr(st_c[b], n) for n in _STATE_INTS + ("sum_logprob", "no_speech_prob")} for b in range(B)],
           "gen": [list(gen_c[b * DR.SAMPLE_LEN:(b + 1) * DR.SAMPLE_LEN]) for b in range(B)],
           "cur_tok": list(cur_c), "pos": list(pos_c), "n_done": nd_c[0], "x": x_d.cpu()}
    inp = {"states": states, "prompts": prompts, "gens": gens, "cur_tok": cur_in, "pos": pos_in, "x": x_in}
    return inp, out


def _f32(x):
    return float(np.float32(x))


def _check_row(b, case, inp, out, res, what, tokens_only=False):
    """everything the kernel leaves for row b against the reference's step `res`; returns 1 if the row finished in this launch"""
    st_in, got = inp["states"][b], out["state"][b]
    for n in _STATE_INTS:
        assert got[n] == getattr(res.state, n), (what, n, got[n], getattr(res.state, n))
    assert out["gen"][b] == res.gen, (what, out["gen"][b], res.gen)                 # the whole row: nothing written elsewhere
    assert out["cur_tok"][b] == (inp["cur_tok"][b] if res.cur_tok is None else res.cur_tok), what
    assert out["pos"][b] == (inp["pos"][b] if res.pos is None else res.pos), what
    want_x = inp["x"][b] if res.x is None else res.x                                # untouched for rows that stop
    assert torch.equal(out["x"][b], want_x), what
    if res.token is None:                                                           # prompt phase / finished row: the floats stand
        assert got["sum_logprob"] == _f32(st_in.sum_logprob) and got["no_speech_prob"] == _f32(st_in.no_speech_prob), what
        return 0
    if not tokens_only:
        within(N_LOGPROB, abs((got["sum_logprob"] - _f32(st_in.sum_logprob)) - res.logprob), TOL_LOGPROB, what)
        if st_in.n_gen == 0:
            within(N_NO_SPEECH, abs(got["no_speech_prob"] / res.state.no_speech_prob - 1.0), TOL_NO_SPEECH, what)
        else:
            assert got["no_speech_prob"] == _f32(st_in.no_speech_prob), what
    return res.finished


def _reference(V, rules, cases, inp, emb, temperature=0.0, seed=0, row0=0):
    return [DR.select_step_ref(c.logits, inp["states"][b], inp["prompts"][b], inp["gens"][b], rules, DR.SAMPLE_LEN, emb[0], emb[1],
                               temperature=temperature, seed=seed, row=row0 + b) for b, c in enumerate(cases)]


@pytest.mark.parametrize("max_initial_ts", [50, 0, -1])
@pytest.mark.parametrize("vocab", list(DR.VOCABS))
def test_greedy_cases_exactly(ccx_ctx, embeddings, vocab, max_initial_ts):
    V = DR.VOCABS[vocab]
    rules = DR.rules_for(V, max_initial_ts)
    cases = DR.select_cases(V, rules, seed=max_initial_ts + 1)
    emb = embeddings(V)
    inp, out = _launch(ccx_ctx, V, rules, cases, emb)
    refs = _reference(V, rules, cases, inp, emb)
    finished = 0
    for b, c in enumerate(cases):
        if c.expect is not None:
            assert out["gen"][b][len(c.sampled)] == c.expect, (c.name, out["gen"][b], c.expect)
        finished += _check_row(b, c, inp, out, refs[b], (vocab, max_initial_ts, c.name))
    assert out["n_done"] == N_DONE_IN + finished and finished >= 3
    # the sampling kernel at temperature 0 leaves the greedy kernel's bits
    inp2, out2 = _launch(ccx_ctx, V, rules, cases, emb, sample=1, temperature=0.0, seed=77)
    assert out2["state"] == out["state"] and out2["gen"] == out["gen"] and out2["cur_tok"] == out["cur_tok"]
    assert out2["pos"] == out["pos"] and out2["n_done"] == out["n_done"] and torch.equal(out2["x"], out["x"])


def test_force_rule_normalises_over_timestamps_only(ccx_ctx, embeddings):
    """the forced step's log-probability is log_softmax over the timestamps alone: with the text mass counted it would be ~0.62 lower"""
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = [c for c in DR.select_cases(V, rules, seed=51) if c.name.startswith("force rule")]
    assert len(cases) == 4
    emb = embeddings(V)
    inp, out = _launch(ccx_ctx, V, rules, cases, emb)
    refs = _reference(V, rules, cases, inp, emb)
    for b, c in enumerate(cases):
        _check_row(b, c, inp, out, refs[b], c.name)
        tsb = rules.timestamp_begin
        forced = refs[b].token >= tsb
        assert forced == ("just below" not in c.name)
        if forced:
            allowed_ts = c.logits[tsb:].double()[tsb + 3 + 1 - tsb:]            # timestamps behind the last one (tsb + 3)
            assert abs(refs[b].logprob - float(c.logits[refs[b].token].double() - torch.logsumexp(allowed_ts, 0))) < 1e-9


@pytest.mark.parametrize("temperature", [0.1, 0.7, 5.0])
def test_sampling_equals_the_reference_draw(ccx_ctx, embeddings, temperature):
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.sampling_cases(V, rules)
    emb = embeddings(V)
    eps = DR.sampling_eps(temperature)
    draws = close = 0
    for seed in (99, 2 ** 40 + 5, 7):
        inp, out = _launch(ccx_ctx, V, rules, cases, emb, sample=1, temperature=temperature, seed=seed)
        refs = _reference(V, rules, cases, inp, emb, temperature=temperature, seed=seed)
        worst = 0.0
        for b, c in enumerate(cases):
            got_tok = out["gen"][b][len(c.sampled)]
            draws += 1
            close += refs[b].margin <= eps
            if got_tok != refs[b].token:
                assert 0 <= got_tok < V
                worst = max(worst, float(refs[b].scores[refs[b].token] - refs[b].scores[got_tok]))
                continue
            _check_row(b, c, inp, out, refs[b], (temperature, seed, c.name))
        within(N_SAMPLING, worst, eps, (temperature, seed))        # a disagreeing draw lies within eps of the reference's maximum
        if seed == 99:
            # the noise of a row depends on its batch row, not on how the batch is cut into launches
            cut = 10
            _, lo = _launch(ccx_ctx, V, rules, cases[:cut], emb, sample=1, temperature=temperature, seed=seed, row0=0)
            _, hi = _launch(ccx_ctx, V, rules, cases[cut:], emb, sample=1, temperature=temperature, seed=seed, row0=cut)
            assert lo["gen"] + hi["gen"] == out["gen"] and lo["state"] + hi["state"] == out["state"]
            x_in = inp["x"]
            # (the launches fill x from the same sentinel rows 0.., so only rows that moved on are comparable)
            for b in range(len(cases)):
                part, i = (lo, b) if b < cut else (hi, b - cut)
                if not torch.equal(out["x"][b], x_in[b]):
                    assert torch.equal(part["x"][i], out["x"][b]), b
    assert close <= 0.02 * draws, (close, draws)


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections: one per host check
# ---------------------------------------------------------------------------------------------------------------------------------
def _bump(p):
    return p + 4


def _poke_prompt(p):
    p[1] = 60000                    # row 0's second prompt token
    return p


SELECT_REJECTIONS = [
    ("no rows", {"B": 0}, None, "B = 0"),
    ("n_vocab no multiple of 4", {"n_vocab": 51862}, None, "multiple of 4"),
    ("n_vocab beyond 13 groups", {"n_vocab": 53252, "ld": 53376}, None, "<= 53248"),
    ("ld below n_vocab", {"ld": 51860}, None, "ld = 51860"),
    ("logits_elems short", {"logits_elems": 51968 + 51863}, None, "logits are read"),
    ("logits misaligned", {"logits": _bump}, None, "logits null or not 16-byte"),
    ("eot out of range", {"rules.eot": 51864}, None, "ccx_dec_select_step: rules.eot = 51864"),
    ("blank out of range", {"rules.blank": 51864}, None, "ccx_dec_select_step: rules.blank = 51864"),
    ("timestamp_begin behind the vocabulary", {"rules.timestamp_begin": 51865}, None, "rules.timestamp_begin = 51865"),
    ("suppress id out of range", {"rules.n_suppress": 1, "rules.suppress": "big"}, None, "ccx_dec_select_step: rules.suppress[0] = 51864"),
    ("negative no_speech", {"rules.no_speech": -1}, None, "no_speech"),
    ("n_gen beyond sample_len", {}, (0, ("n_gen", 7)), "n_gen = 7"),
    ("a live row with a full gen table", {}, (0, ("n_gen", 6)), "leaves no room"),
    ("pos + 1 behind pos_emb", {}, (0, ("pos", 447)), "pos = 447"),
    ("negative pos", {}, (0, ("pos", -1)), "pos = -1"),
    ("prompt_len beyond max_prompt", {}, (0, ("prompt_len", 5)), "prompt_len = 5"),
    ("done neither 0 nor 1", {}, (1, ("done", 2)), "done = 2"),
    ("tok_emb_elems short", {"tok_emb_elems": 51864 * 64 - 1}, None, "tok_emb is read"),
    ("x_elems short", {"x_elems": 2 * 64 - 1}, None, "x is written"),
    ("D no multiple of 4", {"D": 62}, None, "D = 62"),
    ("temperature without the sampling kernel", {"temperature": 0.5}, None, "needs sample = 1"),
    ("sample_len zero", {"sample_len": 0}, None, "sample_len = 0"),
    ("gen null", {"gen": None}, None, "is NULL"),
    ("prompt null", {"prompt": None}, None, "prompt is NULL"),
    ("negative max_prompt", {"max_prompt": -1}, None, "max_prompt = -1"),
    ("tok_emb null", {"tok_emb": None}, None, "tok_emb, pos_emb or x null"),
    ("pos_emb misaligned", {"pos_emb": _bump}, None, "tok_emb, pos_emb or x null or not 16-byte"),
    ("x misaligned", {"x": _bump}, None, "tok_emb, pos_emb or x null or not 16-byte"),
    ("sample neither 0 nor 1", {"sample": 2}, None, "sample = 2"),
    ("negative temperature", {"sample": 1, "temperature": -0.5}, None, "temperature or row0 negative"),
    ("negative row0", {"row0": -1}, None, "temperature or row0 negative"),
    ("a prompt token out of range", {"prompt": _poke_prompt}, (0, ("prompt_len", 3)), "prompt[0][1] = 60000"),
    ("last_tok behind the vocabulary", {}, (0, ("last_tok", 51864)), "token id >= n_vocab"),
    ("pen_tok behind the vocabulary", {}, (0, ("pen_tok", 51864)), "token id >= n_vocab"),
    ("last_ts_tok behind the vocabulary", {}, (0, ("last_ts_tok", 51864)), "token id >= n_vocab"),
]


@pytest.mark.parametrize("name,override,state_change,fragment", SELECT_REJECTIONS, ids=[r[0] for r in SELECT_REJECTIONS])
def test_rejections(ccx_ctx, embeddings, name, override, state_change, fragment):
    from clearconverse_amd import _lib
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.select_cases(V, rules)[:2]
    override = dict(override)
    if override.get("rules.suppress") == "big":
        big = (C.c_int * 1)(V)
        override["rules.suppress"] = big
    so = None if state_change is None else {state_change[0]: state_change[1]}
    with pytest.raises(_lib.CcxError) as e:
        _launch(ccx_ctx, V, rules, cases, embeddings(V), override=override, state_override=so)
    assert fragment in str(e.value) and "(1)" in str(e.value), str(e.value)
