"""GPU: sequence_bias, bad_words_ids and hotwords through the model handle (ccx_whisper_set_bias_options; csrc/dec_bias.hip in
dec_head), at the mini dims and on the PATHS of tests/test_decode_history_gpu.py, against oracle/whisper_ref.WhisperRef under the
rule of tests/bias_reference.py, then the history rules, then the filters of tests/decoding_options_reference.py.

On the two K / V paths and on the X-stream path: greedy decodes of 24 tokens under the two walk tables (bias_reference.walk_tables,
built from the oracle's own free walks: `ban`, bad words only; `boost`, finite biases with a length-1 entry), with the default prompt
and with without_timestamps, each teacher-forced through the oracle by the eps-argmax walk (eps 0.02).  The walk does not pass
vacuously: tests/test_bias_reference_cpu.py walks the same decodes by the oracle alone and finds at least half of the steps decisive
and at least 3 steps changed by each table; here a walk must hold 0.8 of that decisive count, and where the oracle's walk on the
GPU's encoder output changes at least 3 steps the model's tokens differ from its default decode.

sum_logprob and no_speech_prob: inside the bounds of tests/test_decode_options_gpu.py (1.5e-3 relative, 1e-6 + 1e-3 p), recorded
under names of their own and held to tighter figures -- at most 2.5 x the worst an MI355X run of this file recorded (DESIGN.md
section 3): sum_logprob 8.12e-4 relative -> 2.03e-3, which lies above the outer bound, so 1.5e-3 is held; no_speech_prob 8.04e-9
absolute -> 2e-8.  no_speech_prob under `ban` (no length-1 entry) is bit-identical to the unbiased decode's; under `boost`
with the default prompt it is the softmax of the edited row (it differs from the unbiased one and follows the oracle); with
without_timestamps it is read at an earlier prompt position and stays bit-identical.

Exact, on every path: no banned sequence occurs in any row's tokens -- under greedy, under sampling through decode_rows with stream
ids, in beam size 2 (every hypothesis).  Then graph against eager bit for bit, a table changed between two graph decodes, default,
option and history decodes that keep their bits and graphs, bias and history together, stickiness, ccx_whisper_set_rules.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import bias_reference as BR
from tests import decoding_options_reference as DO
from tests import history_rules_reference as HR
from tests.conftest import within

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
ORULES = R.Rules(suppress=tuple(RULES.suppress))
EOT = RULES.eot
SL = BR.WALK_FREE_LEN
N_SLP = "decode bias: |sum_logprob - oracle (teacher forced)| / max(1, |oracle|)"
N_NSP = "decode bias: |no_speech_prob - oracle|"
TOL_SLP = 1.5e-3                  # measured 8.12e-4; 2.5 x it exceeds the 1.5e-3 of tests/test_decode_options_gpu.py, which is held
TOL_NSP = 2e-8                    # measured 8.04e-9 (there: 1e-6 + 1e-3 p, which stays the outer bound)
ROWS = 18                         # > 16: the lean streaming kernel on per-layer K / V
PATHS = [("kv16", 2, None), ("kv_stream", ROWS, None), ("xa_stream", 2, "1")]
TABLES = ("ban", "boost")


def _mels(seeds, seconds):
    clips = [synthetic_clip(s, 30.0)[: int(t * 16000)] for s, t in zip(seeds, seconds)]
    ns = [len(c) for c in clips]
    host = np.zeros((len(clips), max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return clips, ns, torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def model(ccx_ctx):
    """the instance with 18 windows encoded (the two clips, cyclic), the oracle, the GPU's encoder output of the two, per prompt the
    walk tables, and the free oracle walks of every case on the oracle's OWN encoder output (what the CPU test counts)"""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    m = WhisperModel(dims, sd, max_batch=20, ctx=ccx_ctx, decoding_options=True, repetition_control=True, contextual_bias=True)
    clips, ns, dev = _mels(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS)
    mel = m.log_mel(dev, ns, return_mel=True).clone()
    m.set_mel(mel[torch.arange(ROWS, device=mel.device) % 2].contiguous())
    xa = m.encode(ROWS, return_xa=True)[:2].cpu()
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    xa_ref = []
    for c in clips:
        ref_mel = R.pad_or_trim(R.log_mel_spectrogram(torch.from_numpy(c))[:, : len(c) // 160], 3000)
        xa_ref.append(orc.encode(ref_mel[None]))
    tables, free = {}, {}
    for name, (prompt, opts) in BR.walk_prompts(ORULES).items():
        plains = [BR.oracle_walk(orc, x, prompt, ORULES, opts, SL) for x in xa_ref]
        tables[name] = BR.walk_tables([p["tokens"] for p in plains], ORULES)
        for b in range(2):
            free[name, b, None] = plains[b]
            for t in TABLES:
                free[name, b, t] = BR.oracle_walk(orc, xa_ref[b], prompt, ORULES, opts, SL, tables[name][t])
    yield m, orc, xa, tables, free
    m.close()


def _as_arg(entries):
    """a table as the list form of sequence_bias (a -inf value is a bad word there too)"""
    return [[list(ids), b] for ids, b in entries]


def _decode(m, name, rows, entries, **kw):
    prompt, opts = BR.walk_prompts(ORULES)[name]
    m.set_sot_tail(len(prompt) - 1)
    try:
        dec = {"without_timestamps": True} if opts.without_timestamps else {}
        if entries:
            kw["sequence_bias"] = _as_arg(entries)
        return prompt, opts, m.decode([prompt] * rows, sample_len=SL, **dec, **kw)
    finally:
        m.set_sot_tail(0)


def _forced(r):
    return r["tokens"] + ([EOT] if len(r["tokens"]) < SL else [])


def _flat(res):
    return [(r["tokens"], r["sum_logprob"], r["no_speech_prob"]) for r in res]


_FREE = {}


def _free_on_gpu_xa(orc, xa, prompt, opts, name, b, table, T):
    """the oracle's free walk on the GPU's encoder output, computed once per case and shared by the three paths"""
    if (name, b, table) not in _FREE:
        _FREE[name, b, table] = BR.oracle_walk(orc, xa[b:b + 1], prompt, ORULES, opts, SL, T)
    return _FREE[name, b, table]


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("name", ["default", "without_timestamps"])
@pytest.mark.parametrize("path,rows,env", PATHS)
def test_bias_decodes_follow_the_oracle(model, monkeypatch, path, rows, env, name, table):
    m, orc, xa, tables, free = model
    if env is not None:
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", env)
    T = tables[name][table]
    prompt, opts, res = _decode(m, name, rows, T)
    assert m.last_cross_path == path
    _, _, plain = _decode(m, name, rows, None)
    for b in range(rows):                     # within one path a row's numbers do not depend on its batch mates
        assert res[b]["tokens"] == res[b % 2]["tokens"] and res[b]["sum_logprob"] == res[b % 2]["sum_logprob"], b
        assert not BR.banned_occurrences(res[b]["tokens"], BR.bad_words_of(T)), (b, res[b]["tokens"])
    has_len1 = any(len(ids) == 1 for ids, _ in T)
    for b in range(2):
        r = res[b]
        what = (path, name, table, b)
        w = BR.oracle_walk(orc, xa[b:b + 1], prompt, ORULES, opts, SL, T, forced=_forced(r))
        assert not w["violations"], (what, w["violations"])
        f = free[name, b, table]
        assert 2 * f["decisive"] >= f["steps"]                                        # what the CPU test asserts
        assert w["decisive"] >= 0.8 * f["decisive"], (what, w["decisive"], f["decisive"])
        within(N_SLP, abs(w["sum_logprob"] - r["sum_logprob"]) / max(1.0, abs(w["sum_logprob"])), TOL_SLP, what)
        within(N_NSP, abs(w["no_speech_prob"] - r["no_speech_prob"]), min(TOL_NSP, 1e-6 + 1e-3 * w["no_speech_prob"]), what)
        # no_speech_prob: the edited row exactly where a length-1 entry exists and the prompt ends in <|startoftranscript|>
        if has_len1 and name == "default":
            assert r["no_speech_prob"] != plain[b]["no_speech_prob"], what
            w0 = BR.oracle_walk(orc, xa[b:b + 1], prompt, ORULES, opts, 1)["no_speech_prob"]
            assert abs(r["no_speech_prob"] - w["no_speech_prob"]) < abs(r["no_speech_prob"] - w0), what     # the edited softmax, not the raw one
        else:
            assert r["no_speech_prob"] == plain[b]["no_speech_prob"], what             # bit-identical to the unbiased decode
        # where the oracle's own walk moves at least 3 steps under the table, the model's decode is not its default decode
        f0 = _free_on_gpu_xa(orc, xa, prompt, opts, name, b, None, ())
        fT = _free_on_gpu_xa(orc, xa, prompt, opts, name, b, table, T)
        if sum(x != y for x, y in zip(fT["tokens"], f0["tokens"])) >= 3:
            assert r["tokens"] != plain[b]["tokens"], what


def test_the_three_arguments_reach_the_kernel(model):
    """bad_words_ids and hotwords are the same table as their sequence_bias spelling"""
    m, orc, xa, tables, free = model
    prompt = [RULES.sot]
    T = tables["default"]["ban"]
    a = _flat(m.decode([prompt] * 2, sample_len=SL, sequence_bias=_as_arg(T)))
    b = _flat(m.decode([prompt] * 2, sample_len=SL, bad_words_ids=[list(ids) for ids, _ in T]))
    c = _flat(m.decode([prompt] * 2, sample_len=SL, sequence_bias={ids: v for ids, v in T}))
    base = _flat(m.decode([prompt] * 2, sample_len=SL))
    assert a == b == c and a != base
    # a hotword: the ids of the boosted phrase show up where the default decode has none of them
    word = [t for t in range(3000, 3100) if t not in RULES.suppress and all(t not in r[0] for r in base)][:2]
    text = m.tokenizer.decode(word)
    expanded = []                              # every prefix of the phrase as written and with a leading space, each once
    for enc in (m.tokenizer.encode(text), m.tokenizer.encode(" " + text)):
        for k in range(1, len(enc) + 1):
            if tuple(enc[:k]) not in [e[0] for e in expanded]:
                expanded.append((tuple(enc[:k]), 40.0))
    assert ((word[0],), 40.0) in expanded and (tuple(word), 40.0) in expanded
    hot = m.decode([prompt] * 2, sample_len=SL, hotwords=text, hotword_boost=40.0)
    same = m.decode([prompt] * 2, sample_len=SL, sequence_bias=_as_arg(expanded))
    assert _flat(hot) == _flat(same)
    for r in hot:
        assert word[0] in r["tokens"], r["tokens"]
    with pytest.raises(ValueError, match="hotword_boost"):
        m.decode([prompt] * 2, sample_len=SL, hotwords=text)
    assert _flat(m.decode([prompt] * 2, sample_len=SL)) == base                        # nothing outlives a call


def test_sampling_rows_never_emit_a_banned_sequence_and_keep_their_noise(model):
    m, orc, xa, tables, free = model
    prompt, _ = BR.walk_prompts(ORULES)["default"]
    kw0 = dict(sample_len=SL, temperature=0.7, seed=11, n_windows=2)
    off = m.decode_rows([prompt] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw0)
    # ban what the sampled rows themselves emit: their first bigrams that end in a text id
    words = []
    for r in off:
        for x, y in zip(r["tokens"], r["tokens"][1:]):
            if y < EOT and [x, y] not in words:
                words.append([x, y])
                break
    assert words and BR.banned_occurrences(off[0]["tokens"], words)
    kw = dict(kw0, bad_words_ids=words)
    a = m.decode_rows([prompt] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw)
    b = m.decode_rows([prompt] * 4, [0, 0, 1, 1], [0, 1, 2, 3], **kw)
    assert _flat(a) == _flat(b)                                                        # reproducible
    for r in a:
        assert not BR.banned_occurrences(r["tokens"], words), r["tokens"]
    sub = m.decode_rows([prompt] * 2, [0, 1], [1, 2], **kw)                            # a row does not depend on its batch mates
    assert _flat(sub) == _flat([a[1], a[2]])
    assert _flat(off) != _flat(a)


def test_beam_hypotheses_never_hold_a_banned_sequence(model):
    m, orc, xa, tables, free = model
    prompt, _ = BR.walk_prompts(ORULES)["default"]
    beam = 2
    ruled = m.decode_beam([prompt, prompt], beam, sample_len=SL, windows=[0, 1], n_windows=2)
    words = []
    for g in ruled:                                                                    # ban bigrams the unbiased hypotheses hold
        for h in g:
            for x, y in zip(h["tokens"], h["tokens"][1:]):
                if y < EOT and [x, y] not in words:
                    words.append([x, y])
                    break
    assert words
    hyps, tr = m.decode_beam([prompt, prompt], beam, sample_len=SL, windows=[0, 1], n_windows=2, trace=True, bad_words_ids=words)
    graph = m.decode_beam([prompt, prompt], beam, sample_len=SL, windows=[0, 1], n_windows=2, bad_words_ids=words)
    assert [[(h["tokens"], h["sum_logprob"]) for h in g] for g in graph] == [[(h["tokens"], h["sum_logprob"]) for h in g] for g in hyps]
    for g in range(2):
        assert len(hyps[g]) >= beam
        for h in hyps[g]:
            assert not BR.banned_occurrences(h["tokens"], words), (g, h["tokens"])
    assert [[h["tokens"] for h in g] for g in hyps] != [[h["tokens"] for h in g] for g in ruled]
    # the trace: no proposal of a row completes a banned bigram behind the hypothesis the row holds
    R_ = 2 * beam
    hist = [[] for _ in range(R_)]
    checked = 0
    for s in range(SL):
        for r in range(R_):
            ban = {w[1] for w in words if hist[r] and hist[r][-1] == w[0]}
            for c in tr["cand_id"][s, r]:
                if c >= 0 and ban:
                    assert int(c) not in ban, (s, r, int(c), hist[r])
                    checked += 1
        nxt = [list(h) for h in hist]
        for r in range(R_):
            if tr["tok"][s, r] >= 0:
                nxt[r] = hist[int(tr["parent"][s, r])] + [int(tr["tok"][s, r])]
        hist = nxt
    assert checked > 0


def test_graphs_tables_and_the_other_plans(model, monkeypatch):
    m, orc, xa, tables, free = model
    plain = [[RULES.sot], [RULES.sot_prev, 5000, RULES.sot]]
    T1, T2 = tables["default"]["ban"], tables["default"]["boost"]
    others = lambda: m.graph_count() - m.bias_graph_count()                # default, option and history plans
    before = _flat(m.decode(plain, sample_len=SL))
    opt = _flat(m.decode(plain, sample_len=SL, suppress_tokens=[5000, 5001]))
    hist = _flat(m.decode(plain, sample_len=SL, no_repeat_ngram_size=2))
    n0, n_opt, n_hist = others(), m.graph_count(True), m.history_graph_count()
    assert n0 >= 3 and n_opt >= 1 and n_hist >= 1
    nb0 = m.bias_graph_count()
    a = _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T1)))
    assert a != before
    nb = m.bias_graph_count()
    assert nb > nb0 and others() == n0
    # a table changed between two graph decodes takes effect, through the graphs that are there
    b = _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T2)))
    assert b != a and b != before and m.bias_graph_count() == nb
    assert _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T1))) == a and m.bias_graph_count() == nb
    # default, option and history decodes after bias decodes: the bits they had, the graphs they had
    assert _flat(m.decode(plain, sample_len=SL)) == before
    assert _flat(m.decode(plain, sample_len=SL, suppress_tokens=[5000, 5001])) == opt
    assert _flat(m.decode(plain, sample_len=SL, no_repeat_ngram_size=2)) == hist
    assert others() == n0 and m.graph_count(True) == n_opt and m.history_graph_count() == n_hist and m.bias_graph_count() == nb
    # bias and history set together: another plan beside them (it counts as both), the rule's order
    both = m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T2), repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert m.bias_graph_count() > nb and m.history_graph_count() > n_hist
    assert _flat(both) not in (a, b, hist)
    for r in both:
        assert not HR.ngram_invariant_violations(r["tokens"], EOT, 2) and not BR.banned_occurrences(r["tokens"], BR.bad_words_of(T2))
    w = BR.oracle_walk(orc, xa[0:1], plain[0], ORULES, DO.Options(), SL, T2, 1.3, 2, forced=_forced(both[0]))
    assert not w["violations"], w["violations"]
    # an empty table, set explicitly: the default plan, no graph more, the same bits
    total = m.graph_count()
    m.set_bias_options()
    assert _flat(m.decode(plain, sample_len=SL, sequence_bias=[], bad_words_ids=[])) == before
    assert m.graph_count() == total
    # graph against eager, bit for bit
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    assert _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T1))) == a
    assert _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T2))) == b
    assert _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T2), repetition_penalty=1.3, no_repeat_ngram_size=2)) == _flat(both)
    assert _flat(m.decode(plain, sample_len=SL)) == before
    monkeypatch.delenv("CCX_NO_GRAPH")
    # without the prompt prefill the rows walk their prompt step by step: rows in the prompt phase are not touched
    monkeypatch.setenv("CCX_PREFILL", "0")
    stepped = m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T1))
    for r in stepped:
        assert len(r["tokens"]) >= 4 and not BR.banned_occurrences(r["tokens"], BR.bad_words_of(T1)), r["tokens"]


def test_setting_is_sticky_checked_and_reset_by_set_rules(model):
    from clearconverse_amd import _lib
    m, orc, xa, tables, free = model
    plain = [[RULES.sot], [RULES.sot]]
    T = tables["default"]["ban"]
    before = _flat(m.decode(plain, sample_len=SL))
    m.set_bias_options(sequence_bias=_as_arg(T))
    try:
        sticky = _flat(m.decode(plain, sample_len=SL))
        assert sticky == _flat(m.decode(plain, sample_len=SL)) and sticky != before
    finally:
        m.reset_bias_options()
    assert _flat(m.decode(plain, sample_len=SL)) == before
    assert sticky == _flat(m.decode(plain, sample_len=SL, sequence_bias=_as_arg(T)))
    # the C check names the entry point and the field
    def refused(offsets, ids, bias, n=None):
        o_, i_, b_ = np.array(offsets, dtype=np.int32), np.array(ids, dtype=np.int32), np.array(bias, dtype=np.float32)
        o = _lib.DecodeBiasOptions(len(bias) if n is None else n, o_.ctypes.data_as(C.POINTER(C.c_int)), i_.ctypes.data_as(C.POINTER(C.c_int)),
                                   b_.ctypes.data_as(C.POINTER(C.c_float)))
        rc = m.lib.ccx_whisper_set_bias_options(m.handle, C.byref(o))
        assert rc == 1
        with pytest.raises(_lib.CcxError) as e:
            m.ctx.check(rc, "set")
        assert "ccx_whisper_set_bias_options" in str(e.value)
        return str(e.value)
    assert "opts.offsets[0]" in refused([1, 2], [5, 6], [1.0])
    assert "does not ascend" in refused([0, 2, 1], [5, 6], [1.0, 1.0])
    assert "has 0 ids" in refused([0, 0], [5], [1.0])
    assert "has 33 ids" in refused([0, 33], list(range(33)), [1.0])
    assert "opts.n_entries = 8193" in refused([0, 1], [5], [1.0], n=8193)
    assert "opts.ids[0] = 60000" in refused([0, 2], [60000, 6], [1.0])
    assert "opts.ids[1] = -1" in refused([0, 2], [5, -1], [1.0])
    assert f"must be < eot = {EOT}" in refused([0, 2], [5, EOT], [1.0])
    assert f"must be < eot = {EOT}" in refused([0, 1], [RULES.timestamp_begin], [-np.inf])
    assert "opts.bias[0] = inf" in refused([0, 1], [5], [np.inf])
    assert "opts.bias[0]" in refused([0, 1], [5], [np.nan])
    assert _flat(m.decode(plain, sample_len=SL)) == before                   # a refused setting changes nothing
    # the Python side refuses the same before anything reaches the library
    with pytest.raises(ValueError):
        m.decode(plain, sample_len=SL, bad_words_ids=[[EOT]])
    with pytest.raises(ValueError):
        m.decode(plain, sample_len=SL, sequence_bias={(5,): float("inf")})
    # ccx_whisper_set_rules resets the setting (and drops every graph: last in this module)
    m.set_bias_options(sequence_bias=_as_arg(T))
    m.set_rules(m.rules)
    assert _flat(m.decode(plain, sample_len=SL)) == before
    assert m.bias_graph_count() == 0
