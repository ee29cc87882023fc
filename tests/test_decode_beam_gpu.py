"""GPU: WhisperModel.decode_beam (ccx_whisper_decode_beam) on the mini model -- beam search through the whole decode: prefill, eager first
step, step graphs, the beam head (csrc/dec_beam.hip) and the self attention through the cache indirection.

 (a) beam_size 1 is greedy: tokens equal `decode` exactly and sum_logprob bit for bit (the top-k kernel forms the log-probability as the
     select kernel does and the update kernel adds it to the row's sum in fp32, as the select kernel does).
 (b) with trace=True the reference walk (tests/beam_reference.py) fed the device's own proposals reproduces every step's survivors,
     parents, scores and finished lists, and the returned hypotheses, exactly.
 (c) every returned hypothesis is teacher-forced through oracle/whisper_ref on the GPU's encoder output: the filtered log-softmax sum
     matches the reported sum_logprob under the bound the greedy tests allow a decode (tests/test_whisper_gpu.py: 1.5e-3 relative to
     max(1, |oracle|), which is n_tokens x their per-token allowance).  A hypothesis that read another row's cache is far outside it.
 (d) graph replay equals eager (CCX_NO_GRAPH) bit for bit.   (e) a window decoded in a group equals the same window decoded alone.
 (f) on kv16, kv_stream and xa_stream, with prompts of 1, 2 and 18 tokens.   (g) 1280 wide.   (h) patience.   (i) rejections.
"""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import beam_reference as BR
from tests.conftest import within

pytestmark = pytest.mark.gpu

LENS_S = [6.0, 11.0, 30.0, 3.5]
N_ORACLE = "decode beam: |sum_logprob - oracle (teacher forced)| / max(1, |oracle|)"
TOL_ORACLE = 1.5e-3


def _encode(m, n):
    clips = [synthetic_clip(70 + i, 30.0)[: int(LENS_S[i % 4] * 16000)] for i in range(n)]
    ns = [len(c) for c in clips]
    host = np.zeros((n, max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    m.log_mel(torch.from_numpy(host).cuda(), ns)
    return m.encode(n, return_xa=True).cpu()


def _prompt(rules, n, seed):
    g = np.random.default_rng(seed)
    return [rules.sot] if n <= 1 else [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, n - 2)] + [rules.sot]


@pytest.fixture(scope="module")
def model(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    xa = _encode(m, 3)
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    yield m, xa, orc
    m.close()


def _replay(res, tr, beam, patience, sample_len, eot):
    """(b): the reference walk over the device's own proposals, window by window.  Returns per window (finished count, hypotheses)."""
    mc = BR.max_candidates(beam, patience)
    f32 = np.float32
    out = []
    for g, hyps in enumerate(res):
        r0 = g * beam
        win = BR.Window([BR.Row([], f32(0.0)) for _ in range(beam)])
        for s in range(sample_len):
            if tr["tok"][s, r0] < 0:
                assert (tr["tok"][s:, r0:r0 + beam] == -1).all(), (g, s)      # a frozen window stays frozen
                break
            cands = []
            for j in range(beam):
                for k in range(beam + 1):
                    i = int(tr["cand_id"][s, r0 + j, k])
                    if i >= 0:
                        cands.append((f32(win.rows[j].sum_logprob) + f32(tr["cand_lp"][s, r0 + j, k]), j, i))    # fp32, as the kernel adds
                if s == 0 and j > 0:
                    assert (tr["cand_id"][s, r0 + j] == -1).all(), (g, j)      # the first step: row 0 alone proposes
            assert not win.complete
            rec = BR.apply_walk(win, cands, beam, mc, eot, sample_len)
            assert [int(t) for t in tr["tok"][s, r0:r0 + beam]] == rec["tokens"], (g, s)
            assert [int(p) - r0 for p in tr["parent"][s, r0:r0 + beam]] == rec["parents"], (g, s)
            assert [f32(x) for x in tr["score"][s, r0:r0 + beam]] == [f32(x) for x in rec["scores"]], (g, s)
        assert win.complete
        want = BR.finalize(win, beam)
        assert [(h["tokens"], f32(h["sum_logprob"])) for h in hyps] == [(t, f32(sc)) for t, sc in want], (g, hyps, want)
        out.append((len(win.finished), want))
    return out


def _teacher_force(m, orc, xa, prompts, windows, res, replay, sample_len, what):
    """(c): finished hypotheses carry their eot's log-probability, live rows that topped the list up do not"""
    rules = m.rules
    orules = R.Rules(suppress=tuple(rules.suppress))
    for g, hyps in enumerate(res):
        n_fin = replay[g][0]
        w = windows[g] if windows is not None else g
        for k, h in enumerate(hyps):
            forced = h["tokens"] + ([rules.eot] if k < n_fin else [])
            o = R.greedy_decode(orc, xa[w:w + 1], [prompts[g]], orules, sample_len=sample_len + 1, forced=[forced])[0]
            within(N_ORACLE, abs(o.sum_logprob - h["sum_logprob"]) / max(1.0, abs(o.sum_logprob)), TOL_ORACLE, (what, g, k))
            if k == 0:
                assert abs(o.no_speech_prob - h["no_speech_prob"]) <= 1e-6 + 1e-3 * o.no_speech_prob


def test_beam_1_is_greedy(model):
    m, xa, orc = model
    prompts = [_prompt(m.rules, n, 5 + n) for n in (1, 4, 18)]
    greedy = m.decode(prompts, sample_len=10)
    beam = m.decode_beam(prompts, 1, sample_len=10)
    for g, (a, hyps) in enumerate(zip(greedy, beam)):
        assert len(hyps) == 1 and hyps[0]["tokens"] == a["tokens"], (g, hyps, a)
        assert hyps[0]["sum_logprob"] == a["sum_logprob"], (g, hyps[0]["sum_logprob"], a["sum_logprob"])
        assert hyps[0]["no_speech_prob"] == a["no_speech_prob"]
    assert any(len(a["tokens"]) > 0 for a in greedy)


@pytest.mark.parametrize("beam,patience,sample_len", [(5, None, 8), (2, 2.0, 10), (3, 0.5, 6)])
def test_trace_replay_and_oracle(model, beam, patience, sample_len):
    m, xa, orc = model
    prompts = [_prompt(m.rules, n, 9 + n) for n in (1, 2, 18)]              # one-token (no prefill row), two-row and 16 + 2-row prefill passes
    res, tr = m.decode_beam(prompts, beam, patience=patience, sample_len=sample_len, trace=True)
    assert m.last_cross_path == "kv16"
    replay = _replay(res, tr, beam, patience, sample_len, m.rules.eot)
    mc = BR.max_candidates(beam, patience)
    for hyps in res:
        assert beam <= len(hyps) <= max(beam, mc)
    assert any(int(p) != r for s in range(1, sample_len) for r, p in enumerate(tr["parent"][s]) if p >= 0)     # hypotheses did move rows
    _teacher_force(m, orc, xa, prompts, None, res, replay, sample_len, ("kv16", beam, patience))
    # the untraced decode (step graphs) returns the same hypotheses, bit for bit
    again = m.decode_beam(prompts, beam, patience=patience, sample_len=sample_len)
    assert again == res


def test_graph_replay_equals_eager(model, monkeypatch):
    m, xa, orc = model
    prompts = [_prompt(m.rules, n, 3 + n) for n in (3, 1, 6)]
    a = m.decode_beam(prompts, 4, sample_len=9)
    b = m.decode_beam(prompts, 4, sample_len=9)            # replays the captured step graph
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    c = m.decode_beam(prompts, 4, sample_len=9)
    assert a == b == c and any(h["tokens"] for hyps in a for h in hyps)


def test_group_equals_alone(model):
    """15 rows over 3 windows against 5 rows on one window: both on the <= 16-row kernels, whose rows do not depend on the rows beside
    them (the precedent of tests/test_decode_rows_gpu.py's subsets) -- tokens and scores bit for bit"""
    m, xa, orc = model
    prompts = [_prompt(m.rules, n, 20 + n) for n in (2, 5, 1)]
    grp = m.decode_beam(prompts, 5, sample_len=8)
    for w in range(3):
        alone = m.decode_beam([prompts[w]], 5, sample_len=8, windows=[w], n_windows=3)
        assert alone[0] == grp[w], w


def test_streaming_paths(model, monkeypatch):
    m, xa, orc = model
    windows = [0, 1, 2, 1]
    prompts = [_prompt(m.rules, n, 30 + n) for n in (1, 2, 18, 7)]
    res, tr = m.decode_beam(prompts, 5, sample_len=7, windows=windows, n_windows=3, trace=True)      # 20 rows
    assert m.last_cross_path == "kv_stream"
    replay = _replay(res, tr, 5, None, 7, m.rules.eot)
    _teacher_force(m, orc, xa, prompts, windows, res, replay, 7, "kv_stream")
    assert m.decode_beam(prompts, 5, sample_len=7, windows=windows, n_windows=3) == res
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
    res, tr = m.decode_beam(prompts[:3], 2, sample_len=7, trace=True)
    assert m.last_cross_path == "xa_stream"
    replay = _replay(res, tr, 2, None, 7, m.rules.eot)
    _teacher_force(m, orc, xa, prompts[:3], None, res, replay, 7, "xa_stream")
    assert m.decode_beam(prompts[:3], 2, sample_len=7) == res


def test_patience_returns_up_to_twice_the_beam(model):
    m, xa, orc = model
    prompts = [_prompt(m.rules, 1, 0)] * 3
    res = m.decode_beam(prompts, 2, patience=2.0, sample_len=40)
    assert all(2 <= len(h) <= 4 for h in res)
    one = m.decode_beam(prompts, 2, sample_len=40)
    assert all(len(h) == 2 for h in one)
    # insertion order: finished hypotheses first, each list what the reference's ranker reads
    for hyps in res:
        assert BR.rank([(h["tokens"], h["sum_logprob"]) for h in hyps], m.rules.eot) in range(len(hyps))


def test_1280_wide(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=1280)
    sd = synthetic_whisper_state_dict(dims, seed=5)
    m = WhisperModel(dims, sd, max_batch=8, ctx=ccx_ctx)
    try:
        xa = _encode(m, 2)
        prompts = [_prompt(m.rules, n, 40 + n) for n in (1, 3)]
        res, tr = m.decode_beam(prompts, 3, sample_len=6, trace=True)
        replay = _replay(res, tr, 3, None, 6, m.rules.eot)
        orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
        _teacher_force(m, orc, xa, prompts, None, res, replay, 6, "1280 wide")
        assert m.decode_beam(prompts, 3, sample_len=6) == res
    finally:
        m.close()


@pytest.mark.parametrize("what,kw", [
    ("beam_size = 0", dict(beam_size=0)),
    ("beam_size = 9", dict(beam_size=9)),
    ("max_candidates = 18", dict(beam_size=8, patience=2.2)),
    ("G * beam_size", dict(beam_size=8, n_prompts=6)),
    ("window_of_group[1] = 3", dict(beam_size=2, windows=[0, 3, 1], n_windows=3)),
    ("n_windows = 4", dict(beam_size=2, windows=[0, 1, 2], n_windows=4)),
    ("CCX_PREFILL=0", dict(beam_size=2, env=("CCX_PREFILL", "0"))),
])
def test_rejections(model, monkeypatch, what, kw):
    from clearconverse_amd import _lib
    m, xa, orc = model
    kw = dict(kw)
    env = kw.pop("env", None)
    if env:
        monkeypatch.setenv(*env)
    prompts = [_prompt(m.rules, 3, 1)] * kw.pop("n_prompts", 3)
    with pytest.raises(_lib.CcxError) as e:
        m.decode_beam(prompts, kw.pop("beam_size"), sample_len=6, **kw)
    assert "ccx_whisper_decode_beam" in str(e.value) and what in str(e.value), str(e.value)
