"""GPU: what the step-graph key is for.  A captured step graph is replayed only by a decode whose steps launch exactly what it holds.

Every call of the list below has the SAME row count, sample_len and max_prompt, so the mode alone (sampling, row -> window map, stream
ids, beam size, max_candidates; the chain switches; the lane trace) has to tell the graphs of one instance apart.  The list runs
forwards and then backwards on one instance -- every second visit replays a cached graph -- and each result is compared bit for bit
(tokens, lengths, sum log-probabilities, no-speech probabilities) with the same call on a second instance of the same weights that
steps eagerly (CCX_NO_GRAPH=1).  A graph replayed for the wrong mode shows as a difference.

The 8 mel windows are computed once; an instance encodes max(8, rows) of them (cyclic) once, so that row r of a plain `decode` has a
window of its own, and the maps address the first 8.
"""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict

pytestmark = pytest.mark.gpu

LENS_S = [6.0, 11.0, 30.0, 3.5, 17.0, 8.0, 24.0, 13.0]
SAMPLE_LEN = 6
PROMPT_LENS = [1, 4, 3, 6, 2]          # max_prompt 6 in every call


def _prompt(rules, n, seed):
    g = np.random.default_rng(seed)
    return [rules.sot] if n <= 1 else [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, n - 2)] + [rules.sot]


def _prompts(rules, n):
    """n prompts; the first is the longest, so that every call's max_prompt is the same whatever n is"""
    lens = [max(PROMPT_LENS)] + [PROMPT_LENS[i % len(PROMPT_LENS)] for i in range(1, n)]
    return [_prompt(rules, k, 11 + i) for i, k in enumerate(lens)]


def _calls(rules, rows):
    """(name, call) of the list: every call decodes `rows` rows of SAMPLE_LEN tokens from prompts of at most 6 tokens"""
    assert rows in (8, 18)
    p = _prompts(rules, rows)
    mixed = [(5 * r + 3) % 8 for r in range(rows)]
    ids = [3 * r + 1 for r in range(rows)]
    (g2, b2), (g4, b4) = ((4, 2), (2, 4)) if rows == 8 else ((9, 2), (6, 3))

    def beam(G, bs, patience):
        win = [(3 * g + 1) % 8 for g in range(G)]
        return lambda m: m.decode_beam(p[:G], bs, patience=patience, sample_len=SAMPLE_LEN, windows=win, n_windows=8)

    return [
        ("greedy", lambda m: m.decode(p, sample_len=SAMPLE_LEN)),
        ("sampled", lambda m: m.decode(p, sample_len=SAMPLE_LEN, temperature=0.7, seed=3)),
        ("rows identity", lambda m: m.decode_rows(p, list(range(rows)), sample_len=SAMPLE_LEN, n_windows=rows)),
        ("rows mapped ids sampled", lambda m: m.decode_rows(p, mixed, ids, sample_len=SAMPLE_LEN, temperature=0.7, seed=3, n_windows=8)),
        (f"beam {b2} x {g2}", beam(g2, b2, None)),
        (f"beam {b4} x {g4}", beam(g4, b4, None)),
        (f"beam {b2} x {g2} patience 2", beam(g2, b2, 2.0)),      # max_candidates 4 instead of 2
    ]


def _flat(res):
    """rows of a decode, or hypotheses of a beam decode (window-major, with the hypothesis counts): the compared quantities"""
    if res and isinstance(res[0], list):
        return [len(h) for h in res], [(r["tokens"], len(r["tokens"]), r["sum_logprob"], r["no_speech_prob"]) for h in res for r in h]
    return None, [(r["tokens"], len(r["tokens"]), r["sum_logprob"], r["no_speech_prob"]) for r in res]


def _same(got, want, what):
    (gn, g), (wn, w) = _flat(got), _flat(want)
    assert gn == wn and len(g) == len(w), (what, gn, wn)
    for r, (x, y) in enumerate(zip(g, w)):
        assert x == y, (what, r, x, y)


@pytest.fixture(scope="module")
def weights():
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return dims, synthetic_whisper_state_dict(dims, seed=3)


@pytest.fixture(scope="module")
def mels(ccx_ctx, weights):
    from clearconverse_amd.whisper import WhisperModel
    m = WhisperModel(*weights, max_batch=20, ctx=ccx_ctx)
    clips = [synthetic_clip(70 + i, 30.0)[: int(LENS_S[i] * 16000)] for i in range(8)]
    ns = [len(c) for c in clips]
    host = np.zeros((8, max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    mel = m.log_mel(torch.from_numpy(host).cuda(), ns, return_mel=True).clone()
    m.close()
    return mel


def _pair(ccx_ctx, weights, mels, rows):
    """instance A (graphs) and the eager instance, each with its windows encoded once"""
    from clearconverse_amd.whisper import WhisperModel
    pair = []
    for _ in range(2):
        m = WhisperModel(*weights, max_batch=20, ctx=ccx_ctx)
        n = max(8, rows)
        m.set_mel(mels[torch.arange(n, device=mels.device) % 8].contiguous())
        m.encode(n)
        pair.append(m)
    return pair


def _eager(m, calls, monkeypatch):
    """the reference of every call, computed once"""
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    ref = {name: call(m) for name, call in calls}
    monkeypatch.delenv("CCX_NO_GRAPH")
    return ref


@pytest.mark.parametrize("rows,path", [(8, "kv16"), (18, "kv_stream")])
def test_mode_alone_tells_the_graphs_apart(ccx_ctx, weights, mels, monkeypatch, rows, path):
    a, e = _pair(ccx_ctx, weights, mels, rows)
    try:
        calls = _calls(a.rules, rows)
        ref = _eager(e, calls, monkeypatch)
        assert e.last_cross_path == path
        # the list is no list of one decode under seven names
        assert len({repr(_flat(r)) for r in ref.values()}) >= 5 and any(t[0] for t in _flat(ref["greedy"])[1])
        for visit, order in (("forwards", calls), ("backwards", calls[::-1])):
            for name, call in order:
                _same(call(a), ref[name], (rows, visit, name))
                assert a.last_cross_path == path
    finally:
        a.close(); e.close()


def test_chain_switches_between_visits_x_stream(ccx_ctx, weights, mels, monkeypatch):
    """8 rows on the X-stream path: the query form of the chain changes between visits of one instance"""
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
    a, e = _pair(ccx_ctx, weights, mels, 8)
    try:
        calls = _calls(a.rules, 8)
        envs = [{}, {"CCX_DEC_LNFREE": "0"}, {"CCX_DEC_LNFREE": "0", "CCX_XS_FUSE_Q": "0"}]
        refs = []
        for env in envs:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            refs.append(_eager(e, calls, monkeypatch))
            assert e.last_cross_path == "xa_stream"
            for k in env:
                monkeypatch.delenv(k)
        for visit, order in (("forwards", [0, 1, 2]), ("backwards", [2, 1, 0])):
            for i in order:
                for k, v in envs[i].items():
                    monkeypatch.setenv(k, v)
                for name, call in (calls if visit == "forwards" else calls[::-1]):
                    _same(call(a), refs[i][name], ("x-stream", visit, envs[i], name))
                    assert a.last_cross_path == "xa_stream"
                for k in envs[i]:
                    monkeypatch.delenv(k)
    finally:
        a.close(); e.close()


def test_lane_trace_on_and_off(ccx_ctx, weights, mels, monkeypatch, tmp_path):
    """the stamp nodes belong to the graphs captured while the trace is on, and to no other: a traced decode leaves as many stamps as
    the same decode stepping eagerly, whether or not an untraced graph of the same rows was captured before it, and an untraced
    decode appends nothing"""
    def stamps(path):
        return [int(ln.split()[2]) for ln in path.read_text().splitlines() if ln.startswith("lane 0 ")]

    a, e = _pair(ccx_ctx, weights, mels, 8)
    try:
        name, call = _calls(a.rules, 8)[0]
        path, epath = tmp_path / "stamps.txt", tmp_path / "stamps_eager.txt"
        e.trace_lanes(str(epath))
        ref = _eager(e, [(name, call)], monkeypatch)[name]
        e.trace_lanes(None)
        (n_eager,) = stamps(epath)
        assert epath.read_text().startswith("decode B 8 lanes 1\nlane 0 ") and n_eager > 0
        _same(call(a), ref, "before the trace")     # captures the untraced graph
        a.trace_lanes(str(path))
        _same(call(a), ref, "traced")
        a.trace_lanes(None)
        traced = path.read_text()
        assert stamps(path) == [n_eager]
        _same(call(a), ref, "after the trace")
        assert path.read_text() == traced
        a.trace_lanes(str(path))            # and the traced graph is still the traced one
        _same(call(a), ref, "traced again")
        a.trace_lanes(None)
        assert stamps(path) == [n_eager, n_eager]
    finally:
        a.close(); e.close()
