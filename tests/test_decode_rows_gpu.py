"""GPU: WhisperModel.decode_rows (ccx_whisper_decode_rows) -- decode rows over a row -> window map.

The control is always a plain `decode` of windows laid out PHYSICALLY in map order: the mel rows gathered by the map go in through
`set_mel`, are encoded, and every row decodes "its own" window.  The two runs differ only in addresses, so tokens, sum_logprob and
no_speech_prob must be bit-equal -- on each of the three cross-attention paths, with lanes, with the prompt prefill (16-row passes,
two-row and one-row tails), on a multilingual instance (no-speech probability read at the SOT position) and at small.en size, where
a mapped decode of <= 16 rows runs the two-launch query instead of the fused one (the control sets CCX_FUSE_CROSS_Q=0).
"""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict

pytestmark = pytest.mark.gpu

LENS_S = [6.0, 11.0, 30.0, 3.5, 17.0, 8.0, 24.0, 13.0]


def _mels(m, n):
    clips = [synthetic_clip(70 + i, 30.0)[: int(LENS_S[i % 8] * 16000)] for i in range(n)]
    ns = [len(c) for c in clips]
    host = np.zeros((n, max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return m.log_mel(torch.from_numpy(host).cuda(), ns, return_mel=True).clone()


def _prompts(rules, R, lens, seed=1, tail=None):
    """R prompts of the lengths lens[r % len(lens)]: [sot_prev, text ..., *tail] (length 1 on an English-only model: [sot])"""
    tail = list(tail) if tail is not None else [rules.sot]
    g = np.random.default_rng(seed)
    out = []
    for r in range(R):
        n = lens[r % len(lens)]
        out.append(list(tail) if n <= len(tail) else [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, n - 1 - len(tail))] + tail)
        assert len(out[-1]) == max(n, len(tail))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for r, (x, y) in enumerate(zip(a, b)):
        assert x["tokens"] == y["tokens"], (what, r, x["tokens"], y["tokens"])
        assert x["sum_logprob"] == y["sum_logprob"], (what, r, x["sum_logprob"], y["sum_logprob"])
        assert x["no_speech_prob"] == y["no_speech_prob"], (what, r, x["no_speech_prob"], y["no_speech_prob"])


def _mapped_and_control(m, mel, n_windows, win, prompts, sample_len, control_env=None, monkeypatch=None, **kw):
    m.set_mel(mel[:n_windows].contiguous())
    m.encode(n_windows)
    rows = m.decode_rows(prompts, win, sample_len=sample_len, n_windows=n_windows, **kw)
    path = m.last_cross_path
    m.set_mel(mel[torch.tensor(win, device=mel.device)].contiguous())
    m.encode(len(win))
    for k, v in (control_env or {}).items():
        monkeypatch.setenv(k, v)
    ctl = m.decode(prompts, sample_len=sample_len, **kw)
    for k in (control_env or {}):
        monkeypatch.delenv(k)
    assert m.last_cross_path == path
    return rows, ctl, path


@pytest.fixture(scope="module")
def model(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    m = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=40, ctx=ccx_ctx)
    mel = _mels(m, 8)
    yield m, mel
    m.close()


WIN7 = [2, 0, 2, 1, 0, 1, 1]
WIN18 = [4, 0, 2, 2, 1, 3, 0, 4, 4, 1, 2, 0, 3, 3, 1, 0, 2, 4]


def test_7_rows_over_3_windows_split_kv(model):
    m, mel = model
    prompts = _prompts(m.rules, 7, [1, 4, 18, 3, 6])              # prefill passes of 16 and 2 rows per sequence
    rows, ctl, path = _mapped_and_control(m, mel, 3, WIN7, prompts, 8)
    assert path == "kv16" and any(len(r["tokens"]) > 0 for r in rows)
    _same(rows, ctl, "7 over 3")
    rows, ctl, _ = _mapped_and_control(m, mel, 3, WIN7, prompts, 8, temperature=0.7, seed=21)     # NULL ids: the row is the stream
    _same(rows, ctl, "7 over 3, sampled")
    # rows of one window with one prompt are the same decode
    twins = m.rules.sot
    m.set_mel(mel[:3].contiguous()); m.encode(3)
    r = m.decode_rows([[twins]] * 4, [1, 1, 0, 1], sample_len=6, n_windows=3)
    assert r[0]["tokens"] == r[1]["tokens"] == r[3]["tokens"] and r[0]["sum_logprob"] == r[1]["sum_logprob"] == r[3]["sum_logprob"]


def test_18_rows_over_5_windows_streaming(model):
    m, mel = model
    prompts = _prompts(m.rules, 18, [1, 5, 17, 2, 9], seed=2)     # prefill passes of 16 rows and ONE row per sequence
    rows, ctl, path = _mapped_and_control(m, mel, 5, WIN18, prompts, 7)
    assert path == "kv_stream"
    _same(rows, ctl, "18 over 5")
    # a two-token maximum: the two-row prefill kernel; all one-token prompts: no prefill at all
    for lens in ([1, 2], [1]):
        rows, ctl, _ = _mapped_and_control(m, mel, 5, WIN18, _prompts(m.rules, 18, lens), 6)
        _same(rows, ctl, ("18 over 5", lens))


def test_6_rows_over_3_windows_x_stream(model, monkeypatch):
    m, mel = model
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
    prompts = _prompts(m.rules, 6, [3, 1, 6, 18], seed=3)
    rows, ctl, path = _mapped_and_control(m, mel, 3, [2, 0, 2, 1, 0, 0], prompts, 8)
    assert path == "xa_stream"
    _same(rows, ctl, "6 over 3, X-stream")
    for env in ({"CCX_DEC_LNFREE": "0"}, {"CCX_DEC_LNFREE": "0", "CCX_XS_FUSE_Q": "0"}):      # the other two query forms of the path
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rows, ctl, _ = _mapped_and_control(m, mel, 3, [2, 0, 2, 1, 0, 0], prompts, 6)
        _same(rows, ctl, ("6 over 3, X-stream", env))
        for k in env:
            monkeypatch.delenv(k)


def test_40_rows_over_8_windows_two_lanes(model, monkeypatch):
    m, mel = model
    monkeypatch.setenv("CCX_DEC_LANES", "2")                    # lanes of 32 and 8 rows: the map is offset by the lane's first row
    win = [(5 * r + 3) % 8 for r in range(40)]
    prompts = _prompts(m.rules, 40, [1, 4, 2, 3], seed=4)
    rows, ctl, path = _mapped_and_control(m, mel, 8, win, prompts, 10)
    assert path == "kv_stream"
    _same(rows, ctl, "40 over 8, 2 lanes")
    monkeypatch.setenv("CCX_DEC_LANES", "1")
    m.set_mel(mel[:8].contiguous()); m.encode(8)
    one = m.decode_rows(prompts, win, sample_len=10, n_windows=8)
    _same(one, rows, "1 lane against 2")


def test_graph_on_and_off_agree(model, monkeypatch):
    m, mel = model
    prompts = _prompts(m.rules, 18, [1, 5, 3], seed=5)
    m.set_mel(mel[:5].contiguous()); m.encode(5)
    ids = [3 * r + 1 for r in range(18)]
    on = m.decode_rows(prompts, WIN18, ids, sample_len=9, temperature=0.7, seed=5, n_windows=5)
    again = m.decode_rows(prompts, WIN18, ids, sample_len=9, temperature=0.7, seed=5, n_windows=5)      # replays the captured graph
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    off = m.decode_rows(prompts, WIN18, ids, sample_len=9, temperature=0.7, seed=5, n_windows=5)
    monkeypatch.delenv("CCX_NO_GRAPH")
    _same(on, off, "graph on / off")
    _same(on, again, "graph replay")
    # the ids are part of the draw: other ids, other tokens somewhere
    other = m.decode_rows(prompts, WIN18, None, sample_len=9, temperature=0.7, seed=5, n_windows=5)
    assert [r["tokens"] for r in other] != [r["tokens"] for r in on]


@pytest.mark.parametrize("B", [5, 18])
def test_identity_map_with_null_ids_equals_decode(model, B):
    m, mel = model
    big = mel[torch.arange(B, device=mel.device) % 8].contiguous()
    m.set_mel(big); m.encode(B)
    prompts = _prompts(m.rules, B, [1, 4, 17], seed=6)
    for kw in (dict(), dict(temperature=0.7, seed=8)):
        plain = m.decode(prompts, sample_len=8, **kw)
        mapped = m.decode_rows(prompts, list(range(B)), sample_len=8, n_windows=B, **kw)
        after = m.decode(prompts, sample_len=8, **kw)       # a captured step graph of the mapped decode is not replayed for a plain one
        _same(mapped, plain, ("identity", B, kw))
        _same(after, plain, ("plain after mapped", B, kw))


@pytest.mark.parametrize("n_all,subset", [(5, [1, 4]), (24, [1, 4] + list(range(6, 22)))], ids=["split-KV", "streaming"])
def test_a_subset_draws_what_it_draws_among_all(model, n_all, subset):
    """temperature 0.7: rows for a subset of the windows, under those windows' stream ids, equal the same windows' rows in the decode
    of all of them (both sizes on one cross-attention path)"""
    m, mel = model
    big = mel[torch.arange(n_all, device=mel.device) % 8].contiguous()
    m.set_mel(big); m.encode(n_all)
    prompts = _prompts(m.rules, n_all, [1, 3, 5], seed=7)
    every = m.decode(prompts, sample_len=8, temperature=0.7, seed=31)
    path = m.last_cross_path
    some = m.decode_rows([prompts[w] for w in subset], subset, subset, sample_len=8, temperature=0.7, seed=31, n_windows=n_all)
    assert m.last_cross_path == path
    _same(some, [every[w] for w in subset], ("subset", subset))
    assert len({tuple(r["tokens"]) for r in every}) > 1


def test_rejections(model):
    from clearconverse_amd import _lib
    m, mel = model
    m.set_mel(mel[:3].contiguous()); m.encode(3)
    sot = [[m.rules.sot]]
    for win, frag in (([0, 3], "window_of_row[1] = 3"), ([-1, 0], "window_of_row[0] = -1")):
        with pytest.raises(_lib.CcxError) as e:
            m.decode_rows(sot * 2, win, sample_len=4, n_windows=3)
        assert frag in str(e.value) and "(1)" in str(e.value), str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        m.decode_rows(sot * 41, [0] * 41, sample_len=4, n_windows=3)
    assert "R = 41" in str(e.value) and "(1)" in str(e.value), str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        m.decode_rows(sot * 2, [0, 1], sample_len=4, n_windows=41)
    assert "n_windows = 41" in str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        m.decode_rows(sot * 2, [0, 1], sample_len=4, n_windows=4)           # more windows than the last encode left
    assert "n_windows = 4" in str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        m.decode_rows(sot * 2, [0, 1], [0, -5], sample_len=4, n_windows=3)
    assert "stream_ids[1] = -5" in str(e.value)
    with pytest.raises(_lib.CcxError):
        m.decode_rows(sot * 2, [0, 1], sample_len=4, n_windows=3, temperature=-1.0)
    assert len(m.decode_rows(sot * 2, [0, 1], sample_len=4, n_windows=3)) == 2          # the instance is fine afterwards


def test_multilingual_no_speech_at_the_sot_position(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128, n_vocab=51865)
    m = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=20, ctx=ccx_ctx)
    try:
        m.set_sot_tail(2)
        assert m.rules.is_multilingual
        mel = _mels(m, 4)
        tail = m.rules.sot_sequence("de", "transcribe")
        for R, win in ((6, [3, 0, 3, 1, 0, 2]), (18, [(3 * r + 1) % 4 for r in range(18)])):
            prompts = _prompts(m.rules, R, [3, 7, 19, 5], seed=9, tail=tail)      # 19: the SOT row and the last row in different passes
            rows, ctl, _ = _mapped_and_control(m, mel, 4, win, prompts, 6)
            _same(rows, ctl, ("multilingual", R))
            assert len({r["no_speech_prob"] for r in rows}) > 1
    finally:
        m.close()


def test_small_en_size_bypasses_the_fused_query(ccx_ctx, monkeypatch):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.small_en()
    m = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=0), max_batch=5, ctx=ccx_ctx)
    try:
        mel = _mels(m, 2)
        prompts = _prompts(m.rules, 5, [1, 4, 3], seed=10)
        rows, ctl, path = _mapped_and_control(m, mel, 2, [1, 0, 1, 1, 0], prompts, 4, control_env={"CCX_FUSE_CROSS_Q": "0"}, monkeypatch=monkeypatch)
        assert path == "kv16"
        _same(rows, ctl, "small.en, 5 over 2")
    finally:
        m.close()
