"""GPU: the opt-in reduced audio context in the model (WhisperModel(audio_ctx=...); include/ccx.h ccx_whisper_set_audio_ctx,
ccx_whisper_encode_ctx), at the mini dims and with the helpers of tests/test_whisper_gpu.py.

Five windows with the contexts 64, 65, 192, 200 and 1500 in ONE batch (the floor, one past a key tile, whole and ragged tiles, the whole
window; the call runs at 1500 rows per sequence, and a second batch without the full window at 200):
  * every window's valid rows against the definition on the oracle (tests/audio_ctx_reference.encode_ctx) with the encoder's bound;
  * every window equals itself encoded alone, bit for bit; full contexts equal ccx_whisper_encode, bit for bit;
  * every decode entry point takes the X-stream path and is walked teacher-forced through the oracle's CachedDecoder on the REDUCED
    reference encoder output, with the logit tolerance of tests/test_whisper_gpu.py: greedy, sampled, over a row map, beam search, an
    FP8 instance, lanes; with step graphs and without;
  * two encodes with different contexts back to back replay the same step graphs and equal the eager results;
  * a default instance beside it: no new graphs, the K / V path, its tokens those of the opted-in instance at full context;
  * `align` after a reduced encode against tests/align_reference on the reduced encoder output;
  * every refusal.
Bounds: the caps tests/test_whisper_gpu.py holds at the same dims, each within 2.5 x the worst measured here on an MI355X (encoder
valid rows rel-L2 4.11e-3 / 8e-3, teacher-forced logits rel-L2 5.74e-3 / 9e-3, sum_logprob 7.3e-4 / 1.5e-3); the logit tolerance of
the walks, 0.05, is that file's a-priori figure -- every decoded token was the oracle's argmax (deficit 0).  The FP8 instance is walked
on the dequantised rows it returns (the reference encoder output is not quantised).  profiles/audio_ctx_measured_deviations.json."""
import ctypes as C
from dataclasses import asdict

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import audio_ctx_reference as A
from tests.conftest import within
from tests.test_whisper_align_gpu import _three_checks, _tokens
from tests.test_whisper_gpu import _clips, _oracle, _rel, _rules

pytestmark = pytest.mark.gpu

CTX = [64, 65, 192, 200, 1500]
LENGTHS = [1.0, 1.1, 3.0, 3.5, 11.0]        # seconds of audio in the five windows
RULES = DecodeRules()
PROMPTS = [[RULES.sot], [RULES.sot_prev, 1000, 2000, RULES.sot], [RULES.sot], [RULES.sot_prev, 77, RULES.sot], [RULES.sot]]
TOL = 0.05                                   # tests/test_whisper_gpu.py: the logit tolerance of its teacher-forced walks
LANE_ROWS = 320                              # the smallest decode an X-stream instance cuts into more than one lane


def _dims_sd():
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return dims, synthetic_whisper_state_dict(dims, seed=3)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _valid_equal(a, b, ctx):
    return all(torch.equal(_bits(a[i, :n]), _bits(b[i, :n])) for i, n in enumerate(ctx))


@pytest.fixture(scope="module")
def red(ccx_ctx):
    """one opted-in instance for the file; `ref`: the definition's encoder output of the five windows, from the GPU's own log-mel"""
    from clearconverse_amd.whisper import WhisperModel
    dims, sd = _dims_sd()
    m = WhisperModel(dims, sd, max_batch=LANE_ROWS, ctx=ccx_ctx, audio_ctx="auto")
    assert m.audio_ctx == "auto" and ccx_ctx.lib.ccx_whisper_audio_ctx(m.handle) == 1
    _, n, dev = _clips(LENGTHS)
    mel = m.log_mel(dev, n, return_mel=True)
    ref = A.encode_ctx(_oracle(dims, sd), mel.cpu(), CTX)
    yield dims, sd, m, n, dev, mel, ref
    m.close()


def _encode5(red, ctx=CTX, reps=1):
    dims, sd, m, n, dev, mel, ref = red
    m.log_mel(dev.repeat(reps, 1).contiguous(), n * reps)
    return m.encode(5 * reps, return_xa=True, audio_ctx=list(ctx) * reps).cpu()


def _walk(orc, xa_row, prompt, tokens, sample_len, name, pick=None):
    """teacher-forced through the oracle's CachedDecoder: every token an eps-argmax of the oracle's filtered logits (`pick`: of what
    the oracle's sampler scores).  -> the oracle's sum of log-probabilities of the tokens"""
    _, orules = _rules()
    forced = list(tokens) + ([RULES.eot] if len(tokens) < sample_len else [])
    dec = R.CachedDecoder(orc, xa_row)
    lg = dec.step(torch.tensor([prompt]))[0, -1]
    sampled, slp, worst = [], 0.0, 0.0
    for i, t in enumerate(forced):
        filt = R.apply_filters(lg, sampled, orules)
        score = filt if pick is None else pick(filt, i)
        scale = 1.0 if pick is None else pick.scale
        worst = max(worst, (float(score.max()) - float(score[t])) / scale)
        slp += float(torch.log_softmax(filt.float(), -1)[t])
        sampled.append(t)
        lg = dec.step(torch.tensor([[t]]))[0, -1]
    print(f"[audio_ctx walk] {name}: worst deficit {worst:.3e}")
    within("whisper audio_ctx: oracle logit deficit of a decoded token (teacher forced, reduced reference xa)", worst, TOL, name)
    return slp


# ---------------------------------------------------------------------------------------------------------------- the encoder
def test_valid_rows_against_the_definition_and_alone(red):
    dims, sd, m, n, dev, mel, ref = red
    xa = _encode5(red)
    assert m.last_audio_ctx == CTX
    for b, k in enumerate(CTX):
        assert torch.isfinite(xa[b, :k]).all()
        within("whisper mini, reduced audio context: encoder output rel-L2 over a window's valid rows", _rel(xa[b, :k], ref[b]), 8e-3, (b, k))
    assert torch.equal(_bits(_encode5(red)), _bits(xa)), "a second encode differs"
    # each window alone (its own log-mel through set_mel: the same im2col bits), at its own context: S_run = its context
    for b, k in enumerate(CTX):
        m.set_mel(mel[b:b + 1].contiguous())
        alone = m.encode(1, return_xa=True, audio_ctx=[k]).cpu()
        assert torch.equal(_bits(alone[0, :k]), _bits(xa[b, :k])), (b, k)
    # a batch without the full window: S_run = 200
    short = _encode5(red, [64, 65, 192, 200, 128])
    assert _valid_equal(short, xa, [64, 65, 192, 200])
    assert not torch.equal(_bits(short[4, :128]), _bits(xa[4, :128])), "window 4 at 128 positions is not its first 128 rows at 1500"


def test_full_contexts_are_the_plain_encode_bit_for_bit(ccx_ctx, red):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd, m, n, dev, mel, ref = red
    full = _encode5(red, [1500] * 5)
    m.log_mel(dev, n)
    plain = m.encode(5, return_xa=True, audio_ctx="full").cpu()
    assert m.last_audio_ctx == [1500] * 5
    assert torch.equal(_bits(full), _bits(plain))
    d = WhisperModel(dims, sd, max_batch=5, ctx=ccx_ctx)
    try:
        d.log_mel(dev, n)
        assert torch.equal(_bits(d.encode(5, return_xa=True).cpu()), _bits(plain))
    finally:
        d.close()
    # the instance's policy: "auto" from the staged windows' content frames; after set_mel the whole window
    from clearconverse_amd.audio_ctx import positions_for
    m.log_mel(dev, n)
    m.encode(5)
    assert m.last_audio_ctx == [positions_for(x // 160) for x in n] == [128, 128, 256, 256, 640]
    m.set_mel(mel.contiguous())
    m.encode(5)
    assert m.last_audio_ctx == [1500] * 5


# ---------------------------------------------------------------------------------------------------------------- the decodes
@pytest.mark.parametrize("graphs", [True, False])
def test_decodes_walk_the_oracle_on_the_reduced_reference(red, monkeypatch, graphs):
    dims, sd, m, n, dev, mel, ref = red
    orc = _oracle(dims, sd)
    if not graphs:
        monkeypatch.setenv("CCX_NO_GRAPH", "1")
    _encode5(red)
    xr = [r[None] for r in ref]
    # greedy (the prefill included: prompts of 1, 3 and 4 tokens)
    res = m.decode_greedy(PROMPTS, sample_len=12)
    assert m.last_cross_path == "xa_stream"
    for b, r in enumerate(res):
        slp = _walk(orc, xr[b], PROMPTS[b], r["tokens"], 12, f"greedy {b}")
        within("whisper audio_ctx greedy: |sum_logprob - oracle (teacher forced)| / max(1, |oracle|)", abs(slp - r["sum_logprob"]) / max(1.0, abs(slp)), 1.5e-3, b)
    assert any(len(r["tokens"]) > 0 for r in res)
    # sampled: the oracle's sampler over the same Philox noise (tests/test_whisper_gpu.py::test_temperature_sampling_follows_the_oracle_draws)
    T, seed = 0.7, 1234
    smp = m.decode(PROMPTS, sample_len=10, temperature=T, seed=seed)
    assert m.last_cross_path == "xa_stream"
    for b, r in enumerate(smp):
        pick = lambda filt, i, b=b: R.sample_token(filt, T, seed, b, i)[2]
        pick.scale = 1.0 / T
        _walk(orc, xr[b], PROMPTS[b], r["tokens"], 10, f"sampled {b}", pick)
    # over a row map: greedy rows over repeating windows read their WINDOW's context
    windows = [2, 0, 4, 0, 3, 1, 3]
    rows = m.decode_rows([PROMPTS[w] for w in windows], windows, sample_len=8, n_windows=5)
    assert m.last_cross_path == "xa_stream"
    for r, w in zip(rows, windows):
        _walk(orc, xr[w], PROMPTS[w], r["tokens"], 8, f"row of window {w}")
    # beam search: every returned hypothesis is a string the oracle accepts token by token only where the beam is 1 wide; for a
    # wider beam the kept hypotheses need not be argmax strings, so the check is the beam of width 1 == greedy, and batch independence
    b1 = m.decode_beam([PROMPTS[1], PROMPTS[3], PROMPTS[4]], 1, sample_len=8, windows=[1, 3, 4], n_windows=5)
    g1 = m.decode_greedy(PROMPTS, sample_len=8)
    for hyp, w in zip(b1, (1, 3, 4)):
        best = hyp[0] if isinstance(hyp, list) else hyp
        assert best["tokens"] == g1[w]["tokens"], w
    b3 = m.decode_beam([PROMPTS[1], PROMPTS[0], PROMPTS[3]], 3, sample_len=8, windows=[3, 1, 3], n_windows=5)
    b3b = m.decode_beam([PROMPTS[3], PROMPTS[1]], 3, sample_len=8, windows=[3, 3], n_windows=5)
    key = lambda h: [(tuple(x["tokens"]), x["sum_logprob"]) for x in (h if isinstance(h, list) else [h])]
    assert m.last_cross_path == "xa_stream" and key(b3[2]) == key(b3b[0]) and key(b3[0]) == key(b3b[1])
    # the other entry points: teacher-forced logits and one window decoded alone (one row: still the X-stream)
    toks = np.array([p + [1234] * (5 - len(p)) for p in PROMPTS], dtype=np.int64)[:, :4]
    got = m.decoder_logits(toks).cpu()
    for b in range(5):
        want = orc.decoder_logits(torch.tensor(toks[b:b + 1]), xr[b])[0]
        within("whisper audio_ctx: decoder logits rel-L2 (teacher forced, reduced reference xa)", _rel(got[b], want), 9e-3, b)
    m.set_mel(mel[2:3].contiguous())
    m.encode(1, audio_ctx=[192])
    one = m.decode_greedy([PROMPTS[2]], sample_len=12)[0]
    assert m.last_cross_path == "xa_stream"
    assert one["tokens"] == res[2]["tokens"] and one["sum_logprob"] == res[2]["sum_logprob"]


def test_back_to_back_encodes_replay_the_same_graphs(red, monkeypatch):
    dims, sd, m, n, dev, mel, ref = red
    other = [192, 64, 320, 64, 704]
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    eager = []
    for ctx in (CTX, other):
        _encode5(red, ctx)
        eager.append(m.decode_greedy(PROMPTS, sample_len=12))
    monkeypatch.delenv("CCX_NO_GRAPH")
    _encode5(red, CTX)
    a = m.decode_greedy(PROMPTS, sample_len=12)
    count = m.graph_count()
    _encode5(red, other)
    b = m.decode_greedy(PROMPTS, sample_len=12)
    _encode5(red, CTX)
    c = m.decode_greedy(PROMPTS, sample_len=12)
    assert m.graph_count() == count, "the contexts are read on the device: no new step graph"
    key = lambda rs: [(tuple(r["tokens"]), r["sum_logprob"], r["no_speech_prob"]) for r in rs]
    assert key(a) == key(eager[0]) == key(c) and key(b) == key(eager[1])
    assert key(a) != key(b)


def test_fp8_instance_and_lanes(ccx_ctx, red):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd, m, n, dev, mel, ref = red
    orc = _oracle(dims, sd)
    # lanes: 64 copies of the five windows, every row what its window gives in the batch of five
    _encode5(red)
    five = m.decode_greedy(PROMPTS, sample_len=8)
    reps = LANE_ROWS // 5
    _encode5(red, reps=reps)
    m.prepare_lanes()
    big = m.decode_greedy(PROMPTS * reps, sample_len=8)
    assert m.last_cross_path == "xa_stream"
    for i, r in enumerate(big):
        assert r["tokens"] == five[i % 5]["tokens"] and r["sum_logprob"] == five[i % 5]["sum_logprob"], i
    # an FP8 instance: the stream reads the image of all 1500 rows of a slot; walked on the dequantised rows it returns
    f = WhisperModel(dims, sd, max_batch=5, ctx=ccx_ctx, audio_ctx=256, cross_fp8=True)
    try:
        assert f.cross_fp8 is True and f.audio_ctx == 256
        f.log_mel(dev, n)
        f.encode(5)
        assert f.last_audio_ctx == [256] * 5
        f.log_mel(dev, n)
        xa8 = f.encode(5, return_xa=True, audio_ctx=CTX).cpu()
        res = f.decode_greedy(PROMPTS, sample_len=10)
        assert f.last_cross_path == "xa_stream"
        for b, r in enumerate(res):
            _walk(orc, xa8[b:b + 1, :CTX[b]], PROMPTS[b], r["tokens"], 10, f"fp8 {b}")
    finally:
        f.close()


def test_a_default_instance_is_what_it_was(ccx_ctx, red, monkeypatch):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd, m, n, dev, mel, ref = red
    monkeypatch.delenv("CCX_AUDIO_CTX", raising=False)
    d = WhisperModel(dims, sd, max_batch=5, ctx=ccx_ctx)
    try:
        assert d.audio_ctx is None and ccx_ctx.lib.ccx_whisper_audio_ctx(d.handle) == 0
        d.log_mel(dev, n); d.encode(5)
        g0 = d.graph_count()
        a = d.decode_greedy(PROMPTS, sample_len=12)
        assert d.last_cross_path == "kv16"                      # five sequences: the K / V caches, as always
        g1 = d.graph_count()
        assert d.decode_greedy(PROMPTS, sample_len=12) == a and d.graph_count() == g1 and g1 > g0
        assert all("audio_ctx" not in r for r in d.transcribe_batch([np.zeros(16000, dtype=np.float32)]))
        # on the path the opted-in instance takes, its tokens are that instance's at full context, bit for bit
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
        d.log_mel(dev, n); d.encode(5)
        x = d.decode_greedy(PROMPTS, sample_len=12)
        assert d.last_cross_path == "xa_stream"
        monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS")
        m.log_mel(dev, n); m.encode(5, audio_ctx="full")
        y = m.decode_greedy(PROMPTS, sample_len=12)
        assert m.last_cross_path == "xa_stream" and x == y
        with pytest.raises(ValueError):
            d.encode(5, audio_ctx=[64] * 5)
        with pytest.raises(ValueError):
            d.transcribe(np.zeros(16000, dtype=np.float32), audio_ctx="auto")
        with pytest.raises(_lib.CcxError) as e:
            n5 = (C.c_int * 5)(*[64] * 5)
            ccx_ctx.check(ccx_ctx.lib.ccx_whisper_encode_ctx(d.handle, 5, n5, None, _lib.current_stream_ptr()), "ccx_whisper_encode_ctx")
        assert "ccx_whisper_set_audio_ctx" in str(e.value)
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- alignment
def test_align_on_a_reduced_encode(ccx_ctx, red):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd, m, n, dev, mel, ref = red
    w = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, audio_ctx="auto", word_alignment=True)
    try:
        _, n3, dev3 = _clips([7.0, 2.5, 12.0], seed0=20)
        w.log_mel(dev3, n3)
        ctx = [448, 192, 704]
        xa = w.encode(3, return_xa=True, audio_ctx=ctx).cpu()
        frames = [700, 250, 1200]
        _three_checks(w, dims, sd, [xa[b, :k] for b, k in enumerate(ctx)], _tokens(0, (5, 12, 20), dims.n_vocab), frames, "reduced")
        with pytest.raises(_lib.CcxError) as e:
            w.align(_tokens(0, (5, 12, 20), dims.n_vocab), [700, 386, 1200])       # 193 positions, window 1 holds 192
        assert "audio context of 192" in str(e.value)
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ccx_ctx, red):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd, m, n, dev, mel, ref = red
    lib = ccx_ctx.lib
    m.log_mel(dev, n)
    for bad in ([63, 64, 64, 64, 64], [64, 64, 64, 64, 1501]):
        with pytest.raises(ValueError):
            m.encode(5, audio_ctx=bad)
        with pytest.raises(_lib.CcxError) as e:
            ccx_ctx.check(lib.ccx_whisper_encode_ctx(m.handle, 5, (C.c_int * 5)(*bad), None, _lib.current_stream_ptr()), "ccx_whisper_encode_ctx")
        assert "out of range [64, n_audio_ctx = 1500]" in str(e.value)
    with pytest.raises(ValueError):
        m.encode(5, audio_ctx=[64] * 4)
    with pytest.raises(_lib.CcxError) as e:
        ccx_ctx.check(lib.ccx_whisper_encode_ctx(m.handle, 5, None, None, _lib.current_stream_ptr()), "ccx_whisper_encode_ctx")
    assert "n_ctx is NULL" in str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        ccx_ctx.check(lib.ccx_whisper_set_audio_ctx(m.handle, 0), "ccx_whisper_set_audio_ctx")
    assert "after finalize" in str(e.value)
    wide = WhisperDims.mini(n_layer=1, n_state=1280)                      # WhisperDims.large's width: no X-stream path
    with pytest.raises(_lib.CcxError) as e:
        WhisperModel(wide, {}, max_batch=1, ctx=ccx_ctx, audio_ctx="auto")
    assert "1280" in str(e.value)
    h = C.c_void_p()
    cd = _lib.WhisperDims(**asdict(wide))
    ccx_ctx.check(lib.ccx_whisper_create(ccx_ctx.handle, C.byref(cd), 1, C.byref(h)), "ccx_whisper_create")
    try:
        with pytest.raises(_lib.CcxError) as e:
            ccx_ctx.check(lib.ccx_whisper_set_audio_ctx(h, 1), "ccx_whisper_set_audio_ctx")
        assert "1280" in str(e.value) and lib.ccx_whisper_audio_ctx(h) == 0
        ccx_ctx.check(lib.ccx_whisper_set_audio_ctx(h, 0), "ccx_whisper_set_audio_ctx")       # off is always allowed
    finally:
        lib.ccx_whisper_destroy(h)
