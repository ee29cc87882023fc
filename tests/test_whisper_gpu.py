"""-m gpu: Whisper path through the C ABI vs oracle/whisper_ref.py (CPU fp32 restatement).

Tolerances (fp32 oracle vs bf16-MFMA / fp32-accumulate kernels):
  log-mel            abs 2e-3 (fp32 direct DFT vs torch.stft's FFT)
  encoder output     rel-L2 2e-2
  decoder logits     rel-L2 3e-2, and greedy choice must be an eps-argmax of the oracle's filtered logits
Token ids are compared exactly wherever the oracle's own top-1/top-2 margin exceeds the logit
tolerance; with seeded random weights margins are often below bf16 resolution, so a free-running
"identical ids" assertion would be a coin flip, not a parity check (Parity).
"""
import numpy as np
import pytest
import torch

from tests.conftest import within

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _oracle(dims, sd):
    return R.WhisperRef(R.Dims(**dims.__dict__), sd)


def _rules():
    r = DecodeRules()
    return r, R.Rules(suppress=tuple(r.suppress))


@pytest.fixture(scope="module")
def mini(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx)
    yield dims, sd, m
    m.close()


def _clips(lengths_s, seed0=0):
    clips = [synthetic_clip(seed0 + i, 30.0)[: int(s * 16000)] for i, s in enumerate(lengths_s)]
    n = [len(c) for c in clips]
    stride = max(n)
    host = np.zeros((len(clips), stride), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return clips, n, torch.from_numpy(host).cuda()


def test_logmel_matches_oracle(mini):
    dims, sd, m = mini
    clips, n, dev = _clips([30.0, 9.0, 0.7, 2.013])
    mel = m.log_mel(dev, n, return_mel=True).cpu()
    for b, c in enumerate(clips):
        full = R.log_mel_spectrogram(torch.from_numpy(c))
        content = len(c) // 160
        ref = R.pad_or_trim(full[:, : min(3000, content)], 3000)
        within("whisper: log-mel max abs error", float((mel[b] - ref).abs().max()), 1e-4, b)


def test_logmel_seek_window(mini):
    dims, sd, m = mini
    clips, n, dev = _clips([12.0])
    seek = 500
    mel = m.log_mel(dev, n, seek=[seek], return_mel=True).cpu()
    full = R.log_mel_spectrogram(torch.from_numpy(clips[0]))
    content = len(clips[0]) // 160
    ref = R.pad_or_trim(full[:, seek: seek + min(3000, content - seek)], 3000)
    assert float((mel[0] - ref).abs().max()) < 2e-3


def test_encoder_mini(mini):
    dims, sd, m = mini
    clips, n, dev = _clips([30.0, 5.0])
    mel = m.log_mel(dev, n, return_mel=True)
    xa = m.encode(2, return_xa=True).cpu()
    ref = _oracle(dims, sd).encode(mel.cpu())
    assert torch.isfinite(xa).all()
    within("whisper mini: encoder output rel-L2", _rel(xa, ref), 8e-3)


def test_set_mel_path_equals_logmel_path(mini):
    dims, sd, m = mini
    clips, n, dev = _clips([8.0])
    mel = m.log_mel(dev, n, return_mel=True)
    xa1 = m.encode(1, return_xa=True).clone()
    m.set_mel(mel.contiguous())
    xa2 = m.encode(1, return_xa=True)
    assert torch.equal(xa1, xa2)   # same im2col bits -> same kernels -> bit-identical


def test_decoder_logits_mini(mini):
    dims, sd, m = mini
    clips, n, dev = _clips([6.0, 11.0])
    mel = m.log_mel(dev, n, return_mel=True)
    xa = m.encode(2, return_xa=True)
    g = torch.Generator().manual_seed(0)
    toks = torch.randint(0, dims.n_vocab, (2, 9), generator=g)
    toks[:, 0] = 50257
    got = m.decoder_logits(toks.numpy()).cpu()
    ref = _oracle(dims, sd).decoder_logits(toks, xa.cpu())   # oracle decoder on the GPU's own xa: isolates the decoder
    within("whisper mini: decoder logits rel-L2 (teacher forced, 2 x 9 positions)", _rel(got, ref), 9e-3)
    # n_vocab % 16 == 8: the logits GEMM stores whole 16-column groups, so an in-place [B, T, V] store would overwrite the first
    # 8 logits of the next row (b + 1, t = 0) at t = T - 1 -- every (b, t) row is checked on its own
    for b in range(2):
        for t in range(9):
            within("whisper mini: decoder logits rel-L2 (per position)", _rel(got[b, t], ref[b, t]), 1e-2, (b, t))
    assert float((got[1, 0, :8] - ref[1, 0, :8]).abs().max()) < 0.05 * float(ref[1, 0].abs().max())
    # T == 1 (a single teacher-forced position)
    one = m.decoder_logits(toks[:, :1].numpy()).cpu()
    assert one.shape == (2, 1, dims.n_vocab) and _rel(one[:, 0], ref[:, 0]) < 3e-2


def test_set_rules_invalidates_captured_graphs(mini):
    """ccx_whisper_set_rules after a decode: the captured step graphs hold the old rule ids in their kernel parameters and must
    be dropped.  With eot moved to another id the finished flag follows the NEW id."""
    dims, sd, m = mini
    rules, _ = _rules()
    clips, n, dev = _clips([4.0])
    m.log_mel(dev, n); m.encode(1)
    a = m.decode_greedy([[rules.sot]], sample_len=6)[0]["tokens"]
    r2 = DecodeRules()
    r2.max_initial_timestamp_index = 3           # first token must now be a timestamp <= 0.06 s
    m.set_rules(r2)
    try:
        b = m.decode_greedy([[r2.sot_prev, 900, r2.sot]], sample_len=6)[0]["tokens"]     # prompt > 1: the first sampling step is a replayed step
        assert r2.timestamp_begin <= b[0] <= r2.timestamp_begin + 3, b
        c = m.decode_greedy([[r2.sot]], sample_len=6)[0]["tokens"]
        assert r2.timestamp_begin <= c[0] <= r2.timestamp_begin + 3, c
    finally:
        m.set_rules(rules)
    assert m.decode_greedy([[rules.sot]], sample_len=6)[0]["tokens"] == a


def _check_greedy(dims, sd, m, xa, prompts, sample_len, tol):
    rules, orules = _rules()
    res = m.decode_greedy(prompts, sample_len=sample_len)
    orc = _oracle(dims, sd)
    n_exact_required = 0
    for b, r in enumerate(res):
        toks = r["tokens"]
        forced = toks + ([rules.eot] if len(toks) < sample_len else [])
        o = R.greedy_decode(orc, xa[b:b + 1], [prompts[b]], orules, sample_len=sample_len, forced=[forced])[0]
        # re-walk: at every step the GPU token must be an eps-argmax of the oracle's filtered logits
        seq = list(prompts[b]); sampled = []
        for i, t in enumerate(forced):
            lg = R.apply_filters(orc.decoder_logits(torch.tensor([seq]), xa[b:b + 1])[0, -1], sampled, orules)
            best = float(lg.max())
            assert float(lg[t]) >= best - tol, (b, i, t, int(lg.argmax()), best - float(lg[t]))
            if o.margins[i] > 2 * tol:
                assert t == int(lg.argmax())
                n_exact_required += 1
            seq.append(t); sampled.append(t)
        within("whisper greedy: |sum_logprob - oracle (teacher forced)| / max(1, |oracle|)", abs(o.sum_logprob - r["sum_logprob"]) / max(1.0, abs(o.sum_logprob)), 1.5e-3)
        within("whisper greedy: |no_speech_prob - oracle|", abs(o.no_speech_prob - r["no_speech_prob"]), 1e-6 + 1e-3 * o.no_speech_prob)
    return res, n_exact_required


def _oracle_accepts(orc, xa_row, prompt, result, sample_len, tol):
    """every token of `result` is an eps-argmax of the oracle's filtered logits under teacher forcing"""
    rules, orules = _rules()
    toks = result["tokens"]
    forced = toks + ([rules.eot] if len(toks) < sample_len else [])
    seq, sampled = list(prompt), []
    for i, t in enumerate(forced):
        lg = R.apply_filters(orc.decoder_logits(torch.tensor([seq]), xa_row)[0, -1], sampled, orules)
        assert float(lg[t]) >= float(lg.max()) - tol, (i, t, int(lg.argmax()), float(lg.max()) - float(lg[t]))
        seq.append(t); sampled.append(t)


def _two_paths_agree(name, orc, xa_row, prompt, ra, rb, sample_len, tol, bound=9e-4):
    """The same window decoded by the two cross-attention formulations (split-KV kernels on K / V caches for decodes of <= 16
    sequences, one pass over the encoder output for larger ones): equal tokens and log-probabilities to `bound` relative -- or,
    where a near-tie tips the other way, both token strings must be eps-argmax strings of the oracle.  Returns 1 for a divergence."""
    if ra["tokens"] == rb["tokens"]:
        within(name, abs(ra["sum_logprob"] - rb["sum_logprob"]) / max(1.0, abs(rb["sum_logprob"])), bound)
        assert abs(ra["no_speech_prob"] - rb["no_speech_prob"]) <= 1e-4 + 2e-3 * rb["no_speech_prob"]
        return 0
    _oracle_accepts(orc, xa_row, prompt, ra, sample_len, tol)
    _oracle_accepts(orc, xa_row, prompt, rb, sample_len, tol)
    return 1


def _batch_mates(m, dims, sd, dev, n, prompts, reps, sample_len, monkeypatch, lanes=None):
    """4 windows decoded alone and as `reps` copies in one batch.  On ONE cross-attention path (CCX_CROSS_X_MIN_ROWS=1 puts the four
    on the path of the large batch) a sequence's tokens and log-probability must not depend on its batch mates, lanes or graph; the
    default small-batch path (split-KV kernels) must agree with it to rounding."""
    m.log_mel(dev, n); xa = m.encode(4, return_xa=True).cpu()
    a_small = m.decode_greedy(prompts, sample_len=sample_len)
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")          # by default decodes of <= 80 sequences take the K / V path
    a = m.decode_greedy(prompts, sample_len=sample_len)
    big = dev.repeat(reps, 1).contiguous()
    m.log_mel(big, n * reps); m.encode(4 * reps)
    if lanes:
        monkeypatch.setenv("CCX_DEC_LANES", str(lanes))
    b = m.decode_greedy(prompts * reps, sample_len=sample_len)
    monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS")
    if 4 * reps <= 80:
        # the default path of 17 .. 80 sequences: per-layer K / V through the lean streaming kernel (round 2's large-batch path)
        bd = m.decode_greedy(prompts * reps, sample_len=sample_len)
        for i in range(4 * reps):
            assert bd[i]["tokens"] == a_small[i % 4]["tokens"], i
            assert abs(bd[i]["sum_logprob"] - a_small[i % 4]["sum_logprob"]) < 1e-3, i
    for i in range(4 * reps):
        assert b[i]["tokens"] == a[i % 4]["tokens"], i
        assert abs(b[i]["sum_logprob"] - a[i % 4]["sum_logprob"]) < 1e-4, i
    orc = _oracle(dims, sd)
    div = sum(_two_paths_agree("whisper mini: |sum_logprob K/V-cache path - X-stream path| / max(1, |.|)", orc, xa[i:i + 1], prompts[i],
                               a_small[i], a[i], sample_len, 0.05) for i in range(4))
    assert div <= 1
    return a, b, xa


def test_greedy_mini(mini):
    dims, sd, m = mini
    rules, _ = _rules()
    clips, n, dev = _clips([6.0, 11.0, 3.0])
    m.log_mel(dev, n)
    xa = m.encode(3, return_xa=True).cpu()
    prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, 3000, rules.sot], [rules.sot_prev, 464, rules.sot]]
    res, n_req = _check_greedy(dims, sd, m, xa, prompts, sample_len=20, tol=0.05)
    for r in res:
        assert len(r["tokens"]) >= 1
        assert r["tokens"][0] >= rules.timestamp_begin      # first sampled token is a timestamp <= 1.0 s
        assert r["tokens"][0] <= rules.timestamp_begin + 50
    assert n_req > 0


def test_greedy_graph_equals_eager(mini, monkeypatch):
    dims, sd, m = mini
    rules, _ = _rules()
    clips, n, dev = _clips([4.0, 7.0])
    m.log_mel(dev, n)
    m.encode(2)
    prompts = [[rules.sot], [rules.sot_prev, 5000, rules.sot]]
    a = m.decode_greedy(prompts, sample_len=24)
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    b = m.decode_greedy(prompts, sample_len=24)
    assert [r["tokens"] for r in a] == [r["tokens"] for r in b]
    assert [r["sum_logprob"] for r in a] == [r["sum_logprob"] for r in b]


def test_temperature_sampling_follows_the_oracle_draws(mini):
    """the reference decodes at temperature 0.1 (back/api.py:128).  Both sides draw by Gumbel-max over the
    same Philox noise, so under teacher forcing every GPU token must be an eps-argmax of the oracle's perturbed
    scores logits / T + g, exactly equal where the oracle's perturbed margin exceeds 2 eps / T."""
    dims, sd, m = mini
    rules, orules = _rules()
    clips, n, dev = _clips([6.0, 11.0])
    m.log_mel(dev, n)
    xa = m.encode(2, return_xa=True).cpu()
    prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot]]
    orc = _oracle(dims, sd)
    tol = 0.05
    for T, seed in [(0.7, 1234), (0.1, 99)]:
        res = m.decode(prompts, sample_len=16, temperature=T, seed=seed)
        again = m.decode(prompts, sample_len=16, temperature=T, seed=seed)
        assert [r["tokens"] for r in res] == [r["tokens"] for r in again]            # reproducible
        n_exact = 0
        for b, r in enumerate(res):
            toks = r["tokens"]
            forced = toks + ([rules.eot] if len(toks) < 16 else [])
            seq = list(prompts[b]); sampled = []; slp = 0.0
            for i, t in enumerate(forced):
                lg = R.apply_filters(orc.decoder_logits(torch.tensor([seq]), xa[b:b + 1])[0, -1], sampled, orules)
                nxt, _, score = R.sample_token(lg, T, seed, b, i)
                top2 = torch.topk(score, 2).values
                assert float(score[t]) >= float(top2[0]) - tol / T, (T, b, i, t, nxt)
                if float(top2[0] - top2[1]) > 2 * tol / T:
                    assert t == nxt
                    n_exact += 1
                slp += float(torch.log_softmax(lg.float(), -1)[t])
                seq.append(t); sampled.append(t)
            assert abs(slp - r["sum_logprob"]) < 0.05 * max(1.0, abs(slp)) + tol * len(forced)
        assert n_exact > 0
    # other seeds give other samples at a high temperature; temperature 0 through the same entry point is greedy
    other = m.decode(prompts, sample_len=16, temperature=5.0, seed=1)
    assert [r["tokens"] for r in other] != [r["tokens"] for r in m.decode(prompts, sample_len=16, temperature=5.0, seed=2)]
    assert [r["tokens"] for r in m.decode(prompts, sample_len=16)] == [r["tokens"] for r in m.decode_greedy(prompts, sample_len=16)]


def test_sampling_is_independent_of_batch_split(ccx_ctx, monkeypatch):
    """The noise of a sequence is keyed by its batch row, not by the lane it is decoded in."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini()
    sd = synthetic_whisper_state_dict(dims, seed=0, gain=3.0)
    m = WhisperModel(dims, sd, max_batch=32, device=0, ctx=ccx_ctx)
    rules, _ = _rules()
    clips, n, dev = _clips([3.0] * 32)
    m.log_mel(dev, n)
    m.encode(32)
    prompts = [[rules.sot]] * 32
    monkeypatch.setenv("CCX_DEC_LANES", "1")
    a = m.decode(prompts, sample_len=8, temperature=1.0, seed=7)
    monkeypatch.setenv("CCX_DEC_LANES", "2")
    b = m.decode(prompts, sample_len=8, temperature=1.0, seed=7)
    assert [r["tokens"] for r in a] == [r["tokens"] for r in b]


def test_fused_cross_query_equals_two_launches(ccx_ctx, monkeypatch):
    """Batches of <= 16 sequences compute the cross-attention query INSIDE the cross-attention blocks (dec_cross_fused_q_kernel: the
    reference's own pattern is one window per decode, back/api.py:1286-1292).  It repeats the two launches it replaces operation
    for operation, so at full small.en size the tokens, log-probabilities and no-speech probabilities of 1, 5 and 16 sequences
    (prompts of different lengths, stepwise prompt feeding and prefill, greedy and sampled) must equal the two-launch path exactly;
    a 20-sequence batch (cross attention against the encoder output, never fused) agrees to rounding: the same tokens, or -- at a
    near-tie of these gain-3 weights -- two eps-argmax strings of the oracle."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.small_en()
    sd = synthetic_whisper_state_dict(dims, seed=3, gain=3.0)
    m = WhisperModel(dims, sd, max_batch=20, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([30.0, 9.0, 4.0, 17.5, 2.0] * 4)
        m.log_mel(dev, n)
        xa = m.encode(20, return_xa=True).cpu()
        base = [[rules.sot], [rules.sot_prev, 1212, 318, rules.sot], [rules.sot_prev, 464, 1917, 11, 262, rules.sot], [rules.sot], [rules.sot_prev, 50, rules.sot]]
        for B in (1, 5, 16):
            prompts = [base[i % 5] for i in range(B)]
            for kw in (dict(temperature=0.0), dict(temperature=0.7, seed=11)):
                monkeypatch.setenv("CCX_FUSE_CROSS_Q", "0")
                two = m.decode(prompts, sample_len=7, **kw)
                monkeypatch.setenv("CCX_FUSE_CROSS_Q", "1")
                one = m.decode(prompts, sample_len=7, **kw)
                again = m.decode(prompts, sample_len=7, **kw)          # replays the captured step graph
                for a, b, c in zip(two, one, again):
                    assert a["tokens"] == b["tokens"] == c["tokens"] and len(b["tokens"]) > 0
                    assert a["sum_logprob"] == b["sum_logprob"] == c["sum_logprob"], (B, kw, a["sum_logprob"], b["sum_logprob"])
                    assert a["no_speech_prob"] == b["no_speech_prob"]
        monkeypatch.setenv("CCX_FUSE_CROSS_Q", "1")
        small = m.decode([base[i % 5] for i in range(16)], sample_len=7)
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "17")       # the 20 on the X-stream path (default: K / V up to 80 sequences)
        large = m.decode([base[i % 5] for i in range(20)], sample_len=7)
        monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS")
        # (gain-3 weights: sharper softmaxes and smaller margins than the other path-equivalence tests, whose bound is 2e-3; the 20
        #  sequences take the cross attention against the encoder output, the 16 the split-KV kernels on K / V caches)
        orc = _oracle(dims, sd)
        div = sum(_two_paths_agree("whisper small.en gain 3: |sum_logprob K/V-cache path - X-stream path| / max(1, |.|)", orc, xa[i:i + 1],
                                   base[i % 5], small[i], large[i], 7, 0.15, bound=1.5e-2) for i in range(16))
        assert div <= 4, div
        # ... and each of the two against the oracle under teacher forcing (these weights amplify every rounding ~3x per layer)
        _, orules = _rules()
        for i in range(5):
            for path, res in (("K/V-cache", small[i]), ("X-stream", large[i])):
                forced = res["tokens"] + ([rules.eot] if len(res["tokens"]) < 7 else [])
                o = R.greedy_decode(orc, xa[i:i + 1], [base[i]], orules, sample_len=7, forced=[forced])[0]
                within(f"whisper small.en gain 3: |sum_logprob {path} path - oracle (teacher forced)| / max(1, |oracle|)",
                       abs(o.sum_logprob - res["sum_logprob"]) / max(1.0, abs(o.sum_logprob)), 2e-2, i)
    finally:
        m.close()


def test_small_en_full_size(ccx_ctx):
    """Full small.en dimensions (the BASELINE architecture), B=2, encoder + short greedy decode."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.small_en()
    sd = synthetic_whisper_state_dict(dims, seed=0)
    m = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([30.0, 9.0])
        mel = m.log_mel(dev, n, return_mel=True)
        xa = m.encode(2, return_xa=True).cpu()
        ref = _oracle(dims, sd).encode(mel.cpu())
        within("whisper small.en FULL size: encoder output rel-L2", _rel(xa, ref), 9.5e-3)
        _check_greedy(dims, sd, m, xa, [[rules.sot], [rules.sot_prev, 1212, 318, rules.sot]], sample_len=6, tol=0.08)
    finally:
        m.close()


def test_transcribe_call_surface(mini):
    dims, sd, m = mini
    audio = synthetic_clip(5, 30.0)[: 16000 * 4]
    out = m.transcribe(audio, initial_prompt="This is a conversation between two people.", word_timestamps=True,
                       condition_on_previous_text=True, temperature=0.0)
    assert isinstance(out["text"], str) and "segments" in out
    # the reference's own setting (Config.temperature = 0.1, back/api.py:128): sampled, reproducible per seed + call index
    m.sample_seed, m._sample_calls = 5, 0
    a = m.transcribe(audio, temperature=0.1)
    m.sample_seed, m._sample_calls = 5, 0
    b = m.transcribe(audio, temperature=0.1)
    assert a["tokens"] == b["tokens"] and isinstance(a["text"], str)
    with pytest.raises(Exception):
        m.transcribe(audio, temperature=(0.0, 0.2, 0.4))      # fallback schedules: not implemented, must fail loudly


def test_large_batch_decode_path_matches_small_batch(ccx_ctx, monkeypatch):
    """More than 16 sequences switch the decode chain to the stand-alone resolve+LayerNorm kernel, multi-tile skinny GEMMs and the
    cross attention against the encoder output (cross_x.hip); the tokens of a sequence must not depend on how many batch mates it has."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot], [rules.sot], [rules.sot_prev, 77, rules.sot]]
        _batch_mates(m, dims, sd, dev, n, prompts, 10, 16, monkeypatch)     # 40 sequences: the same 4 windows, 10 times
    finally:
        m.close()


def test_xstream_query_projection_inside_the_expansion_equals_three_launches(ccx_ctx, monkeypatch):
    """X-stream path: resolve + LayerNorm, the query linear and the per-head expansion run as ONE kernel (dec_xq_fused_kernel) or, with
    CCX_XS_FUSE_Q=0, as the three launches it replaces.  Same LayerNorm pieces, another summation order in the 768-long query dot
    products: the same tokens and log-probabilities to 6e-5 relative (2.1e-5 measured), stepwise and prefilled, 40 sequences in lanes -- and both are
    eps-argmax strings of the oracle."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        big = dev.repeat(10, 1).contiguous()
        m.log_mel(big, n * 10); xa = m.encode(40, return_xa=True).cpu()
        prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot], [rules.sot], [rules.sot_prev, 77, 88, 99, rules.sot]] * 10
        orc = _oracle(dims, sd)
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")        # 40 sequences would take the K / V path by default
        monkeypatch.setenv("CCX_DEC_LNFREE", "0")              # round 3's chain (the default chain has its own query kernel, dec_xq_lnfree_kernel)
        for prefill in ("1", "0"):
            monkeypatch.setenv("CCX_PREFILL", prefill)
            monkeypatch.setenv("CCX_XS_FUSE_Q", "1")
            one = m.decode_greedy(prompts, sample_len=12)
            monkeypatch.setenv("CCX_XS_FUSE_Q", "0")
            three = m.decode_greedy(prompts, sample_len=12)
            for i in range(40):
                assert one[i]["tokens"] == three[i]["tokens"], (prefill, i)
                within("whisper mini X-stream: |sum_logprob fused query - three launches| / max(1, |.|)",
                       abs(one[i]["sum_logprob"] - three[i]["sum_logprob"]) / max(1.0, abs(three[i]["sum_logprob"])), 6e-5, i)
            for i in range(4):
                _oracle_accepts(orc, xa[i:i + 1], prompts[i], one[i], 12, 0.05)
    finally:
        m.close()


def test_lane_of_256_rows_and_more_matches_small_batch(ccx_ctx, monkeypatch):
    """Lanes of 128 rows and more (the 768-sequence decode groups of bench.py: 384 per lane) use 32-column blocks in the skinny
    linears -- another grid, the same sums: 264 sequences in ONE lane must decode exactly like a batch of 4."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=264, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot], [rules.sot], [rules.sot_prev, 77, rules.sot]]
        _batch_mates(m, dims, sd, dev, n, prompts, 66, 12, monkeypatch, lanes=1)
    finally:
        m.close()


def test_uneven_lane_partition_matches_small_batch(ccx_ctx, monkeypatch):
    """100 sequences in 3 lanes are cut 48 / 48 / 4: the last lane takes the <= 16-row kernels of the linears, the others the
    large-batch ones, each on its own stream and graph -- every sequence must still decode exactly as in a batch of 4."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=100, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot], [rules.sot], [rules.sot_prev, 77, rules.sot]]
        _batch_mates(m, dims, sd, dev, n, prompts, 25, 12, monkeypatch, lanes=3)
    finally:
        m.close()


def test_long_audio_multi_window_logmel_and_transcribe(ccx_ctx):
    """Audio longer than 30 s: the log-mel is normalised over the WHOLE clip and transcribe() walks 30 s
    windows with `seek` (transcribe.py main loop)."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx, max_audio_seconds=80.0)
    try:
        clip = np.concatenate([synthetic_clip(0, 30.0), 0.3 * synthetic_clip(1, 30.0), synthetic_clip(2, 30.0)[: 16000 * 11]])
        dev = torch.from_numpy(clip[None]).cuda()
        full = R.log_mel_spectrogram(torch.from_numpy(clip))
        content = len(clip) // 160
        for seek in (0, 3000, 6500):
            mel = m.log_mel(dev, [len(clip)], seek=[seek], return_mel=True).cpu()[0]
            ref = R.pad_or_trim(full[:, seek: seek + min(3000, content - seek)], 3000)
            assert float((mel - ref).abs().max()) < 2e-3, seek
        out = m.transcribe(clip, initial_prompt="This is a conversation between two people.")
        seeks = [s["seek"] for s in out["segments"]]
        assert len(set(seeks)) >= 3 and seeks == sorted(seeks)          # at least three 30 s windows were decoded, in order
        with pytest.raises(Exception):
            m.transcribe(np.zeros(16000 * 90, dtype=np.float32))          # beyond max_audio_seconds: loud failure
    finally:
        m.close()


def test_prompt_prefill_equals_stepwise_prompt_feeding(ccx_ctx, monkeypatch):
    """Prompts of 2..16 tokens are prefilled in ONE pass over all prompt positions (rows = sequence x position, the rows of a
    sequence sharing its cross K/V; openai-whisper's first forward) instead of one decode step per prompt token (CCX_PREFILL=0).
    Same kernels per row, so the sampled tokens must agree -- ragged prompt lengths (2, 9, 5, 16 tokens; a 1-token prompt keeps the
    stepwise path), small batch and a 40-sequence batch in lanes, greedy and sampled.  Both are checked against the oracle too."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        g = np.random.default_rng(5)
        prompts = [[rules.sot_prev, 1000, rules.sot],
                   [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, 7)] + [rules.sot],
                   [rules.sot_prev, 300, 400, 500, rules.sot],
                   [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, 14)] + [rules.sot]]
        m.log_mel(dev, n); xa = m.encode(4, return_xa=True).cpu()
        a = m.decode_greedy(prompts, sample_len=10)
        monkeypatch.setenv("CCX_PREFILL", "0")
        b = m.decode_greedy(prompts, sample_len=10)
        monkeypatch.delenv("CCX_PREFILL")
        for i in range(4):
            assert a[i]["tokens"] == b[i]["tokens"], (i, a[i]["tokens"], b[i]["tokens"])
            assert abs(a[i]["sum_logprob"] - b[i]["sum_logprob"]) < 2e-3 * max(1.0, abs(b[i]["sum_logprob"]))
            assert abs(a[i]["no_speech_prob"] - b[i]["no_speech_prob"]) < 1e-5
        _check_greedy(dims, sd, m, xa, prompts, sample_len=10, tol=0.08)            # the prefilled path against the oracle
        s1 = m.decode(prompts, sample_len=8, temperature=0.7, seed=11)
        monkeypatch.setenv("CCX_PREFILL", "0")
        s0 = m.decode(prompts, sample_len=8, temperature=0.7, seed=11)
        monkeypatch.delenv("CCX_PREFILL")
        assert [r["tokens"] for r in s1] == [r["tokens"] for r in s0]
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")                            # the four on the large batch's cross-attention path
        ax = m.decode_greedy(prompts, sample_len=10)
        monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS")
        orc = _oracle(dims, sd)
        for i in range(4):
            _two_paths_agree("whisper mini: |sum_logprob K/V-cache path - X-stream path| / max(1, |.|)", orc, xa[i:i + 1], prompts[i], a[i], ax[i], 10, 0.08)
            _oracle_accepts(orc, xa[i:i + 1], prompts[i], ax[i], 10, 0.08)        # prefill rows through the X-stream kernel (row -> sequence map)
        big = dev.repeat(10, 1).contiguous()
        m.log_mel(big, n * 10); m.encode(40)
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
        c = m.decode_greedy(prompts * 10, sample_len=10)                          # 40 x 16 = 640 prefill rows, X-stream path
        monkeypatch.delenv("CCX_CROSS_X_MIN_ROWS")
        for i in range(40):
            assert c[i]["tokens"] == ax[i % 4]["tokens"], i
            assert abs(c[i]["sum_logprob"] - ax[i % 4]["sum_logprob"]) < 1e-4, i
        m.log_mel(dev, n); m.encode(4)
        one = m.decode_greedy([prompts[1]], sample_len=1)                         # sample_len 1: the prefill's own sample is the only one
        assert one[0]["tokens"] == a[1]["tokens"][:1]
    finally:
        m.close()


def test_long_prompts_are_prefilled_in_passes_of_16_positions(ccx_ctx, monkeypatch):
    """The reference feeds the previous segment's transcript as `initial_prompt` (back/api.py:1424-1426: up to 223 tokens after
    transcribe()'s truncation).  Prompts longer than 16 tokens are prefilled in several passes of 16 positions, each seeing the
    self-K/V of the earlier ones in the caches: ragged lengths 40 / 17 / 3 / 33 (passes of 16 + 16 + 8 rows, sequences ending in
    different passes) must decode exactly like stepwise prompt feeding (CCX_PREFILL=0), on the K/V path (4 sequences) and on the
    X-stream path (40 sequences in lanes), greedy and sampled -- and are checked against the oracle."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        g = np.random.default_rng(9)
        prompts = [[rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, k)] + [rules.sot] for k in (38, 15, 1, 31)]
        assert [len(p) for p in prompts] == [40, 17, 3, 33]
        m.log_mel(dev, n); xa = m.encode(4, return_xa=True).cpu()
        orc = _oracle(dims, sd)
        for B, reps in ((4, 1), (40, 10)):
            if reps > 1:
                big = dev.repeat(reps, 1).contiguous()
                m.log_mel(big, n * reps); m.encode(B)
                monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")        # the 40 on the X-stream path (default: K / V up to 80 sequences)
            a = m.decode_greedy(prompts * reps, sample_len=8)
            s1 = m.decode(prompts * reps, sample_len=6, temperature=0.7, seed=5)
            monkeypatch.setenv("CCX_PREFILL", "0")
            b = m.decode_greedy(prompts * reps, sample_len=8)
            s0 = m.decode(prompts * reps, sample_len=6, temperature=0.7, seed=5)
            monkeypatch.delenv("CCX_PREFILL")
            for i in range(B):
                assert a[i]["tokens"] == b[i]["tokens"], (B, i, a[i]["tokens"], b[i]["tokens"])
                assert a[i]["sum_logprob"] == b[i]["sum_logprob"] and a[i]["no_speech_prob"] == b[i]["no_speech_prob"], (B, i)   # same kernels per row
                assert s1[i]["tokens"] == s0[i]["tokens"], (B, i)
            for i in range(4):
                _oracle_accepts(orc, xa[i:i + 1], prompts[i], a[i], 8, 0.08)
    finally:
        m.close()


def test_layernorm_free_chain_matches_round3_chain(ccx_ctx, monkeypatch):
    """The default chain of the X-stream path is LayerNorm-free at the cross-attention query: the self-attention output projection
    adds its product to the residual stream in place and leaves bf16 rows + per-tile statistics (csrc/decoder.hip DEPI_RESOLVE), and
    the query applies its LayerNorm algebraically (cross_x.hip dec_xq_lnfree_kernel).  CCX_DEC_LNFREE=0 selects round 3's chain.
    The default: the same tokens as round 3's chain, log-probabilities to rounding, every token accepted by the oracle, and a
    sequence's numbers independent of its batch (4 alone = 40 in lanes, bit for bit).  (The other LayerNorm-free variants were
    measured slower and removed: profiles/r04_ab_decode_lnfree_chain.txt, r04_ab_decode_lnfree_hybrids.txt.)"""
    from clearconverse_amd.whisper import WhisperModel
    monkeypatch.setenv("CCX_DEC_LNFREE", "0")              # round 3's chain: the reference
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        clips, n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        g = np.random.default_rng(9)
        prompts = [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot], [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, 20)] + [rules.sot], [rules.sot_prev, 77, rules.sot]]
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
        m.log_mel(dev, n); xa = m.encode(4, return_xa=True).cpu()
        base = m.decode_greedy(prompts, sample_len=40)
        orc = _oracle(dims, sd)
        monkeypatch.delenv("CCX_DEC_LNFREE")                 # the default chain
        m.log_mel(dev, n); m.encode(4)
        small = m.decode_greedy(prompts, sample_len=40)
        big = dev.repeat(10, 1).contiguous()
        m.log_mel(big, n * 10); m.encode(40)
        large = m.decode_greedy(prompts * 10, sample_len=40)
        for i in range(40):
            assert large[i]["tokens"] == small[i % 4]["tokens"] and large[i]["sum_logprob"] == small[i % 4]["sum_logprob"], i
        for i in range(4):
            _oracle_accepts(orc, xa[i:i + 1], prompts[i], small[i], 40, 0.05)
            if small[i]["tokens"] == base[i]["tokens"]:
                within("whisper mini: |sum_logprob LayerNorm-free chain - default chain| / max(1, |.|)",
                       abs(small[i]["sum_logprob"] - base[i]["sum_logprob"]) / max(1.0, abs(base[i]["sum_logprob"])), 6e-4, i)
    finally:
        m.close()
