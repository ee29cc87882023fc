"""GPU: the per-call decoding options through the model handle, at the mini dims of tests/test_whisper_gpu.py, against
oracle/whisper_ref.WhisperRef under the filters of tests/decoding_options_reference.py.

On the two K / V paths (2 rows: split-KV kernels; 18 rows: the lean streaming kernel) and on the X-stream path
(CCX_CROSS_X_MIN_ROWS=1): a decode with without_timestamps whose prompts end in <|notimestamps|>, one with a 3-token prefix behind
the SOT sequence, one with a call-level suppress list -- each teacher-forced through the oracle by the eps-argmax walk (eps 0.02:
every token within eps of the oracle's filtered maximum, exact where the oracle's margin exceeds 2 eps).  The walk does not pass
vacuously: tests/test_decoding_options_reference_cpu.py walks the same decodes by the oracle alone and finds at least half of the
steps decisive; here a walk must hold 0.8 of that count.  sum_logprob and no_speech_prob: the bounds of the greedy tests
(tests/test_whisper_gpu.py::_check_greedy), recorded under names of their own.

Then: graph against eager, bit for bit; a default decode after an option decode equals the one before it and finds its graph where it
left it (ccx_whisper_graph_count); beam size 2 and best_of 2 with without_timestamps; a multilingual instance with a SOT tail of 3.
"""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests import decoding_options_reference as DO
from tests.conftest import within

pytestmark = pytest.mark.gpu

RULES = DecodeRules()
ORULES = R.Rules(suppress=tuple(RULES.suppress))
SL = DO.WALK_SAMPLE_LEN
N_SLP = "decode options: |sum_logprob - oracle (teacher forced)| / max(1, |oracle|)"
N_NSP = "decode options: |no_speech_prob - oracle|"
ROWS = 18                         # > 16: the lean streaming kernel on per-layer K / V


def _mels(seeds, seconds):
    clips = [synthetic_clip(s, 30.0)[: int(t * 16000)] for s, t in zip(seeds, seconds)]
    ns = [len(c) for c in clips]
    host = np.zeros((len(clips), max(ns)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return clips, ns, torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def model(ccx_ctx):
    """the instance with 18 windows encoded (the two clips, cyclic), the oracle, the GPU's encoder output of the two, and the free
    oracle walks of every case on the oracle's OWN encoder output (what the CPU test counts)"""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    m = WhisperModel(dims, sd, max_batch=20, ctx=ccx_ctx, decoding_options=True)
    clips, ns, dev = _mels(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS)
    mel = m.log_mel(dev, ns, return_mel=True).clone()
    m.set_mel(mel[torch.arange(ROWS, device=mel.device) % 2].contiguous())
    xa = m.encode(ROWS, return_xa=True)[:2].cpu()
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    free = {}
    for b, c in enumerate(clips):
        ref_mel = R.pad_or_trim(R.log_mel_spectrogram(torch.from_numpy(c))[:, : len(c) // 160], 3000)
        xa_ref = orc.encode(ref_mel[None])
        for name, (prompt, opts) in DO.walk_cases(ORULES).items():
            free[name, b] = DO.oracle_walk(orc, xa_ref, prompt, ORULES, opts, SL)
    yield m, orc, xa, free
    m.close()


def _decode(m, name, rows, **kw):
    prompt, opts = DO.walk_cases(ORULES)[name]
    n_prefix = len(DO.WALK_PREFIX) if name == "prefix" else 0
    m.set_sot_tail(len(prompt) - 1 - n_prefix)
    m.set_prefix_len(n_prefix)
    try:
        dec = {}
        if opts.without_timestamps:
            dec["without_timestamps"] = True
        if opts.suppress is not None:
            dec["suppress_tokens"] = list(opts.suppress)
        return prompt, opts, m.decode([prompt] * rows, sample_len=SL, **dec, **kw)
    finally:
        m.set_sot_tail(0)
        m.set_prefix_len(0)


def _forced(r):
    return r["tokens"] + ([RULES.eot] if len(r["tokens"]) < SL else [])


@pytest.mark.parametrize("name", ["without_timestamps", "prefix", "suppress list"])
@pytest.mark.parametrize("path,rows,env", [("kv16", 2, None), ("kv_stream", ROWS, None), ("xa_stream", 2, "1")])
def test_option_decodes_follow_the_oracle(model, monkeypatch, path, rows, env, name):
    m, orc, xa, free = model
    if env is not None:
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", env)
    prompt, opts, res = _decode(m, name, rows)
    assert m.last_cross_path == path
    for b in range(rows):                      # within one path a row's numbers do not depend on its batch mates
        assert res[b]["tokens"] == res[b % 2]["tokens"] and res[b]["sum_logprob"] == res[b % 2]["sum_logprob"], b
    for b in range(2):
        r = res[b]
        w = DO.oracle_walk(orc, xa[b:b + 1], prompt, ORULES, opts, SL, forced=_forced(r))
        assert not w["violations"], (path, name, b, w["violations"])
        assert 2 * free[name, b]["decisive"] >= free[name, b]["steps"]                # what the CPU test asserts
        assert w["decisive"] >= 0.8 * free[name, b]["decisive"], (path, name, b, w["decisive"], free[name, b]["decisive"])
        within(N_SLP, abs(w["sum_logprob"] - r["sum_logprob"]) / max(1.0, abs(w["sum_logprob"])), 1.5e-3, (path, name, b))
        within(N_NSP, abs(w["no_speech_prob"] - r["no_speech_prob"]), 1e-6 + 1e-3 * w["no_speech_prob"], (path, name, b))
        toks = r["tokens"]
        assert len(toks) >= 1
        if name == "prefix":                   # the first-step rules apply to the first token BEHIND the prefix
            assert RULES.timestamp_begin <= toks[0] <= RULES.timestamp_begin + 50
        if name == "suppress list":
            assert all(t >= 20000 for t in toks)


def test_graph_equals_eager_and_default_decodes_keep_their_graphs(model, monkeypatch):
    m, orc, xa, free = model
    plain = [[RULES.sot], [RULES.sot_prev, 5000, RULES.sot]]
    flat = lambda res: [(r["tokens"], r["sum_logprob"], r["no_speech_prob"]) for r in res]
    before = flat(m.decode(plain, sample_len=SL))
    n_default = m.graph_count() - m.graph_count(True)       # (the module's instance: option plans of earlier tests may be cached)
    assert n_default >= 1
    _, _, a = _decode(m, "without_timestamps", 2)
    assert m.graph_count(True) >= 1 and m.graph_count() - m.graph_count(True) == n_default
    # a default decode after an option decode: the bits it had, the graph it had
    assert flat(m.decode(plain, sample_len=SL)) == before
    assert m.graph_count() - m.graph_count(True) == n_default
    n_opt = m.graph_count(True)
    _, _, a2 = _decode(m, "without_timestamps", 2)          # alternating captures each plan once
    assert flat(a2) == flat(a) and m.graph_count(True) == n_opt
    # another mask drops the option plans' graphs, and those alone
    _, _, s1 = _decode(m, "suppress list", 2)
    assert m.graph_count() - m.graph_count(True) == n_default
    assert flat(m.decode(plain, sample_len=SL)) == before
    # graph against eager, bit for bit
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    _, _, e = _decode(m, "without_timestamps", 2)
    _, _, s2 = _decode(m, "suppress list", 2)
    assert flat(m.decode(plain, sample_len=SL)) == before
    assert flat(e) == flat(a) and flat(s2) == flat(s1)


def _teacher_forced(orc, xa_row, prompt, opts, tokens):
    """fp64 sum of the tokens' log-probabilities under the options' filters; every token must be allowed"""
    seq, sampled, slp = list(prompt), [], 0.0
    for i, t in enumerate(tokens):
        lg = DO.apply_filters(orc.decoder_logits(torch.tensor([seq]), xa_row)[0, -1].float(), sampled, ORULES, opts)
        assert torch.isfinite(lg[t]), (i, t)
        slp += float(torch.log_softmax(lg.double(), dim=-1)[t])
        seq.append(t); sampled.append(t)
    return slp


def test_beam_and_best_of_without_timestamps(model):
    m, orc, xa, free = model
    prompt, opts = DO.walk_cases(ORULES)["without_timestamps"]
    m.set_sot_tail(1)
    try:
        hyps = m.decode_beam([prompt, prompt], 2, sample_len=SL, windows=[0, 1], n_windows=2, without_timestamps=True)
        rows = m.decode_rows([prompt] * 4, [0, 0, 1, 1], [0, 1, 2, 3], sample_len=SL, temperature=0.7, seed=11, n_windows=2,
                             without_timestamps=True)
        ruled = m.decode_beam([prompt, prompt], 2, sample_len=SL, windows=[0, 1], n_windows=2)
    finally:
        m.set_sot_tail(0)
    for g in range(2):
        assert len(hyps[g]) >= 2
        for h in hyps[g]:
            slp = _teacher_forced(orc, xa[g:g + 1], prompt, opts, _forced(h))
            within(N_SLP, abs(slp - h["sum_logprob"]) / max(1.0, abs(slp)), 1.5e-3, ("beam", g))
        assert [h["tokens"] for h in hyps[g]] != [h["tokens"] for h in ruled[g]]       # the rules would have forced timestamps
    for r, w in zip(rows, [0, 0, 1, 1]):
        slp = _teacher_forced(orc, xa[w:w + 1], prompt, opts, _forced(r))
        within(N_SLP, abs(slp - r["sum_logprob"]) / max(1.0, abs(slp)), 1.5e-3, ("best_of", w))
    assert rows[0]["tokens"] != rows[1]["tokens"] or rows[2]["tokens"] != rows[3]["tokens"]      # two draws per window


def test_multilingual_sot_tail_of_three(ccx_ctx):
    """[sot, <|de|>, <|transcribe|>, <|notimestamps|>]: no_speech_prob is the oracle's at the <|startoftranscript|> position"""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128, n_vocab=51865)
    sd = synthetic_whisper_state_dict(dims, seed=5)
    rules = DecodeRules.for_dims(dims)
    orules = R.Rules(eot=rules.eot, sot=rules.sot, sot_prev=rules.sot_prev, no_speech=rules.no_speech, no_timestamps=rules.no_timestamps,
                     timestamp_begin=rules.timestamp_begin, blank=rules.blank, suppress=tuple(rules.suppress))
    m = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx, decoding_options=True)
    try:
        clips, ns, dev = _mels((42,), (7.0,))
        m.log_mel(dev, ns)
        xa = m.encode(1, return_xa=True).cpu()
        prompt = rules.sot_sequence("de") + [rules.no_timestamps]
        assert len(prompt) == 4
        m.set_sot_tail(3)
        r = m.decode([prompt], sample_len=SL, without_timestamps=True)[0]
        opts = DO.Options(True)
        orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
        w = DO.oracle_walk(orc, xa, prompt, orules, opts, SL, forced=_forced(r))
        assert not w["violations"], w["violations"]
        within(N_NSP, abs(w["no_speech_prob"] - r["no_speech_prob"]), 1e-6 + 1e-3 * w["no_speech_prob"], "multilingual")
        within(N_SLP, abs(w["sum_logprob"] - r["sum_logprob"]) / max(1.0, abs(w["sum_logprob"])), 1.5e-3, "multilingual")
        # (the position matters: at the prompt's last token the oracle's probability is 3.1e-6 against 5.4e-6 here, twice the bound away)
    finally:
        m.close()
