"""-m gpu: token probabilities out of the alignment pass (ccx_whisper_align_probs, WhisperModel.align(token_probs=True)), the words'
`probability` and `hallucination_silence_threshold` through transcribe(), at mini dims
[UPSTREAM-RECALL: timing.py::find_alignment, transcribe.py; parity unpinned].

Bounds -- none is chosen here:
  TOL_LOG   tests/test_pick_probs_gpu.py (imported): the kernel's own bound.  The alignment pass and ccx_whisper_decoder_logits run the
            same step chain on <= 16 rows and one cross-attention path, so the logits the kernel read are the logits the test
            reads back, and nothing is added to the kernel's bound.
  2 EPS     4e-2 against oracle/whisper_ref.py: a log-softmax moves by at most 2 x the sup-norm error of its logits, and EPS = 0.02 is
            how far a teacher-forced GPU logit may sit from the oracle's at mini dims (restated from tests/test_multilingual_gpu.py,
            which takes it from tests/test_whisper_long_gpu.py).
"""
import copy
import math

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from clearconverse_amd.word_timing import alignment_tokens, get_end
from oracle import whisper_ref as R
from tests import wordprob_reference as WR
from tests.conftest import within
from tests.test_multilingual_gpu import clip_batch, weights
from tests.test_pick_probs_gpu import TOL_LOG
from tests.test_whisper_align_gpu import _stage, _tokens

pytestmark = pytest.mark.gpu

EPS = 0.02
RULES = DecodeRules()
N_OWN = "whisper word probs: |log token prob - fp64 softmax of the instance's own logits|"
N_ORACLE = "whisper word probs: |log token prob - oracle|"
LENS = (5, 12, 20)
FRAMES = [3000, 1501, 700]
THRESHOLD = 2.0


def _padded(toks, eot):
    T = max(len(t) for t in toks)
    out = np.full((len(toks), T), eot, dtype=np.int64)
    for b, t in enumerate(toks):
        out[b, :len(t)] = t
    return out


def _check_against_own_logits(m, toks, probs, row0, what):
    """probs[b][i] against the fp64 softmax over [0, eot) of the instance's own teacher-forced logits at row row0 + i"""
    pad = _padded(toks, m.rules.eot)
    own = m.decoder_logits(pad).cpu().numpy()
    for b, t in enumerate(toks):
        n = len(t) - row0 - 2
        assert probs[b].shape == (n,) and probs[b].dtype == np.float32, (what, b)
        picks = t[row0 + 1: row0 + 1 + n]
        _, logp = WR.pick_probs_ref(own[b, row0: row0 + n], m.rules.eot, picks)
        for i in range(n):
            assert 0.0 < probs[b][i] <= 1.0, (what, b, i, probs[b][i])
            d = abs(math.log(float(probs[b][i])) - logp[i])
            within(N_OWN, d, TOL_LOG, (what, b, i))
        print(f"[word probs {what} seq {b}] {n} tokens, worst |dlog p| vs own logits {max(abs(math.log(float(p)) - l) for p, l in zip(probs[b], logp)):.3e}")
    return pad


@pytest.fixture(scope="module")
def mini(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(2, 128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, max_audio_seconds=46.0, word_alignment=True, word_probabilities=True)
    yield dims, sd, m
    m.close()


def test_word_probabilities_need_word_alignment(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(2, 128)
    with pytest.raises(_lib.CcxError, match="word_alignment"):
        WhisperModel(dims, {}, ctx=ccx_ctx, word_probabilities=True)


def test_token_probs_against_own_logits_and_the_oracle(mini):
    dims, sd, m = mini
    xa = _stage(m, [30.0, 15.01, 7.0])
    toks = _tokens(0, LENS, dims.n_vocab)
    jumps, _, _, probs = m.align(toks, FRAMES, token_probs=True)
    assert [len(p) for p in probs] == [n - 3 for n in LENS] and [len(j) for j in jumps] == [n - 2 for n in LENS]
    pad = _check_against_own_logits(m, toks, probs, 1, "mini")
    ref = R.WhisperRef(R.Dims(**dims.__dict__), sd).decoder_logits(torch.from_numpy(pad), xa).double().numpy()
    for b, t in enumerate(toks):
        n = len(t) - 3
        _, logp = WR.pick_probs_ref(ref[b, 1: 1 + n], RULES.eot, t[2: 2 + n])
        err = max(abs(math.log(float(p)) - l) for p, l in zip(probs[b], logp))
        print(f"[word probs mini seq {b}] worst |dlog p| vs oracle {err:.3e}")
        within(N_ORACLE, err, 2 * EPS, b)


def test_pass_outputs_are_bit_identical_with_and_without_token_probs(mini, ccx_ctx):
    dims, sd, m = mini
    _stage(m, [30.0, 15.01, 7.0])
    toks = _tokens(0, LENS, dims.n_vocab)
    names = {}
    m.align(toks, FRAMES)                      # the first pass over freshly encoded windows also projects their K / V
    ccx_ctx.prof_enable(True)
    try:
        j0, P0, A0 = m.align(toks, FRAMES, return_probs=True, return_matrix=True)
        names[False] = [r[0] for r in ccx_ctx.prof_records()]
    finally:
        ccx_ctx.prof_enable(False)
    ccx_ctx.prof_enable(True)
    try:
        j1, P1, A1, probs = m.align(toks, FRAMES, return_probs=True, return_matrix=True, token_probs=True)
        names[True] = [r[0] for r in ccx_ctx.prof_records()]
    finally:
        ccx_ctx.prof_enable(False)
    assert all(np.array_equal(a, b) for a, b in zip(j0, j1)) and torch.equal(P0, P1) and torch.equal(A0, A1)
    # without probabilities the pass launches what it launched before; with them, one launch per row that holds a text token
    assert "dec_pick_probs_kernel" not in names[False]
    assert names[True].count("dec_pick_probs_kernel") == max(LENS) - 3
    assert [n for n in names[True] if n != "dec_pick_probs_kernel"] == names[False]
    # a text token at or behind prob_hi is refused, naming the position
    bad = [list(t) for t in toks]
    bad[1][4] = RULES.eot + 5
    with pytest.raises(_lib.CcxError, match=r"tokens\[1\]\[4\]"):
        m.align(bad, FRAMES, token_probs=True)
    m.align(bad, FRAMES)                                                  # ... by the probabilities only


def test_a_window_alone_equals_the_window_inside_a_group(mini):
    dims, sd, m = mini
    lengths = [30.0, 15.01, 7.0]
    xa = _stage(m, lengths)
    toks = _tokens(0, LENS, dims.n_vocab)
    _, _, _, grouped = m.align(toks, FRAMES, token_probs=True)
    _, _, _, first = m.align(toks[:1], FRAMES[:1], token_probs=True)      # window 0 of the same encoding, as a batch of one
    assert np.array_equal(first[0], grouped[0])
    for k in range(3):
        clip = synthetic_clip(20 + k, 30.0)[: int(lengths[k] * 16000)].astype(np.float32)
        m.log_mel(torch.from_numpy(clip[None].copy()).cuda(), [len(clip)])
        alone_xa = m.encode(1, return_xa=True).cpu()
        assert torch.equal(alone_xa[0], xa[k]), k                          # the encoder's rows do not depend on the batch
        _, _, _, alone = m.align([toks[k]], [FRAMES[k]], token_probs=True)
        assert np.array_equal(alone[0], grouped[k]), k


def test_multilingual_rows_behind_a_three_token_sot_sequence(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd, rules = weights()
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, word_alignment=True, word_probabilities=True)
    try:
        ns, host = clip_batch(2, 2)
        m.log_mel(torch.from_numpy(host).cuda(), ns)
        m.encode(2)
        g = torch.Generator().manual_seed(0)
        seq = rules.sot_sequence("de")
        texts = [torch.randint(0, rules.eot, (n,), generator=g).tolist() for n in (7, 15)]
        toks = [alignment_tokens(t, rules, seq) for t in texts]
        n_frames = [min(3000, n // 160) for n in ns]
        jumps, _, _, probs = m.align(toks, n_frames, row0=3, token_probs=True)
        assert [len(p) for p in probs] == [7, 15] and [len(j) for j in jumps] == [8, 16]
        assert m.rules.eot == 50257
        _check_against_own_logits(m, toks, probs, 3, "multilingual")
    finally:
        m.close()


def _clip45():
    return np.concatenate([synthetic_clip(0, 30.0), 0.5 * synthetic_clip(1, 30.0)[: 16000 * 15]]).astype(np.float32)


def _strip(out, drop_probability):
    segs = []
    for s in out["segments"]:
        words = [{k: v for k, v in w.items() if not (drop_probability and k == "probability")} for w in s.get("words", [])]
        segs.append((s["seek"], s["start"], s["end"], s["text"], s["tokens"], words))
    return dict(text=out["text"], tokens=out["tokens"], segments=segs)


@pytest.fixture(scope="module")
def transcripts(mini, ccx_ctx):
    """One 45 s clip through: an instance without word_probabilities; this one without a threshold (every align call recorded);
    this one with the threshold (every advance call recorded)."""
    from clearconverse_amd.whisper import WhisperModel, WindowLoop
    dims, sd, m = mini
    clip = _clip45()
    plain_m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, max_audio_seconds=46.0, word_alignment=True)
    try:
        plain = plain_m.transcribe(clip, word_timestamps=True, hallucination_silence_threshold=THRESHOLD)      # no effect without the flag
        plain_none = plain_m.transcribe(clip, word_timestamps=True)
    finally:
        plain_m.close()
    aligns, advances = [], []
    align, advance = WhisperModel.align, WindowLoop.advance

    def spy_align(self, tokens_per_seq, n_frames, **kw):
        out = align(self, tokens_per_seq, n_frames, **kw)
        aligns.append(dict(tokens=[list(t) for t in tokens_per_seq], row0=kw.get("row0", 1), probs=out[3] if kw.get("token_probs") else None))
        return out

    def spy_advance(self, r, temperature=0.0, last_word_end=None, segments=None, **kw):
        rec = dict(seek=self.seek, content=self.content, last_speech=self.last_speech_timestamp, r=r, last_word_end=last_word_end,
                   segments=copy.deepcopy(segments), kw=dict(kw), n_before=len(self.segments))
        advance(self, r, temperature, last_word_end=last_word_end, segments=segments, **kw)
        rec.update(seek_after=self.seek, added=copy.deepcopy(self.segments[rec["n_before"]:]), last_speech_after=self.last_speech_timestamp)
        advances.append(rec)

    WhisperModel.align, WindowLoop.advance = spy_align, spy_advance
    try:
        with_p = m.transcribe(clip, word_timestamps=True)
        aligns_none, advances_none = list(aligns), list(advances)
        aligns.clear(); advances.clear()
        with_none = m.transcribe(clip, word_timestamps=True, hallucination_silence_threshold=None)
        aligns.clear(); advances.clear()
        with_thr = m.transcribe(clip, word_timestamps=True, hallucination_silence_threshold=THRESHOLD)
        advances_thr = list(advances)
        off = m.transcribe(clip, word_timestamps=False, hallucination_silence_threshold=THRESHOLD)
    finally:
        WhisperModel.align, WindowLoop.advance = align, advance
    return dict(plain=plain, plain_none=plain_none, with_p=with_p, with_none=with_none, with_thr=with_thr, off=off, aligns_none=aligns_none,
                advances_none=advances_none, advances_thr=advances_thr, clip=clip)


def test_transcribe_words_carry_the_mean_of_their_token_probabilities(mini, transcripts):
    dims, sd, m = mini
    t = transcripts
    words = [w for s in t["with_p"]["segments"] for w in s["words"]]
    assert len(words) > 0 and all("probability" in w and 0.0 < w["probability"] <= 1.0 for w in words)
    # on an instance without the flag: no such key, everything else equal; the threshold has no effect there
    assert not any("probability" in w for s in t["plain"]["segments"] for w in s["words"])
    assert _strip(t["with_p"], True) == _strip(t["plain"], False) == _strip(t["plain_none"], False)
    # the mean of its tokens' probabilities: the recorded align calls (one window each: a single clip) give the token probabilities,
    # the tokenizer's word split the token counts -- every " <id>" of the IdTokenizer is a word of its own, asserted
    assert len(t["aligns_none"]) >= 2 and all(a["probs"] is not None and len(a["probs"]) == 1 for a in t["aligns_none"])
    from clearconverse_amd.word_timing import split_to_word_tokens
    want = []
    for a in t["aligns_none"]:
        text = a["tokens"][0][a["row0"] + 1: -1]
        assert len(a["probs"][0]) == len(text)
        _, wt = split_to_word_tokens(m.tokenizer, text + [RULES.eot], RULES.eot)
        counts = [len(x) for x in wt[:-1]]
        assert sum(counts) == len(text)
        want += WR.word_probs_ref(a["probs"][0], counts)
    assert len(want) == len(words)
    assert [w["probability"] for w in words] == pytest.approx(want, rel=1e-12, abs=0.0)
    # without word_timestamps the threshold is ignored, as upstream ignores it
    assert not any("words" in s for s in t["off"]["segments"])


def test_hallucination_silence_threshold_none_and_replayed_through_the_reference(mini, transcripts):
    from clearconverse_amd.whisper import WindowLoop
    dims, sd, m = mini
    t = transcripts
    assert t["with_none"] == t["with_p"]                                   # None: bit for bit the run without the argument
    assert all(a["kw"] == {} for a in t["advances_none"])                 # ... and advance is not even told
    # every recorded window of the threshold run through the reference rule
    thr_seeks = [a["seek"] for a in t["advances_thr"]]
    none_seeks = [a["seek"] for a in t["advances_none"]]
    print(f"[hallucination threshold] seeks without {none_seeks}\n[hallucination threshold] seeks with {THRESHOLD}: {thr_seeks}")
    fired = set()
    for a in t["advances_thr"]:
        assert a["kw"] == dict(hallucination_silence_threshold=THRESHOLD)
        loop = WindowLoop(RULES, m.tokenizer, a["content"], None, dims.n_text_ctx)
        loop.seek = a["seek"]
        built = loop.window_segments(a["r"])
        if built is None:                                                  # the silence rule skipped the window: nothing to replay
            assert a["seek_after"] == a["seek"] + min(3000, a["content"] - a["seek"]) and a["added"] == []
            continue
        _, single, seek_in = built
        lwe = get_end(a["segments"])
        assert lwe == a["last_word_end"]
        if not single and lwe > a["seek"] / 100:
            seek_in = round(lwe * 100)
        ref = WR.silence_rule_ref(copy.deepcopy(a["segments"]), a["seek"], seek_in, a["content"], single, lwe, a["last_speech"], THRESHOLD)
        fired |= ref["branches"]
        assert a["seek_after"] == ref["seek"], (a["seek"], a["seek_after"], ref["seek"], ref["branches"])
        assert [(s["start"], s["end"], s["words"]) for s in a["added"]] == [(s["start"], s["end"], s["words"]) for s in ref["segments"]]
        assert a["last_speech_after"] == ref["last_speech_timestamp"]
    print(f"[hallucination threshold] branches that fired: {sorted(fired)}")
    # the rule fired: seeded weights give near-uniform logits, every word is improbable and every segment with words anomalous
    assert thr_seeks != none_seeks
    assert fired & {"truncate", "leading_gap_drop"}
