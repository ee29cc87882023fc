"""GPU: word alignment through the model handle (ccx_whisper_align, WhisperModel.align) and through transcribe(word_timestamps=True)
on an instance built with word_alignment=True -- what the reference asks for at back/api.py:1435, 1477.

The parity check is cut in three, so that no step amplifies the rounding of the step before it:
  1. probs_out against the fp64 oracle's cross-attention softmax (tests/align_reference.cross_attention_probs: WhisperRef's decoder
     arithmetic on the GPU's own encoder output, truncated to n_frames // 2 keys), as max |p - oracle| / max_j p per row.  A priori:
     |dp| / max_j p <= 2 |ds| and a score carries |ds| <= (4 * 2^-9 + 9e-3) S -- keys are stored in bf16 and come, like the query,
     from bf16 weights and bf16 activations (four roundings of 2^-9 per product), the residual stream the query is projected from
     agrees with the oracle to the 9e-3 of the decoder-logits test, S = max sum_i |q_i k_i| / 8 (7.3 .. 8.7 here): 0.29.  Measured on
     an MI355X: 6.9e-3 .. 9.6e-3 (mini), 1.00e-2 and 1.08e-2 (small.en); the bound is 2.5 x the worst.
  2. matrix_out against the fp64 matrix reference applied to the GPU's OWN probs_out.  The kernel-level bound of
     tests/test_align_kernels_gpu.py holds for columns whose std / mean over the tokens is above 0.1; the near-uniform attention of
     seeded weights gives 1.1e-2 .. 7.9e-2 here (asserted to stay above 1e-2), where the same rounding of the mean weighs up to ten
     times more.  Measured: 1.06e-6 .. 3.79e-6; the bound is a fixed 2.5 x the worst.
  3. jump frames against the fp32 host DTW on the GPU's OWN matrix_out: exact.
The measured values are in profiles/align_kernels_measured_deviations.json.
"""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from oracle import whisper_transcribe_ref as TR
from tests import align_reference as AR
from tests.conftest import within

pytestmark = pytest.mark.gpu

TOL_PROBS = 2.7e-2          # a priori 0.29; measured 1.083e-02
TOL_MODEL_MATRIX = 9.4e-6   # measured 3.793e-06 at std / mean = 1.24e-2
MIN_COND = 1e-2             # std / mean of every (head, frame) column of the model's probabilities; measured 1.144e-2 at the least
N_PROBS = "whisper align: probs_out max |p - oracle| / max_j p"
N_MATRIX = "whisper align: matrix_out max |A - ref(own probs)|"
RULES = DecodeRules()


def _stage(m, lengths_s):
    clips = [synthetic_clip(20 + i, 30.0)[: int(s * 16000)] for i, s in enumerate(lengths_s)]
    n = [len(c) for c in clips]
    host = np.zeros((len(clips), max(n)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    m.log_mel(torch.from_numpy(host).cuda(), n)
    return m.encode(len(clips), return_xa=True).cpu()


def _tokens(seed, lens, n_vocab):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        t = torch.randint(0, RULES.eot, (n,), generator=g).tolist()
        t[0], t[1], t[-1] = RULES.sot, RULES.no_timestamps, RULES.eot
        out.append(t)
    return out


def _three_checks(m, dims, sd, xa, toks, n_frames, what):
    jumps, P, A = m.align(toks, n_frames, return_probs=True, return_matrix=True)
    P, A = P.cpu(), A.cpu()
    ref = R.WhisperRef(R.Dims(**dims.__dict__), sd, dtype=torch.float64)
    heads = m.alignment_heads
    for b, t in enumerate(toks):
        T, M = len(t), n_frames[b] // 2
        # 1. probabilities against the oracle
        want, S = AR.cross_attention_probs(ref, torch.tensor(t, dtype=torch.long), xa[b], heads, M)
        got = P[b, :, :T, :M]
        assert torch.isfinite(got).all() and bool((P[b, :, :T, M:] == 0).all()), (what, b)
        err = float(((got.double() - want).abs().amax(-1) / want.amax(-1)).max())
        print(f"[align {what} seq {b}] T={T} M={M} S={S:.3f} probs err={err:.3e} rel-L2={float((got.double() - want).norm() / want.norm()):.3e}")
        assert S < 10.0, (what, b, S)                                      # the S of the a-priori figure
        within(N_PROBS, err, TOL_PROBS, (what, b, S))
        # 2. the matrix against the reference applied to the GPU's own probabilities
        std, mean = torch.std_mean(got.double(), dim=1, unbiased=False)
        cond = float((std / mean).min())
        merr = float((A[b, :T, :M].double() - AR.matrix_ref(got)).abs().max())
        print(f"[align {what} seq {b}] min std/mean={cond:.3e} matrix err={merr:.3e}")
        assert cond > MIN_COND, (what, b, cond)                            # flatter columns would be another input, not a wider bound
        within(N_MATRIX, merr, TOL_MODEL_MATRIX, (what, b, cond))
        assert bool((A[b, T:] == 0).all()) and bool((A[b, :, M:] == 0).all()), (what, b)
        # 3. the DTW on the GPU's own matrix: exact
        x = -A[b, 1:T - 1, :M].numpy()
        ri, rj = AR.dtw_ref_fast(x)
        assert np.array_equal(jumps[b], AR.jump_frames(ri, rj)), (what, b)
        assert len(jumps[b]) == T - 2


def test_align_mini_ragged_batch(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(2, 128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx, word_alignment=True)
    try:
        assert m.alignment_heads == [(1, 0), (1, 1)]
        xa = _stage(m, [30.0, 15.01, 7.0])
        _three_checks(m, dims, sd, xa, _tokens(0, (5, 12, 20), dims.n_vocab), [3000, 1501, 700], "mini")
        # a decode of the same windows in between does not disturb the alignment, and the alignment does not disturb the decode
        toks = _tokens(0, (5, 12, 20), dims.n_vocab)
        a = m.decode([[RULES.sot]] * 3, sample_len=6)
        j1, _, _ = m.align(toks, [3000, 1501, 700])
        b = m.decode([[RULES.sot]] * 3, sample_len=6)
        j2, _, _ = m.align(toks, [3000, 1501, 700])
        assert [r["tokens"] for r in a] == [r["tokens"] for r in b] and [r["sum_logprob"] for r in a] == [r["sum_logprob"] for r in b]
        assert all(np.array_equal(x, y) for x, y in zip(j1, j2))
        with pytest.raises(Exception, match="ccx_whisper_align"):
            m.align([[RULES.sot, RULES.eot]], [3000])                 # no row between row0 and the last
        with pytest.raises(Exception, match="ccx_whisper_align"):
            m.align(toks[:1], [3001])
    finally:
        m.close()


def test_align_small_en_full_size(ccx_ctx):
    """the real width once: 72 heads over layers 6 .. 11 (the default: upper half of the decoder)"""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.small_en()
    sd = synthetic_whisper_state_dict(dims, seed=0)
    m = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx, word_alignment=True)
    try:
        assert len(m.alignment_heads) == 72 and m.alignment_heads[0] == (6, 0) and m.alignment_heads[-1] == (11, 11)
        xa = _stage(m, [30.0, 9.0])
        _three_checks(m, dims, sd, xa, _tokens(1, (30, 30), dims.n_vocab), [3000, 900], "small.en")
    finally:
        m.close()


def _strip(out):
    return dict(text=out["text"], tokens=out["tokens"],
                segments=[(s["seek"], s["start"], s["end"], s["text"], s["tokens"], "words" in s) for s in out["segments"]])


def test_transcribe_with_word_alignment_end_to_end(ccx_ctx, monkeypatch):
    from clearconverse_amd.whisper import WhisperModel, WindowLoop
    log = []
    advance = WindowLoop.advance

    def recording_advance(self, r, temperature=0.0, last_word_end=None, segments=None):
        log.append(dict(seek=self.seek, result=r, last_word_end=last_word_end))
        return advance(self, r, temperature, last_word_end=last_word_end, segments=segments)
    dims = WhisperDims.mini(2, 128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    clip = np.concatenate([synthetic_clip(0, 30.0), 0.5 * synthetic_clip(1, 30.0)[: 16000 * 15]])
    prompt = "This is a conversation between two people."
    m = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx, max_audio_seconds=60.0, word_alignment=True)
    plain = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx, max_audio_seconds=60.0)
    try:
        monkeypatch.setattr(WindowLoop, "advance", recording_advance)       # the decode result and last-word end of every window
        out = m.transcribe(clip, initial_prompt=prompt, word_timestamps=True)
        monkeypatch.setattr(WindowLoop, "advance", advance)
        assert len(log) >= 2
        # every segment that kept text has words; times are ordered inside a window
        by_seek = {}
        for s in out["segments"]:
            assert "words" in s
            if s["text"].strip():
                assert len(s["words"]) > 0, s
            by_seek.setdefault(s["seek"], []).extend(s["words"])
        for seek, words in by_seek.items():
            assert all(w["start"] <= w["end"] for w in words), seek
            starts = [w["start"] for w in words]
            assert starts == sorted(starts), seek
        # the window walk equals upstream's loop driven with the product's own decode results and its own last-word ends
        results = {w["seek"]: w for w in log}

        def decode_fn(seek, segment_size, prompt_tokens):
            r = results[seek]["result"]
            return TR.ScriptedResult(list(r["tokens"]), r["avg_logprob"], r["no_speech_prob"], 0.0)

        ref = TR.transcribe_loop(len(clip) // 160, decode_fn, TR.TokenizerIds(RULES.eot, RULES.timestamp_begin), m.tokenizer.encode,
                                 m.tokenizer.decode, initial_prompt=prompt, word_timestamps=True,
                                 last_word_end_fn=lambda segs: results[segs[0]["seek"]]["last_word_end"])
        assert [w["seek"] for w in log] == ref["seeks"]
        # word_timestamps without word_alignment: today's output, from this instance's flag off and from an instance built without it
        base = plain.transcribe(clip, initial_prompt=prompt)
        assert _strip(plain.transcribe(clip, initial_prompt=prompt, word_timestamps=True)) == _strip(base)
        m.word_alignment = False
        assert _strip(m.transcribe(clip, initial_prompt=prompt, word_timestamps=True)) == _strip(base)
        assert not any("words" in s for s in base["segments"])
    finally:
        m.close()
        plain.close()


def test_instance_without_word_alignment_never_launches_an_align_kernel(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(2, 128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    audio = synthetic_clip(5, 30.0)[: 16000 * 6]
    names = {}
    for flag in (False, True):
        m = WhisperModel(dims, sd, max_batch=2, ctx=ccx_ctx, **({"word_alignment": True} if flag else {}))
        try:
            ccx_ctx.prof_enable(True)
            try:
                m.transcribe(audio, word_timestamps=True)
                if flag:       # whatever the window decoded to: one alignment of the window still encoded
                    m.align([[RULES.sot, RULES.no_timestamps, 1000, 2000, RULES.eot]], [600])
                names[flag] = [r[0] for r in ccx_ctx.prof_records()]
            finally:
                ccx_ctx.prof_enable(False)
        finally:
            m.close()
    assert len(names[False]) > 0 and not any(n.startswith("align_") for n in names[False])
    # the same call on an instance built with it does launch them (the names are what the check above looks for)
    assert {"align_scores_kernel", "align_matrix_kernel", "align_dtw_kernel"} <= set(names[True])
