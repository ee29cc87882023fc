"""`WhisperModel`: drop-in for the `self.whisper_model` object of the reference
(created at /root/reference/back/api.py:665-703; called at 1286-1292, 1432-1438, 1474-1480).

Only `.transcribe(audio_np, initial_prompt=, word_timestamps=, condition_on_previous_text=,
temperature=)['text']` is consumed by the reference (back/api.py:1103, 1447, 1488); the same call
shape is kept.  All arithmetic runs in libccx (hand-written HIP for gfx950) through the C ABI; this
module drives it and adds a batch entry point the reference lacks.  The window/segment bookkeeping of
openai-whisper's transcribe.py [UPSTREAM-RECALL] is clearconverse_amd/window_loop.py (GPU-free).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import asdict
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, audio_ctx as audio_ctx_policy, decoding_options, fallback
from .audio import mel_filterbank
from .tokenizer import DecodeRules, IdTokenizer, get_tokenizer
from .weights import WhisperDims
from .window_loop import (FRAMES_PER_SECOND, HOP, INPUT_STRIDE, N_FRAMES, SAMPLE_RATE, TIME_PRECISION,  # noqa: F401 (re-exported)
                          WindowLoop, decode_cap, groups_by_cap, is_segment_anomaly, next_words_segment, word_anomaly_score)
from .word_timing import add_word_timestamps, alignment_tokens, get_end

N_SAMPLES = 480000
CROSS_PATHS = {0: "kv16", 1: "kv_stream", 2: "xa_stream"}
XS_WIDTHS = (128, 256, 384, 512, 768)      # widths the X-stream cross attention is instantiated for (csrc/cross_x.hip ccx_xs_supported)


def cross_fp8_refusal(dims: WhisperDims) -> Optional[str]:
    """Why an instance of these dims cannot keep the FP8 encoder-output image (include/ccx.h ccx_whisper_set_cross_fp8), or None: the
    library's own conditions, checked here before anything is created."""
    if dims.n_text_state != dims.n_audio_state or dims.n_text_head != dims.n_audio_head:
        return (f"decoder width {dims.n_text_state} ({dims.n_text_head} heads) differs from the encoder's {dims.n_audio_state} "
                f"({dims.n_audio_head} heads): the instance has no X-stream path")
    if dims.n_audio_state not in XS_WIDTHS or dims.n_audio_head * 64 != dims.n_audio_state:
        return (f"width {dims.n_audio_state} is not one the X-stream cross attention is instantiated for {XS_WIDTHS} "
                "(the 1280-wide family keeps per-layer K / V caches)")
    e = os.environ.get("CCX_CROSS_X")
    if e is not None and e.strip().lstrip("+-").isdigit() and int(e) == 0:
        return "CCX_CROSS_X=0 turns the X-stream path off, which is the only reader of the FP8 image"
    return None


def audio_ctx_refusal(dims: WhisperDims) -> Optional[str]:
    """Why an instance of these dims cannot run a reduced audio context (include/ccx.h ccx_whisper_set_audio_ctx), or None: the rule of
    `cross_fp8_refusal` -- the X-stream is the only cross attention with a key count per sequence -- checked before anything is created."""
    why = cross_fp8_refusal(dims)
    if why is None:
        return None
    return why.replace("which is the only reader of the FP8 image", "which is the only cross attention with a key count per sequence")


class CallSettings(NamedTuple):
    """What one call wants set on the instance while it runs (`WhisperModel._settings`); a field that is None sets nothing."""
    options: Optional[decoding_options.CallOptions] = None      # -> set_decode_options
    history: Optional[Tuple[float, int]] = None                 # (repetition_penalty, no_repeat_ngram_size)
    bias: Optional[tuple] = None                                # the compiled table (offsets, ids, bias)
    sot_tail: Optional[int] = None
    prefix_len: Optional[int] = None
    sampling: Optional[Tuple[int, float, float]] = None         # (top_k, top_p, min_p)
    logprobs: Optional[int] = None                              # top_n of the per-token log-probabilities


class WhisperModel:
    temperature_fallback = False      # opt-in (the constructor's keyword)
    beam_search = False               # opt-in too
    decoding_options = False          # and so are upstream's remaining per-call decoding options
    repetition_control = False        # and repetition_penalty / no_repeat_ngram_size
    contextual_bias = False           # and sequence_bias / bad_words_ids / hotwords
    truncated_sampling = False        # and top_k / top_p / min_p
    token_logprobs = False            # and per-token log-probabilities with top-N alternatives (a property of the instance: buffers)
    cross_fp8 = False                 # the FP8 encoder-output stream (a property of the instance; the library's state after finalize)
    audio_ctx = None                  # the reduced audio context: None (off), "auto" or the positions every window keeps
    _staged_frames = None             # content frames of the windows `log_mel` staged last (None: `set_mel`, or nothing staged)
    last_audio_ctx: Sequence[int] = ()  # the contexts of the windows of the last `encode`

    def __init__(self, dims: WhisperDims, state_dict: Dict[str, torch.Tensor], max_batch: int = 8,
                 device: int = 0, rules: Optional[DecodeRules] = None, tokenizer=None,
                 ctx: Optional[_lib.Context] = None, max_audio_seconds: float = 30.0,
                 share_encoder_scratch_with: Optional["WhisperModel"] = None, word_alignment: bool = False,
                 alignment_heads: Optional[Sequence[Sequence[int]]] = None, word_probabilities: bool = False,
                 temperature_fallback: bool = False, beam_search: bool = False, decoding_options: bool = False,
                 repetition_control: bool = False, contextual_bias: bool = False, truncated_sampling: bool = False,
                 cross_fp8: bool = False, audio_ctx=None, token_logprobs: bool = False):
        """token_logprobs (default False: the instance allocates nothing more, launches what it always launched and keeps its bits; a
        `logprobs` that is not None is then REFUSED with ValueError -- a caller who asks must not silently get nothing): with it, the
        instance holds three buffers beside its token histories and `decode`, `decode_rows`, `transcribe`, `transcribe_batch` take
        `logprobs=n`, n an int in [0, 8]: every record (every segment) gains `token_logprobs`, the log-probability of each sampled
        token under the row the step drew from -- after every filter, not divided by the temperature, not truncated; the eot's entry
        last when the row ended by eot; their fp32 sum in step order is `sum_logprob`, bit for bit -- and, for n > 0, `top_logprobs`,
        per step the n most probable allowed (id, logprob) pairs in descending order, the lower id first among equals (the rule is
        this project's, include/ccx.h ccx_decode_logprob_options; parity unpinned).  Formed inside the select kernel
        (csrc/dec_logprobs.h); tokens, sum_logprob and no_speech_prob keep their bits.  Not available to beam search.
        audio_ctx (default None: the instance allocates nothing more, launches what it always launched and keeps its bits): "auto" or
        an integer in [64, n_audio_ctx] builds the instance for a REDUCED AUDIO CONTEXT -- `encode` keeps only the first n encoder
        positions of a window (n = `audio_ctx.positions_for(content frames)` per window under "auto", the integer otherwise), every
        encoder layer attends over those only, and the cross attention of every decode reads those n rows (every decode then takes
        the "xa_stream" path, whatever its size).  `encode(audio_ctx=)`, `transcribe(audio_ctx=)` override it per call ("full": the
        whole window).  This is NOT upstream's arithmetic: Whisper was trained on zero-padded 30 s windows, and what fewer positions
        cost in transcript quality on real checkpoints is NOT measured: that is why it is off by default.  Refused with CcxError,
        before anything is allocated, under the rule of cross_fp8 (the 1280-wide family, unequal widths, CCX_CROSS_X=0); a value
        that is neither raises ValueError.  Where the keyword is absent, CCX_AUDIO_CTX (`auto` or an integer) in the environment
        sets it on instances that can run it -- for A/B runs of an unmodified bench.py only.
        cross_fp8 (default False: the instance allocates nothing more, runs no other kernel and keeps its bits): with it, the
        instance keeps a block-scaled FP8 image of the encoder output (32-feature blocks, E4M3 codes, power-of-two scales; the rule
        is in include/ccx.h) and the cross attention of decodes on the "xa_stream" path reads it instead of the bf16 rows.  `encode`
        then leaves the DEQUANTISED encoder output with the instance -- what `encode(return_xa=True)` returns and every decode path
        and `align` read.  A property of the instance, like max_batch; refused with CcxError, before anything is allocated, for dims
        without that path (the 1280-wide family, unequal widths) or under CCX_CROSS_X=0.  `self.cross_fp8` is the library's state.
        What the quantisation costs in transcript quality on real checkpoints is NOT measured: that is why it is off by default.
        truncated_sampling (default False: a `top_k`, `top_p` or `min_p` off its default 0, 1.0, 0.0 is REFUSED with ValueError --
        a caller who asks for a cut must not get the whole vocabulary): with it, `transcribe` / `transcribe_batch` and `decode`,
        `decode_rows` honour them (Hugging Face's names and order: temperature, top-k, top-p, min-p; the rule is this project's,
        include/ccx.h ccx_decode_sampling_options; parity unpinned) on every decode at temperature > 0 -- the warm rounds of a
        fallback walk, best_of candidates included; a temperature-0 round, greedy or beam, is bit-identical to one without them.  The
        cut is computed inside the select kernel (csrc/dec_truncate.h) after every filter; the draw is the untruncated sampler's
        Gumbel-max over the same noise, restricted to the kept ids; sum_logprob stays the log-probability under the untruncated row.
        contextual_bias (default False: `sequence_bias`, `bad_words_ids`, `hotwords` and `hotword_boost` are accepted and ignored):
        with it, `transcribe` / `transcribe_batch` and `decode`, `decode_rows`, `decode_beam` honour them (Hugging Face's names and
        forms for the first two, faster-whisper's name for hotwords; the rule is this project's, include/ccx.h
        ccx_decode_bias_options; parity unpinned): a bias is added to the logit of the last id of a sequence whenever the tokens THIS
        decode has just sampled end in the ids before it (no prompt, SOT sequence or prefix; a target >= eot is refused); a bad word is
        a bias of -inf; a hotword boosts its first token always and each next one once the ones before it were sampled
        (`decode_bias.compile_bias_table`).  One kernel more per step (csrc/dec_bias.hip) and only on calls that give a table.
        repetition_control (default False: `repetition_penalty` and `no_repeat_ngram_size` are accepted and ignored): with it,
        `transcribe` / `transcribe_batch` and `decode`, `decode_rows`, `decode_beam` honour them (the names CTranslate2 /
        faster-whisper and Hugging Face use; the rule is this project's, include/ccx.h ccx_decode_history_options; parity unpinned):
        the logit of every text id a window has sampled so far is divided (> 0) or multiplied (<= 0) by repetition_penalty, and an id
        that would complete an n-gram the window already holds is banned -- over the tokens THIS decode sampled only (no prompt, SOT
        sequence or prefix), ids >= eot exempt.  One kernel more per step (csrc/dec_history.hip) and only on calls that set a value:
        with the defaults 1.0 and 0 a call is what it is without the opt-in.
        decoding_options (default False: `without_timestamps`, `prefix`, `suppress_blank`, `suppress_tokens`, `max_initial_timestamp`,
        `sample_len`, `clip_timestamps` and `carry_initial_prompt` are accepted and ignored, as before): with it, `transcribe` /
        `transcribe_batch` honour them [UPSTREAM-RECALL: decoding.py::DecodingOptions, transcribe.py; parity unpinned] -- see
        `transcribe_batch`; `decode`, `decode_rows` and `decode_beam` take the ones a single decode reads.
        beam_search (default False: `beam_size`, `patience` and `length_penalty` are accepted and ignored, as before): with it,
        `transcribe` / `transcribe_batch` honour them [UPSTREAM-RECALL: decoding.py::BeamSearchDecoder, transcribe.py::decode_with_fallback;
        parity unpinned] -- a temperature-0 round with `beam_size` set decodes every window by beam search on the GPU (`decode_beam`),
        `length_penalty` enters the ranker of beam and best_of rounds alike.
        temperature_fallback (default False: a tuple or list temperature raises, `best_of` and `compression_ratio_threshold` are
        ignored, as before): with it, `transcribe` / `transcribe_batch` take a temperature schedule, `compression_ratio_threshold` and
        `best_of` and decode a window again, warmer, while it is too repetitive or too improbable (clearconverse_amd/fallback.py) --
        only the failing windows, over a row -> window map (`decode_rows`), nothing encoded again.
        word_alignment (default False: nothing below runs, `transcribe(word_timestamps=True)` has no effect, as before): with it,
        `transcribe(word_timestamps=True)` aligns the words of every window by cross-attention DTW on the GPU (`align`), attaches
        `words` to the segments and moves `seek` by upstream's last-word rule (WindowLoop.advance).
        alignment_heads: (layer, head) pairs whose cross attention is aligned.  Default: every head of the upper half of the decoder
        layers -- upstream's fallback for a model without a head table [UPSTREAM-RECALL: model.py, `all_heads[n_text_layer // 2:] =
        True`].  A group of windows is aligned as one batch (windows without text go in as [sot, no_timestamps, eot]), so
        max_batch must not exceed the sequences the cross-attention K / V caches hold (80 on the instances that read the encoder
        output directly): a larger group fails in `transcribe` with the library's message.  small.en's published table (`_ALIGNMENT_HEADS`) is not on disk and is not restated here; pass its pairs to use it.
        word_probabilities (default False; needs word_alignment): every word also carries `probability`, the mean of its tokens'
        softmax probabilities over the text ids [UPSTREAM-RECALL: timing.py::find_alignment] -- one more small kernel per step of
        the alignment pass -- and `transcribe(hallucination_silence_threshold=)` is honoured, which is built on them."""
        if word_probabilities and not word_alignment:
            raise _lib.CcxError("word_probabilities=True needs word_alignment=True: the probabilities come out of the alignment pass")
        if cross_fp8:
            why = cross_fp8_refusal(dims)
            if why is not None:
                raise _lib.CcxError(f"cross_fp8=True refused: {why}")
        if audio_ctx is not None:
            audio_ctx = audio_ctx_policy.parse_setting(audio_ctx, dims.n_audio_ctx)
            why = audio_ctx_refusal(dims)
            if why is not None:
                raise _lib.CcxError(f"audio_ctx={audio_ctx!r} refused: {why}")
        elif audio_ctx_refusal(dims) is None:       # the environment: ignored, not refused, where the instance cannot run it
            audio_ctx = audio_ctx_policy.from_environment(dims.n_audio_ctx)
        if not torch.cuda.is_available():
            raise _lib.CcxError("WhisperModel needs a ROCm GPU: the HIP path has no CPU fallback")
        self.dims = dims
        self.audio_ctx = audio_ctx
        self.max_batch = int(max_batch)
        self.device = torch.device("cuda", device)
        self.ctx = ctx or _lib.Context(device)
        self.lib = self.ctx.lib
        self.rules = rules or DecodeRules.for_dims(dims)     # model.py::Whisper.is_multilingual: the vocabulary size decides
        self.tokenizer = tokenizer or get_tokenizer(rules=self.rules)
        h = C.c_void_p()
        cd = _lib.WhisperDims(**asdict(dims))
        self.ctx.check(self.lib.ccx_whisper_create(self.ctx.handle, C.byref(cd), self.max_batch, C.byref(h)),
                       "ccx_whisper_create")
        self.handle = h
        self.max_audio_seconds = float(max_audio_seconds)
        self.sample_seed, self._sample_calls = 0, 0     # temperature > 0: Philox seed and per-call counter
        self.last_cross_path = None
        self.prefix_len = 0     # what the library starts with; `set_prefix_len` keeps it
        self.word_alignment = bool(word_alignment)
        self.word_probabilities = bool(word_probabilities)
        self.temperature_fallback = bool(temperature_fallback)
        self.beam_search = bool(beam_search)
        self.decoding_options = bool(decoding_options)
        self.repetition_control = bool(repetition_control)
        self.contextual_bias = bool(contextual_bias)
        self.truncated_sampling = bool(truncated_sampling)
        self.token_logprobs = bool(token_logprobs)
        if alignment_heads is None:
            alignment_heads = [(l, h) for l in range(dims.n_text_layer // 2, dims.n_text_layer) for h in range(dims.n_text_head)]
        self.alignment_heads = [(int(l), int(h)) for l, h in alignment_heads]
        self.ctx.check(self.lib.ccx_whisper_set_max_audio(self.handle, self.max_audio_seconds), "ccx_whisper_set_max_audio")
        if cross_fp8:
            self.ctx.check(self.lib.ccx_whisper_set_cross_fp8(self.handle, 1), "ccx_whisper_set_cross_fp8")
        if self.audio_ctx is not None:
            self.ctx.check(self.lib.ccx_whisper_set_audio_ctx(self.handle, 1), "ccx_whisper_set_audio_ctx")
        if self.token_logprobs:
            self.ctx.check(self.lib.ccx_whisper_set_token_logprobs(self.handle, 1), "ccx_whisper_set_token_logprobs")
        # log-mel / encoder workspaces of another instance (kept alive here): only for instances whose log_mel / encode calls
        # are ordered on one stream, as in BatchPipeline.run_pinned_pipelined (include/ccx.h)
        self._scratch_donor = share_encoder_scratch_with
        if share_encoder_scratch_with is not None:
            self.ctx.check(self.lib.ccx_whisper_share_encoder_scratch(self.handle, share_encoder_scratch_with.handle),
                           "ccx_whisper_share_encoder_scratch")
        self._load(state_dict)
        self.set_rules(self.rules)

    # ------------------------------------------------------------------ weights / rules
    def _load(self, sd: Dict[str, torch.Tensor]):
        tensors = dict(sd)
        tensors["mel_filters"] = torch.from_numpy(mel_filterbank(self.dims.n_mels))
        for name, t in tensors.items():
            t = t.detach().to("cpu")
            if t.dtype == torch.float32:
                code = 0
            elif t.dtype == torch.bfloat16:
                code = 1
            elif t.dtype == torch.float16:
                code = 2
            else:
                t, code = t.float(), 0
            t = t.contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            self.ctx.check(self.lib.ccx_whisper_set_tensor(self.handle, name.encode(), t.data_ptr(), code, t.dim(), shape),
                           f"set_tensor({name})")
        self.ctx.check(self.lib.ccx_whisper_finalize(self.handle), "ccx_whisper_finalize")
        self.cross_fp8 = bool(self.lib.ccx_whisper_cross_fp8(self.handle))      # CCX_CROSS_FP8 at finalize included

    def set_rules(self, rules: DecodeRules):
        sup = (C.c_int * len(rules.suppress))(*[int(x) for x in rules.suppress])
        r = _lib.DecodeRules(rules.eot, rules.sot, rules.sot_prev, rules.no_speech, rules.no_timestamps,
                             rules.timestamp_begin, rules.blank, rules.max_initial_timestamp_index,
                             len(rules.suppress), sup)
        self.ctx.check(self.lib.ccx_whisper_set_rules(self.handle, C.byref(r)), "ccx_whisper_set_rules")
        self.rules = rules
        # tokens of the SOT sequence behind sot: the no-speech probability is read at sot's position (decoding.py `sot_index`)
        self.set_sot_tail(len(rules.sot_sequence()) - 1)

    def set_decode_options(self, without_timestamps: bool = False, suppress_blank: bool = True,
                           suppress: Optional[Sequence[int]] = None, max_initial_timestamp_index: int = -2):
        """ccx_whisper_set_decode_options (sticky, like the rules; `set_rules` resets it): without_timestamps -- the select / beam
        kernels without ApplyTimestampRules (the prompts then end in <|notimestamps|>: the caller's part); suppress -- the id list that
        replaces the rules' (None: the rules'; []: nothing suppressed); max_initial_timestamp_index -- -2 the rules' own, -1 off."""
        sup = None if suppress is None else (C.c_int * max(len(suppress), 1))(*[int(x) for x in suppress])
        o = _lib.DecodeOptions(int(bool(without_timestamps)), int(bool(suppress_blank)), int(max_initial_timestamp_index),
                               0 if suppress is None else len(suppress), sup)
        self.ctx.check(self.lib.ccx_whisper_set_decode_options(self.handle, C.byref(o)), "ccx_whisper_set_decode_options")

    def graph_count(self, options_only: bool = False) -> int:
        """captured step graphs the instance holds (ccx_whisper_graph_count)"""
        return int(self.lib.ccx_whisper_graph_count(self.handle, int(bool(options_only))))

    def reset_decode_options(self):
        self.ctx.check(self.lib.ccx_whisper_set_decode_options(self.handle, None), "ccx_whisper_set_decode_options")

    @staticmethod
    def check_history_options(repetition_penalty: float, no_repeat_ngram_size: int):
        """the ranges ccx_whisper_set_history_options checks -> (float, int), or ValueError naming the argument"""
        try:
            p = float(repetition_penalty)
        except (TypeError, ValueError) as e:
            raise ValueError(f"repetition_penalty = {repetition_penalty!r} must be a finite number > 0") from e
        if not (1.5e-45 <= p <= 3.4028234e38):       # what a C float holds as a finite number > 0
            raise ValueError(f"repetition_penalty = {repetition_penalty!r} must be a finite number > 0")
        n = no_repeat_ngram_size
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or n > 2 ** 31 - 1:
            raise ValueError(f"no_repeat_ngram_size = {no_repeat_ngram_size!r} must be an integer >= 0")
        return p, int(n)

    def set_history_options(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """ccx_whisper_set_history_options (sticky, like the rules; `set_rules` resets it); (1.0, 0) is the default decode"""
        p, n = self.check_history_options(repetition_penalty, no_repeat_ngram_size)
        o = _lib.DecodeHistoryOptions(p, n)
        self.ctx.check(self.lib.ccx_whisper_set_history_options(self.handle, C.byref(o)), "ccx_whisper_set_history_options")

    def reset_history_options(self):
        self.ctx.check(self.lib.ccx_whisper_set_history_options(self.handle, None), "ccx_whisper_set_history_options")

    def history_graph_count(self) -> int:
        """captured step graphs of history plans (ccx_whisper_history_graph_count)"""
        return int(self.lib.ccx_whisper_history_graph_count(self.handle))

    def compile_bias_options(self, sequence_bias=None, bad_words_ids=None, hotwords=None, hotword_boost=None):
        """`decode_bias.compile_bias_table` with this model's tokenizer, eot and vocabulary -> (offsets, ids, bias)"""
        from .decode_bias import compile_bias_table
        return compile_bias_table(sequence_bias, bad_words_ids, hotwords, hotword_boost, encode=self.tokenizer.encode,
                                  eot=self.rules.eot, n_vocab=self.dims.n_vocab)

    def set_bias_options(self, sequence_bias=None, bad_words_ids=None, hotwords=None, hotword_boost=None):
        """ccx_whisper_set_bias_options (sticky, like the rules; `set_rules` resets it); nothing given: off, the default decode"""
        self._set_bias_table(*self.compile_bias_options(sequence_bias, bad_words_ids, hotwords, hotword_boost))

    def _set_bias_table(self, offsets, ids, bias):
        """a compiled table (`compile_bias_options`) -> ccx_whisper_set_bias_options, which copies the arrays"""
        o = _lib.DecodeBiasOptions(len(bias), offsets.ctypes.data_as(C.POINTER(C.c_int)), ids.ctypes.data_as(C.POINTER(C.c_int)),
                                   bias.ctypes.data_as(C.POINTER(C.c_float)))
        self.ctx.check(self.lib.ccx_whisper_set_bias_options(self.handle, C.byref(o)), "ccx_whisper_set_bias_options")

    def reset_bias_options(self):
        self.ctx.check(self.lib.ccx_whisper_set_bias_options(self.handle, None), "ccx_whisper_set_bias_options")

    def bias_graph_count(self) -> int:
        """captured step graphs of bias plans (ccx_whisper_bias_graph_count)"""
        return int(self.lib.ccx_whisper_bias_graph_count(self.handle))

    @staticmethod
    def check_sampling_options(top_k: int, top_p: float, min_p: float):
        """the ranges ccx_whisper_set_sampling_options checks -> (int, float, float), or ValueError naming the argument"""
        k = top_k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0 or k > 2 ** 31 - 1:
            raise ValueError(f"top_k = {top_k!r} must be an integer >= 0")
        try:
            p = float(np.float32(top_p))       # the value the library will see
        except (TypeError, ValueError) as e:
            raise ValueError(f"top_p = {top_p!r} must be a number in (0, 1]") from e
        if not (0.0 < p <= 1.0):
            raise ValueError(f"top_p = {top_p!r} must be a number in (0, 1]")
        try:
            m = float(np.float32(min_p))
        except (TypeError, ValueError) as e:
            raise ValueError(f"min_p = {min_p!r} must be a number in [0, 1]") from e
        if not (0.0 <= m <= 1.0):
            raise ValueError(f"min_p = {min_p!r} must be a number in [0, 1]")
        return int(k), p, m

    def set_sampling_options(self, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """ccx_whisper_set_sampling_options (sticky, like the rules; `set_rules` resets it); (0, 1.0, 0.0) is the default decode"""
        k, p, m = self.check_sampling_options(top_k, top_p, min_p)
        o = _lib.DecodeSamplingOptions(k, p, m)
        self.ctx.check(self.lib.ccx_whisper_set_sampling_options(self.handle, C.byref(o)), "ccx_whisper_set_sampling_options")

    def reset_sampling_options(self):
        self.ctx.check(self.lib.ccx_whisper_set_sampling_options(self.handle, None), "ccx_whisper_set_sampling_options")

    def sampling_graph_count(self) -> int:
        """captured step graphs of truncation plans (ccx_whisper_sampling_graph_count)"""
        return int(self.lib.ccx_whisper_sampling_graph_count(self.handle))

    def set_prefix_len(self, n_prefix: int):
        """prompt tokens behind the SOT sequence (a decode with a prefix): ccx_whisper_set_prefix_len"""
        self.ctx.check(self.lib.ccx_whisper_set_prefix_len(self.handle, int(n_prefix)), "ccx_whisper_set_prefix_len")
        self.prefix_len = int(n_prefix)

    def set_sot_tail(self, n_tail: int):
        self.ctx.check(self.lib.ccx_whisper_set_sot_tail(self.handle, int(n_tail)), "ccx_whisper_set_sot_tail")
        self.sot_tail = int(n_tail)

    # ------------------------------------------------------------------ a call's settings: resolved first, then set in one scope
    def _bias_setting(self, sequence_bias, bad_words_ids, hotwords, hotword_boost):
        """the call's compiled bias table; None without the opt-in, with none of the three given, or for an empty table"""
        if not self.contextual_bias or (sequence_bias is None and bad_words_ids is None and hotwords is None):
            return None
        table = self.compile_bias_options(sequence_bias, bad_words_ids, hotwords, hotword_boost)
        return table if len(table[2]) else None

    def _history_setting(self, repetition_penalty, no_repeat_ngram_size):
        """the call's checked (repetition_penalty, no_repeat_ngram_size); None without the opt-in or for the defaults (1.0, 0)"""
        if not self.repetition_control:
            return None
        history = self.check_history_options(repetition_penalty, no_repeat_ngram_size)
        return None if history == (1.0, 0) else history

    def _sampling_setting(self, top_k, top_p, min_p):
        """the call's checked (top_k, top_p, min_p); None for the defaults (0, 1.0, 0.0).  Anything else is refused without the
        opt-in: ValueError, like a value outside its range."""
        sampling = self.check_sampling_options(top_k, top_p, min_p)
        if sampling == (0, 1.0, 0.0):
            return None
        if not self.truncated_sampling:
            raise ValueError("top_k / top_p / min_p need a model built with truncated_sampling=True")
        return sampling

    def set_logprob_options(self, top_n: int):
        """ccx_whisper_set_logprob_options (sticky, like the rules; `set_rules` resets it): record every sampled token's
        log-probability and its top_n alternatives"""
        o = _lib.DecodeLogprobOptions(int(top_n))
        self.ctx.check(self.lib.ccx_whisper_set_logprob_options(self.handle, C.byref(o)), "ccx_whisper_set_logprob_options")

    def reset_logprob_options(self):
        self.ctx.check(self.lib.ccx_whisper_set_logprob_options(self.handle, None), "ccx_whisper_set_logprob_options")

    def logprob_graph_count(self) -> int:
        """captured step graphs of log-probability plans (ccx_whisper_logprob_graph_count)"""
        return int(self.lib.ccx_whisper_logprob_graph_count(self.handle))

    def _logprob_setting(self, logprobs, beam_size=None):
        """the call's checked top_n; None for None.  Anything else is refused with ValueError: without the opt-in, outside [0, 8],
        not an int (a bool is not one), or together with beam search."""
        if logprobs is None:
            return None
        if not self.token_logprobs:
            raise ValueError("logprobs needs a model built with token_logprobs=True")
        if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or not 0 <= int(logprobs) <= _lib.LOGPROB_MAX_TOP:
            raise ValueError(f"logprobs = {logprobs!r} must be None or an int in [0, {_lib.LOGPROB_MAX_TOP}]")
        if beam_size is not None:
            raise ValueError("logprobs is not available to beam search (beam_size): its rows are rewritten every step")
        return int(logprobs)

    def _with_logprobs(self, records: List[dict], n: Optional[int], sample_len: int) -> List[dict]:
        """the records of the decode that just ran, with `token_logprobs` (and, n > 0, `top_logprobs`) of its rows
        (ccx_whisper_token_logprobs): one entry per sampled step -- the row's tokens, and the eot's where the fetch holds one"""
        if n is None:
            return records
        R = len(records)
        lp = np.full((R, sample_len), np.nan, dtype=np.float32)
        tid = np.full((R, sample_len, n), -1, dtype=np.int32)
        tlp = np.full((R, sample_len, n), -np.inf, dtype=np.float32)
        self.ctx.check(self.lib.ccx_whisper_token_logprobs(
            self.handle, R, int(sample_len), lp.ctypes.data_as(C.POINTER(C.c_float)), n,
            tid.ctypes.data_as(C.POINTER(C.c_int)) if n else None, tlp.ctypes.data_as(C.POINTER(C.c_float)) if n else None,
            _lib.current_stream_ptr()), "ccx_whisper_token_logprobs")
        for b, r in enumerate(records):
            # a row with fewer tokens than sample_len ended by eot, and that step has an entry too
            steps = min(len(r["tokens"]) + 1, sample_len)
            r["token_logprobs"] = lp[b, :steps].tolist()
            if n:
                r["top_logprobs"] = [[(int(i), float(v)) for i, v in zip(tid[b, t], tlp[b, t]) if i >= 0] for t in range(steps)]
        return records

    def _decode_settings(self, bias_args, repetition_penalty, no_repeat_ngram_size, decoding: dict,
                         top_k=0, top_p=1.0, min_p=0.0, logprobs=None) -> CallSettings:
        """What a single decode sets, every refusal made before anything is set: the bias compile (ValueError), the history ranges
        (ValueError), then the decoding keys (TypeError, with or without the opt-in) and `resolve` (CcxError).  **decoding is the
        subset a single decode takes: without_timestamps, suppress_blank, suppress_tokens, max_initial_timestamp."""
        bias = self._bias_setting(*bias_args)
        sampling = self._sampling_setting(top_k, top_p, min_p)
        logprobs = self._logprob_setting(logprobs, decoding.get("beam_size"))
        history = None
        if repetition_penalty != 1.0 or no_repeat_ngram_size != 0:
            history = self._history_setting(repetition_penalty, no_repeat_ngram_size)
        unknown = set(decoding) - {"without_timestamps", "suppress_blank", "suppress_tokens", "max_initial_timestamp"}
        if unknown:
            raise TypeError(f"unexpected decoding option(s): {sorted(unknown)}")
        options = None
        if self.decoding_options and decoding:
            try:
                options = decoding_options.resolve(self.rules, **decoding)
            except ValueError as e:
                raise _lib.CcxError(str(e)) from e
        return CallSettings(options, history, bias, sampling=sampling, logprobs=logprobs)

    def _transcribe_settings(self, n: int, hallucination_silence_threshold, without_timestamps, prefixes, suppress_blank,
                             suppress_tokens, max_initial_timestamp, sample_len, carry_initial_prompt, repetition_penalty,
                             no_repeat_ngram_size, sequence_bias, bad_words_ids, hotwords, hotword_boost, top_k=0, top_p=1.0,
                             min_p=0.0):
        """What a `transcribe_batch` of n clips sets, every refusal made before anything is set -> (CallSettings, the resolved
        decoding options, every clip's prefix tokens); the last two are None without the decoding_options opt-in."""
        bias = self._bias_setting(sequence_bias, bad_words_ids, hotwords, hotword_boost)
        history = self._history_setting(repetition_penalty, no_repeat_ngram_size)
        sampling = self._sampling_setting(top_k, top_p, min_p)
        if not self.decoding_options:
            return CallSettings(history=history, bias=bias, sampling=sampling), None, None
        try:
            opt = decoding_options.resolve(self.rules, without_timestamps, suppress_blank, suppress_tokens, max_initial_timestamp,
                                           sample_len, carry_initial_prompt)
        except ValueError as e:
            raise _lib.CcxError(str(e)) from e
        if opt.without_timestamps and hallucination_silence_threshold is not None:
            raise _lib.CcxError("without_timestamps=True cannot be combined with hallucination_silence_threshold: that rule is "
                                "defined on segment timestamps")
        prefixes = list(prefixes) if prefixes is not None else [None] * n
        if len(prefixes) != n:
            raise _lib.CcxError("transcribe_batch: one prefix (or None) per clip")
        prefix_toks = [decoding_options.prefix_tokens(self.tokenizer, p, self.dims.n_text_ctx, opt.sample_len) for p in prefixes]
        if len(set(len(t) for t in prefix_toks)) > 1:
            raise _lib.CcxError("transcribe_batch: the prefixes of one call must hold equally many tokens (transcribe the clips "
                                "one by one otherwise)")
        # the SOT tail the call's prompts carry (WindowLoop.sot_tail: one length per model) and the length of their prefix
        tail = len(self.rules.sot_sequence()) - 1 + int(opt.without_timestamps)
        n_prefix = len(prefix_toks[0]) if n > 0 else 0
        return CallSettings(None if opt.device_default(self.rules) else opt, history, bias,
                            tail if n > 0 and tail != self.sot_tail else None, n_prefix or None, sampling), opt, prefix_toks

    @contextlib.contextmanager
    def _settings(self, s: CallSettings):
        """The call's settings on the instance while the body runs, for however many decodes: applied once, in one order (options, SOT
        tail, prefix length, history, bias, sampling, logprobs), and taken back in reverse -- exactly those that were applied, also when a later setter
        or the body raises.  The SOT tail and the prefix length go back to what the instance held before."""
        with contextlib.ExitStack() as undo:
            if s.options is not None:
                o = s.options
                self.set_decode_options(o.without_timestamps, o.suppress_blank, None if o.suppress_default else o.suppress,
                                        o.max_initial_timestamp_index)
                undo.callback(self.reset_decode_options)
            if s.sot_tail is not None:
                tail0 = self.sot_tail
                self.set_sot_tail(s.sot_tail)
                undo.callback(self.set_sot_tail, tail0)
            if s.prefix_len is not None:
                prefix0 = self.prefix_len
                self.set_prefix_len(s.prefix_len)
                undo.callback(self.set_prefix_len, prefix0)
            if s.history is not None:
                self.set_history_options(*s.history)
                undo.callback(self.reset_history_options)
            if s.bias is not None:
                self._set_bias_table(*s.bias)
                undo.callback(self.reset_bias_options)
            if s.sampling is not None:
                self.set_sampling_options(*s.sampling)
                undo.callback(self.reset_sampling_options)
            if s.logprobs is not None:
                self.set_logprob_options(s.logprobs)
                undo.callback(self.reset_logprob_options)
            yield

    @contextlib.contextmanager
    def _logprobs_of_call(self, n: Optional[int]):
        """while the body runs, `_call_decode` fetches the lists of every decode (n: the top_n `_settings` has set; None: nothing)"""
        self._call_logprobs = n
        try:
            yield
        finally:
            self._call_logprobs = None

    def _pack_prompts(self, seqs: Sequence[Sequence[int]]):
        """-> (ids [n, max_len] int32, padded with eot; lens [n] int32; max_len)"""
        max_len = max(len(p) for p in seqs)
        ids = np.full((len(seqs), max_len), self.rules.eot, dtype=np.int32)
        lens = np.zeros(len(seqs), dtype=np.int32)
        for b, p in enumerate(seqs):
            ids[b, :len(p)] = p
            lens[b] = len(p)
        return ids, lens, max_len

    def _records(self, toks, ntok, slp, nsp) -> List[dict]:
        """One record per row of a decode's outputs (toks [n, sample_len]; ntok, slp, nsp [n]).  Which cross-attention formulation the
        decode ran (include/ccx.h: ccx_whisper_last_cross_path) is read here and kept in every record."""
        self.last_cross_path = CROSS_PATHS.get(int(self.lib.ccx_whisper_last_cross_path(self.handle)), "unknown")
        return [dict(tokens=toks[b, :ntok[b]].tolist(), sum_logprob=float(slp[b]),
                     avg_logprob=float(slp[b]) / (int(ntok[b]) + 1), no_speech_prob=float(nsp[b]),
                     cross_path=self.last_cross_path) for b in range(len(ntok))]

    def detect_language(self, B: int):
        """whisper.decoding.detect_language for the B currently encoded windows (ccx_whisper_detect_language): one decoder step
        on [sot], softmax over the language tokens.  -> (codes [B], probs [B, num_languages] float32 numpy, in LANGUAGES order).
        A decode of the same windows afterwards is what it is without this call."""
        if not self.rules.is_multilingual:
            raise _lib.CcxError("detect_language needs a multilingual model (this one's vocabulary is English-only)")
        n = self.rules.num_languages
        tok = np.zeros(B, dtype=np.int32)
        probs = np.zeros((B, n), dtype=np.float32)
        self.ctx.check(self.lib.ccx_whisper_detect_language(
            self.handle, int(B), self.rules.language_begin, n, tok.ctypes.data_as(C.POINTER(C.c_int32)),
            probs.ctypes.data_as(C.POINTER(C.c_float)), _lib.current_stream_ptr()), "ccx_whisper_detect_language")
        return [self.rules.language_code(t) for t in tok], probs

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ccx_whisper_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ stage entry points
    def log_mel(self, audio: torch.Tensor, n_samples: Sequence[int], seek: Optional[Sequence[int]] = None,
                return_mel: bool = False, max_frames: Optional[Sequence[int]] = None) -> Optional[torch.Tensor]:
        """audio: [B, stride] f32 on the GPU.  Stages the conv-stem input inside the model.  max_frames (ccx_whisper_logmel_ex): a
        cap on every window's frames -- zeros behind it, as pad_or_trim leaves a cropped mel."""
        B = audio.shape[0]
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.is_contiguous()
        # every staged window's content frames (the library's segment_size): what `encode` sizes a reduced audio context from
        self._staged_frames = [min(max(int(n_samples[b]) // HOP - (int(seek[b]) if seek is not None else 0), 0), N_FRAMES) for b in range(B)]
        if max_frames is not None:
            self._staged_frames = [min(f, int(m)) for f, m in zip(self._staged_frames, max_frames)]
        ns = (C.c_int * B)(*[int(x) for x in n_samples])
        sk = (C.c_int * B)(*[int(x) for x in seek]) if seek is not None else None
        mel = torch.empty(B, self.dims.n_mels, N_FRAMES, device=self.device, dtype=torch.float32) if return_mel else None
        if max_frames is not None:
            mf = (C.c_int * B)(*[int(x) for x in max_frames])
            self.ctx.check(self.lib.ccx_whisper_logmel_ex(self.handle, audio.data_ptr(), audio.shape[1], ns, sk, mf, B,
                                                          _lib.ptr(mel), _lib.current_stream_ptr()), "ccx_whisper_logmel_ex")
            return mel
        self.ctx.check(self.lib.ccx_whisper_logmel(self.handle, audio.data_ptr(), audio.shape[1], ns, sk, B,
                                                   _lib.ptr(mel), _lib.current_stream_ptr()), "ccx_whisper_logmel")
        return mel

    def set_mel(self, mel: torch.Tensor):
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous() and mel.shape[1:] == (self.dims.n_mels, N_FRAMES)
        self.ctx.check(self.lib.ccx_whisper_set_mel(self.handle, mel.data_ptr(), mel.shape[0], _lib.current_stream_ptr()),
                       "ccx_whisper_set_mel")
        self._staged_frames = None      # a ready mel says nothing about its content: the whole window

    def _window_contexts(self, B: int, audio_ctx) -> Optional[List[int]]:
        """The audio context of each of the B staged windows, or None for the plain encode: audio_ctx None applies the instance's policy
        (the whole window when it is off, or after `set_mel`), "full" the whole window, "auto" / an int that setting, a list explicit
        values.  Anything but None / "full" needs an instance built with `audio_ctx`."""
        S = self.dims.n_audio_ctx
        if isinstance(audio_ctx, str) and audio_ctx.strip().lower() == "full":
            return None
        if audio_ctx is None:
            setting = self.audio_ctx
        elif self.audio_ctx is None:
            raise ValueError(f"audio_ctx={audio_ctx!r}: the instance was not built for a reduced audio context (WhisperModel(audio_ctx=...))")
        elif isinstance(audio_ctx, (list, tuple, np.ndarray)):
            vals = [int(v) for v in audio_ctx]
            if len(vals) != B or any(not audio_ctx_policy.FLOOR <= v <= S for v in vals):
                raise ValueError(f"audio_ctx={vals}: one value in [{audio_ctx_policy.FLOOR}, {S}] per window ({B}) expected")
            return vals
        else:
            setting = audio_ctx_policy.parse_setting(audio_ctx, S)
        if setting is None or (setting == "auto" and self._staged_frames is None):
            return None
        if setting == "auto" and len(self._staged_frames) < B:
            raise _lib.CcxError(f"encode: {B} windows asked for, `log_mel` staged {len(self._staged_frames)}")
        return [audio_ctx_policy.context_of(setting, self._staged_frames[b] if setting == "auto" else 0, S) for b in range(B)]

    def encode(self, B: int, return_xa: bool = False, audio_ctx=None) -> Optional[torch.Tensor]:
        """AudioEncoder.forward for the B staged windows.  audio_ctx (instances built with `audio_ctx` only): None -- the instance's
        policy, sized from the content frames `log_mel` staged (the whole window after `set_mel`); "full"; "auto"; an int; or a list of
        B explicit contexts.  `self.last_audio_ctx` holds what the windows were encoded with.  return_xa: [B, n_audio_ctx, D]; the rows
        of window b at or beyond its context are unspecified."""
        xa = torch.empty(B, self.dims.n_audio_ctx, self.dims.n_audio_state, device=self.device, dtype=torch.float32) if return_xa else None
        ctxs = self._window_contexts(B, audio_ctx)
        if ctxs is None:
            self.ctx.check(self.lib.ccx_whisper_encode(self.handle, B, _lib.ptr(xa), _lib.current_stream_ptr()), "ccx_whisper_encode")
            self.last_audio_ctx = [self.dims.n_audio_ctx] * B
        else:
            n = (C.c_int * B)(*ctxs)
            self.ctx.check(self.lib.ccx_whisper_encode_ctx(self.handle, B, n, _lib.ptr(xa), _lib.current_stream_ptr()), "ccx_whisper_encode_ctx")
            self.last_audio_ctx = list(ctxs)
        return xa

    def decoder_logits(self, tokens: np.ndarray) -> torch.Tensor:
        """Teacher-forced logits [B, T, V] for the currently encoded windows."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        B, T = tok.shape
        out = torch.empty(B, T, self.dims.n_vocab, device=self.device, dtype=torch.float32)
        self.ctx.check(self.lib.ccx_whisper_decoder_logits(self.handle, tok.ctypes.data_as(C.POINTER(C.c_int32)), B, T,
                                                           out.data_ptr(), _lib.current_stream_ptr()), "ccx_whisper_decoder_logits")
        return out

    def prepare_lanes(self, stream: Optional[torch.cuda.Stream] = None):
        """Pick the decode lanes' internal streams for decodes issued on `stream` (default: the current stream) now, on an
        idle device -- needed before decodes are overlapped with work on other streams (batch.run_pinned_pipelined)."""
        sp = int((stream or torch.cuda.current_stream()).cuda_stream)
        self.ctx.check(self.lib.ccx_whisper_prepare_lanes(self.handle, sp), "ccx_whisper_prepare_lanes")

    def trace_lanes(self, path: Optional[str], level: int = 1):
        """Switch the in-graph lane trace on (path) or off (None): ccx_whisper_trace_lanes.  The stamp level is part of the step plan: traced and
        untraced step graphs live side by side."""
        self.ctx.check(self.lib.ccx_whisper_trace_lanes(self.handle, path.encode() if path else None, int(level)), "ccx_whisper_trace_lanes")

    def decode_greedy(self, prompts: Sequence[Sequence[int]], sample_len: Optional[int] = None) -> List[dict]:
        """Greedy DecodingTask.run over the currently encoded windows (temperature 0)."""
        return self.decode(prompts, sample_len, temperature=0.0)

    def decode(self, prompts: Sequence[Sequence[int]], sample_len: Optional[int] = None, temperature: float = 0.0,
               seed: int = 0, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, sequence_bias=None,
               bad_words_ids=None, hotwords=None, hotword_boost=None, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
               logprobs: Optional[int] = None, **decoding) -> List[dict]:
        """DecodingTask.run over the currently encoded windows; prompts[b] are the full initial tokens
        (sot_prev + prompt + sot).  temperature 0: argmax.  temperature > 0: one Categorical(logits / T) sample per
        step (decoding.py::GreedyDecoder.update), drawn on the device from Philox noise keyed by
        (seed, row, step, token id) -- reproducible, not bit-equal to torch's sampler.
        sample_len None: decode_cap of the longest prompt -- n_text_ctx // 2 = 224 for every prompt of up to 225 tokens (what the
        default always was), fewer for a longer one, which the fixed 224 made the library refuse.
        **decoding (decoding_options instances; ignored otherwise): without_timestamps, suppress_blank, suppress_tokens,
        max_initial_timestamp for this call; the prompts, the SOT tail, the prefix length and sample_len stay the caller's.
        repetition_penalty / no_repeat_ngram_size (repetition_control instances; ignored otherwise): this call's history rules.
        sequence_bias / bad_words_ids / hotwords / hotword_boost (contextual_bias instances; ignored otherwise): this call's bias
        table, which a step adds before the history rules.
        top_k / top_p / min_p (truncated_sampling instances; a non-default value raises ValueError otherwise): this call's cut of the
        distribution a temperature > 0 step draws from; without effect at temperature 0.
        logprobs (token_logprobs instances; not None raises ValueError otherwise, as does a value that is no int in [0, 8]): every
        record gains `token_logprobs` and, for n > 0, `top_logprobs` (see the constructor).  All of them are resolved first (`_decode_settings`: a refused call sets
        nothing) and hold for this call alone (`_settings`)."""
        settings = self._decode_settings((sequence_bias, bad_words_ids, hotwords, hotword_boost), repetition_penalty,
                                         no_repeat_ngram_size, decoding, top_k, top_p, min_p, logprobs)
        if not (temperature >= 0.0):
            raise _lib.CcxError("temperature must be >= 0")
        B = len(prompts)
        ids, lens, mp = self._pack_prompts(prompts)
        sample_len = sample_len or decode_cap(mp, self.dims.n_text_ctx)
        toks = np.zeros((B, sample_len), dtype=np.int32)
        ntok = np.zeros(B, dtype=np.int32)
        slp = np.zeros(B, dtype=np.float32)
        nsp = np.zeros(B, dtype=np.float32)
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        with self._settings(settings):
            self.ctx.check(self.lib.ccx_whisper_decode(
                self.handle, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), mp, B, sample_len, float(temperature),
                int(seed) & 0xFFFFFFFFFFFFFFFF, toks.ctypes.data_as(i32p), ntok.ctypes.data_as(i32p), slp.ctypes.data_as(fp),
                nsp.ctypes.data_as(fp), _lib.current_stream_ptr()), "ccx_whisper_decode")
            return self._with_logprobs(self._records(toks, ntok, slp, nsp), settings.logprobs, sample_len)

    def decode_rows(self, prompts: Sequence[Sequence[int]], windows: Sequence[int], stream_ids: Optional[Sequence[int]] = None,
                    sample_len: Optional[int] = None, temperature: float = 0.0, seed: int = 0, n_windows: Optional[int] = None,
                    repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, sequence_bias=None, bad_words_ids=None,
                    hotwords=None, hotword_boost=None, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
                    logprobs: Optional[int] = None, **decoding) -> List[dict]:
        """`decode` for len(prompts) <= max_batch rows over the currently encoded windows (ccx_whisper_decode_rows): row r decodes
        window windows[r] -- entries may repeat (best_of), need not be monotone, and windows may go unused (a fallback round decodes
        only the failing ones).  stream_ids[r]: the row's noise stream at temperature > 0 (None: r), so that its draws do not depend on
        the rows it shares the call with.  n_windows: how many windows are encoded (default: max(windows) + 1).  repetition_penalty,
        no_repeat_ngram_size, sequence_bias, bad_words_ids, hotwords, hotword_boost, top_k, top_p, min_p, logprobs, **decoding: as `decode`."""
        settings = self._decode_settings((sequence_bias, bad_words_ids, hotwords, hotword_boost), repetition_penalty,
                                         no_repeat_ngram_size, decoding, top_k, top_p, min_p, logprobs)
        if not (temperature >= 0.0):
            raise _lib.CcxError("temperature must be >= 0")
        R = len(prompts)
        if len(windows) != R or (stream_ids is not None and len(stream_ids) != R):
            raise _lib.CcxError("decode_rows: one window (and one stream id) per prompt")
        ids, lens, mp = self._pack_prompts(prompts)
        sample_len = sample_len or decode_cap(mp, self.dims.n_text_ctx)
        win = np.ascontiguousarray(windows, dtype=np.int32)
        sid = np.ascontiguousarray(stream_ids, dtype=np.int32) if stream_ids is not None else None
        nw = int(n_windows) if n_windows is not None else int(win.max()) + 1
        toks = np.zeros((R, sample_len), dtype=np.int32)
        ntok = np.zeros(R, dtype=np.int32)
        slp = np.zeros(R, dtype=np.float32)
        nsp = np.zeros(R, dtype=np.float32)
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        with self._settings(settings):
            self.ctx.check(self.lib.ccx_whisper_decode_rows(
                self.handle, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), mp, R, win.ctypes.data_as(i32p), nw,
                sid.ctypes.data_as(i32p) if sid is not None else None, sample_len, float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF,
                toks.ctypes.data_as(i32p), ntok.ctypes.data_as(i32p), slp.ctypes.data_as(fp), nsp.ctypes.data_as(fp),
                _lib.current_stream_ptr()), "ccx_whisper_decode_rows")
            return self._with_logprobs(self._records(toks, ntok, slp, nsp), settings.logprobs, sample_len)

    def decode_beam(self, prompts: Sequence[Sequence[int]], beam_size: int, patience: Optional[float] = None,
                    sample_len: Optional[int] = None, windows: Optional[Sequence[int]] = None, n_windows: Optional[int] = None,
                    trace: bool = False, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, sequence_bias=None,
                    bad_words_ids=None, hotwords=None, hotword_boost=None, **decoding):
        """Beam search at temperature 0 over the currently encoded windows (ccx_whisper_decode_beam) [UPSTREAM-RECALL:
        decoding.py::BeamSearchDecoder]: prompts[g] is decoded on window windows[g] (None: window g) by beam_size rows that share the
        window's encoder output; len(prompts) * beam_size <= max_batch.  patience (None: 1.0): a window is complete once
        round(beam_size * patience) hypotheses have finished.  -> per prompt the list of its hypotheses in insertion order (finished
        ones first, then live rows by descending score while fewer than beam_size finished): dicts of tokens (before the eot),
        sum_logprob, avg_logprob, no_speech_prob (the window's), cross_path.  The ranker (`fallback.rank_candidates`) picks among them.
        trace=True (a test aid; the steps then run eagerly): -> (results, dict of numpy arrays cand_id / cand_lp [steps, rows,
        beam_size + 1], tok / parent / score [steps, rows]; rows = prompt-major; -1 / NaN where a window no longer stepped).
        repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids, hotwords, hotword_boost, **decoding: as `decode`; every
        row reads the history that follows its hypothesis."""
        settings = self._decode_settings((sequence_bias, bad_words_ids, hotwords, hotword_boost), repetition_penalty,
                                         no_repeat_ngram_size, decoding)
        G, bs = len(prompts), int(beam_size)
        if patience is not None and not (patience > 0):
            raise _lib.CcxError("decode_beam: patience must be > 0")
        mc = round(bs * (1.0 if patience is None else float(patience)))
        ids, lens, mp = self._pack_prompts(prompts)
        sample_len = sample_len or decode_cap(mp, self.dims.n_text_ctx)
        win = np.ascontiguousarray(windows, dtype=np.int32) if windows is not None else None
        if win is not None and win.shape != (G,):
            raise _lib.CcxError("decode_beam: one window per prompt")
        nw = int(n_windows) if n_windows is not None else (int(win.max()) + 1 if win is not None else G)
        Cn = max(bs, mc, 1)
        toks = np.zeros((G, Cn, sample_len), dtype=np.int32)
        ntok = np.zeros((G, Cn), dtype=np.int32)
        slp = np.zeros((G, Cn), dtype=np.float32)
        nhyp = np.zeros(G, dtype=np.int32)
        nsp = np.zeros(G, dtype=np.float32)
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        tr, tr_c = None, None
        if trace:
            R, K = G * max(bs, 1), bs + 1
            tr = dict(cand_id=np.full((sample_len, R, K), -1, dtype=np.int32), cand_lp=np.full((sample_len, R, K), np.nan, dtype=np.float32),
                      tok=np.full((sample_len, R), -1, dtype=np.int32), parent=np.full((sample_len, R), -1, dtype=np.int32),
                      score=np.full((sample_len, R), np.nan, dtype=np.float32))
            tr_c = _lib.BeamTrace(sample_len, tr["cand_id"].ctypes.data_as(i32p), tr["cand_lp"].ctypes.data_as(fp),
                                  tr["tok"].ctypes.data_as(i32p), tr["parent"].ctypes.data_as(i32p), tr["score"].ctypes.data_as(fp))
        with self._settings(settings):
            self.ctx.check(self.lib.ccx_whisper_decode_beam(
                self.handle, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), mp, G, win.ctypes.data_as(i32p) if win is not None else None,
                nw, bs, mc, sample_len, toks.ctypes.data_as(i32p), ntok.ctypes.data_as(i32p), slp.ctypes.data_as(fp), nhyp.ctypes.data_as(i32p),
                nsp.ctypes.data_as(fp), C.byref(tr_c) if tr_c is not None else None, _lib.current_stream_ptr()), "ccx_whisper_decode_beam")
            # the candidate slots as rows, every one with its window's no-speech probability; a window keeps its first nhyp[g]
            rows = self._records(toks.reshape(G * Cn, sample_len), ntok.reshape(-1), slp.reshape(-1), np.repeat(nsp, Cn))
        out = [rows[g * Cn:g * Cn + int(nhyp[g])] for g in range(G)]
        return (out, tr) if trace else out

    _call_logprobs: Optional[int] = None      # the top_n the running `transcribe_batch` has set (`_settings`); None: not set

    def _call_decode(self, prompts, cap, temperature, seed, windows=None, stream_ids=None, n_windows=None) -> List[dict]:
        """A decode inside `transcribe_batch`: `decode` (windows None) or `decode_rows` under the call's settings, which are set
        already -- so nothing is passed again; only the lists of a call with logprobs are fetched behind it."""
        if windows is None:
            rows = self.decode(prompts, sample_len=cap, temperature=temperature, seed=seed)
        else:
            rows = self.decode_rows(prompts, windows, stream_ids, sample_len=cap, temperature=temperature, seed=seed, n_windows=n_windows)
        return self._with_logprobs(rows, self._call_logprobs, cap)

    def _decode_with_fallback(self, prompts, cap: int, schedule, best_of, compression_ratio_threshold, logprob_threshold,
                              no_speech_threshold, beam_size=None, patience=None, length_penalty=None) -> List[dict]:
        """The schedule walk of one encoded group [UPSTREAM-RECALL: transcribe.py::decode_with_fallback]: round 0 over every window,
        each later round one `decode_rows` (chunked to max_batch rows) over the windows still failing, times best_of above
        temperature 0.  Round 0 is a plain `decode` whenever it has one row per window, so a group whose windows all pass at the
        first temperature costs what it costs without a schedule.  One seed per round -- the chunks of a round are one decode split
        by capacity -- and stream ids from the window's place in the group: a window's outcome does not depend on which other
        windows fell back.  beam_size (beam_search instances): a temperature-0 round is a beam search instead -- `decode_beam` over the
        group's window map, max_batch // beam_size windows per call -- and best_of rounds above 0 stay what they are; length_penalty
        enters the ranker of both.  -> one result per window: tokens, avg_logprob, no_speech_prob, temperature, compression_ratio."""
        walk = fallback.FallbackWalk(len(prompts), schedule, compression_ratio_threshold, logprob_threshold, no_speech_threshold)
        self.fallback_walks.append(walk)        # (tests replay every window's rounds from walk.trace)
        eot = self.rules.eot
        while not walk.done():
            t = walk.temperature()
            n_rows = fallback.rows_per_window(t, best_of)
            failing = walk.pending()
            self._sample_calls += 1
            seed = (int(self.sample_seed) << 32) + self._sample_calls
            cands: Dict[int, List[dict]] = {w: [] for w in failing}
            if t == 0.0 and beam_size is not None:
                per_call = self.max_batch // int(beam_size)
                if per_call < 1:
                    raise _lib.CcxError(f"beam_size = {beam_size} exceeds max_batch = {self.max_batch}")
                for at in range(0, len(failing), per_call):
                    part = failing[at:at + per_call]
                    hyps = self.decode_beam([prompts[w] for w in part], beam_size, patience=patience, sample_len=cap, windows=part,
                                            n_windows=len(prompts))
                    for w, h in zip(part, hyps):
                        cands[w] = h
            elif walk.round == 0 and n_rows == 1:
                for w, r in enumerate(self._call_decode(prompts, cap, t, seed)):
                    cands[w].append(r)
            else:
                for ch in fallback.plan_round(failing, prompts, n_rows, self.max_batch):
                    rows = self._call_decode(ch["prompts"], cap, t, seed, ch["windows"], ch["stream_ids"], len(prompts))
                    for (w, _), r in zip(ch["owners"], rows):
                        cands[w].append(r)
            walk.submit({w: fallback.window_result(cands[w], t, self.tokenizer, eot, length_penalty) for w in failing})
        return [walk.accepted[w] for w in range(len(prompts))]

    def align(self, tokens_per_seq: Sequence[Sequence[int]], n_frames: Sequence[int], return_probs: bool = False,
              return_matrix: bool = False, row0: int = 1, token_probs: bool = False):
        """Word alignment of the currently encoded windows (ccx_whisper_align; valid after `encode` or a decode of the same
        windows): a teacher-forced pass over tokens_per_seq[b] (alignment_tokens: [sot, no_timestamps, *text, eot]), the alignment
        matrix of `alignment_heads` over the first n_frames[b] // 2 encoder positions, and the DTW over rows row0 .. -1.
        Returns (jump_frames, P, A): jump_frames[b] = int array, the encoder position at which each of those rows starts; P
        [B, heads, T, n_audio_ctx] / A [B, T, n_audio_ctx] device tensors when asked for, else None.
        token_probs: (jump_frames, P, A, probs) instead -- probs[b] = float32 array, one entry per text token: its softmax
        probability over the ids [0, eot) at the row that predicts it (ccx_whisper_align_probs; timing.py::find_alignment)."""
        B = len(tokens_per_seq)
        toks, lens, T = self._pack_prompts(tokens_per_seq)
        nf =np.ascontiguousarray(n_frames, dtype=np.int32)
        if nf.shape != (B,):
            raise _lib.CcxError("align: one n_frames entry per sequence")
        heads = np.ascontiguousarray(self.alignment_heads, dtype=np.int32).reshape(-1, 2)
        P = torch.empty(B, len(heads), T, self.dims.n_audio_ctx, device=self.device, dtype=torch.float32) if return_probs else None
        A = torch.empty(B, T, self.dims.n_audio_ctx, device=self.device, dtype=torch.float32) if return_matrix else None
        jump = np.full((B, T), -1, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        if token_probs:
            tp = np.full((B, T), -1.0, dtype=np.float32)
            self.ctx.check(self.lib.ccx_whisper_align_probs(
                self.handle, toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), T, B, nf.ctypes.data_as(i32p),
                heads.ctypes.data_as(i32p), len(heads), int(row0), _lib.ptr(P), _lib.ptr(A), jump.ctypes.data_as(i32p),
                int(self.rules.eot), tp.ctypes.data_as(C.POINTER(C.c_float)), _lib.current_stream_ptr()), "ccx_whisper_align_probs")
        else:
            self.ctx.check(self.lib.ccx_whisper_align(
                self.handle, toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), T, B, nf.ctypes.data_as(i32p),
                heads.ctypes.data_as(i32p), len(heads), int(row0), _lib.ptr(P), _lib.ptr(A), jump.ctypes.data_as(i32p),
                _lib.current_stream_ptr()), "ccx_whisper_align")
        jumps = [jump[b, :max(int(lens[b]) - 1 - int(row0), 0)].copy() for b in range(B)]
        if token_probs:
            return jumps, P, A, [tp[b, :max(int(lens[b]) - 2 - int(row0), 0)].copy() for b in range(B)]
        return jumps, P, A

    def _advance_with_words(self, grp, results, state, temps: Sequence[float], hallucination_silence_threshold: Optional[float] = None):
        """word_alignment and word_timestamps: align every window of the group that produced text while the windows are still
        encoded, attach the words, and advance each clip with the end of its last word [UPSTREAM-RECALL: transcribe.py].  On an
        instance with word_probabilities the same pass gives the token probabilities, the words carry `probability` and the
        threshold reaches `advance`.  temps: the temperature every window was decoded at."""
        built = [state[i].window_segments(r) for i, r in zip(grp, results)]
        texts = []
        for bt in built:
            texts.append([t for s in bt[0] for t in s["tokens"] if t < self.rules.eot] if bt is not None else [])
        jumps, probs = None, None
        if any(texts):
            frames = [max(2, state[i].segment_size()) for i in grp]
            # one teacher-forced batch: every window with its own SOT sequence (all of one length: the DTW starts behind it)
            seqs = [state[i].sot_sequence for i in grp]
            assert all(len(sq) == len(seqs[0]) for sq in seqs), "one model, one SOT-sequence length: the DTW's row0 is per call"
            got = self.align([alignment_tokens(t, self.rules, sq) for t, sq in zip(texts, seqs)], frames, row0=len(seqs[0]),
                             token_probs=self.word_probabilities)
            jumps, probs = got[0], (got[3] if self.word_probabilities else None)
        for b, (i, r) in enumerate(zip(grp, results)):
            segs, end = None, None
            if built[b] is not None:
                segs = built[b][0]
                add_word_timestamps(segs, self.tokenizer, self.rules, lambda toks, b=b: jumps[b], state[i].last_speech_timestamp,
                                    prob_fn=(lambda toks, b=b: probs[b]) if self.word_probabilities else None)
                end = get_end(segs)
            if self.word_probabilities and hallucination_silence_threshold is not None:
                state[i].advance(r, temps[b], last_word_end=end, segments=segs,
                                 hallucination_silence_threshold=hallucination_silence_threshold)
            else:
                state[i].advance(r, temps[b], last_word_end=end, segments=segs)

    # ------------------------------------------------------------------ transcribe (reference call surface)
    def initial_tokens(self, prompt_tokens: Sequence[int], sot_sequence: Optional[Sequence[int]] = None) -> List[int]:
        """decoding.py::_get_initial_tokens: [sot_prev] + prompt[-(n_ctx//2 - 1):] + sot_sequence (default: the rules' own --
        [sot], or [sot, <|en|>, <|transcribe|>] on a multilingual model)."""
        toks: List[int] = []
        if len(prompt_tokens):
            toks = [self.rules.sot_prev] + list(prompt_tokens)[-(self.dims.n_text_ctx // 2 - 1):]
        return toks + list(sot_sequence if sot_sequence is not None else self.rules.sot_sequence())

    def _walk_options(self, temperature, best_of, beam_size, patience, length_penalty):
        """A `transcribe_batch` call's temperature / best_of / beam arguments, refused or dropped as its opt-ins say -> (schedule,
        whether the windows walk it (`_decode_with_fallback`), best_of, beam_size, patience, length_penalty)"""
        if not self.temperature_fallback:
            if isinstance(temperature, (tuple, list)):
                raise _lib.CcxError("temperature fallback schedules need an instance built with temperature_fallback=True: "
                                    "pass one temperature (the reference does)")
            best_of = None          # ignored, as compression_ratio_threshold is
        if not self.beam_search:
            beam_size = patience = length_penalty = None     # accepted and ignored
        if patience is not None and beam_size is None:
            raise _lib.CcxError("patience needs beam_size")
        if beam_size is not None and not isinstance(temperature, (tuple, list)) and float(temperature) > 0.0:
            raise _lib.CcxError("beam_size needs temperature 0 (or a schedule that starts there): beam search does not sample")
        try:
            schedule = fallback.normalize_schedule(temperature)
        except ValueError as e:
            raise _lib.CcxError(str(e)) from e
        walk_on = (self.temperature_fallback and (isinstance(temperature, (tuple, list)) or best_of is not None)) or \
            beam_size is not None or length_penalty is not None
        return schedule, walk_on, best_of, beam_size, patience, length_penalty

    def _stage_clips(self, audios: Sequence):
        """The clips as one zero-padded [n, longest] float32 tensor that stays on the device for all their windows -> (it, the clips'
        lengths in samples).  Device tensors (the processor's crops) stay on the device; host arrays go up in one transfer."""
        n = len(audios)
        on_dev = n > 0 and all(isinstance(a, torch.Tensor) and a.is_cuda for a in audios)
        if on_dev:
            clips = [a.detach().reshape(-1) for a in audios]
            lens = [int(c.numel()) for c in clips]
        else:
            clips = []
            for a in audios:
                a = a.detach().to("cpu").numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
                clips.append(np.ascontiguousarray(a.reshape(-1), dtype=np.float32))
            lens = [len(c) for c in clips]
        stride = max(max(lens, default=1), 1)
        if stride > self.max_audio_seconds * SAMPLE_RATE:
            raise _lib.CcxError(f"clip of {stride / SAMPLE_RATE:.1f} s exceeds max_audio_seconds={self.max_audio_seconds}")
        if on_dev:
            dev_audio = torch.zeros(n, stride, device=self.device, dtype=torch.float32)
            for i, c in enumerate(clips):
                dev_audio[i, :lens[i]] = c.to(self.device, torch.float32)
        else:
            host = np.zeros((n, stride), dtype=np.float32)
            for i, c in enumerate(clips):
                host[i, :lens[i]] = c
            dev_audio = torch.from_numpy(host).to(self.device)
        return dev_audio, lens

    def transcribe(self, audio, initial_prompt: Optional[str] = None, word_timestamps: bool = False,
                   condition_on_previous_text: bool = True, temperature: float = 0.0,
                   no_speech_threshold: Optional[float] = 0.6, logprob_threshold: Optional[float] = -1.0,
                   language: Optional[str] = None, task: str = "transcribe",
                   hallucination_silence_threshold: Optional[float] = None, compression_ratio_threshold: Optional[float] = 2.4,
                   best_of: Optional[int] = None, beam_size: Optional[int] = None, patience: Optional[float] = None,
                   length_penalty: Optional[float] = None, without_timestamps: bool = False, prefix=None,
                   suppress_blank: bool = True, suppress_tokens="-1", max_initial_timestamp: Optional[float] = 1.0,
                   sample_len: Optional[int] = None, clip_timestamps="0", carry_initial_prompt: bool = False,
                   repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, sequence_bias=None, bad_words_ids=None,
                   hotwords=None, hotword_boost=None, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0, audio_ctx=None,
                   logprobs: Optional[int] = None, **_ignored):
        """One clip, same signature as whisper.transcribe as the reference uses it.  temperature 0 is the
        parity mode (greedy); a positive float (the reference's Config.temperature = 0.1,
        back/api.py:128) samples every token from Categorical(logits / T) -- a single temperature means no
        fallback loop upstream either.  Draws are reproducible: seeded by `self.sample_seed` and a per-call
        counter.  word_timestamps only changes fields the reference never reads, and only on an instance built with
        `word_alignment=True` (segments get `words`, `seek` follows the last aligned word); otherwise it has no effect.
        language / task: on a multilingual model the SOT sequence is [sot, <|language|>, <|task|>]; language None (upstream's
        default, what the reference's calls leave it at) detects it on the first window.  An English-only model reports "en" and
        ignores both, as upstream's transcribe does.
        hallucination_silence_threshold (seconds): with word_timestamps on an instance built with `word_probabilities=True`, silence
        longer than this around a probable hallucination is skipped (WindowLoop.advance); otherwise no effect -- upstream ignores
        it without word_timestamps too.
        On an instance built with `temperature_fallback=True`: temperature may be a schedule (upstream's default is (0.0, 0.2, 0.4,
        0.6, 0.8, 1.0); here the default stays 0.0), and compression_ratio_threshold / best_of are honoured
        [UPSTREAM-RECALL: transcribe.py::decode_with_fallback; parity unpinned] -- see `transcribe_batch`.  Otherwise a schedule
        raises and the two are ignored.
        On an instance built with `beam_search=True`: beam_size / patience / length_penalty are honoured (see `transcribe_batch`);
        otherwise they are accepted and ignored.
        On an instance built with `decoding_options=True`: without_timestamps, prefix, suppress_blank, suppress_tokens,
        max_initial_timestamp, sample_len, clip_timestamps and carry_initial_prompt are honoured (see `transcribe_batch`); otherwise
        they are accepted and ignored.
        On an instance built with `repetition_control=True`: repetition_penalty and no_repeat_ngram_size are honoured (see
        `transcribe_batch`); otherwise they are accepted and ignored.
        On an instance built with `contextual_bias=True`: sequence_bias, bad_words_ids, hotwords and hotword_boost are honoured (see
        `transcribe_batch`); otherwise they are accepted and ignored.
        On an instance built with `truncated_sampling=True`: top_k, top_p and min_p are honoured (see `transcribe_batch`); otherwise
        a value off its default raises ValueError.
        On an instance built with `token_logprobs=True`: logprobs=n gives every segment `token_logprobs` (and `top_logprobs` for
        n > 0; see `transcribe_batch`); otherwise anything but None raises ValueError.
        On an instance built with `audio_ctx`: audio_ctx overrides the instance's setting for this call ("full", "auto" or an int;
        see `transcribe_batch`), and the result carries `audio_ctx`; otherwise anything but None / "full" raises ValueError."""
        return self.transcribe_batch([audio], [initial_prompt], condition_on_previous_text=condition_on_previous_text,
                                     compression_ratio_threshold=compression_ratio_threshold, best_of=best_of,
                                     temperature=temperature, no_speech_threshold=no_speech_threshold,
                                     logprob_threshold=logprob_threshold, word_timestamps=word_timestamps,
                                     languages=[language], task=task,
                                     hallucination_silence_threshold=hallucination_silence_threshold, beam_size=beam_size,
                                     patience=patience, length_penalty=length_penalty, without_timestamps=without_timestamps,
                                     prefixes=[prefix], suppress_blank=suppress_blank, suppress_tokens=suppress_tokens,
                                     max_initial_timestamp=max_initial_timestamp, sample_len=sample_len,
                                     clip_timestamps=clip_timestamps, carry_initial_prompt=carry_initial_prompt,
                                     repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                     sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotwords=hotwords,
                                     hotword_boost=hotword_boost, top_k=top_k, top_p=top_p, min_p=min_p, audio_ctx=audio_ctx,
                                     logprobs=logprobs)[0]

    def transcribe_batch(self, audios: Sequence, initial_prompts: Optional[Sequence[Optional[str]]] = None,
                         condition_on_previous_text: bool = True, temperature: float = 0.0,
                         no_speech_threshold: Optional[float] = 0.6, logprob_threshold: Optional[float] = -1.0,
                         word_timestamps: bool = False, languages: Optional[Sequence[Optional[str]]] = None,
                         task: str = "transcribe", hallucination_silence_threshold: Optional[float] = None,
                         compression_ratio_threshold: Optional[float] = 2.4, best_of: Optional[int] = None,
                         beam_size: Optional[int] = None, patience: Optional[float] = None,
                         length_penalty: Optional[float] = None, without_timestamps: bool = False,
                         prefixes: Optional[Sequence] = None, suppress_blank: bool = True, suppress_tokens="-1",
                         max_initial_timestamp: Optional[float] = 1.0, sample_len: Optional[int] = None, clip_timestamps="0",
                         carry_initial_prompt: bool = False, repetition_penalty: float = 1.0,
                         no_repeat_ngram_size: int = 0, sequence_bias=None, bad_words_ids=None, hotwords=None,
                         hotword_boost=None, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0, audio_ctx=None,
                         logprobs: Optional[int] = None) -> List[dict]:
        """Independent clips decoded together (each window of each clip is one sequence of a batch).
        languages[i] (multilingual models): the clip's language code or name; None: detected on the clip's first window, after its
        group's `encode` and before its `decode` [UPSTREAM-RECALL: transcribe.py, `if decode_options.get("language") is None`].
        A pass over the active clips is split into groups of one sample cap (decode_cap) of at most max_batch windows.
        hallucination_silence_threshold: as in `transcribe`, for every clip.
        temperature_fallback instances [UPSTREAM-RECALL: transcribe.py::decode_with_fallback; parity unpinned]: with a temperature
        sequence or a best_of, every window walks the schedule (clearconverse_amd/fallback.py): accepted at the first temperature at
        which its compression ratio is not above compression_ratio_threshold and its mean log-probability not below
        logprob_threshold (silence by no_speech_threshold excepted), at the last one whatever it scores; above temperature 0,
        best_of candidates per window, the most probable per token kept.  Per group `log_mel` and `encode` run once; word alignment
        runs after the walk on the accepted tokens.  On such calls every segment also carries `temperature`, `avg_logprob`,
        `compression_ratio` and `no_speech_prob`, as upstream's do; a single float without best_of returns what it always did.
        beam_search instances [UPSTREAM-RECALL: decode_with_fallback, BeamSearchDecoder; parity unpinned]: with beam_size, every
        temperature-0 round decodes its windows by beam search (`decode_beam`: beam_size rows per window over the group's window map,
        nothing encoded again; `patience` sets when a window is complete) and keeps the ranker's pick among the hypotheses; above 0
        beam_size and patience are dropped as best_of is at 0; length_penalty enters the ranker of both.  The same thresholds apply, the
        segments carry the walk's fields, word alignment runs afterwards on the accepted tokens.  beam_size with a single temperature
        above 0, or patience without beam_size, raises.  Without the opt-in all three are ignored: the call is what it is without them.
        decoding_options instances [UPSTREAM-RECALL: decoding.py::DecodingOptions, transcribe.py; parity unpinned]:
        without_timestamps -- every window's SOT sequence ends in <|notimestamps|> and the steps run the kernels without
        ApplyTimestampRules: plain text, one segment per window, `seek` advances by the window; prefixes[i] -- a string (encoded as
        " " + prefix.strip()) or token ids appended behind the SOT sequence of every window of clip i: part of the prompt, never of
        the result (with sample_len, its last n_ctx // 2 - sample_len tokens; the prefixes of one call must hold equally many tokens
        -- the library reads the no-speech probability a fixed number of positions before the prompt's end); suppress_blank;
        suppress_tokens -- comma-separated ids or a list, -1 = the non-speech list, the specials always added, empty or None = no
        SuppressTokens at all; max_initial_timestamp -- seconds, None = rule off; sample_len -- caps every window's samples;
        clip_timestamps -- comma-separated seconds or a list: the window loop walks the (start, end) pairs (an odd count is closed by
        the clip's end), a window ends where its pair ends (`log_mel(max_frames=)`); carry_initial_prompt -- the initial prompt leads
        every window's prompt.  One ccx_whisper_set_decode_options per call serves every round of a fallback walk or beam search;
        the defaults are back when the call returns.  without_timestamps with hallucination_silence_threshold raises.  Without the
        opt-in all of them are ignored.
        repetition_control instances: repetition_penalty (finite, > 0; 1.0 = off) and no_repeat_ngram_size (>= 0; 0 = off) hold for
        every window of the call -- every round of a fallback walk, every best_of row and every beam row gets them (one
        ccx_whisper_set_history_options per call, the defaults back when it returns); a value outside its range raises ValueError.
        A window's history is what that window's decode sampled: nothing carries over from the prompt or from earlier windows.
        Without the opt-in both are ignored.
        contextual_bias instances: sequence_bias (dict tuple -> float, or list of [ids, float]), bad_words_ids (list of id lists) and
        hotwords (a phrase or a list of them, with hotword_boost, which has no default) are compiled into one table
        (`decode_bias.compile_bias_table`) that holds for every window of the call and every round of a fallback walk (one
        ccx_whisper_set_bias_options per call, no table set when it returns); what the compile refuses raises ValueError.  A window
        matches over what that window's decode sampled only.  Without the opt-in all four are ignored.
        truncated_sampling instances: top_k (>= 0; 0 = off), top_p (in (0, 1]; 1 = off) and min_p (in [0, 1]; 0 = off) hold for every
        decode of the call at temperature > 0 -- a single positive temperature, the warm rounds of a fallback walk, every best_of
        candidate (one ccx_whisper_set_sampling_options per call, the defaults back when it returns); a temperature-0 round, greedy
        or beam, is what it is without them, and so are the thresholds: avg_logprob stays the log-probability under the untruncated
        distribution.  A value outside its range raises ValueError; so does a value off its default without the opt-in.
        audio_ctx instances (the reduced audio context, WhisperModel.__init__; not upstream's arithmetic, quality unmeasured): every
        window is encoded with the instance's setting, or with this call's audio_ctx -- "full" (all n_audio_ctx positions: the tokens of
        an instance without the opt-in), "auto" or an int; every result carries `audio_ctx`, the context of each of the clip's
        windows, in order.  Without the opt-in anything but None / "full" raises ValueError.
        token_logprobs instances: logprobs=n (an int in [0, 8]) holds for every decode of the call (one
        ccx_whisper_set_logprob_options per call, off again when it returns): every segment carries `token_logprobs` and, n > 0,
        `top_logprobs`, the slices of its window's lists over the index range its `tokens` are cut with (a segment whose tokens are
        cleared gets empty lists); on a fallback walk or best_of they are the accepted candidate's.  None (the default): the result
        and its segments are what they always were.  Anything but None without the opt-in, a value that is no int in [0, 8], and
        logprobs together with beam_size on a beam_search instance raise ValueError before anything runs."""
        n = len(audios)
        if audio_ctx is not None:       # refuse before anything runs
            self._window_contexts(0, audio_ctx)
        clip_ctx: List[List[int]] = [[] for _ in range(n)]
        settings, opt, prefix_toks = self._transcribe_settings(
            n, hallucination_silence_threshold, without_timestamps, prefixes, suppress_blank, suppress_tokens, max_initial_timestamp,
            sample_len, carry_initial_prompt, repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids, hotwords,
            hotword_boost, top_k, top_p, min_p)
        schedule, walk_on, best_of, beam_size, patience, length_penalty = self._walk_options(temperature, best_of, beam_size, patience,
                                                                                            length_penalty)
        settings = settings._replace(logprobs=self._logprob_setting(logprobs, beam_size))
        with_words = bool(word_timestamps) and self.word_alignment
        self.fallback_walks: List[fallback.FallbackWalk] = []     # this call's walks, one per encoded group, in order
        initial_prompts = list(initial_prompts) if initial_prompts is not None else [None] * n
        multi = self.rules.is_multilingual
        languages = list(languages) if languages is not None else [None] * n
        if len(languages) != n:
            raise _lib.CcxError("transcribe_batch: one language entry (or None) per clip")
        dev_audio, lens = self._stage_clips(audios)
        # English-only: language "en", task ignored.  Multilingual: the clip's SOT sequence; language None: pending until detected
        def loop_options(i):
            if opt is None:
                return {}
            try:
                clips_i = decoding_options.parse_clip_timestamps(clip_timestamps, lens[i] // HOP)
            except ValueError as e:
                raise _lib.CcxError(f"clip_timestamps: {e}") from e
            return dict(without_timestamps=opt.without_timestamps, prefix_tokens=prefix_toks[i], sample_len=opt.sample_len,
                        clips=clips_i, carry_initial_prompt=opt.carry_initial_prompt)

        state = [WindowLoop(self.rules, self.tokenizer, lens[i] // HOP, initial_prompts[i], self.dims.n_text_ctx,
                            condition_on_previous_text, no_speech_threshold, logprob_threshold,
                            language=languages[i] if multi else "en", task=task, **loop_options(i)) for i in range(n)]
        # one set per family for every window, group and round of the call; the instance's own values are back when it returns
        with self._settings(settings), self._logprobs_of_call(settings.logprobs):
            while True:
                active = [i for i in range(n) if state[i].active()]
                if not active:
                    break
                # (a clip whose language is still to be detected already holds a three-token SOT sequence: its cap is known)
                caps = [state[i].sample_cap() for i in active]
                for cap, grp in groups_by_cap(active, caps, self.max_batch):
                    if len(grp) == n:
                        a = dev_audio
                    else:
                        a = dev_audio.index_select(0, torch.tensor(grp, device=self.device)).contiguous()
                    if opt is not None:     # a window ends where its clip ends
                        self.log_mel(a, [lens[i] for i in grp], [state[i].seek for i in grp],
                                     max_frames=[state[i].segment_size() for i in grp])
                    else:
                        self.log_mel(a, [lens[i] for i in grp], [state[i].seek for i in grp])
                    if audio_ctx is None:       # (the instance's setting; a call without the keyword is the call it always was)
                        self.encode(len(grp))
                    else:
                        self.encode(len(grp), audio_ctx=audio_ctx)
                    if self.audio_ctx is not None:
                        for b, i in enumerate(grp):
                            clip_ctx[i].append(self.last_audio_ctx[b])
                    if any(not state[i].language_known for i in grp):     # first window of a clip without a language
                        codes, _ = self.detect_language(len(grp))
                        for b, i in enumerate(grp):
                            if not state[i].language_known:
                                state[i].set_language(codes[b])
                    prompts = [state[i].initial_tokens() for i in grp]
                    if walk_on:
                        results = self._decode_with_fallback(prompts, cap, schedule, best_of, compression_ratio_threshold,
                                                             logprob_threshold, no_speech_threshold, beam_size, patience, length_penalty)
                        self.fallback_walks[-1].clips, self.fallback_walks[-1].seeks = list(grp), [state[i].seek for i in grp]
                        temps = [r["temperature"] for r in results]     # what each window was accepted at
                    else:
                        self._sample_calls += 1
                        results = self._call_decode(prompts, cap, schedule[0], (int(self.sample_seed) << 32) + self._sample_calls)
                        temps = [schedule[0]] * len(grp)
                    n_seg = [len(state[i].segments) for i in grp]
                    if with_words:     # before the next log_mel: the group's windows are still encoded, aligned as one batch
                        self._advance_with_words(grp, results, state, temps, hallucination_silence_threshold)
                    else:
                        for i, r, t in zip(grp, results, temps):
                            state[i].advance(r, t)
                    if walk_on:     # the walk's fields on the window's new segments, as upstream's carry them
                        for b, (i, r) in enumerate(zip(grp, results)):
                            for s in state[i].segments[n_seg[b]:]:
                                s.update(temperature=r["temperature"], avg_logprob=r["avg_logprob"], compression_ratio=r["compression_ratio"],
                                         no_speech_prob=r["no_speech_prob"])
        results_out = [st.result() for st in state]
        if self.audio_ctx is not None:
            for r, c in zip(results_out, clip_ctx):
                r["audio_ctx"] = c
        return results_out
