"""Plain-Python statement of openai-whisper's per-call decoding options [UPSTREAM-RECALL: whisper/decoding.py (SuppressBlank,
SuppressTokens, ApplyTimestampRules, _get_initial_tokens, _get_suppress_tokens), whisper/transcribe.py (clip_timestamps,
carry_initial_prompt); upstream is not on disk: parity unpinned] for the tests of `WhisperModel(decoding_options=True)`:

  * `apply_filters` with the options -- oracle/whisper_ref.apply_filters for the defaults (tests/test_decoding_options_reference_cpu.py)
  * one select step and one beam top-k proposal with them
  * the initial-token builder with prefix and <|notimestamps|>, the suppress_tokens expansion
  * the window loop with clips and carry_initial_prompt, written as upstream's flat loop (the product's WindowLoop is an object
    that is stepped: two independent statements)
  * the case generators of the kernel tests: every case decided by a margin of at least 0.5 and sensitive to a one-unit mutation
    of the rule it probes (MUTATIONS).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import whisper_ref as R
from tests import beam_reference as BR
from tests import dec_reference as DR

N_FRAMES, HOP, SAMPLE_RATE, FRAMES_PER_SECOND, TIME_PRECISION, INPUT_STRIDE = 3000, 160, 16000, 100, 0.02, 2


@dataclass
class Options:
    """ccx_decode_options as the tests hold it.  suppress None: the rules' list; a tuple replaces it (empty: SuppressTokens off).
    max_initial_timestamp_index -2: the rules' own, -1 / None: rule off."""
    without_timestamps: bool = False
    suppress_blank: bool = True
    suppress: Optional[Tuple[int, ...]] = None
    max_initial_timestamp_index: Optional[int] = -2


def suppress_list(rules, opts: Options) -> Tuple[int, ...]:
    return tuple(rules.suppress) if opts.suppress is None else tuple(opts.suppress)


def apply_filters(logits: torch.Tensor, sampled: Sequence[int], rules, opts: Options = Options()) -> torch.Tensor:
    """SuppressBlank, SuppressTokens, ApplyTimestampRules, in upstream's order, for ONE row; each only where its option has it on."""
    logits = logits.clone()
    ninf = float("-inf")
    tsb = rules.timestamp_begin
    n = len(sampled)
    if opts.suppress_blank and n == 0:
        logits[rules.blank] = ninf
        logits[rules.eot] = ninf
    sup = suppress_list(rules, opts)
    if len(sup):
        logits[torch.as_tensor(list(sup), dtype=torch.long)] = ninf
    if opts.without_timestamps:
        return logits                                    # no timestamp rule: <|notimestamps|> and the timestamps stay what they are
    logits[rules.no_timestamps] = ninf
    last_ts = n >= 1 and sampled[-1] >= tsb
    pen_ts = n < 2 or sampled[-2] >= tsb
    if last_ts:
        if pen_ts:
            logits[tsb:] = ninf
        else:
            logits[: rules.eot] = ninf
    stamps = [t for t in sampled if t >= tsb]
    if stamps:
        floor = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
        logits[tsb:floor] = ninf
    if n == 0:
        logits[:tsb] = ninf
        mit = rules.max_initial_timestamp_index if opts.max_initial_timestamp_index == -2 else opts.max_initial_timestamp_index
        if mit is not None and mit >= 0:
            logits[tsb + mit + 1:] = ninf
    lp = torch.log_softmax(logits.float(), dim=-1)
    if lp[tsb:].logsumexp(dim=-1) > lp[:tsb].max():
        logits[:tsb] = ninf
    return logits


def select_step_ref(logits, st: DR.SeqState, prompt, gen, rules, opts: Options, sample_len, tok_emb, pos_emb, temperature=0.0, seed=0,
                    row=0) -> DR.StepResult:
    """tests/dec_reference.select_step_ref with the options' filters: one launch of the select kernel for ONE row."""
    st = replace(st)
    gen = list(gen)
    if st.pos < st.prompt_len - 1:
        st.pos += 1
        tok = int(prompt[st.pos])
        return DR.StepResult(st, gen, tok, st.pos, tok_emb[tok] + pos_emb[st.pos], 0)
    if st.done:
        if st.n_gen < sample_len:
            gen[st.n_gen] = rules.eot
            st.n_gen += 1
        return DR.StepResult(st, gen, None, None, None, 0)
    i_gen = st.n_gen
    lg32 = logits.float()
    if i_gen == 0:
        st.no_speech_prob = float(torch.softmax(lg32.double(), dim=-1)[rules.no_speech])
    flt = apply_filters(lg32, gen[:i_gen], rules, opts)
    nxt, _, score = R.sample_token(flt, temperature, seed, row, i_gen)
    top2 = torch.topk(score.double(), 2).values
    logprob = float(torch.log_softmax(flt.double(), dim=-1)[nxt])
    st.sum_logprob = st.sum_logprob + logprob
    gen[i_gen] = nxt
    st.n_gen = i_gen + 1
    st.pen_tok, st.last_tok = st.last_tok, nxt
    if nxt >= rules.timestamp_begin:
        st.last_ts_tok = nxt
    res = DR.StepResult(st, gen, None, None, None, 0, token=nxt, logprob=logprob, margin=float(top2[0] - top2[1]), scores=score)
    if nxt == rules.eot:
        st.done, st.n_tokens, res.finished = 1, i_gen, 1
    elif st.n_gen >= sample_len:
        st.done, st.n_tokens, res.finished = 1, st.n_gen, 1
    else:
        st.pos += 1
        res.cur_tok, res.pos, res.x = nxt, st.pos, tok_emb[nxt] + pos_emb[st.pos]
    return res


def propose(logits, sampled, rules, opts: Options, k: int) -> List[Tuple[int, float]]:
    """a row's top k (id, fp64 log-probability) under the options' filters, best first, equal values by ascending id"""
    lp = torch.log_softmax(apply_filters(logits.float(), list(sampled), rules, opts).double(), dim=-1).numpy()
    order = np.lexsort((np.arange(len(lp)), -lp))[:k]
    return [(int(i), float(lp[i])) for i in order if np.isfinite(lp[i])]


# ---------------------------------------------------------------------------------------------------------------------------------
# the no-rules kernel, restated with one-unit mutations
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("blank_not_banned", "eot_not_banned", "ban_at_step_1", "no_timestamps_banned", "timestamp_banned", "call_list_ignored",
             "rules_list_kept", "force_rule_on", "tie_order")


def select_no_rules(logits, sampled, rules, opts: Options, mutation: Optional[str] = None) -> int:
    """The greedy token as the kernels without ApplyTimestampRules derive it: one allowed set, one argmax, ties to the lowest id."""
    V, tsb, n = logits.shape[0], rules.timestamp_begin, len(sampled)
    banned = np.zeros(V, dtype=bool)
    sup = suppress_list(rules, opts)
    if mutation == "call_list_ignored":
        sup = tuple(rules.suppress)
    if mutation == "rules_list_kept":
        sup = tuple(sup) + tuple(rules.suppress)
    banned[list(sup)] = True
    first = n == 0 or (mutation == "ban_at_step_1" and n == 1)
    if opts.suppress_blank and first:
        if mutation != "blank_not_banned":
            banned[rules.blank] = True
        if mutation != "eot_not_banned":
            banned[rules.eot] = True
    if mutation == "no_timestamps_banned":
        banned[rules.no_timestamps] = True
    if mutation == "timestamp_banned":                       # what ApplyTimestampRules would do to the timestamps of these cases
        stamps = [t for t in sampled if t >= tsb]
        banned[tsb:(stamps[-1] + 1 if stamps else tsb)] = True
        if n == 0:
            banned[tsb + 51:] = True
    x = np.where(banned, -np.inf, logits.double().numpy())
    if mutation == "force_rule_on":
        fin = x[tsb:][np.isfinite(x[tsb:])]
        if len(fin) and fin.max() + np.log(np.exp(fin - fin.max()).sum()) > x[:tsb].max():
            x[:tsb] = -np.inf
    best = x.max()
    ids = np.flatnonzero(x == best)
    return int(ids[-1] if mutation == "tie_order" else ids[0])


def option_sets(rules) -> dict:
    """The option sets the kernel tests launch.  "call list": the rules' list without its first id and with one id it lacks."""
    extra = 500
    assert extra not in rules.suppress
    call = tuple(sorted(set(rules.suppress[1:]) | {extra}))
    return {"rules' list": Options(True), "call list": Options(True, True, call), "no SuppressTokens": Options(True, True, ()),
            "suppress_blank off": Options(True, False, call)}


def select_cases(V, rules, opts: Options, seed=0) -> List[DR.SelectCase]:
    """The greedy cases of one launch of the kernels without the rules: background -20 +- 0.5, the winner at 6, a legal rival at 5,
    banned decoys at 9 (tests/dec_reference.select_cases' conventions)."""
    assert opts.without_timestamps
    g = torch.Generator().manual_seed(4000 + seed + V)
    tsb, eot, blank, nts_tok = rules.timestamp_begin, rules.eot, rules.blank, rules.no_timestamps
    WIN, RIVAL, DECOY, TEXT = DR.WIN, DR.RIVAL, DR.DECOY, DR.TEXT
    nts = V - tsb
    sot = [rules.sot]
    sup = suppress_list(rules, opts)
    cases: List[DR.SelectCase] = []

    def add(name, sampled, winner=None, rival=None, decoys=(), extra=None, expect=None, **kw):
        lg = DR.BACKGROUND + 0.5 * torch.randn(V, generator=g)
        if rival is not None:
            lg[rival] = RIVAL
        for d_ in decoys:
            lg[d_] = DECOY
        if winner is not None:
            lg[winner] = WIN
        if extra:
            extra(lg)
        if not sampled:
            lg[rules.no_speech] = 2.0
        kw.setdefault("prompt", sot)
        kw.setdefault("sum_logprob", -1.5 if sampled else 0.0)
        cases.append(DR.SelectCase(name, lg, list(sampled), expect=winner if expect is None else expect, **kw))

    mid = [TEXT, TEXT + 1]
    first_decoys = (blank, eot) if opts.suppress_blank else ()
    # ---- the first-step ban ----
    if opts.suppress_blank:
        add("step 0: blank banned", [], 234, 77, decoys=(blank,))
        add("step 0: eot banned", [], 235, 78, decoys=(eot,))
    else:
        add("step 0, suppress_blank off: blank wins", [], blank, 77)
        add("step 0, suppress_blank off: eot wins (the row ends empty)", [], eot, 78)
    add("step 1: blank is allowed again", [TEXT], blank, 79)
    add("step 1: eot is allowed again", [TEXT], eot, 80)
    # ---- no timestamp rule ----
    add("step 0: a text id wins (no 'must start with a timestamp')", [], 950, 5, decoys=first_decoys)
    add("step 0: a timestamp beyond max_initial_timestamp wins", [], V - 1, 5, decoys=first_decoys)
    add("<|notimestamps|> is an id like any other", mid, nts_tok, 81)
    add("a timestamp below the last one is allowed", [tsb + min(7, nts - 1), TEXT], tsb, 82)
    add("the last timestamp itself, after a closed pair", [tsb + 1, tsb + 1], tsb + 1, 83)
    add("text after 'text, timestamp' (no pairing rule)", [tsb, TEXT, tsb + 1], 321, eot)
    if nts >= 8:
        def mass(lg):
            ids = torch.arange(tsb, tsb + min(nts, 400))
            lg[ids] = 2.0 + 0.15 - math.log(len(ids))       # summed timestamp mass 0.15 above the best text token ...
            lg[610] = 2.0                                   # ... which wins all the same: no force rule
            lg[611] = 1.4
        add("the timestamps' summed mass beats the best text token: text wins", mid, None, extra=mass, expect=610)
    # ---- the call's list ----
    if opts.suppress is not None:
        dropped = [t for t in rules.suppress if t not in sup and t < V]
        added = [t for t in sup if t not in rules.suppress]
        if added:
            add("decoy at an id only the call's list suppresses", mid, 910, 911, decoys=(added[0],))
        if dropped:
            add("an id of the rules' list that the call's list dropped wins", mid, dropped[0], 912)
    if sup:
        add("decoys at suppressed ids", mid, 913, 914, decoys=(sup[0], sup[-1]))
    # ---- the state machine ----
    add("n_gen + 1 == sample_len: the row stops without eot", [TEXT + i for i in range(DR.SAMPLE_LEN - 1)], 222, 333)
    add("eot chosen in mid text", mid, eot, 600)
    add("a timestamp chosen: last_ts_tok follows", mid, tsb + min(3, nts - 1), 601)
    add("prompt phase", [], None, prompt=[rules.sot_prev, 11, 22, rules.sot], pos=1)
    add("sampling phase behind a long prompt", [], 236, 84, decoys=first_decoys, prompt=[rules.sot_prev, 11, rules.sot, nts_tok])
    add("finished row", [TEXT, eot], None, done=1, sum_logprob=-1.5)
    # ---- placements ----
    tail = (V - 1) // 4096 * 4096
    add("winner at the last id of a thread's float4", mid, 71, 72)
    add("winner at the first id of the next thread's float4", mid, 72, 71)
    if V > 4096:
        add("winner at the last id of the first 4096-id group", mid, 4095, 4096)
        add("winner at the first id of the second 4096-id group", mid, 4096, 4095)
    if tail > 0:
        add("winner at the first id of the vocabulary tail group", mid, tail, tail - 1)
    add("winner at V - 1", mid, V - 1, V - 2)
    add("winner at id 0", mid, 0, 3)

    def tie(i, j):
        def f(lg):
            lg[i] = WIN
            lg[j] = WIN
        return f
    add("tie of two text ids", mid, None, 3, extra=tie(802, 801), tie=True, expect=801)
    add("tie of a text id and a timestamp", mid, None, 3, extra=tie(900, tsb + 1), tie=True, expect=900)
    for off in (3e4, -3e4):
        add(f"logits offset by {off:+.0e}", mid, 700, 701, extra=lambda lg, off=off: lg.add_(off))
    return cases


def case_margin(case: DR.SelectCase, rules, opts: Options) -> float:
    """top1 - top2 of the case's filtered logits (0 for a constructed tie)"""
    x = apply_filters(case.logits, case.sampled, rules, opts).double()
    top = torch.topk(x, 2).values
    return float(top[0] - top[1])


def sampling_cases(V, rules, n_rows=24, seed=0) -> List[DR.SelectCase]:
    """Rows for the temperature > 0 kernel without the rules: first-step, second-step and mid-text states over a few dozen plausible
    candidates among text ids, timestamps, blank and eot."""
    g = torch.Generator().manual_seed(8000 + seed + V)
    tsb = rules.timestamp_begin
    cases = []
    for r in range(n_rows):
        lg = DR.BACKGROUND + 0.5 * torch.randn(V, generator=g)
        ids = torch.cat([torch.randperm(tsb, generator=g)[:40], tsb + torch.randperm(V - tsb, generator=g)[:8],
                         torch.tensor([rules.blank, rules.eot])])
        lg[ids] = 3.0 * torch.rand(len(ids), generator=g)
        lg[rules.no_speech] = 1.0
        sampled = [[], [DR.TEXT], [DR.TEXT, tsb + 2], [DR.TEXT, DR.TEXT + 1, DR.TEXT + 2]][r % 4]
        cases.append(DR.SelectCase(f"sampling row {r}", lg, list(sampled), prompt=[rules.sot]))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# beam: three windows per launch -- one on its first sampled step (the blank / eot ban shows), two mid-decode
# ---------------------------------------------------------------------------------------------------------------------------------
def beam_case(V: int, rules, opts: Options, beam: int, seed: int = 0) -> BR.BeamCase:
    tsb, eot, blank = rules.timestamp_begin, rules.eot, rules.blank
    K, mc = beam + 1, BR.max_candidates(beam)
    TEXT = BR.TEXT
    banned = set(suppress_list(rules, opts)) | {rules.no_timestamps, blank, eot}
    pool = torch.tensor([i for i in range(10, min(eot, tsb)) if i not in banned and not (TEXT <= i < TEXT + 32)])
    tops = 6.0 - 0.8 * torch.arange(K, dtype=torch.float32)
    for attempt in range(200):
        g = torch.Generator().manual_seed(70000 + 1000 * seed + 17 * beam + V % 101 + 100003 * attempt)
        R_ = 3 * beam
        logits = BR.BACKGROUND + 0.5 * torch.randn(R_, V, generator=g)
        sampled, slp = [], []
        # window 0: first sampled step; row 0 decides.  A text id, a timestamp and <|notimestamps|> are among the proposals; blank and
        # eot stand above all of them and are banned (suppress_blank) -- or lead the proposals (suppress_blank off)
        for j in range(beam):
            sampled.append([]); slp.append(0.0)
            ids = pool[torch.randperm(len(pool), generator=g)[:K]].clone()
            ids[0] = tsb + 3
            if K > 2:
                ids[2] = rules.no_timestamps
            logits[j, ids] = tops + (0.0 if j == 0 else 3.0)
            logits[j, blank] = 9.0
            logits[j, eot] = 8.0
            logits[j, rules.no_speech] = 0.5              # (below every proposal: a call without SuppressTokens allows it)
        # windows 1 and 2: three tokens / one token in
        for w, hist in ((1, lambda j: [tsb + 7, TEXT + j, TEXT + 10 + j]), (2, lambda j: [TEXT + j])):
            res = torch.randperm(8, generator=g)[:beam].tolist()
            ms = torch.randint(0, 3, (beam,), generator=g).tolist()
            if w == 1:
                ms[0] = 0                                # row 0 stands high: its eot is walked before `beam` rows survive
            for j in range(beam):
                r = w * beam + j
                sampled.append(hist(j)); slp.append(-(1.0 + 0.1 * res[j] + 0.8 * ms[j]))
                ids = pool[torch.randperm(len(pool), generator=g)[:K]].clone()
                if w == 1:
                    if j == 0:
                        ids[0] = eot                         # a hypothesis finishes
                    if j == beam - 1:
                        ids[K - 1] = tsb + 2                 # a timestamp below the last one: allowed without the rules
                else:
                    if j == 0:
                        ids[0] = blank                       # step 1: the ban is over
                    if j == beam - 1 and beam > 1:
                        ids[K - 1] = eot
                logits[r, ids] = tops
        case = BR.BeamCase(beam, mc, "no rules", logits, sampled, slp, [0] * R_, 1, [0, 0, 0])
        if beam_gaps_ok(case, rules, opts):
            return case
    raise AssertionError("no decided case found")


def beam_candidates(case: BR.BeamCase, rules, opts: Options, window: int):
    beam = case.beam
    first = len(case.sampled[window * beam]) == 0
    props, cands = [], []
    for j in range(beam):
        r = window * beam + j
        pr = [] if (first and j > 0) else propose(case.logits[r], case.sampled[r], rules, opts, beam + 1)
        props.append(pr)
        cands += [(case.sum_logprob[r] + lp, j, i) for i, lp in pr]
    return cands, props


def beam_gaps_ok(case: BR.BeamCase, rules, opts: Options) -> bool:
    beam = case.beam
    for w in range(3):
        for j in range(beam):
            r = w * beam + j
            if len(case.sampled[r]) == 0 and j > 0:
                continue
            x = apply_filters(case.logits[r], case.sampled[r], rules, opts).double().numpy()
            x = np.sort(x[np.isfinite(x)])[::-1]
            if len(x) < beam + 2 or x[beam] - x[beam + 1] < BR.ROW_GAP:
                return False
        sc = sorted(c[0] for c in beam_candidates(case, rules, opts, w)[0])
        if any(b - a < BR.SCORE_GAP for a, b in zip(sc, sc[1:])):
            return False
        if len(BR.walk(beam_candidates(case, rules, opts, w)[0], beam, rules.eot)[0]) < beam:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
# prompts
# ---------------------------------------------------------------------------------------------------------------------------------
def expand_suppress_tokens(spec, non_speech: Sequence[int], specials: Sequence[int]) -> Optional[List[int]]:
    """decoding.py::_get_suppress_tokens; None: the filter is skipped (the option is falsy)"""
    if spec is None:
        return None
    ids = [int(t) for t in spec.split(",") if t.strip()] if isinstance(spec, str) else [int(t) for t in spec]
    if len(ids) == 0:
        return None
    if -1 in ids:
        ids = [t for t in ids if t >= 0]
        ids.extend(non_speech)
    ids.extend(specials)
    return sorted(set(ids))


def prefix_tokens(encode: Callable[[str], List[int]], prefix, n_ctx: int, sample_len: Optional[int]) -> List[int]:
    if not prefix:
        return []
    toks = encode(" " + prefix.strip()) if isinstance(prefix, str) else list(prefix)
    if sample_len is not None:
        room = min(max(n_ctx // 2 - sample_len, 0), len(toks))     # the last `room` tokens (none where sample_len leaves no room)
        toks = toks[len(toks) - room:]
    return list(toks)


def initial_tokens(rules, prompt: Sequence[int], sot_sequence: Sequence[int], n_ctx: int, without_timestamps: bool = False,
                   prefix: Sequence[int] = ()) -> List[int]:
    """decoding.py::_get_initial_tokens: [sot_prev] + prompt[-(n_ctx // 2 - 1):] + sot_sequence [+ <|notimestamps|>] + prefix"""
    tokens = list(sot_sequence)
    if without_timestamps:
        tokens.append(rules.no_timestamps)
    tokens += list(prefix)
    if len(prompt):
        tokens = [rules.sot_prev] + list(prompt)[-(n_ctx // 2 - 1):] + tokens
    return tokens


# ---------------------------------------------------------------------------------------------------------------------------------
# the window loop with clips and carry_initial_prompt, as upstream's flat loop
# ---------------------------------------------------------------------------------------------------------------------------------
def seek_clips(clip_timestamps, content_frames: int) -> List[Tuple[int, int]]:
    if isinstance(clip_timestamps, str):
        clip_timestamps = [float(ts) for ts in (clip_timestamps.split(",") if clip_timestamps else [])]
    points = [round(ts * FRAMES_PER_SECOND) for ts in clip_timestamps]
    if len(points) == 0:
        points.append(0)
    if len(points) % 2 == 1:
        points.append(content_frames)
    return list(zip(points[::2], points[1::2]))


def transcribe_loop(content_frames: int, rules, n_ctx: int, decode: Callable[[dict], dict], decode_text: Callable[[List[int]], str],
                    initial_prompt_tokens: Sequence[int] = (), clip_timestamps="0", carry_initial_prompt: bool = False,
                    condition_on_previous_text: bool = True, without_timestamps: bool = False, prefix: Sequence[int] = (),
                    sot_sequence: Optional[Sequence[int]] = None, no_speech_threshold: Optional[float] = 0.6,
                    logprob_threshold: Optional[float] = -1.0, max_windows: int = 10000) -> dict:
    """transcribe.py's main loop.  decode(window) -> dict(tokens, temperature, avg_logprob, no_speech_prob) for window = dict(seek,
    segment_size, prompt = the initial tokens).  A clip that starts at or behind the content's end holds no window (upstream leaves
    that case to a negative segment size).  -> dict(windows, segments, tokens)."""
    tsb, eot = rules.timestamp_begin, rules.eot
    sot_sequence = [rules.sot] if sot_sequence is None else list(sot_sequence)
    clips = seek_clips(clip_timestamps, content_frames)
    ipt = list(initial_prompt_tokens)
    all_tokens = list(ipt)
    remaining_prompt_length = n_ctx // 2 - 1 - len(ipt)
    prompt_reset_since = 0
    windows, all_segments = [], []
    clip_idx = 0
    seek = clips[0][0]
    while clip_idx < len(clips) and len(windows) < max_windows:
        clip_start, clip_end = clips[clip_idx]
        if seek < clip_start:
            seek = clip_start
        if seek >= clip_end or seek >= content_frames:
            clip_idx += 1
            if clip_idx < len(clips):
                seek = clips[clip_idx][0]
            continue
        time_offset = seek * HOP / SAMPLE_RATE
        segment_size = min(N_FRAMES, content_frames - seek, clip_end - seek)
        segment_duration = segment_size * HOP / SAMPLE_RATE
        if carry_initial_prompt:
            nignored = max(len(ipt), prompt_reset_since)
            prompt = ipt + all_tokens[nignored:][-remaining_prompt_length:]
        else:
            prompt = all_tokens[prompt_reset_since:]
        window = dict(seek=seek, segment_size=segment_size,
                      prompt=initial_tokens(rules, prompt, sot_sequence, n_ctx, without_timestamps, prefix))
        result = decode(window)
        windows.append(window)
        tokens = list(result["tokens"])
        if no_speech_threshold is not None:
            should_skip = result["no_speech_prob"] > no_speech_threshold
            if logprob_threshold is not None and result["avg_logprob"] > logprob_threshold:
                should_skip = False
            if should_skip:
                seek += segment_size
                continue
        previous_seek = seek
        current = []

        def new_segment(start, end, toks):
            return dict(seek=previous_seek, start=start, end=end, tokens=list(toks), text=decode_text([t for t in toks if t < eot]))

        stamp = [t >= tsb for t in tokens]
        single_ending = stamp[-2:] == [False, True]
        consecutive = [i + 1 for i in range(len(tokens) - 1) if stamp[i] and stamp[i + 1]]
        if consecutive:
            slices = consecutive + ([len(tokens)] if single_ending else [])
            last_slice = 0
            for cur in slices:
                sl = tokens[last_slice:cur]
                current.append(new_segment(time_offset + (sl[0] - tsb) * TIME_PRECISION, time_offset + (sl[-1] - tsb) * TIME_PRECISION, sl))
                last_slice = cur
            if single_ending:
                seek += segment_size
            else:
                seek += (tokens[last_slice - 1] - tsb) * INPUT_STRIDE
        else:
            duration = segment_duration
            stamps = [t for t in tokens if t >= tsb]
            if len(stamps) > 0 and stamps[-1] != tsb:
                duration = (stamps[-1] - tsb) * TIME_PRECISION
            current.append(new_segment(time_offset, time_offset + duration, tokens))
            seek += segment_size
        for sg in current:
            if sg["start"] == sg["end"] or sg["text"].strip() == "":
                sg["text"], sg["tokens"] = "", []
        all_segments.extend(current)
        all_tokens.extend(t for sg in current for t in sg["tokens"])
        if not condition_on_previous_text or result["temperature"] > 0.5:
            prompt_reset_since = len(all_tokens)
        if seek <= previous_seek:                                # (the product's guard: never loop on one window)
            seek = previous_seek + segment_size
    return dict(windows=windows, segments=all_segments, tokens=all_tokens[len(ipt):])


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk of a decode through oracle/whisper_ref.WhisperRef under the options' filters
# ---------------------------------------------------------------------------------------------------------------------------------
WALK_EPS = 0.02
WALK_SAMPLE_LEN = 12
WALK_MODEL_SEED, WALK_CLIP_SEEDS, WALK_CLIP_SECONDS = 3, (40, 41), (6.0, 11.0)
WALK_PREFIX = (1200, 2300, 3400)


def oracle_walk(orc, xa_row, prompt: Sequence[int], rules, opts: Options, sample_len: int, forced: Optional[Sequence[int]] = None,
                eps: float = WALK_EPS) -> dict:
    """The eps-argmax walk of ONE window: free-running (forced None: the oracle's own argmax) or teacher-forced with a decode's tokens
    (eot appended by the caller where the decode ended on it).  Every forced token must lie within eps of the oracle's filtered
    maximum and equal its argmax where the oracle's margin exceeds 2 eps (`decisive` counts those steps); `violations` lists the
    steps that do not.  sum_logprob (fp64, eot's step included) and no_speech_prob (at <|startoftranscript|>) are the oracle's."""
    seq, sampled, decisive, violations, slp = list(prompt), [], 0, [], 0.0
    sot_index = list(prompt).index(rules.sot)
    no_speech = None
    n = sample_len if forced is None else len(forced)
    for i in range(n):
        logits = orc.decoder_logits(torch.tensor([seq]), xa_row)[0]
        if no_speech is None:
            no_speech = float(torch.softmax(logits[sot_index].double(), dim=-1)[rules.no_speech])
        lg = apply_filters(logits[-1].float(), sampled, rules, opts)
        top = torch.topk(lg.double(), 2).values
        margin = float(top[0] - top[1])
        t = int(lg.argmax()) if forced is None else int(forced[i])
        if float(lg[t]) < float(lg.max()) - eps:
            violations.append((i, t, int(lg.argmax()), float(lg.max()) - float(lg[t])))
        if margin > 2 * eps:
            decisive += 1
            if t != int(lg.argmax()):
                violations.append((i, t, int(lg.argmax()), "decisive"))
        slp += float(torch.log_softmax(lg.double(), dim=-1)[t])
        seq.append(t); sampled.append(t)
        if t == rules.eot:
            break
    return dict(tokens=sampled, steps=len(sampled), decisive=decisive, violations=violations, sum_logprob=slp, no_speech_prob=no_speech)


def walk_cases(rules) -> dict:
    """The decodes tests/test_decode_options_gpu.py runs through the model (and the CPU test walks through the oracle alone):
    name -> (prompt, Options).  "suppress list" bans every text id below 20000 on top of the rules' list."""
    call = tuple(sorted(set(rules.suppress) | set(range(0, 20000))))
    return {
        "without_timestamps": ([rules.sot, rules.no_timestamps], Options(True)),
        "prefix": ([rules.sot] + list(WALK_PREFIX), Options()),
        "suppress list": ([rules.sot], Options(False, True, call)),
    }
