"""Plain fp64 references of the decode step's attention forms and of its token-select kernel (csrc/decoder.hip), the generator of
the select kernel's test cases and the comparators the kernel tests use.  CPU only: tests/test_dec_reference_cpu.py checks this file
against torch's scaled_dot_product_attention, against oracle.whisper_ref.greedy_decode_cached and against one-unit mutations of the
select kernel's folded filter ranges; tests/test_dec_attention_gpu.py and tests/test_dec_select_gpu.py check the kernels against it.

Attention: out[r][h] = softmax(q[r][h] . K[seq(r)][h][j] / 8 over the row's keys j) V[seq(r)][h], from the operands the kernel sees
(f32 q, bf16-rounded K and V).  The partial forms leave, per key split s = [s per, min((s + 1) per, T)) with per = ceil(T / nsplit),
(m, l, o) = (max_j t_j, sum_j 2^(t_j - m), sum_j 2^(t_j - m) v_j) with t = score * log2(e) / 8; any m' with l, o rescaled to it is the
same partial, so partials are compared after the merge sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s, and per split as o / l.

Select: one step of the per-sequence state machine of dec_select_kernel (prompt phase, finished rows, filters, force-timestamp rule,
argmax / Gumbel-max draw, log-probability, sample_len exhaustion, next embedding) on oracle.whisper_ref.apply_filters / sample_token.
"""
import math
from dataclasses import dataclass, field, replace
from typing import List, Optional

import numpy as np
import torch

from oracle import whisper_ref as R

LOG2E = 1.4426950408889634
U24 = 2.0 ** -24          # unit roundoff of fp32


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def half_ulp_bf16(ref):
    """half a bf16 ulp at |ref| (fp64 tensor): bf16 keeps 8 significant bits."""
    a = ref.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 8.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def attention_ref(q, k, v, n_keys, row_seq=None, nsplit=0):
    """q [rows, H, 64] f32, k / v [n_seq, H, kv_T, 64] (bf16-rounded values in any float dtype; entries at and behind a row's key
    count are never read, they may be NaN), n_keys [rows] -> out [rows, H, 64] fp64 and vmax [rows, H] (max |v| over the row's keys).
    nsplit >= 1: also the exact partials (m [rows, H, nsplit], l [rows, H, nsplit], o [rows, H, nsplit, 64]) of the kernel's key
    splits; an empty split has m = -inf, l = 0, o = 0."""
    rows, H, _ = q.shape
    out = torch.zeros(rows, H, 64, dtype=torch.float64)
    vmax = torch.zeros(rows, H, dtype=torch.float64)
    ns = max(nsplit, 1)
    pm = torch.full((rows, H, ns), -math.inf, dtype=torch.float64)
    pl = torch.zeros(rows, H, ns, dtype=torch.float64)
    po = torch.zeros(rows, H, ns, 64, dtype=torch.float64)
    for r in range(rows):
        s = r if row_seq is None else int(row_seq[r])
        T = int(n_keys[r])
        kk, vv = k[s, :, :T].double(), v[s, :, :T].double()
        sc = torch.einsum("hd,htd->ht", q[r].double(), kk) * 0.125
        out[r] = torch.einsum("ht,htd->hd", torch.softmax(sc, dim=-1), vv)
        vmax[r] = vv.abs().amax(dim=(1, 2))
        if nsplit >= 1:
            per = -(-T // nsplit)
            t2 = sc * LOG2E
            for i in range(nsplit):
                a, b = i * per, min((i + 1) * per, T)
                if a >= b:
                    continue
                m = t2[:, a:b].amax(dim=1)
                p = torch.exp2(t2[:, a:b] - m[:, None])
                pm[r, :, i], pl[r, :, i] = m, p.sum(dim=1)
                po[r, :, i] = torch.einsum("ht,htd->hd", p, vv[:, a:b])
    if nsplit >= 1:
        return out, vmax, (pm, pl, po)
    return out, vmax


def merge_partials(part_o, part_ml):
    """GPU partials part_o [rows, H, ns, 64], part_ml [rows, H, ns, 2] (f32) merged in fp64 -> [rows, H, 64]."""
    m, l, o = part_ml[..., 0].double(), part_ml[..., 1].double(), part_o.double()
    w = torch.exp2(m - m.amax(dim=-1, keepdim=True))
    return (w[..., None] * o).sum(dim=-2) / (w * l).sum(dim=-1)[..., None]


def bf16_out_excess(got, ref, vmax):
    """worst excess of |got - ref| over half a bf16 ulp of ref, relative to the head's max |v|.  got [rows, H, 64] (the kernel's bf16
    output widened), ref fp64, vmax [rows, H]."""
    ex = ((got.double() - ref).abs() - half_ulp_bf16(ref)).clamp_min(0.0)
    return float((ex / vmax[..., None]).max())


def f32_rel_err(got, ref, vmax):
    return float(((got.double() - ref).abs() / vmax[..., None]).max())


def fused_q_ref(x, pend, pend_n, ln_g, ln_b, eps, wq, bq):
    """The cross-attention query of the fused / two-launch forms: q = bf16(LayerNorm(x + the pending slabs)) bf16(Wq)^T + bq in fp64, the
    LayerNorm output rounded to bf16 as the kernel rounds it.  Also the resolved rows as the kernel adds them (f32, slab by slab)."""
    xr = x.clone()
    for s in range(pend_n):
        xr = xr + pend[s]
    xd = xr.double()
    mean = xd.mean(dim=-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=-1, keepdim=True)
    xn = (xd - mean) / torch.sqrt(var + eps) * ln_g.double() + ln_b.double()
    xn = bf16_round(xn.float()).double()
    return xn @ bf16_round(wq).double().T + bq.double(), xr


def np_pieces(T, nsplit=1):
    """32-key pieces per wave the launcher picks an instantiation for (ccx_launch_dec_attention): 4, 6 or 12; None: the fallback."""
    need = (((T + nsplit - 1) // nsplit + 3) // 4 + 31) // 32
    return 4 if need <= 4 else 6 if need <= 6 else 12 if need <= 12 else None


def pattern_keys(T, streaming, nsplit=1):
    """Keys at which a dominant score exercises the softmax rescale and the merges: key 0, the last key, the first key of the last
    wave that owns keys and a key of the last 32-key piece.  streaming: a wave owns a contiguous range of per_w = ceil(T / 4) rounded up
    to 32 keys (dec_cross_stream_kernel, dec_cross_prefill_kernel); else the waves of a block take the 64-key chunks of its split in
    turn (dec_attention_kernel, dec_cross_fused_q_kernel): the last wave of split 0."""
    if streaming:
        per_w = ((T + 3) // 4 + 31) // 32 * 32
        last_wave = (T - 1) // per_w * per_w
    else:
        n = min((T + nsplit - 1) // nsplit, T)
        last_wave = min(192, (n - 1) // 64 * 64)
    return {"first": 0, "last": T - 1, "last_wave": last_wave, "last_piece": T - 1 - min(5, (T - 1) % 32)}


# ---------------------------------------------------------------------------------------------------------------------------------
# select: one step of the state machine
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class SeqState:
    """DecSeqState (csrc/decoder.h), plus what a launch keeps per row outside it"""
    pos: int = 0
    prompt_len: int = 1
    n_gen: int = 0
    done: int = 0
    last_tok: int = -1
    pen_tok: int = -1
    last_ts_tok: int = -1
    n_tokens: int = 0
    sum_logprob: float = 0.0
    no_speech_prob: float = 0.0


@dataclass
class StepResult:
    state: SeqState
    gen: List[int]                   # the row of the gen table after the step
    cur_tok: Optional[int]           # None: left as it was
    pos: Optional[int]
    x: Optional[torch.Tensor]        # next embedding [D] f32; None: left as it was
    finished: int                    # 1 if the row finished in this step (n_done increment)
    token: Optional[int] = None      # the token chosen (None: prompt phase / finished row)
    logprob: Optional[float] = None  # fp64 log-probability of the token under the filtered logits
    margin: Optional[float] = None   # top1 - top2 of what the argmax ran over (filtered logits, or perturbed scores when sampling)
    force_gap: Optional[float] = None  # lse(timestamps) - max(text) of the filtered logits before the force-timestamp rule (fp64)
    scores: Optional[torch.Tensor] = None   # what the argmax ran over [V]


def state_from_sampled(sampled, prompt_len=1, sum_logprob=0.0, no_speech_prob=0.0, tsb=50363):
    ts = [t for t in sampled if t >= tsb]
    return SeqState(pos=prompt_len - 1 + len(sampled), prompt_len=prompt_len, n_gen=len(sampled), done=0,
                    last_tok=sampled[-1] if sampled else -1, pen_tok=sampled[-2] if len(sampled) >= 2 else -1,
                    last_ts_tok=ts[-1] if ts else -1, n_tokens=0, sum_logprob=sum_logprob, no_speech_prob=no_speech_prob)


def _force_gap(logits, sampled, rules):
    """lse over the allowed timestamps minus the best allowed text logit in fp64: what the force-timestamp rule compares (+-inf if
    one side is empty, 0 if both are)"""
    tsb = rules.timestamp_begin
    z = torch.zeros_like(logits)
    z[:tsb] = 1e4                                          # text far above the timestamp mass: the rule stays out, the filters remain
    allowed = torch.isfinite(R.apply_filters(z, sampled, rules))
    x = logits.double()
    ts, tx = x[tsb:][allowed[tsb:]], x[:tsb][allowed[:tsb]]
    lse = float(torch.logsumexp(ts, 0)) if len(ts) else -math.inf
    mx = float(tx.max()) if len(tx) else -math.inf
    return 0.0 if lse == mx == -math.inf else lse - mx


def select_step_ref(logits, st: SeqState, prompt, gen, rules, sample_len, tok_emb, pos_emb, temperature=0.0, seed=0, row=0):
    """One launch of the select kernel for ONE row.  logits [V] f32 (NaN behind V never enters: pass the first V), prompt: the row of
    the prompt table, gen: the row of the gen table (tokens sampled so far first)."""
    st = replace(st)
    gen = list(gen)
    if st.pos < st.prompt_len - 1:                                   # prompt phase: feed the next prompt token
        st.pos += 1
        tok = int(prompt[st.pos])
        return StepResult(st, gen, tok, st.pos, tok_emb[tok] + pos_emb[st.pos], 0)
    if st.done:                                                      # finished rows keep emitting eot
        if st.n_gen < sample_len:
            gen[st.n_gen] = rules.eot
            st.n_gen += 1
        return StepResult(st, gen, None, None, None, 0)
    i_gen = st.n_gen
    sampled = gen[:i_gen]
    lg32 = logits.float()
    if i_gen == 0:
        st.no_speech_prob = float(torch.softmax(lg32.double(), dim=-1)[rules.no_speech])
    gap = _force_gap(lg32, sampled, rules)
    flt = R.apply_filters(lg32, sampled, rules)
    nxt, _, score = R.sample_token(flt, temperature, seed, row, i_gen)
    top2 = torch.topk(score.double(), 2).values
    margin = float(top2[0] - top2[1])
    logprob = float(torch.log_softmax(flt.double(), dim=-1)[nxt])
    st.sum_logprob = st.sum_logprob + logprob
    gen[i_gen] = nxt
    st.n_gen = i_gen + 1
    st.pen_tok, st.last_tok = st.last_tok, nxt
    if nxt >= rules.timestamp_begin:
        st.last_ts_tok = nxt
    res = StepResult(st, gen, None, None, None, 0, token=nxt, logprob=logprob, margin=margin, force_gap=gap, scores=score)
    if nxt == rules.eot:
        st.done, st.n_tokens, res.finished = 1, i_gen, 1
    elif st.n_gen >= sample_len:
        st.done, st.n_tokens, res.finished = 1, st.n_gen, 1
    else:
        st.pos += 1
        res.cur_tok, res.pos, res.x = nxt, st.pos, tok_emb[nxt] + pos_emb[st.pos]
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# select: the kernel's folded ranges, restated, with one-unit mutations (the proof that the cases below are sensitive)
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("t_lo+1", "t_lo-1", "s_lo+1", "s_lo-1", "s_hi+1", "s_hi-1", "no_suppress", "no_force", "tie_order")


def folded_select(logits, sampled, rules, mutation=None):
    """The greedy token as dec_select_kernel derives it: text ids [t_lo, tsb) and timestamps [s_lo, s_hi) minus the suppress mask, the
    force-timestamp rule, ties to the lowest id.  `mutation`: one of MUTATIONS."""
    V, tsb, i_gen = logits.shape[0], rules.timestamp_begin, len(sampled)
    last_tok = sampled[-1] if sampled else -1
    pen_tok = sampled[-2] if len(sampled) >= 2 else -1
    ts = [t for t in sampled if t >= tsb]
    last_ts_tok = ts[-1] if ts else -1
    last_ts = i_gen >= 1 and last_tok >= tsb
    pen_ts = i_gen < 2 or pen_tok >= tsb
    s_lo = tsb
    if last_ts_tok >= 0:
        s_lo = last_ts_tok if (last_ts and not pen_ts) else last_ts_tok + 1
    s_hi = V
    mit = rules.max_initial_timestamp_index
    if i_gen == 0 and mit is not None and mit >= 0:
        s_hi = tsb + mit + 1
    if last_ts and pen_ts:
        s_hi = s_lo
    t_lo = tsb if i_gen == 0 else (rules.eot if (last_ts and not pen_ts) else 0)
    if mutation in ("t_lo+1", "t_lo-1"):
        t_lo += 1 if mutation[-2] == "+" else -1
    if mutation in ("s_lo+1", "s_lo-1"):
        s_lo += 1 if mutation[-2] == "+" else -1
    if mutation in ("s_hi+1", "s_hi-1"):
        s_hi += 1 if mutation[-2] == "+" else -1
    ids = np.arange(V)
    banned = np.zeros(V, dtype=bool)
    if mutation != "no_suppress":
        banned[list(rules.suppress)] = True
        banned[rules.no_timestamps] = True
    allowed = ~banned & np.where(ids < tsb, ids >= t_lo, (ids >= s_lo) & (ids < s_hi))
    x = np.where(allowed, logits.double().numpy(), -np.inf)
    text, stamps = x[:tsb], x[tsb:]
    bt, it = (text.max(), int(text.argmax())) if len(text) else (-np.inf, 2 ** 31 - 1)
    bs, is_ = (stamps.max(), tsb + int(stamps.argmax())) if len(stamps) else (-np.inf, 2 ** 31 - 1)
    if bt == -np.inf:
        it = 2 ** 31 - 1
    if bs == -np.inf:
        is_ = 2 ** 31 - 1
    fin = stamps[np.isfinite(stamps)]
    lse_ts = float(fin.max() + np.log(np.exp(fin - fin.max()).sum())) if len(fin) else -np.inf
    if lse_ts > bt and mutation != "no_force":
        return is_
    if mutation == "tie_order":
        return it if bt > bs or (bt == bs and it > is_) else is_
    return it if bt > bs or (bt == bs and it < is_) else is_


# ---------------------------------------------------------------------------------------------------------------------------------
# select: the cases
# ---------------------------------------------------------------------------------------------------------------------------------
WIN, RIVAL, DECOY, BACKGROUND = 6.0, 5.0, 9.0, -20.0
SAMPLE_LEN = 6          # of every select launch of the tests: the "n_gen + 1 == sample_len" rows hold 5 tokens
MAX_PROMPT = 4
N_POS = 448
TEXT = 400              # an ordinary text token of the histories


@dataclass
class SelectCase:
    name: str
    logits: torch.Tensor                     # [V] f32
    sampled: List[int] = field(default_factory=list)
    prompt: List[int] = field(default_factory=list)
    pos: Optional[int] = None                # None: the sampling phase at its natural position
    done: int = 0
    sum_logprob: float = 0.0
    tie: bool = False                        # the top two allowed logits are EQUAL by construction (the tie order decides)
    expect: Optional[int] = None             # the id the case was built to produce (None: not a placement case)

    def state(self, rules):
        plen = len(self.prompt)
        st = state_from_sampled(self.sampled, plen, self.sum_logprob, 0.25 if self.sampled else 0.0, rules.timestamp_begin)
        if self.pos is not None:
            st.pos = self.pos
        st.done = self.done
        if self.done:
            st.n_tokens = len(self.sampled)
        return st


def rules_for(V, max_initial_ts=50):
    """The English tokenizer's ids with the suppress list of the product; the vocabulary that ends four ids into the timestamps needs a
    timestamp_begin that is a multiple of 4 (n_vocab % 4 == 0): 50364."""
    from clearconverse_amd.tokenizer import SUPPRESS_TOKENS
    r = R.Rules(suppress=tuple(SUPPRESS_TOKENS), max_initial_timestamp_index=max_initial_ts)
    if V < r.timestamp_begin + 16:
        r.timestamp_begin = V - 4
    return r


VOCABS = {"small.en / mini": 51864, "13 full groups": 53248, "timestamp_begin + 4": 50368}


def select_cases(V, rules, seed=0):
    """The greedy cases of one launch (one row each) for a vocabulary and a rule set.  Background logits -20 +- 0.5 (their summed mass
    stays below e^-11), the winner at 6, a legal rival at 5, banned decoys at 9."""
    g = torch.Generator().manual_seed(1000 + seed + V)
    tsb, eot = rules.timestamp_begin, rules.eot
    nts = V - tsb
    a, b, mid = (3, 7, 700) if nts > 1000 else (0, 2, 1)
    sot = [rules.sot]
    cases = []

    def bg():
        return BACKGROUND + 0.5 * torch.randn(V, generator=g)

    def add(name, sampled, winner=None, rival=None, decoys=(), extra=None, **kw):
        if winner is not None and not (0 <= winner < V):
            return
        lg = bg()
        if rival is not None and 0 <= rival < V:
            lg[rival] = RIVAL
        for d_ in decoys:
            if 0 <= d_ < V:
                lg[d_] = DECOY
        if winner is not None:
            lg[winner] = WIN
        if extra:
            extra(lg)
        if not sampled:
            lg[rules.no_speech] = 2.0                         # a no-speech probability well inside fp32's range
        kw.setdefault("prompt", sot)
        kw.setdefault("sum_logprob", -1.5 if sampled else 0.0)
        cases.append(SelectCase(name, lg, list(sampled), expect=winner, **kw))

    mit = rules.max_initial_timestamp_index
    s_hi0 = tsb + mit + 1 if mit is not None and mit >= 0 else V
    # ---- states ----
    first_rival = tsb + 1 if s_hi0 > tsb + 1 and nts > 1 else None
    add("first step: winner at s_hi - 1, decoys at s_hi, a text id and blank", [], min(s_hi0, V) - 1, first_rival,
        decoys=(s_hi0, TEXT, rules.blank, eot))
    add("first step: winner at timestamp_begin", [], tsb, None if first_rival is None else min(s_hi0, V) - 1, decoys=(tsb - 1, 0))
    one_ts, tt, closed, midst = [tsb + a], [tsb + a, TEXT, tsb + b], [tsb + a, TEXT, tsb + b, tsb + b], [tsb + a, TEXT]
    add("after one timestamp: text only, decoys on the timestamps", one_ts, 1234, 77, decoys=(tsb, tsb + a, V - 1))
    add("after text, timestamp: winner at t_lo = eot (eot chosen), decoy at t_lo - 1", tt, eot, 50300, decoys=(eot - 1, 0))
    add("after text, timestamp: winner at s_lo, decoy at s_lo - 1", tt, tsb + b, eot, decoys=(tsb + b - 1, TEXT))
    add("after a closed pair: text wins, decoys at s_lo - 1, s_lo and V - 1", closed, 31000, 5, decoys=(tsb + b - 1, tsb + b, tsb + b + 1, V - 1))
    add("mid text: winner at s_lo = last + 1, decoy at s_lo - 1", midst, tsb + a + 1, 900, decoys=(tsb + a, tsb))
    add("mid text: winner at t_lo = 0", midst, 0, tsb + a + 1, decoys=(tsb + a,))
    add("last timestamp mid-range: winner at s_lo", [tsb + mid, TEXT], tsb + mid + 1, 901, decoys=(tsb + mid, tsb + mid - 1))
    add("last timestamp mid-range, unpaired: winner at s_lo = last", [tsb, TEXT, tsb + mid], tsb + mid, 50300, decoys=(tsb + mid - 1, eot - 1))
    add("last timestamp at V - 1, unpaired: only V - 1 and eot and above", [tsb, TEXT, V - 1], V - 1, eot, decoys=(V - 2, TEXT))
    add("last timestamp at V - 1, text after it: no timestamp left", [V - 1, TEXT], 4321, 5, decoys=(V - 1, V - 2, tsb))
    add("n_gen + 1 == sample_len: the row stops without eot", [tsb + a, TEXT, TEXT + 1, TEXT + 2, TEXT + 3], 2222, 3333, decoys=(tsb + a,))
    add("eot chosen in mid text", midst, eot, 600)
    add("prompt phase", [], None, prompt=[rules.sot_prev, 11, 22, rules.sot], pos=1)
    add("prompt phase, last prompt token next", [], None, prompt=[rules.sot_prev, 11, 22, rules.sot], pos=2)
    add("sampling phase behind a long prompt", [], tsb, first_rival, prompt=[rules.sot_prev, 11, 22, rules.sot])
    add("finished row", [tsb + a, TEXT, eot], None, done=1, sum_logprob=-1.5)
    add("finished row with a full gen table", [tsb + a, TEXT, eot, eot, eot, eot], None, done=1, sum_logprob=-1.5)
    # ---- placements (mid text: every text id and the timestamps behind tsb + a are allowed) ----
    sup = rules.suppress[0]
    tail = (V - 1) // 4096 * 4096
    add("decoy at a suppressed id", midst, 1000, 1001, decoys=(sup, rules.suppress[-1], rules.sot))
    add("decoy at no_timestamps", midst, rules.no_timestamps - 100, 1001, decoys=(rules.no_timestamps,))
    add("winner at the last id of a thread's float4", midst, 71, 72)
    add("winner at the first id of the next thread's float4", midst, 72, 71)
    add("winner at the last id of the first 4096-id group", midst, 4095, 4096)
    add("winner at the first id of the second 4096-id group", midst, 4096, 4095)
    add("winner at the first id of the vocabulary tail group", midst, tail, tail - 1)
    add("winner just before the vocabulary tail group", midst, tail - 1, tail)
    add("winner at V - 1", midst, V - 1, V - 2 if V - 2 > tsb + a else TEXT)
    add("winner at V - 4 (first id of the last float4)", midst, V - 4 if V - 4 > tsb + a else None, TEXT)
    banned = set(rules.suppress) | {rules.no_timestamps}
    last_text = max(i for i in range(tsb - 200, tsb) if i not in banned)
    add("winner at the last allowed text id, decoys on the banned ids up to timestamp_begin", midst, last_text, tsb + a + 1,
        decoys=tuple(range(last_text + 1, tsb)) + (tsb + a,))

    # ---- ties (exact): the lowest id wins ----
    def tie(i, j, val=WIN):
        def f(lg):
            lg[i] = val
            lg[j] = val
        return f
    add("tie of two text ids", midst, None, 3, extra=tie(2001, 2002), tie=True)
    cases[-1].expect = 2001
    add("tie of two text ids in different 4096-id groups", midst, None, 3, extra=tie(8000, 100), tie=True)
    cases[-1].expect = 100
    if nts > a + 3:
        add("tie of two timestamps", midst, None, 3, extra=tie(tsb + a + 2, tsb + a + 1), tie=True)
        cases[-1].expect = tsb + a + 1
    # one text id against the ONLY allowed timestamp (V - 1 after "text, V - 1"): its mass is its logit exactly, the force rule's
    # comparison is an exact tie too and text, the lower id, wins
    add("tie of a text id and the only allowed timestamp", [tsb, TEXT, V - 1], None, 50300, extra=tie(eot, V - 1), tie=True)
    cases[-1].expect = eot

    # ---- force-timestamp rule: n small timestamps whose summed mass is `gap` above / below (0.15: the runner-up stays 0.5 away at two timestamps too) the best text token ----
    def mass(n, gap, text_id, text_val=2.0):
        def f(lg):
            ids = torch.arange(tsb + a + 1, tsb + a + 1 + n)
            top = 0.75                                       # the timestamp argmax stands 0.75 above its n - 1 mates
            base = text_val + gap - math.log(n - 1 + math.exp(top))
            lg[ids] = base
            lg[ids[n // 2]] = base + top
            lg[text_id] = text_val
        return f
    nm = min(400, nts - a - 2)
    if nm >= 2:
        add("force rule: the summed timestamp mass beats the best text token", midst, None, extra=mass(nm, 0.15, 1500))
        cases[-1].expect = tsb + a + 1 + nm // 2
        add("force rule just below: text wins", midst, None, extra=mass(nm, -0.15, 1500))
        cases[-1].expect = 1500
    # ---- offsets ----
    for off in (3e4, -3e4):
        add(f"logits offset by {off:+.0e}", midst, 1700, 1701, decoys=(tsb + a,), extra=lambda lg, off=off: lg.add_(off))
        if nm >= 2:
            add(f"force rule under an offset of {off:+.0e}", midst, None, extra=lambda lg, off=off: (mass(nm, 0.25, 1500)(lg), lg.add_(off)))
            cases[-1].expect = tsb + a + 1 + nm // 2
    return cases


def sampling_cases(V, rules, n_rows=24, seed=0):
    """Rows for the temperature > 0 kernel: mid-text and first-step states over logits with a few dozen plausible candidates (so the
    draw is a real choice at every temperature) whose force-timestamp comparison is decided."""
    g = torch.Generator().manual_seed(7000 + seed + V)
    tsb = rules.timestamp_begin
    nts = V - tsb
    a = 3 if nts > 1000 else 0
    cases = []
    for r in range(n_rows):
        lg = BACKGROUND + 0.5 * torch.randn(V, generator=g)
        first = r % 4 == 3
        if first:
            ids = tsb + torch.randperm(min(51, nts), generator=g)[: min(40, nts)]
        else:
            ids = torch.randperm(tsb, generator=g)[:48]
            if r % 4 == 1 and nts > a + 12:                   # some timestamps too, well below the text mass
                ids = torch.cat([ids, tsb + a + 1 + torch.randperm(min(nts - a - 1, 200), generator=g)[:8]])
        lg[ids] = 3.0 * torch.rand(len(ids), generator=g)
        if not first:
            lg[ids[ids >= tsb]] -= 4.0
            lg[ids[0]] = 4.0                                  # the best text token clearly above the timestamp mass
        lg[rules.no_speech] = 1.0
        sampled = [] if first else [tsb + a, TEXT] + [TEXT + i for i in range(r % 3)]
        cases.append(SelectCase(f"sampling row {r}", lg, sampled, prompt=[rules.sot]))
    return cases


def sampling_eps(temperature, max_logit=6.0):
    """A-priori eps of the perturbed margin: both sides form logit / T + g in fp32; the quotient and the sum round at
    ulp(max |logit| / T + max |g|) (|g| <= 17), the Gumbel transform -log(-log u) adds a few ulp of |g|: 8 ulp of the largest score."""
    big = max_logit / temperature + 17.0
    return 8.0 * 2.0 ** (math.floor(math.log2(big)) - 23)
