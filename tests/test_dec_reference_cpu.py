"""CPU: the references the decode-kernel tests compare with (tests/dec_reference.py) are themselves checked --
the attention reference against torch's scaled_dot_product_attention in fp64, the select step, chained, against
oracle.whisper_ref.greedy_decode_cached on the mini model, and the select cases for being DECIDED (no GPU assertion needs an
eps-argmax escape) and SENSITIVE (a one-unit mutation of the kernel's folded ranges changes an expected token)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import whisper_ref as R
from tests import dec_reference as DR


def _kv(seed, n_seq, H, kv_T):
    g = torch.Generator().manual_seed(seed)
    return DR.bf16_round(torch.randn(n_seq, H, kv_T, 64, generator=g)), DR.bf16_round(torch.randn(n_seq, H, kv_T, 64, generator=g))


@pytest.mark.parametrize("H,T,nsplit", [(2, 37, 1), (12, 257, 6), (2, 5, 8), (3, 1500, 7)])
def test_attention_reference_equals_sdpa(H, T, nsplit):
    k, v = _kv(H + T, 2, H, T + 3)
    k[:, :, T:], v[:, :, T:] = math.nan, math.nan             # the padding is never read
    q = torch.randn(2, H, 64, generator=torch.Generator().manual_seed(1)) * 2.0
    out, vmax, (pm, pl, po) = DR.attention_ref(q, k, v, [T, T], nsplit=nsplit)
    want = F.scaled_dot_product_attention(q.double()[:, :, None, :], k[:, :, :T].double(), v[:, :, :T].double(), scale=0.125)[:, :, 0]
    assert float((out - want).abs().max()) < 1e-12
    assert torch.equal(vmax, v[:, :, :T].double().abs().amax(dim=(2, 3)))
    # the exact partials merge to the same output; splits behind the last key are empty
    merged = DR.merge_partials(po, torch.stack([pm, pl], dim=-1))
    assert float((merged - want).abs().max()) < 1e-12
    per = -(-T // nsplit)
    for s in range(nsplit):
        assert bool((pl[:, :, s] == 0).all()) == (s * per >= T)


def test_attention_reference_causal_length_and_row_map():
    """self attention: row r sees keys [0, pos[r]] of ITS sequence -- against sdpa with an explicit mask"""
    H, kv_T = 2, 12
    k, v = _kv(3, 2, H, kv_T)
    pos, row_seq = [0, 7, 11, 3], [1, 0, 1, 1]
    q = torch.randn(4, H, 64, generator=torch.Generator().manual_seed(2))
    out, _ = DR.attention_ref(q, k, v, [p + 1 for p in pos], row_seq=row_seq)
    for r in range(4):
        mask = torch.arange(kv_T)[None, None, :] <= pos[r]
        want = F.scaled_dot_product_attention(q[r].double()[:, None, :], k[row_seq[r]].double(), v[row_seq[r]].double(),
                                              attn_mask=mask.expand(H, 1, kv_T), scale=0.125)[:, 0]
        assert float((out[r] - want).abs().max()) < 1e-12


def test_half_ulp_and_pattern_keys():
    ref = torch.tensor([1.0, 1.99, 2.0, -0.75, 0.0], dtype=torch.float64)
    assert DR.half_ulp_bf16(ref)[:4].tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9]
    # bf16 rounding of a value never exceeds half an ulp: fp32 draws, so that the value is rounded once and the bound holds exactly
    x = torch.randn(10000, generator=torch.Generator().manual_seed(6))
    assert bool(((DR.bf16_round(x).double() - x.double()).abs() <= DR.half_ulp_bf16(x.double())).all())
    assert [DR.np_pieces(t) for t in (16, 512, 513, 768, 769, 1536, 1537)] == [4, 4, 6, 6, 12, 12, None]
    for T in (1, 5, 37, 257, 1500):
        for streaming in (False, True):
            for ns in (1, 6):
                assert all(0 <= kk < T for kk in DR.pattern_keys(T, streaming, ns).values())
    assert DR.pattern_keys(1500, True)["last_wave"] == 1152 and DR.pattern_keys(1500, False, 6)["last_wave"] == 192


# ---------------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------------
def test_select_step_chained_reproduces_greedy_decode_cached():
    from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=5)
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    rules = DR.rules_for(dims.n_vocab)
    tok_emb, pos_emb = sd["decoder.token_embedding.weight"], sd["decoder.positional_embedding"]
    for seed, prompt, sample_len in ((2, [rules.sot], 6), (3, [rules.sot_prev, 11, 22, rules.sot], 5), (4, [rules.sot], 3)):
        xa = torch.randn(1, dims.n_audio_ctx, dims.n_audio_state, generator=torch.Generator().manual_seed(seed)) * 0.5
        want = R.greedy_decode_cached(orc, xa, prompt, rules, sample_len=sample_len)
        dec = R.CachedDecoder(orc, xa)
        st = DR.SeqState(pos=0, prompt_len=len(prompt))
        gen, cur, n_done, steps = [-7] * sample_len, prompt[0], 0, 0
        x = tok_emb[cur] + pos_emb[0]
        while not st.done:
            logits = dec.step(torch.tensor([[cur]]))[0, -1]
            res = DR.select_step_ref(logits, st, prompt, gen, rules, sample_len, tok_emb, pos_emb)
            st, gen, n_done = res.state, res.gen, n_done + res.finished
            if res.cur_tok is not None:
                cur, x = res.cur_tok, res.x
                assert st.pos == res.pos and torch.equal(x, tok_emb[cur] + pos_emb[st.pos])
            steps += 1
            assert steps < 20
        toks = gen[:st.n_gen]
        text = toks[:toks.index(rules.eot)] if rules.eot in toks else toks
        assert text == want.tokens and st.n_tokens == len(want.tokens) and n_done == 1
        assert abs(st.sum_logprob - want.sum_logprob) < 1e-3
        assert abs(st.no_speech_prob - want.no_speech_prob) < 1e-6
        # a finished row keeps emitting eot until the table is full, then stands still
        for _ in range(sample_len + 1):
            res = DR.select_step_ref(logits, st, prompt, gen, rules, sample_len, tok_emb, pos_emb)
            st, gen = res.state, res.gen
            assert res.x is None and res.finished == 0
        assert st.n_gen == sample_len and all(t == rules.eot for t in gen[toks.index(rules.eot) if rules.eot in toks else sample_len:])


def _groups(V):
    return [(mit, DR.rules_for(V, mit), DR.select_cases(V, DR.rules_for(V, mit), seed=mit + 1)) for mit in (50, 0, -1)]


def _expected(case, rules, V):
    emb = torch.zeros(V, 4), torch.zeros(DR.N_POS, 4)
    gen = (case.sampled + [-7] * DR.SAMPLE_LEN)[:max(DR.SAMPLE_LEN, len(case.sampled))]
    prompt = (case.prompt + [0] * DR.MAX_PROMPT)[:DR.MAX_PROMPT]
    return DR.select_step_ref(case.logits, case.state(rules), prompt, gen, rules, DR.SAMPLE_LEN, *emb)


@pytest.mark.parametrize("vocab", list(DR.VOCABS))
def test_select_cases_are_decided(vocab):
    """margin to the runner-up >= 0.5 (ties: the top two EQUAL and the third 0.5 below), |lse_ts - max_text| >= 0.05 (ties of a text id
    with the only allowed timestamp: exactly 0, the comparison is between equal fp32 numbers), and every case yields what it was built for"""
    V = DR.VOCABS[vocab]
    assert V % 4 == 0 and V <= 53248
    names = set()
    for mit, rules, cases in _groups(V):
        assert len(cases) >= 30
        for c in cases:
            assert c.logits.shape == (V,) and c.logits.dtype == torch.float32 and bool(torch.isfinite(c.logits).all())
            res = _expected(c, rules, V)
            names.add(c.name)
            if res.token is None:
                assert c.expect is None
                continue
            assert c.expect is None or res.token == c.expect, (c.name, res.token, c.expect)
            assert res.token == DR.folded_select(c.logits, c.sampled, rules), c.name
            if c.tie:
                flt = R.apply_filters(c.logits, c.sampled, rules).double()
                top3 = torch.topk(flt, 3).values
                assert top3[0] == top3[1] and top3[1] - top3[2] >= 0.5, c.name
                assert res.token == int(torch.nonzero(flt == top3[0])[0]), c.name
                assert res.force_gap == 0.0 or abs(res.force_gap) >= 0.05, (c.name, res.force_gap)
            else:
                assert res.margin >= 0.5, (c.name, res.margin)
                assert abs(res.force_gap) >= 0.05, (c.name, res.force_gap)
    # the states and outcomes the kernel test relies on are all present
    for needle in ("first step", "one timestamp", "text, timestamp", "closed pair", "mid-range", "V - 1", "prompt phase", "finished row",
                   "sample_len", "eot chosen", "suppressed", "no_timestamps", "float4", "tail group", "tie of", "force rule", "offset"):
        assert any(needle in n for n in names), needle


@pytest.mark.parametrize("vocab", list(DR.VOCABS))
def test_select_cases_are_sensitive_to_every_mutation(vocab):
    V = DR.VOCABS[vocab]
    groups = _groups(V)
    for mutation in DR.MUTATIONS:
        changed = []
        for mit, rules, cases in groups:
            for c in cases:
                st = c.state(rules)
                if st.done or st.pos < st.prompt_len - 1:
                    continue
                if DR.folded_select(c.logits, c.sampled, rules, mutation) != DR.folded_select(c.logits, c.sampled, rules):
                    changed.append(c.name)
        assert changed, f"no case notices the mutation {mutation}"


@pytest.mark.parametrize("temperature", [0.1, 0.7, 5.0])
def test_sampling_cases_leave_out_at_most_two_percent(temperature):
    """the reference's perturbed margin exceeds eps in >= 98 % of the draws, and the force-timestamp comparison is decided in all"""
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.sampling_cases(V, rules)
    eps = DR.sampling_eps(temperature)
    emb = torch.zeros(V, 4), torch.zeros(DR.N_POS, 4)
    close, toks = 0, set()
    for row, c in enumerate(cases):
        gen = (c.sampled + [-7] * DR.SAMPLE_LEN)[:DR.SAMPLE_LEN]
        res = DR.select_step_ref(c.logits, c.state(rules), c.prompt, gen, rules, DR.SAMPLE_LEN, *emb, temperature=temperature, seed=99, row=row)
        assert abs(res.force_gap) >= 0.05
        close += res.margin <= eps
        toks.add(res.token)
        assert math.isfinite(res.logprob)
    assert close <= 0.02 * len(cases)
    assert len(toks) > len(cases) // 2          # the draws are real choices, not one token every time
