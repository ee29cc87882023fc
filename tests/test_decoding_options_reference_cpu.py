"""CPU: tests/decoding_options_reference.py -- the plain-Python statement of the per-call decoding options the GPU tests compare the
kernels and the model against ([UPSTREAM-RECALL: whisper/decoding.py, whisper/transcribe.py]; parity unpinned) -- and the host half of
`WhisperModel(decoding_options=True)`: `clearconverse_amd.decoding_options` and `WindowLoop` with clips, prefix, <|notimestamps|> and
carry_initial_prompt.

  * the restated filters equal oracle/whisper_ref.apply_filters for the defaults; every branch of the new rules by hand
  * the kernel cases are decided (margin >= 0.5, ties only where constructed) and each mutation of MUTATIONS changes some case
  * 300 seeded window-loop scripts: the flat loop of the reference against the product's WindowLoop
  * hand-derived answers for the clips and the carried prompt; prefix truncation; the suppress_tokens expansion
  * the oracle alone walks the decodes of tests/test_decode_options_gpu.py: at least half of every walk's steps are decisive
"""
import numpy as np
import pytest
import torch

from clearconverse_amd import decoding_options as PO
from clearconverse_amd.tokenizer import DecodeRules, IdTokenizer
from clearconverse_amd.whisper import WindowLoop
from oracle import whisper_ref as R
from tests import beam_reference as BR
from tests import dec_reference as DR
from tests import decoding_options_reference as DO

RULES = DecodeRules()
TSB, EOT = RULES.timestamp_begin, RULES.eot
ORULES = R.Rules(suppress=tuple(RULES.suppress))
N_CTX = 448


def ts(seconds: float) -> int:
    return TSB + int(round(seconds / 0.02))


# ---------------------------------------------------------------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------------------------------------------------------------
HISTORIES = [[], [ts(0.4)], [ts(0.4), 400], [ts(0.4), 400, ts(1.0)], [ts(0.4), 400, ts(1.0), ts(1.0)], [ts(0.0), 400, 401, 402]]


@pytest.mark.parametrize("mit", [50, 0, None])
def test_default_options_are_the_oracles_filters(mit):
    g = torch.Generator().manual_seed(5)
    rules = R.Rules(suppress=tuple(RULES.suppress), max_initial_timestamp_index=mit)
    for k, sampled in enumerate(HISTORIES * 3):
        lg = 3.0 * torch.randn(51864, generator=g)
        if k % 2:
            lg[TSB:] += 4.0                                   # the timestamps' mass beats the text: the force rule fires
        assert torch.equal(DO.apply_filters(lg, sampled, rules), R.apply_filters(lg, sampled, rules)), (mit, sampled)
        # max_initial_timestamp given by the call instead of by the rules
        other = R.Rules(suppress=tuple(RULES.suppress), max_initial_timestamp_index=7)
        assert torch.equal(DO.apply_filters(lg, sampled, other, DO.Options(max_initial_timestamp_index=-1 if mit is None else mit)),
                           R.apply_filters(lg, sampled, rules))


def test_every_branch_of_the_new_rules_by_hand():
    lg = torch.zeros(51864)
    banned = lambda x: set(torch.nonzero(torch.isinf(x)).flatten().tolist())
    sup = set(RULES.suppress)
    nt, blank = RULES.no_timestamps, RULES.blank
    # without_timestamps: step 0 bans the list, blank and eot -- and nothing else (no timestamp, no <|notimestamps|>, no text range)
    assert banned(DO.apply_filters(lg, [], ORULES, DO.Options(True))) == sup | {blank, EOT}
    # ... later steps the list alone, whatever the history holds
    for hist in HISTORIES[1:]:
        assert banned(DO.apply_filters(lg, hist, ORULES, DO.Options(True))) == sup
    # suppress_blank off
    assert banned(DO.apply_filters(lg, [], ORULES, DO.Options(True, False))) == sup
    # the call's list replaces the rules'; an empty one switches SuppressTokens off
    assert banned(DO.apply_filters(lg, [400], ORULES, DO.Options(True, True, (5, 6)))) == {5, 6}
    assert banned(DO.apply_filters(lg, [400], ORULES, DO.Options(True, True, ()))) == set()
    assert banned(DO.apply_filters(lg, [], ORULES, DO.Options(True, True, ()))) == {blank, EOT}
    # with the rules on the list is replaced too, <|notimestamps|> stays banned, and suppress_blank is a no-op on step 0
    text_high = lg.clone()
    text_high[:TSB] = 20.0                                    # (keeps the force-timestamp rule out of this check)
    mid = DO.apply_filters(text_high, [ts(0.4), 400], ORULES, DO.Options(False, True, (5, 6)))
    assert banned(mid) == {5, 6, nt} | set(range(TSB, ts(0.4) + 1))
    for sb in (True, False):
        first = DO.apply_filters(lg, [], ORULES, DO.Options(False, sb, (5, 6), 3))
        assert banned(first) == set(range(TSB)) | {nt} | set(range(TSB + 4, 51864))


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1024, 51864])
def test_select_cases_are_decided_and_sensitive(V):
    rules = BR.rules_for(V)
    hit = {m: 0 for m in DO.MUTATIONS}
    for name, opts in DO.option_sets(rules).items():
        cases = DO.select_cases(V, rules, opts)
        assert len(cases) >= 20
        for c in cases:
            if c.expect is None:
                continue
            st = c.state(rules)
            assert not st.done and st.pos >= st.prompt_len - 1
            margin = DO.case_margin(c, rules, opts)
            assert (margin == 0.0) if c.tie else (margin >= 0.5), (name, c.name, margin)
            want = DO.select_no_rules(c.logits, c.sampled, rules, opts)
            assert want == c.expect == int(DO.apply_filters(c.logits, c.sampled, rules, opts).argmax()), (name, c.name)
            for m in DO.MUTATIONS:
                hit[m] += DO.select_no_rules(c.logits, c.sampled, rules, opts, m) != want
    assert all(n >= 1 for n in hit.values()), hit


@pytest.mark.parametrize("V", [1024, 51864])
def test_sampling_cases_have_many_candidates(V):
    rules = BR.rules_for(V)
    for c in DO.sampling_cases(V, rules):
        x = DO.apply_filters(c.logits, c.sampled, rules, DO.Options(True))
        assert int((x > -5.0).sum()) >= 30


@pytest.mark.parametrize("beam", [1, 2, 5])
def test_beam_cases_are_decided(beam):
    rules = BR.rules_for(1024)
    for name, opts in DO.option_sets(rules).items():
        case = DO.beam_case(1024, rules, opts, beam)
        assert DO.beam_gaps_ok(case, rules, opts)
        assert [len(case.sampled[w * beam]) for w in range(3)] == [0, 3, 1]
        cands, props = DO.beam_candidates(case, rules, opts, 0)
        ids0 = [i for i, _ in props[0]]
        if opts.suppress_blank:                               # the ban shows: blank (9.0) and eot (8.0) would lead the proposals
            assert rules.blank not in ids0 and rules.eot not in ids0 and ids0[0] == rules.timestamp_begin + 3
        else:
            assert ids0[:2] == [rules.blank, rules.eot][:len(ids0)]
        assert all(p == [] for p in props[1:])
        # mid-decode: an eot finishes in window 1, blank leads a row of window 2, a timestamp below the last one is proposed
        assert len(BR.walk(DO.beam_candidates(case, rules, opts, 1)[0], beam, rules.eot)[1]) >= 1
        assert DO.beam_candidates(case, rules, opts, 2)[1][0][0][0] == rules.blank
        assert any(i == rules.timestamp_begin + 2 for _, _, i in DO.beam_candidates(case, rules, opts, 1)[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# the window loop
# ---------------------------------------------------------------------------------------------------------------------------------
def run_product(content, script, initial_prompt=None, clip_timestamps="0", carry=False, without_timestamps=False, prefix=(),
                condition=True, sample_len=None):
    tok = IdTokenizer()
    loop = WindowLoop(RULES, tok, content, initial_prompt, N_CTX, condition_on_previous_text=condition,
                      without_timestamps=without_timestamps, prefix_tokens=list(prefix), sample_len=sample_len,
                      clips=PO.parse_clip_timestamps(clip_timestamps, content), carry_initial_prompt=carry)
    windows = []
    while loop.active():
        w = dict(seek=loop.seek, segment_size=loop.segment_size(), prompt=loop.initial_tokens())
        r = script(w)
        windows.append(w)
        loop.advance(dict(tokens=list(r["tokens"]), avg_logprob=r["avg_logprob"], no_speech_prob=r["no_speech_prob"]), r["temperature"])
        assert len(windows) < 400
    out = loop.result()
    return dict(windows=windows, segments=out["segments"], tokens=out["tokens"])


def run_reference(content, script, initial_prompt=None, clip_timestamps="0", carry=False, without_timestamps=False, prefix=(),
                  condition=True):
    tok = IdTokenizer()
    ipt = tok.encode(" " + initial_prompt.strip()) if initial_prompt else []
    return DO.transcribe_loop(content, RULES, N_CTX, script, tok.decode, ipt, clip_timestamps, carry, condition, without_timestamps, prefix)


def seeded_script(seed, without_timestamps):
    """a decode result that depends on (seed, seek, segment_size) only: token strings of every shape the segment rules tell apart"""
    def script(w):
        g = np.random.default_rng([seed, w["seek"], w["segment_size"]])
        dur = w["segment_size"] / 100.0
        text = lambda k: [int(x) for x in g.integers(1000, 40000, k)]
        kind = int(g.integers(0, 6))
        if without_timestamps or kind == 0:
            toks = text(int(g.integers(0, 5)))
        else:
            a = round(float(g.uniform(0, dur / 3)) / 0.02) * 0.02
            b = round(float(g.uniform(a + 0.02, max(a + 0.04, 2 * dur / 3))) / 0.02) * 0.02
            c = round(float(g.uniform(b, max(b + 0.02, dur))) / 0.02) * 0.02
            toks = {1: [ts(a)] + text(2) + [ts(b)],
                    2: [ts(a)] + text(2) + [ts(b), ts(b)] + text(1) + [ts(c)],
                    3: [ts(a)] + text(1) + [ts(b), ts(b)] + text(2),
                    4: [ts(a)] + text(2) + [ts(b), ts(b)],
                    5: [ts(0.0)] + text(3)}[kind]
        silent = g.random() < 0.15
        return dict(tokens=toks, temperature=float(g.choice([0.0, 0.0, 0.4, 0.8])), avg_logprob=-1.5 if silent else -0.4,
                    no_speech_prob=0.9 if silent else 0.1)
    return script


def test_300_seeded_window_loops_against_the_flat_loop():
    seen_windows = 0
    for seed in range(300):
        g = np.random.default_rng(1000 + seed)
        content = int(g.integers(50, 9000))
        n_pts = int(g.integers(0, 6))
        pts = np.sort(g.uniform(0, content / 100.0 + 8.0, n_pts)).round(2).tolist()
        spec = ",".join(str(p) for p in pts) if seed % 2 else pts
        ip = None if seed % 3 == 0 else " ".join(f"<{int(t)}>" for t in g.integers(1000, 40000, int(g.choice([2, 9, 240]))))
        kw = dict(initial_prompt=ip, clip_timestamps=spec, carry=bool(seed % 4 >= 2), without_timestamps=bool(seed % 5 == 0),
                  prefix=tuple(int(t) for t in g.integers(1000, 40000, int(g.integers(0, 4)))), condition=bool(seed % 7))
        script = seeded_script(seed, kw["without_timestamps"])
        got, want = run_product(content, script, **kw), run_reference(content, script, **kw)
        assert got["windows"] == want["windows"], seed
        assert got["segments"] == want["segments"] and got["tokens"] == want["tokens"], seed
        seen_windows += len(got["windows"])
    assert seen_windows > 600


A, B_, C_ = 1000, 2000, 3000


def const_script(tokens, temperature=0.0):
    return lambda w: dict(tokens=list(tokens), temperature=temperature, avg_logprob=-0.4, no_speech_prob=0.1)


@pytest.mark.parametrize("run", [run_product, run_reference])
def test_clips_by_hand(run):
    geometry = lambda out: [(w["seek"], w["segment_size"]) for w in out["windows"]]
    # "5,12,20" on 25 s: (5, 12) and (20, the content's end)
    out = run(2500, const_script([A]), clip_timestamps="5,12,20")
    assert geometry(out) == [(500, 700), (2000, 500)]
    assert [(s["start"], s["end"]) for s in out["segments"]] == [(5.0, 12.0), (20.0, 25.0)]
    # a clip longer than 30 s takes two windows
    assert geometry(run(6000, const_script([A]), clip_timestamps=[0.0, 45.0])) == [(0, 3000), (3000, 1500)]
    # a clip that starts behind the content's end holds no window; one that ends behind it is cut by the content
    assert geometry(run(2500, const_script([A]), clip_timestamps="30,40")) == []
    assert geometry(run(2500, const_script([A]), clip_timestamps="5,10,30,40")) == [(500, 500)]
    assert geometry(run(2500, const_script([A]), clip_timestamps="20,40")) == [(2000, 500)]
    # an empty string is the whole clip, as "0" is
    assert geometry(run(4000, const_script([A]), clip_timestamps="")) == geometry(run(4000, const_script([A]))) == [(0, 3000), (3000, 1000)]
    # inside a clip the timestamp rule moves seek as ever: "<0.00> a <2.00><2.00> b" resumes at 2.0 s into the clip
    out = run(2500, lambda w: dict(tokens=[ts(0), A, ts(2), ts(2), B_] if w["seek"] == 500 else [ts(0), B_, ts(1)], temperature=0.0,
                                   avg_logprob=-0.4, no_speech_prob=0.1), clip_timestamps="5,12")
    assert geometry(out) == [(500, 700), (700, 500)]


@pytest.mark.parametrize("run", [run_product, run_reference])
def test_carry_initial_prompt_by_hand(run):
    sot, prev = RULES.sot, RULES.sot_prev
    temps = {0: 0.8, 3000: 0.0, 6000: 0.0}
    script = lambda w: dict(tokens={0: [A, B_], 3000: [C_], 6000: [A]}[w["seek"]], temperature=temps[w["seek"]], avg_logprob=-0.4,
                            no_speech_prob=0.1)
    # after a high-temperature window the prompt is reset -- the carried initial prompt stays, and later tokens follow it
    out = run(9000, script, initial_prompt="<7000> <7001>", carry=True, without_timestamps=True)
    nt = RULES.no_timestamps
    assert [w["prompt"] for w in out["windows"]] == [[prev, 7000, 7001, sot, nt], [prev, 7000, 7001, sot, nt], [prev, 7000, 7001, C_, sot, nt]]
    out = run(9000, script, initial_prompt="<7000> <7001>", carry=False, without_timestamps=True)
    assert [w["prompt"] for w in out["windows"]] == [[prev, 7000, 7001, sot, nt], [sot, nt], [prev, C_, sot, nt]]
    # an initial prompt longer than n_ctx // 2 - 1 = 223: the remaining length is -7, the slice [-(-7):] drops the first 7 tokens, and
    # the builder keeps the last 223 of the whole
    ipt = list(range(5000, 5230))
    long_prompt = " ".join(f"<{t}>" for t in ipt)
    ten = list(range(9000, 9010))
    script = lambda w: dict(tokens=ten if w["seek"] == 0 else [A], temperature=0.0, avg_logprob=-0.4, no_speech_prob=0.1)
    out = run(6000, script, initial_prompt=long_prompt, carry=True, without_timestamps=True)
    assert out["windows"][0]["prompt"] == [prev] + ipt[7:] + [sot, nt]
    assert out["windows"][1]["prompt"] == [prev] + (ipt + ten[7:])[-223:] + [sot, nt]


def test_prefix_sot_tail_and_sample_len():
    tok = IdTokenizer()
    loop = WindowLoop(RULES, tok, 3000, None, N_CTX, without_timestamps=True, prefix_tokens=[11, 12, 13], sample_len=5)
    assert loop.initial_tokens() == [RULES.sot, RULES.no_timestamps, 11, 12, 13] == DO.initial_tokens(ORULES, [], [RULES.sot], N_CTX, True, [11, 12, 13])
    assert loop.sot_tail() == 1 and loop.sample_cap() == 5     # (the prefix has a length of its own: ccx_whisper_set_prefix_len)
    loop.advance(dict(tokens=[A, B_], avg_logprob=-0.1, no_speech_prob=0.0))
    assert loop.result()["tokens"] == [A, B_] and not loop.active()          # the prefix is no part of the result
    assert WindowLoop(RULES, tok, 3000, None, N_CTX).sot_tail() == 0
    multi = DecodeRules.multilingual()
    assert WindowLoop(multi, IdTokenizer(multi.eot), 3000, None, N_CTX, language="de", without_timestamps=True).sot_tail() == 3
    # truncation: with a sample_len the last n_ctx // 2 - sample_len tokens; without one, all of them
    words = " ".join(f"<{t}>" for t in range(100, 130))
    for fn in (lambda p, sl: PO.prefix_tokens(tok, p, N_CTX, sl), lambda p, sl: DO.prefix_tokens(tok.encode, p, N_CTX, sl)):
        assert fn(words, None) == list(range(100, 130))
        assert fn("  " + words + " ", 214) == list(range(120, 130))
        assert fn(words, 100) == list(range(100, 130))
        assert fn(words, 224) == [] and fn(None, None) == [] and fn(list(range(5)), 222) == [3, 4]


def test_suppress_tokens_expansion():
    non_speech, specials = PO.non_speech_tokens(RULES), PO.always_suppressed(RULES)
    assert sorted(non_speech + specials) == sorted(RULES.suppress) and not set(non_speech) & set(specials)
    for spec in ("-1", [-1], "-1,5", [7, -1], "5, 6", [5, 6], "", [], None):
        assert PO.parse_suppress_tokens(spec, RULES) == DO.expand_suppress_tokens(spec, non_speech, specials), spec
    assert PO.parse_suppress_tokens("-1", RULES) == sorted(RULES.suppress)
    assert PO.parse_suppress_tokens("5,6", RULES) == sorted([5, 6] + specials)
    assert PO.parse_suppress_tokens("-1,5", RULES) == sorted(set(RULES.suppress) | {5})
    assert PO.parse_suppress_tokens("", RULES) is None and PO.parse_suppress_tokens([], RULES) is None
    # what reaches the library: the default is the rules' own list (nothing to replace), an empty option switches the filter off
    assert PO.resolve(RULES).device_default(RULES) and PO.resolve(RULES, suppress_blank=False).device_default(RULES)
    off = PO.resolve(RULES, suppress_tokens=None)
    assert off.suppress == [] and not off.suppress_default and not off.device_default(RULES)
    assert PO.resolve(RULES, max_initial_timestamp=None).max_initial_timestamp_index == -1
    assert PO.resolve(RULES, max_initial_timestamp=0.5).max_initial_timestamp_index == 25
    assert not PO.resolve(RULES, without_timestamps=True).device_default(RULES)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model walks of tests/test_decode_options_gpu.py, by the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------
def test_oracle_walks_are_decisive():
    from clearconverse_amd.audio import synthetic_clip
    from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    sd = synthetic_whisper_state_dict(dims, seed=DO.WALK_MODEL_SEED)
    orc = R.WhisperRef(R.Dims(**dims.__dict__), sd)
    for seed, seconds in zip(DO.WALK_CLIP_SEEDS, DO.WALK_CLIP_SECONDS):
        clip = torch.from_numpy(synthetic_clip(seed, 30.0)[: int(seconds * 16000)])
        mel = R.pad_or_trim(R.log_mel_spectrogram(clip)[:, : len(clip) // 160], 3000)
        xa = orc.encode(mel[None])
        for name, (prompt, opts) in DO.walk_cases(ORULES).items():
            w = DO.oracle_walk(orc, xa, prompt, ORULES, opts, DO.WALK_SAMPLE_LEN)
            assert not w["violations"] and w["steps"] >= 4, (name, w)
            assert 2 * w["decisive"] >= w["steps"], (seed, name, w["decisive"], w["steps"])
