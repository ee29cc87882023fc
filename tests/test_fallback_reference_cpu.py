"""CPU: the temperature-fallback and best_of rules of clearconverse_amd/fallback.py against hand-derived answers and against the
restatement in tests/fallback_reference.py (written from the rules, not from the product), the round planner over seeded pass / fail
tables, the stream-id rule, and the 2 % leave-out cap of the select kernel's stream_ids test on the reference alone."""
import math
import random

import pytest
import torch

from clearconverse_amd import fallback as F
from tests import dec_reference as DR
from tests import fallback_reference as FR

EOT = 9


class _Words:
    """token id -> a word; decode joins them"""
    def __init__(self, words):
        self.words = words

    def decode(self, toks):
        return "".join(" " + self.words[t % len(self.words)] for t in toks)


# ---- needs_fallback: every branch, by hand -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cr,lp,ns,cr_thr,lp_thr,ns_thr,want", [
    (2.5, -0.5, 0.1, 2.4, -1.0, 0.6, True),       # compression alone
    (2.4, -0.5, 0.1, 2.4, -1.0, 0.6, False),      # ... at the threshold: not above it
    (1.5, -1.2, 0.1, 2.4, -1.0, 0.6, True),       # log-probability alone
    (1.5, -1.0, 0.1, 2.4, -1.0, 0.6, False),      # ... at the threshold: not below it
    (2.5, -1.2, 0.1, 2.4, -1.0, 0.6, True),       # both
    (1.5, -0.5, 0.1, 2.4, -1.0, 0.6, False),      # neither
    (2.5, -0.5, 0.1, None, -1.0, 0.6, False),     # compression threshold None: nothing tested
    (1.5, -1.2, 0.1, 2.4, None, 0.6, False),      # log-probability threshold None
    (2.5, -1.2, 0.1, None, None, 0.6, False),     # both None
    (1.5, -1.2, 0.7, 2.4, -1.0, 0.6, False),      # the silence exception: improbable AND no speech
    (2.5, -1.2, 0.7, 2.4, -1.0, 0.6, False),      # ... which also overrides a repetitive text
    (2.5, -0.5, 0.7, 2.4, -1.0, 0.6, True),       # no speech but probable enough: no exception
    (1.5, -1.2, 0.7, 2.4, -1.0, None, True),      # no_speech_threshold None: no exception
    (2.5, -1.2, 0.7, 2.4, None, 0.6, True),       # logprob_threshold None: no exception either (both must be set)
])
def test_needs_fallback_branches(cr, lp, ns, cr_thr, lp_thr, ns_thr, want):
    assert F.needs_fallback(cr, lp, ns, cr_thr, lp_thr, ns_thr) is want
    assert FR.needs_fallback_ref(cr, lp, ns, cr_thr, lp_thr, ns_thr) is want


def test_walk_accepts_at_the_first_pass_and_at_the_last_temperature_whatever():
    sched = (0.0, 0.2, 0.4)
    bad, good = dict(compression_ratio=3.0, avg_logprob=-2.0, no_speech_prob=0.0), dict(compression_ratio=1.0, avg_logprob=-0.1, no_speech_prob=0.0)
    walk = F.FallbackWalk(3, sched, 2.4, -1.0, 0.6)
    # window 0 passes at once, window 1 at 0.2, window 2 never
    walk.submit({0: dict(good, t=0.0), 1: dict(bad, t=0.0), 2: dict(bad, t=0.0)})
    assert walk.pending() == [1, 2] and walk.temperature() == 0.2
    walk.submit({1: dict(good, t=0.2), 2: dict(bad, t=0.2)})
    assert walk.pending() == [2] and walk.temperature() == 0.4
    walk.submit({2: dict(bad, t=0.4)})
    assert walk.done() and [walk.accepted[w]["t"] for w in range(3)] == [0.0, 0.2, 0.4]
    assert [len(walk.trace[w]) for w in range(3)] == [1, 2, 3]
    rounds = [(t, 3.0, -2.0, 0.0) for t in sched]
    assert FR.walk_ref(rounds, 2.4, -1.0, 0.6) == 2 and FR.walk_ref(rounds[:1], 2.4, -1.0, 0.6) == 0
    # a one-entry schedule accepts what it gets
    one = F.FallbackWalk(1, (0.7,), 2.4, -1.0, 0.6)
    one.submit({0: bad})
    assert one.done() and one.accepted[0] is bad


def test_best_of_is_dropped_at_temperature_zero():
    assert F.rows_per_window(0.0, 5) == 1 and F.rows_per_window(0.2, 5) == 5
    assert F.rows_per_window(0.2, None) == 1 and F.rows_per_window(0.0, None) == 1
    for t, n in ((0.0, 5), (0.2, 5), (0.2, None), (1.0, 1)):
        assert F.rows_per_window(t, n) == FR.n_rows_ref(t, n)
    assert F.normalize_schedule(0.3) == (0.3,) and F.normalize_schedule([0, 0.2]) == (0.0, 0.2)
    with pytest.raises(ValueError):
        F.normalize_schedule(())
    with pytest.raises(ValueError):
        F.normalize_schedule((0.0, -0.2))


def test_ranker_by_hand():
    c = lambda toks, slp: dict(tokens=toks, sum_logprob=slp, no_speech_prob=0.0)
    # mean log-probability per token: -1.0, -0.5, -0.75
    assert F.rank_candidates([c([1, 2], -2.0), c([1, 2, 3, 4], -2.0), c([1, 2, 3, 4], -3.0)], EOT) == 1
    # the same sums: the length changes the winner (-3/2 against -3/4)
    assert F.rank_candidates([c([1, 2], -3.0), c([1, 2, 3, 4], -3.0)], EOT) == 1
    assert F.rank_candidates([c([1, 2, 3, 4], -3.0), c([1, 2], -1.6)], EOT) == 0
    # tokens are cut at the first eot: [1, EOT, 5, 5] counts one token (-2.0), [1, 2] two (-1.5)
    assert F.rank_candidates([c([1, EOT, 5, 5], -2.0), c([1, 2], -3.0)], EOT) == 1
    # an empty candidate scores -inf, wherever it stands; all empty: the first
    assert F.rank_candidates([c([], 0.0), c([1], -9.0)], EOT) == 1
    assert F.rank_candidates([c([EOT], -0.1), c([1], -9.0)], EOT) == 1
    assert F.rank_candidates([c([], 0.0), c([EOT, 3], 0.0)], EOT) == 0
    # a tie: the first maximum
    assert F.rank_candidates([c([1, 2], -4.0), c([3], -1.0), c([4, 5], -2.0), c([6], -1.0)], EOT) == 1
    rng = random.Random(5)
    for _ in range(300):
        cands = [([rng.choice([1, 2, 3, EOT]) for _ in range(rng.randrange(0, 5))], -rng.choice([0.5, 1.0, 2.0, 3.0])) for _ in range(rng.randrange(1, 6))]
        assert F.rank_candidates([c(t, s) for t, s in cands], EOT) == FR.rank_ref(cands, EOT), cands


def test_window_result_fields():
    tok = _Words(["alpha", "bravo", "charlie", "delta", "echo", "foxtrot"])
    cands = [dict(tokens=[1, 2], sum_logprob=-3.0, no_speech_prob=0.25), dict(tokens=[1, 2, 3, 4], sum_logprob=-3.0, no_speech_prob=0.9)]
    r = F.window_result(cands, 0.4, tok, EOT)
    assert r["candidate"] == 1 and r["tokens"] == [1, 2, 3, 4] and r["temperature"] == 0.4
    assert r["avg_logprob"] == -3.0 / 5 == FR.avg_logprob_ref(-3.0, 4)
    assert r["no_speech_prob"] == 0.25                       # the group's first row, not the winner's
    assert r["compression_ratio"] == FR.compression_ratio_ref(tok.decode([1, 2, 3, 4]))


def test_compression_ratio_of_repetitive_against_varied_text():
    rep = " la la la" * 40
    varied = " ".join(f"w{i * 7919 % 1009}x{i}" for i in range(60))
    a, b = F.compression_ratio(rep.strip().encode("utf-8")), F.compression_ratio(varied.strip().encode("utf-8"))
    assert a == FR.compression_ratio_ref(rep) and b == FR.compression_ratio_ref(varied)
    assert a > 2.4 > b and a > 8.0, (a, b)
    # a text too short to shrink: zlib's header and checksum alone are 6 bytes, so the ratio is below 1
    assert F.compression_ratio(b"abcde") < 5 / 6
    tok = _Words(["so"])
    assert F.text_compression_ratio(tok, [0] * 100) == FR.compression_ratio_ref(" so" * 100)


# ---- the round planner ----------------------------------------------------------------------------------------------------------
def _drive(table, schedule, best_of, max_batch):
    """the product's walk + planner over a scripted pass / fail table -> the same shape as FR.plan_ref"""
    prompts = [[100 + w] * (1 + w % 3) for w in range(len(table))]
    walk = F.FallbackWalk(len(table), schedule, 2.4, -1.0, None)
    rounds = []
    while not walk.done():
        k, t = walk.round, walk.temperature()
        n = F.rows_per_window(t, best_of)
        chunks = F.plan_round(walk.pending(), prompts, n, max_batch)
        calls = []
        for ch in chunks:
            assert len(ch["prompts"]) == len(ch["windows"]) == len(ch["stream_ids"]) == len(ch["owners"]) <= max_batch
            assert all(p == prompts[w] for p, w in zip(ch["prompts"], ch["windows"]))
            assert [w for w, _ in ch["owners"]] == ch["windows"]
            calls.append([(w, c, s) for (w, c), s in zip(ch["owners"], ch["stream_ids"])])
        rounds.append(calls)
        fail = dict(compression_ratio=9.0, avg_logprob=0.0, no_speech_prob=0.0)
        ok = dict(compression_ratio=1.0, avg_logprob=0.0, no_speech_prob=0.0)
        walk.submit({w: dict(fail if table[w][k] else ok) for w in walk.pending()})
    return rounds, walk


def test_planner_against_the_reference_over_scripted_tables():
    rng = random.Random(2024)
    chunked = multi = 0
    for run in range(320):
        nw = rng.randrange(1, 9)
        schedule = tuple([0.0] + [round(0.2 * (i + 1), 1) for i in range(rng.randrange(0, 5))]) if rng.random() < 0.8 else (0.3, 0.6)
        best_of = rng.choice([None, 1, 2, 3, 5])
        max_batch = rng.randrange(max(2, nw), 12)          # holds the group, small enough to cut the best_of rounds
        table = [[rng.random() < 0.6 for _ in schedule] for _ in range(nw)]
        got, walk = _drive(table, schedule, best_of, max_batch)
        want = FR.plan_ref(table, schedule, best_of, max_batch)
        assert got == want, (run, table, schedule, best_of, max_batch)
        chunked += any(len(calls) > 1 for calls in got)
        multi += len(got) > 1
        for w in range(nw):
            k = next((i for i, f in enumerate(table[w]) if not f), len(schedule) - 1)
            assert len(walk.trace[w]) == min(k, len(schedule) - 1) + 1
    assert chunked >= 60 and multi >= 150, (chunked, multi)


def test_stream_ids_of_a_window_do_not_depend_on_the_other_windows():
    prompts = [[1]] * 6
    for n in (1, 3):
        alone = {w: F.plan_round([w], prompts, n, 4) for w in range(6)}
        for failing in ([0, 1, 2, 3, 4, 5], [1, 4], [4, 1], [5], [0, 2, 5]):
            seen = {}
            for ch in F.plan_round(failing, prompts, n, 4):
                for (w, c), s in zip(ch["owners"], ch["stream_ids"]):
                    seen.setdefault(w, []).append((c, s))
            for w in failing:
                want = [(c, s) for ch in alone[w] for (_, c), s in zip(ch["owners"], ch["stream_ids"])]
                assert seen[w] == want == [(c, w * n + c) for c in range(n)]
        ids = [s for ch in F.plan_round(range(6), prompts, n, 4) for s in ch["stream_ids"]]
        assert len(set(ids)) == len(ids)                     # no two rows of a round share a stream


@pytest.mark.parametrize("temperature", FR.SELECT_TEMPERATURES)
def test_select_stream_id_cases_leave_out_at_most_two_percent(temperature):
    """tests/test_dec_mapped_gpu.py compares the kernel's draws under FR.SELECT_STREAM_IDS with DR.select_step_ref(row=id) wherever the
    reference's margin exceeds eps: on the reference alone, at most 2 % of the draws are that close (the analogue of
    test_dec_reference_cpu.py::test_sampling_cases_leave_out_at_most_two_percent)."""
    V = DR.VOCABS["small.en / mini"]
    rules = DR.rules_for(V)
    cases = DR.sampling_cases(V, rules)
    ids = FR.SELECT_STREAM_IDS
    assert len(ids) == len(cases) and len(set(ids)) == len(ids) and sorted(ids) != list(range(len(ids))) and ids != sorted(ids)
    assert max(ids) >= len(ids)                              # gaps: ids no batch row has
    eps = DR.sampling_eps(temperature)
    emb = torch.zeros(V, 4), torch.zeros(DR.N_POS, 4)
    close = draws = 0
    for seed in FR.SELECT_SEEDS:
        for b, c in enumerate(cases):
            gen = (c.sampled + [-7] * DR.SAMPLE_LEN)[:DR.SAMPLE_LEN]
            res = DR.select_step_ref(c.logits, c.state(rules), c.prompt, gen, rules, DR.SAMPLE_LEN, *emb, temperature=temperature, seed=seed, row=ids[b])
            assert abs(res.force_gap) >= 0.05 and math.isfinite(res.logprob)
            close += res.margin <= eps
            draws += 1
    assert close <= 0.02 * draws, (close, draws)
