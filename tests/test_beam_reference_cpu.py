"""CPU: the beam-search rule of tests/beam_reference.py -- every branch by hand, a few hundred seeded runs against an independent second
statement of the walk (written like upstream's: dictionaries keyed by token sequence), the conditions the generated GPU cases must meet
(so that no GPU comparison needs a leave-out), and the ranker with length_penalty in clearconverse_amd/fallback.py."""
import math
import random

import pytest
import torch

from clearconverse_amd import fallback as F
from tests import beam_reference as BR
from tests import dec_reference as DR
from tests import fallback_reference as FR

EOT = 9


def _win(rows):
    return BR.Window([BR.Row(list(t), s) for t, s in rows])


def test_max_candidates_uses_python_round():
    assert [BR.max_candidates(5, p) for p in (None, 1.0, 2.0, 0.5, 0.3, 0.5001)] == [5, 5, 10, 2, 2, 3]      # round(2.5) = 2: half to even
    assert BR.max_candidates(1, 0.5) == 0 and BR.max_candidates(3, 0.5) == 2 and BR.max_candidates(8, 2.0) == 16


def test_walk_eot_above_and_below_the_last_survivor():
    # (score, source row, id): eot second overall -> finished; eot below the second survivor -> dropped
    cands = [(-1.0, 0, 4), (-1.2, 1, EOT), (-1.5, 0, 5), (-1.7, 1, 6), (-1.9, 0, EOT)]
    surv, fin = BR.walk(cands, 2, EOT)
    assert surv == [(-1.0, 0, 4), (-1.5, 0, 5)] and fin == [(-1.2, 1, EOT)]
    # the walk stops AT the last survivor: an eot right behind it is not seen
    surv, fin = BR.walk([(-1.0, 0, 4), (-1.1, 0, EOT)], 1, EOT)
    assert surv == [(-1.0, 0, 4)] and fin == []
    # ties: the lower source row, then the lower id
    surv, _ = BR.walk([(-1.0, 1, 3), (-1.0, 0, 8), (-1.0, 0, 7)], 3, EOT)
    assert surv == [(-1.0, 0, 7), (-1.0, 0, 8), (-1.0, 1, 3)]


def test_step_moves_rows_and_fills_the_finished_list_mid_step():
    win = _win([([1, 2], -1.0), ([1, 3], -2.0)])
    win.finished = [([7], -0.3)]
    cands = [(-1.1, 0, EOT), (-1.2, 1, EOT), (-1.3, 0, 5), (-2.5, 1, 6), (-2.6, 0, 4)]
    rec = BR.apply_walk(win, cands, 2, 2, EOT, 8)
    # both eot candidates stand above the last survivor, the list had room for one: the better one, and the window is complete
    assert rec["finished"] == [(-1.1, 0, EOT), (-1.2, 1, EOT)] and rec["appended"] == [(-1.1, 0, EOT)]
    assert win.finished == [([7], -0.3), ([1, 2], -1.1)] and win.complete
    assert [(r.tokens, r.sum_logprob) for r in win.rows] == [([1, 2, 5], -1.3), ([1, 3, 6], -2.5)] and rec["parents"] == [0, 1]
    # a row may have two children and another none
    win = _win([([1], -1.0), ([2], -5.0)])
    rec = BR.apply_walk(win, [(-1.1, 0, 3), (-1.2, 0, 4), (-5.1, 1, 3)], 2, 2, EOT, 8)
    assert rec["parents"] == [0, 0] and [r.tokens for r in win.rows] == [[1, 3], [1, 4]] and not win.complete


@pytest.mark.parametrize("patience,want_max,want_complete_after", [(None, 2, 2), (2.0, 4, 4), (0.5, 1, 1)])
def test_patience_sets_when_a_window_completes(patience, want_max, want_complete_after):
    mc = BR.max_candidates(2, patience)
    assert mc == want_max
    win = _win([([1], -1.0), ([2], -1.5)])
    n = 0
    while not win.complete:
        toks = [r.tokens for r in win.rows]
        cands = [(win.rows[0].sum_logprob - 0.1, 0, EOT), (win.rows[0].sum_logprob - 0.2, 0, 3), (win.rows[1].sum_logprob - 0.3, 1, 4)]
        BR.apply_walk(win, cands, 2, mc, EOT, 50)
        n += 1
        assert [r.tokens[:-1] for r in win.rows] == toks
    assert n == want_complete_after and len(win.finished) == mc


def test_sample_len_budget_ends_the_window():
    win = _win([([1, 2], -1.0)])
    BR.apply_walk(win, [(-1.5, 0, 3), (-1.9, 0, 4)], 1, 1, EOT, 3)
    assert win.complete and win.finished == []


def test_finalize_tops_up_from_the_live_rows_in_insertion_order():
    win = _win([([1, 2], -3.0), ([1, 3], -1.0), ([1, 4], -2.0)])
    win.finished = [([5], -4.0)]
    assert BR.finalize(win, 3) == [([5], -4.0), ([1, 3], -1.0), ([1, 4], -2.0)]       # finished first, then live rows best first
    win.finished = [([5], -4.0), ([6], -5.0), ([7], -6.0)]
    assert BR.finalize(win, 3) == win.finished                                         # enough finished: no live row enters
    win.finished = [([5], -4.0)] * 5                                                   # patience 2: more than beam stay
    assert len(BR.finalize(win, 3)) == 5


def test_ranker_length_penalty_by_hand():
    hyps = [([1, 2], -2.0), ([1, 2, 3, 4, 5, 6, 7], -4.5), ([], -0.1)]
    # None: -1.0 against -0.643: the long one; an empty hypothesis scores -inf
    assert BR.rank(hyps, EOT) == 1
    # 1.0: -2 / (7/6) = -1.714 against -4.5 / 2 = -2.25: the short one
    assert BR.rank(hyps, EOT, 1.0) == 0
    # 0.6: -2 / 1.0969 = -1.823 against -4.5 / 1.5157 = -2.969
    assert BR.rank(hyps, EOT, 0.6) == 0
    assert BR.rank([([1, 2, EOT, 4, 4, 4, 4], -2.0), ([1, 2], -2.0)], EOT, 0.6) == 0    # cut at the first eot: a tie, the first wins
    assert BR.rank([([], 0.0), ([EOT], 0.0)], EOT, 1.0) == 0
    c = lambda toks, slp: dict(tokens=list(toks), sum_logprob=slp, no_speech_prob=0.0)
    rng = random.Random(11)
    for _ in range(300):
        cands = [([rng.choice([1, 2, 3, EOT]) for _ in range(rng.randrange(0, 9))], -rng.choice([0.5, 1.0, 2.0, 3.0])) for _ in range(rng.randrange(1, 6))]
        for lp in (None, 0.6, 1.0):
            assert F.rank_candidates([c(t, s) for t, s in cands], EOT, lp) == BR.rank(cands, EOT, lp), (cands, lp)
        assert F.rank_candidates([c(t, s) for t, s in cands], EOT) == FR.rank_ref(cands, EOT)       # the default: today's ranker


class _Words:
    def decode(self, toks):
        return "".join(" w%d" % (t % 7) for t in toks)


def test_window_result_default_penalty_is_todays_output():
    """the inputs of tests/test_fallback_reference_cpu.py (its window_result case and its seeded ranker runs): the default keeps
    every field, bit for bit, of a restatement of today's arithmetic"""
    tok = _Words()
    sets = [[dict(tokens=[1, 2], sum_logprob=-3.0, no_speech_prob=0.25), dict(tokens=[1, 2, 3, 4], sum_logprob=-3.0, no_speech_prob=0.9)]]
    rng = random.Random(5)
    for _ in range(300):
        sets.append([dict(tokens=[rng.choice([1, 2, 3, EOT]) for _ in range(rng.randrange(0, 5))], sum_logprob=-rng.choice([0.5, 1.0, 2.0, 3.0]),
                          no_speech_prob=rng.random()) for _ in range(rng.randrange(1, 6))])
    for cands in sets:
        k = FR.rank_ref([(c["tokens"], c["sum_logprob"]) for c in cands], EOT)
        toks = cands[k]["tokens"][:cands[k]["tokens"].index(EOT)] if EOT in cands[k]["tokens"] else list(cands[k]["tokens"])
        want = dict(cands[k], tokens=toks, avg_logprob=cands[k]["sum_logprob"] / (len(toks) + 1), no_speech_prob=cands[0]["no_speech_prob"],
                    temperature=0.4, compression_ratio=FR.compression_ratio_ref(tok.decode(toks)), candidate=k)
        assert F.window_result(cands, 0.4, tok, EOT) == want
        assert F.window_result(cands, 0.4, tok, EOT, length_penalty=None) == want


# ---- the walk against a second statement, written like upstream's: dictionaries keyed by sequence ----------------------------------
def _second_statement(prefixes, sums, proposals, finished, beam, max_cand, eot):
    """prefixes[j]: tuple of tokens, proposals[j]: [(id, logprob)].  -> (next prefixes, next sums, parents, finished dict in order)"""
    scores, sources = {}, {}
    for j, prefix in enumerate(prefixes):
        for tok, lp in proposals[j]:
            seq = prefix + (tok,)
            if seq in scores:                   # (equal prefixes on the first step: the caller passes row 0's proposals only)
                continue
            scores[seq] = sums[j] + lp
            sources[seq] = j
    nxt, nsum, par, newly = [], [], [], {}
    for seq in sorted(scores, key=lambda s: (-scores[s], sources[s], s[-1])):
        if seq[-1] == eot:
            newly[seq] = scores[seq]
        else:
            nxt.append(seq); nsum.append(scores[seq]); par.append(sources[seq])
            if len(nxt) == beam:
                break
    for seq in sorted(newly, key=newly.get, reverse=True):
        if len(finished) >= max_cand:
            break
        finished[seq] = newly[seq]
    return nxt, nsum, par


@pytest.mark.parametrize("seed", range(6))
def test_seeded_runs_against_the_second_statement(seed):
    rng = random.Random(100 + seed)
    for run in range(50):
        beam = rng.choice([1, 2, 3, 5, 8])
        mc = BR.max_candidates(beam, rng.choice([None, 2.0, 0.5, 1.5])) or 1
        sample_len = rng.randrange(3, 9)
        win = _win([([], 0.0)] * beam)
        prefixes, sums, finished = [()] * beam, [0.0] * beam, {}
        for stepi in range(sample_len):
            props = []
            for j in range(beam):
                ids = rng.sample(range(10, 50), beam + 1)
                if stepi > 0 and rng.random() < 0.4:
                    ids[rng.randrange(beam + 1)] = EOT
                lps = sorted((-rng.random() * 4 - 0.01 * k for k in range(beam + 1)), reverse=True)
                props.append(list(zip(ids, lps)) if (stepi > 0 or j == 0) else [])
            cands = [(win.rows[j].sum_logprob + lp, j, i) for j in range(beam) for i, lp in props[j]]
            rec = BR.apply_walk(win, cands, beam, mc, EOT, sample_len)
            prefixes, sums, par = _second_statement(prefixes, sums, props, finished, beam, mc, EOT)
            assert [tuple(r.tokens) for r in win.rows] == prefixes and [r.sum_logprob for r in win.rows] == sums and rec["parents"] == par
            assert [(tuple(t) + (EOT,), s) for t, s in win.finished] == list(finished.items())
            assert win.complete == (len(finished) >= mc or stepi + 1 >= sample_len)
            if win.complete:
                break
        # finalize, upstream's way
        seqs = dict(finished)
        if len(seqs) < beam:
            for j in sorted(range(beam), key=lambda j: -sums[j]):
                seqs[prefixes[j] + (EOT,)] = sums[j]
                if len(seqs) >= beam:
                    break
        assert [(tuple(t) + (EOT,), s) for t, s in BR.finalize(win, beam)] == list(seqs.items())


# ---- the generated GPU cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam,variant", BR.KERNEL_CASES)
@pytest.mark.parametrize("V", BR.KERNEL_VOCABS)
def test_generated_cases_are_decided(V, beam, variant):
    rules = BR.rules_for(V)
    case = BR.beam_case(V, rules, beam, variant)
    assert BR.case_gaps_ok(case, rules)
    K = beam + 1
    saw_force = False
    for w in (1, 2):
        cands, props = BR.case_candidates(case, rules, w)
        sc = sorted(c[0] for c in cands)
        assert all(b - a >= BR.SCORE_GAP for a, b in zip(sc, sc[1:]))
        for j in range(beam):
            r = w * beam + j
            if w == 1 and j > 0:
                assert props[j] == []
                continue
            assert len(props[j]) == K
            x = BR.sorted_filtered(case.logits[r], case.sampled[r], rules)
            assert x[K - 1] - x[K] >= BR.ROW_GAP
            assert props[j][0][0] == DR.folded_select(case.logits[r], case.sampled[r], rules)        # the select kernel's own arg-max
            if DR.folded_select(case.logits[r], case.sampled[r], rules, "no_force") != props[j][0][0]:
                saw_force = True
    assert saw_force == (variant == "force")          # one row's proposals exist only through the force-timestamp rule
    win = BR.case_window(case, 2)
    win.finished = [(None, None)] * case.fin_count[2]
    cands, _ = BR.case_candidates(case, rules, 2)
    rec = BR.apply_walk(win, cands, beam, case.max_cand, rules.eot, BR.SAMPLE_LEN)
    if variant == "eot":
        assert win.complete and len(rec["appended"]) == 1
        assert len(rec["finished"]) == (2 if beam > 2 else 1)                           # eot above the last survivor (two: the list fills mid-step)
        if beam > 1:
            n_eot = sum(1 for c in cands if c[2] == rules.eot)
            assert n_eot == len(rec["finished"]) + 1                                    # ... and one below it, dropped
    else:
        assert not win.complete and rec["finished"] == []
    if beam >= 5:
        assert len(set(rec["parents"])) < beam                                          # some row has two children, some none
