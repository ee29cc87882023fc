"""CPU: the truncation rule restated in tests/truncation_reference.py -- by hand, against the installed Hugging Face warper chain
(TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper) on tie-free rows, the stated deviation on ties,
the generator's margins on the reference alone, every listed misreading caught by some generated case -- and the C structs of
include/ccx.h against their ctypes mirrors."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.build import _hipcc
from tests import dec_reference as DR
from tests import decoding_options_reference as DO
from tests import truncation_reference as TR

ROOT = Path(__file__).resolve().parent.parent
NINF = -math.inf
RULE_SETS = {"rules": DO.Options(), "no rules": DO.Options(True, True)}


def _kept(x, T=1.0, k=0, p=1.0, m=0.0, mutation=None):
    return np.nonzero(TR.keep_set(np.array(x, dtype=np.float32), TR.Params(T, k, p, m), mutation).mask)[0].tolist()


# ---------------------------------------------------------------------------------------------- the rule by hand
def test_top_k_by_hand():
    x = [1.0, NINF, 3.0, 2.0, 0.0, 2.0]
    assert _kept(x, k=1) == [2]
    assert _kept(x, k=2) == [2, 3, 5]                    # ties at the k-th value all stay
    assert _kept(x, k=3) == [2, 3, 5]
    assert _kept(x, k=4) == [0, 2, 3, 5]
    assert _kept(x, k=5) == _kept(x, k=6) == _kept(x, k=99) == [0, 2, 3, 4, 5]      # |A| < k: the minimum; -inf never enters
    assert _kept(x, k=0) == [0, 2, 3, 4, 5]


def test_top_p_by_hand():
    # probabilities 0.5, 0.25, 0.125, 0.125 at T = 1 (logits ln p); the mass strictly above: 0, 0.5, 0.75, 0.75
    x = np.log([0.5, 0.25, 0.125, 0.125])
    assert _kept(x, p=0.4) == [0]
    assert _kept(x, p=0.6) == [0, 1]
    assert _kept(x, p=0.8) == [0, 1, 2, 3]               # the tie at 0.125: kept as a whole
    assert _kept(x, p=0.74) == [0, 1]                    # ... or dropped as a whole
    assert _kept(x, p=1e-9) == [0]
    assert _kept(x, p=1.0) == [0, 1, 2, 3]
    # the temperature enters: at T = 0.5 the probabilities are 16, 4, 1, 1 of 22
    assert _kept(x, T=0.5, p=0.8) == [0, 1]              # above the second: 16 / 22 = 0.727 < 0.8; above the third: 20 / 22 = 0.909
    # after top_k the survivors are renormalised: top 2 are 2/3, 1/3
    assert _kept(x, k=2, p=0.6) == [0]
    assert _kept(x, k=2, p=0.7) == [0, 1]


def test_min_p_by_hand():
    x = [0.0, -1.0, -2.0, -3.0, NINF]
    assert _kept(x, m=math.exp(-1.5)) == [0, 1]
    assert _kept(x, T=2.0, m=math.exp(-1.5)) == [0, 1, 2, 3]     # the threshold is max + T ln(min_p) = -3.0: fp32 decides the last one
    assert _kept(x, T=0.5, m=math.exp(-1.5)) == [0]
    assert _kept(x, m=1.0) == [0] and _kept(x, m=0.0) == [0, 1, 2, 3]
    k = TR.keep_set(np.array(x, dtype=np.float32), TR.Params(1.0, 0, 1.0, math.exp(-1.5)))
    assert (k.n, k.cut) == (2, -1.0) and abs(k.mass - (1 + math.exp(-1)) / sum(math.exp(-i) for i in range(4))) < 1e-12


def test_one_cut_and_the_empty_row():
    g = np.random.default_rng(0)
    for _ in range(50):
        x = g.normal(0, 2, 40).astype(np.float32)
        x[g.integers(0, 40, 5)] = NINF
        prm = TR.Params(float(g.uniform(0.2, 2)), int(g.integers(0, 12)), float(g.uniform(0.3, 1)), float(g.uniform(0, 0.3)))
        k = TR.keep_set(x, prm)
        assert (k.mask == (x >= np.float32(k.cut))).all() and k.mask[np.argmax(x)] and k.n == k.mask.sum()
    e = TR.keep_set(np.full(8, NINF, dtype=np.float32), TR.Params(1.0, 2, 0.5, 0.1))
    assert (e.n, e.cut, e.mass) == (0, NINF, 0.0) and not e.mask.any()


# ---------------------------------------------------------------------------------------------- Hugging Face's chain
def _hf_kept(x, prm):
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.from_numpy(np.asarray(x, dtype=np.float32))[None].double()
    chain = [TemperatureLogitsWarper(float(prm.temperature))]
    if prm.top_k > 0:
        chain.append(TopKLogitsWarper(top_k=prm.top_k, min_tokens_to_keep=1))
    if prm.top_p < 1.0:
        chain.append(TopPLogitsWarper(top_p=float(prm.top_p), min_tokens_to_keep=1))
    if prm.min_p > 0.0:
        chain.append(MinPLogitsWarper(min_p=float(prm.min_p), min_tokens_to_keep=1))
    for w in chain:
        s = w(None, s)
    return np.nonzero(torch.isfinite(s[0]).numpy())[0].tolist()


def test_tie_free_rows_keep_what_the_installed_warper_chain_keeps():
    """random rows whose every decision has a margin (so fp64 here and there decide alike), some ids banned"""
    g = np.random.default_rng(1)
    checked = 0
    while checked < 200:
        x = g.normal(0, 2.5, 64).astype(np.float32)
        x[g.integers(0, 64, 6)] = NINF
        prm = TR.Params(float(g.choice([0.2, 0.5, 1.0, 1.7])), int(g.choice([0, 0, 3, 10, 80])), float(g.choice([1.0, 0.95, 0.7, 0.3])),
                        float(g.choice([0.0, 0.0, 0.02, 0.2])))
        k = TR.keep_set(x, prm)
        if k.mass_margin < 1e-6 or k.logit_margin < 1e-4:
            continue
        assert np.nonzero(k.mask)[0].tolist() == _hf_kept(x, prm), prm
        checked += 1


def test_the_tie_deviation():
    """probabilities 0.5, 0.2, 0.2, 0.1, top_p 0.6: the mass above the tie is 0.5 < 0.6, so here BOTH 0.2s stay; HF's sort cuts
    between them and keeps one.  With top_p 0.45 both readings drop both."""
    x = np.log([0.5, 0.2, 0.2, 0.1]).astype(np.float32)
    assert _kept(x, p=0.6) == [0, 1, 2]
    hf = _hf_kept(x, TR.Params(1.0, 0, 0.6, 0.0))
    assert len(hf) == 2 and hf[0] == 0 and hf[1] in (1, 2)
    assert _kept(x, p=0.6, mutation="ties_split") in ([0, 1], [0, 2])
    assert _kept(x, p=0.45) == [0] == _hf_kept(x, TR.Params(1.0, 0, 0.45, 0.0))


# ---------------------------------------------------------------------------------------------- the generator
@pytest.fixture(scope="module")
def generated():
    """every launch of tests/test_dec_truncate_gpu.py::test_rows_against_the_rule"""
    out = {}
    for vocab, V in TR.VOCABS.items():
        rules = TR.rules_for(V)
        for rs, opts in RULE_SETS.items():
            for ps, prm in TR.PARAM_SETS.items():
                out[(vocab, rs, ps)] = (V, rules, opts, prm, TR.trunc_cases(V, rules, opts, prm))
    return out


def test_generated_rows_have_their_margins_and_their_kinds(generated):
    tied = 0
    for key, (V, rules, opts, prm, cases) in generated.items():
        names = [c.name for c in cases]
        assert names[:3] == ["finished row", "prompt phase", "first step"] and 6 <= len(cases) <= 8, names
        assert opts.without_timestamps or "forced timestamp" in names
        for c in cases[2:]:
            k = TR.case_kept(c, rules, opts, prm)
            x = TR.filtered_row(c.logits, c.sampled, rules, opts).numpy()
            head = TR.head_of(c, rules, opts, prm)
            assert len(head) >= 2 and k.mass_margin >= TR.MASS_MARGIN and k.logit_margin >= TR.LOGIT_MARGIN, (key, c.name, k)
            if prm.top_p < 1.0:                          # the top_p boundary lies in the head
                assert np.isin(np.nonzero(x == np.float32(k.cut))[0], head).all(), (key, c.name)
            n_allowed = int(np.isfinite(x).sum())        # every row is really cut (the five-id first step may keep all five)
            assert 1 <= k.n <= n_allowed and (k.n < n_allowed or c.name == "first step"), (key, c.name, k.n)
            assert (x[np.isfinite(x)] < TR.DECOY).all()      # the banned decoys are banned
            if "forced" in c.name:
                assert not np.isfinite(x[:rules.timestamp_begin]).any()
            if "tie" in c.name:
                vals = np.sort(x[np.isfinite(x)])[::-1][:12]
                assert (np.diff(vals) == 0).any()
                tied += 1
        if not opts.without_timestamps and key[2] == "all three":
            first = TR.filtered_row(cases[2].logits, [], rules, opts)
            assert int(torch.isfinite(first).sum()) == TR.MAX_INITIAL_TS + 1 < prm.top_k      # fewer allowed ids than top_k
    assert tied >= len(generated)


@pytest.mark.parametrize("mutation", TR.MUTATIONS)
def test_every_misreading_changes_a_generated_case(generated, mutation):
    tok, pos = torch.zeros(1, 4), torch.zeros(DR.N_POS, 4)
    hits = 0
    for key, (V, rules, opts, prm, cases) in generated.items():
        if V != 1024:
            continue
        for c in cases[2:]:
            if mutation == "truncated_logprob":
                st = c.state(rules)
                gen = (c.sampled + [-7] * DR.SAMPLE_LEN)[:DR.SAMPLE_LEN]
                emb = (torch.zeros(V, 4), pos)
                a = TR.select_step_ref(c.logits, st, [rules.sot], gen, rules, opts, DR.SAMPLE_LEN, *emb, prm, seed=1)
                b = TR.select_step_ref(c.logits, st, [rules.sot], gen, rules, opts, DR.SAMPLE_LEN, *emb, prm, seed=1, mutation=mutation)
                assert a.res.token == b.res.token
                hits += abs(a.res.logprob - b.res.logprob) > 1e-3      # far above the select test's 2e-5 bound
            else:
                hits += bool((TR.case_kept(c, rules, opts, prm).mask != TR.case_kept(c, rules, opts, prm, mutation).mask).any())
    assert hits >= 1, mutation


def test_the_truncated_draw_is_the_plain_draw_where_that_lies_in_k(generated):
    V, rules, opts, prm, cases = generated[("1024", "rules", "top_p")]
    inside = outside = 0
    for seed in range(12):
        for c in cases[2:]:
            flt = TR.filtered_row(c.logits, c.sampled, rules, opts)
            k = TR.case_kept(c, rules, opts, prm)
            plain, _, _ = TR.R.sample_token(flt, prm.temperature, seed, 3, len(c.sampled))
            tok, score = TR.truncated_draw(flt, prm, seed, 3, len(c.sampled), k.mask)
            assert k.mask[tok] and int(torch.isfinite(score).sum()) == k.n
            if k.mask[plain]:
                assert tok == plain
                inside += 1
            else:
                outside += 1
    assert inside and outside


# ---------------------------------------------------------------------------------------------- the C ABI
PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "ccx.h"
int main() {
  printf("ccx_decode_sampling_options %zu\n", sizeof(ccx_decode_sampling_options));
  printf("ccx_decode_sampling_options.top_k %zu\n", offsetof(ccx_decode_sampling_options, top_k));
  printf("ccx_decode_sampling_options.top_p %zu\n", offsetof(ccx_decode_sampling_options, top_p));
  printf("ccx_decode_sampling_options.min_p %zu\n", offsetof(ccx_decode_sampling_options, min_p));
  printf("ccx_dec_select_desc %zu\n", sizeof(ccx_dec_select_desc));
  printf("ccx_dec_select_desc.opts %zu\n", offsetof(ccx_dec_select_desc, opts));
  printf("ccx_dec_select_desc.sampling %zu\n", offsetof(ccx_dec_select_desc, sampling));
  printf("ccx_dec_select_desc.cut_out %zu\n", offsetof(ccx_dec_select_desc, cut_out));
  printf("ccx_dec_select_desc.kept_out %zu\n", offsetof(ccx_dec_select_desc, kept_out));
  printf("ccx_dec_select_desc.kept_mass_out %zu\n", offsetof(ccx_dec_select_desc, kept_mass_out));
  return 0;
}
"""


def test_ctypes_mirrors_have_the_c_structs_layout(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    mirrors = {"ccx_decode_sampling_options": _lib.DecodeSamplingOptions, "ccx_dec_select_desc": _lib.DecSelectDesc}
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == c[name], (name, C.sizeof(cls), c[name])
    for key, want in c.items():
        if "." in key:
            name, field = key.split(".")
            assert getattr(mirrors[name], field).offset == want, (key, getattr(mirrors[name], field).offset, want)
    # appended: nothing before the new fields moved
    assert _lib.DecSelectDesc.sampling.offset == _lib.DecSelectDesc.opts.offset + 8


def test_defaults_and_null_handles_need_no_device():
    lib = _lib.load()
    o = _lib.DecodeSamplingOptions(9, 0.5, 0.5)
    lib.ccx_decode_sampling_options_default(C.byref(o))
    assert (o.top_k, o.top_p, o.min_p) == (0, 1.0, 0.0)
    lib.ccx_decode_sampling_options_default(None)
    assert lib.ccx_whisper_set_sampling_options(None, C.byref(o)) == 1        # CCX_ERR_ARG
    assert lib.ccx_whisper_set_sampling_options(None, None) == 1
    assert lib.ccx_whisper_sampling_graph_count(None) == -1
    d = _lib.DecSelectDesc()
    assert not d.sampling and not d.cut_out and not d.kept_out and not d.kept_mass_out
