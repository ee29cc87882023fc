"""-m gpu: dec_token_probs_kernel (csrc/dec_probs.hip) through ccx_dec_token_probs against fp64 on the same fp32 logits
(tests/lang_reference.py::ranged_softmax).

Vocabularies 4097 (one id past a 4096-id round of the block), 51865 and 51866 (the multilingual checkpoints: neither a multiple of
4), row stride = the vocabulary rounded up to 128, 1 and 3 rows.  Ranges: the whole vocabulary, the 99 language tokens [50259, 50358)
(lo no multiple of 4), a range straddling id 4096, a single id, a range ending at n_vocab.  Inputs: random logits, the same offset by
+80 and by -80, -inf entries inside the range, NaN / 1e30 everywhere OUTSIDE the range and in the columns [n_vocab, ld) (they must
not leak), two exactly equal maxima (the lower id wins).  Except in the tie case the winner leads by 1.0 (>= 1e-3), so the argmax
is compared exactly.

Probabilities are compared in log space.  Measured on an MI355X over every case of this file (360 rows), worst |log p - fp64|:
2.849e-6 over the optional distribution, 1.679e-6 for the picked id.  TOL_LOG = 7e-6 is at most 2.5 x the worse of the two (the
project's rule).  Where it comes from, u = 2^-24: the exponent's argument (x - max) * log2(e) with |x - max| < 32
rounds at 0.95e-6 in the difference and 1.3e-6 in the product, the fp32 constant log2(e) is off by u relative (1.9e-6 at 32), and the
<= 53248 terms are added in chains of ~74 (4.4e-6 relative at the very worst, far less on average).
Every case prints its figure before it asserts.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import lang_reference as LR
from tests.conftest import within

pytestmark = pytest.mark.gpu

MEASURED_LOG = 2.849e-6    # worst |log p - fp64| over this file on an MI355X
TOL_LOG = 7e-6             # <= 2.5 x MEASURED_LOG
N_PICK = "dec token probs: |log pick_prob - fp64|"
N_PROBS = "dec token probs: max |log probs - fp64| over the range"

INPUTS = ("random", "offset+80", "offset-80", "neg_inf_inside", "nan_outside", "tie")


def _ranges(V):
    r = {"whole": (0, V), "single": (V - 3, V - 2), "to_end": (V - 865, V)}
    if V > 50358:
        r["languages"] = (50259, 50358)
        r["straddle_4096"] = (4001, 4203)
    else:
        r["odd_lo"] = (3, 102)
        r["straddle_4096"] = (4090, V)
    return r


def _case(V, ld, rows, lo, hi, kind, seed):
    """-> (logits [rows, ld] fp32 numpy, pick, expected argmax per row or None)"""
    g = np.random.default_rng(seed)
    lg = (3.0 * g.standard_normal((rows, ld))).astype(np.float32)
    n = hi - lo
    winners = []
    for r in range(rows):
        w = lo + int(g.integers(0, n))
        lg[r, w] = lg[r, lo:hi].max() + np.float32(1.0)              # top-2 gap 1.0
        winners.append(w)
    pick = lo + int(g.integers(0, n))
    if kind == "offset+80":
        lg += np.float32(80.0)
    elif kind == "offset-80":
        lg -= np.float32(80.0)
    elif kind == "neg_inf_inside" and n > 2:
        for r in range(rows):
            idx = lo + g.choice(n, size=max(1, n // 8), replace=False)
            idx = idx[(idx != winners[r]) & (idx != pick)]
            lg[r, idx] = -np.inf
    elif kind == "tie" and n >= 2:
        for r in range(rows):
            a, b = sorted(lo + g.choice(n, size=2, replace=False))
            top = lg[r, lo:hi].max() + np.float32(0.5)
            lg[r, a] = lg[r, b] = top
            winners[r] = int(a)
    if kind == "nan_outside":
        out = np.ones(ld, dtype=bool)
        out[lo:hi] = False
        fill = np.where(np.arange(ld) % 2 == 0, np.float32(np.nan), np.float32(1e30)).astype(np.float32)
        lg[:, out] = fill[out]
    else:
        lg[:, V:] = np.nan                                            # the padding columns are never valid
    return lg, pick, winners


def _run(ctx, lg_dev, V, ld, rows, lo, hi, pick, want_probs=True, override=None):
    from clearconverse_amd import _lib
    lib = _lib.load()
    arg, pp = (C.c_int * rows)(), (C.c_float * rows)()
    probs = torch.full((rows, hi - lo), -1.0, device="cuda") if want_probs else None
    d = _lib.DecTokenProbsDesc()
    d.logits, d.logits_elems, d.ld, d.n_vocab, d.rows = lg_dev.data_ptr(), lg_dev.numel(), ld, V, rows
    d.lo, d.hi, d.pick, d.argmax, d.pick_prob = lo, hi, pick, arg, pp
    d.probs, d.probs_elems = (probs.data_ptr(), probs.numel()) if want_probs else (None, 0)
    for k, v in (override or {}).items():
        setattr(d, k, v)
    rc = lib.ccx_dec_token_probs(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    return rc, list(arg), list(pp), probs


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V", [4097, 51865, 51866])
def test_token_probs_against_fp64(ccx_ctx, V, rows):
    ld = (V + 127) // 128 * 128
    worst_pick = worst_probs = 0.0
    for ri, (rname, (lo, hi)) in enumerate(_ranges(V).items()):
        for ki, kind in enumerate(INPUTS):
            lg, pick, winners = _case(V, ld, rows, lo, hi, kind, seed=1000 * ri + 10 * ki + rows)
            dev = torch.from_numpy(lg).cuda()
            rc, arg, pp, probs = _run(ccx_ctx, dev, V, ld, rows, lo, hi, pick)
            ccx_ctx.check(rc, "ccx_dec_token_probs")
            probs = probs.cpu().double().numpy()
            for r in range(rows):
                am, lp, logp = LR.ranged_softmax(lg[r, :V], lo, hi, pick)
                name = (V, rows, rname, kind, r)
                assert am == winners[r], name                          # the case is what it was scripted to be
                assert arg[r] == am, (name, arg[r], am)
                assert math.isfinite(pp[r]) and pp[r] > 0.0, (name, pp[r])
                dp = abs(math.log(pp[r]) - lp)
                fin = np.isfinite(logp)
                assert np.all(probs[r][~fin] == 0.0), name            # -inf inside the range contributes exactly 0
                assert np.all(np.isfinite(probs[r])) and np.all(probs[r][fin] > 0.0), name
                da = float(np.abs(np.log(probs[r][fin]) - logp[fin]).max())
                worst_pick, worst_probs = max(worst_pick, dp), max(worst_probs, da)
                print(f"token_probs V={V} rows={rows} {rname:14s} {kind:15s} row {r}: |dlog pick| {dp:.3e}  max |dlog probs| {da:.3e}")
                within(N_PICK, dp, TOL_LOG, name)
                within(N_PROBS, da, TOL_LOG, name)
            # without the optional output the two scalars are the same bits
            rc, arg2, pp2, _ = _run(ccx_ctx, dev, V, ld, rows, lo, hi, pick, want_probs=False)
            ccx_ctx.check(rc, "ccx_dec_token_probs")
            assert arg2 == arg and pp2 == pp, (V, rows, rname, kind)
    print(f"token_probs V={V} rows={rows}: worst |dlog pick| {worst_pick:.3e}, worst |dlog probs| {worst_probs:.3e} (bound {TOL_LOG:.1e})")


def test_a_picked_id_of_minus_infinity_has_probability_zero(ccx_ctx):
    V, ld = 51865, 51968
    lg, pick, _ = _case(V, ld, 1, 50259, 50358, "random", seed=5)
    lg[0, pick] = -np.inf
    rc, arg, pp, probs = _run(ccx_ctx, torch.from_numpy(lg).cuda(), V, ld, 1, 50259, 50358, pick)
    ccx_ctx.check(rc, "ccx_dec_token_probs")
    assert pp[0] == 0.0 and float(probs[0, pick - 50259]) == 0.0 and arg[0] == LR.ranged_softmax(lg[0, :V], 50259, 50358, 50259)[0]


def test_refusals_name_the_field_and_launch_nothing(ccx_ctx):
    V, ld, rows, lo, hi = 51865, 51968, 2, 50259, 50358
    dev = torch.zeros(rows * ld + 4, device="cuda")
    base = dev[:rows * ld]
    # the phrase only the REQUIRE that should fire writes -> the descriptor fields that provoke it
    bad = {
        f"pick = {hi} outside": dict(pick=hi), f"pick = {lo - 1} outside": dict(pick=lo - 1),
        f"hi = {V + 1} behind n_vocab": dict(hi=V + 1, pick=lo),
        f"ld = {V - 1} must be": dict(ld=V - 1),
        f"ld = {ld + 2} must be": dict(ld=ld + 2),
        f"logits_elems = {(rows - 1) * ld + hi}": dict(logits_elems=(rows - 1) * ld + hi),   # the last float4 ends at hi rounded up to 4
        f"probs_elems = {rows * (hi - lo) - 1}": dict(probs_elems=rows * (hi - lo) - 1),
        "logits null or not 16-byte aligned": dict(logits=dev.data_ptr() + 4),
        "rows = 0 out of range": dict(rows=0),
        f"lo = {hi}, hi = {hi} is not a range": dict(lo=hi, pick=hi),
        "n_vocab = 53249 out of range": dict(n_vocab=53249, ld=53376, hi=53249, lo=0, pick=0),
    }
    ccx_ctx.prof_enable(True)
    try:
        n0 = ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle)
        for field, ov in bad.items():
            rc, arg, pp, probs = _run(ccx_ctx, base, V, ld, rows, lo, hi, lo, override=ov)
            msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
            assert rc == 1, (field, rc, msg)
            assert "ccx_dec_token_probs: " in msg and field in msg, (field, msg)
            assert float(probs.min()) == -1.0 and float(probs.max()) == -1.0, field      # nothing was written
        assert ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle) == n0                          # ... and nothing launched
        rc, *_ = _run(ccx_ctx, base, V, ld, rows, lo, hi, lo)
        ccx_ctx.check(rc, "ccx_dec_token_probs")
        assert ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle) == n0 + 1
    finally:
        ccx_ctx.prof_enable(False)
