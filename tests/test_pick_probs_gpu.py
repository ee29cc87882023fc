"""-m gpu: dec_pick_probs_kernel (csrc/dec_probs.hip) through ccx_dec_pick_probs against fp64 on the same fp32 logits
(tests/wordprob_reference.py::pick_probs_ref): the probability of one picked id per logit row over the ids [0, hi) -- what the
alignment pass turns into word probabilities [UPSTREAM-RECALL: timing.py::find_alignment].

hi 1, 5, 7 (ragged tails inside one float4 / two), 50256 and 50257 (eot of the English-only and the multilingual vocabularies), 53248
(all 13 rounds of the block); row stride = hi rounded up to 4, and 51872 where hi fits; 1, 3 and 17 rows.  The columns [hi, ld) hold
NaN and +inf in EVERY case (they must not leak).  Inputs: random logits with the row maximum 1.0 above the rest, the same shifted
so that the maximum is +80 and -80 (exp overflows / underflows without the max subtraction), -inf entries inside the range.  Picks:
id 0, id hi - 1 and the row maximum.  Skipped rows (-1) and strided tables are checked against a sentinel.

Probabilities are compared in log space.  MEASURED_LOG is the worst |log p - fp64| over every case of this file on an MI355X;
TOL_LOG is at most 2.5 x that (the project's rule).  The arithmetic is that of dec_token_probs_kernel's picked
id (tests/test_token_probs_gpu.py: 1.679e-6 for the picked id, 2.849e-6 over a distribution, bound 7e-6) and the error budget
there holds here: u = 2^-24, the exponent's argument (x - max) * log2(e) with |x - max| < 32 rounds at 0.95e-6 in the difference and
1.3e-6 in the product, the fp32 constant log2(e) is off by 1.9e-6 at 32, and the <= 53248 terms are added in chains of ~74.
Every case prints its figure before it asserts.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import wordprob_reference as WR
from tests.conftest import within

pytestmark = pytest.mark.gpu

MEASURED_LOG = 1.563e-6    # worst |log p - fp64| over this file on an MI355X (2785 checks)
TOL_LOG = 3.9e-6           # <= 2.5 x MEASURED_LOG
N_PICK = "dec pick probs: |log p - fp64|"
SENTINEL = -7.0

KINDS = ("random", "max+80", "max-80", "neg_inf_inside")


def _case(hi, ld, rows, kind, seed):
    """-> (logits [rows, ld] fp32 numpy, index of every row's maximum)"""
    g = np.random.default_rng(seed)
    lg = (3.0 * g.standard_normal((rows, ld))).astype(np.float32)
    top = []
    for r in range(rows):
        w = int(g.integers(0, hi))
        lg[r, w] = lg[r, :hi].max() + np.float32(1.0)
        top.append(w)
        if kind == "max+80":
            lg[r] += np.float32(80.0) - lg[r, w]
        elif kind == "max-80":
            lg[r] += np.float32(-80.0) - lg[r, w]
        elif kind == "neg_inf_inside" and hi > 3:
            idx = g.choice(hi, size=max(1, hi // 8), replace=False)
            idx = idx[(idx != w) & (idx != 0) & (idx != hi - 1)]
            lg[r, idx] = -np.inf
    pad = np.where(np.arange(ld) % 2 == 0, np.float32(np.nan), np.float32(np.inf)).astype(np.float32)
    lg[:, hi:] = pad[hi:]
    return lg, top


def _run(ctx, lg_dev, ld, rows, hi, picks_dev, out_dev, pick_stride=1, out_stride=1, override=None):
    from clearconverse_amd import _lib
    lib = _lib.load()
    d = _lib.DecPickProbsDesc()
    d.logits, d.logits_elems, d.ld, d.rows, d.hi = lg_dev.data_ptr(), lg_dev.numel(), ld, rows, hi
    d.picks, d.picks_elems, d.pick_stride = picks_dev.data_ptr(), picks_dev.numel(), pick_stride
    d.out, d.out_elems, d.out_stride = out_dev.data_ptr(), out_dev.numel(), out_stride
    for k, v in (override or {}).items():
        setattr(d, k, v)
    return lib.ccx_dec_pick_probs(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)


def _lds(hi):
    lds = [(hi + 3) // 4 * 4]
    if hi <= 51872 and 51872 not in lds:
        lds.append(51872)
    return lds


@pytest.mark.parametrize("rows", [1, 3, 17])
@pytest.mark.parametrize("hi", [1, 5, 7, 50256, 50257, 53248])
def test_pick_probs_against_fp64(ccx_ctx, hi, rows):
    worst = 0.0
    for li, ld in enumerate(_lds(hi)):
        for ki, kind in enumerate(KINDS):
            lg, top = _case(hi, ld, rows, kind, seed=100000 * li + 1000 * ki + 10 * rows + hi % 7)
            dev = torch.from_numpy(lg).cuda()
            for pname, picks in (("first", [0] * rows), ("last", [hi - 1] * rows), ("max", top)):
                _, logp = WR.pick_probs_ref(lg, hi, picks)
                out = torch.full((rows,), SENTINEL, device="cuda")
                rc = _run(ccx_ctx, dev, ld, rows, hi, torch.tensor(picks, dtype=torch.int32, device="cuda"), out)
                ccx_ctx.check(rc, "ccx_dec_pick_probs")
                got = out.cpu().double().numpy()
                for r in range(rows):
                    name = (hi, ld, rows, kind, pname, r)
                    assert math.isfinite(got[r]) and 0.0 < got[r] <= 1.0, (name, got[r])
                    dp = abs(math.log(got[r]) - logp[r])
                    worst = max(worst, dp)
                    within(N_PICK, dp, TOL_LOG, name)
                if pname == "max":
                    assert all(got[r] > 1.0 / hi for r in range(rows)) or hi == 1      # the case is what it was scripted to be
            print(f"pick_probs hi={hi} ld={ld} rows={rows} {kind:15s}: worst |dlog p| so far {worst:.3e}")
    print(f"pick_probs hi={hi} rows={rows}: worst |dlog p| {worst:.3e} (bound {TOL_LOG:.1e})")
    if hi == 1:
        assert worst == 0.0            # a range of one id: exp2(0) / 1


def test_a_picked_id_of_minus_infinity_has_probability_zero(ccx_ctx):
    hi, ld, rows = 50257, 51872, 2
    lg, top = _case(hi, ld, rows, "random", seed=5)
    lg[0, 123] = -np.inf
    out = torch.full((rows,), SENTINEL, device="cuda")
    rc = _run(ccx_ctx, torch.from_numpy(lg).cuda(), ld, rows, hi, torch.tensor([123, top[1]], dtype=torch.int32, device="cuda"), out)
    ccx_ctx.check(rc, "ccx_dec_pick_probs")
    assert float(out[0]) == 0.0 and 0.0 < float(out[1]) < 1.0


@pytest.mark.parametrize("rows", [1, 3, 17])
def test_skipped_rows_leave_the_output_untouched(ccx_ctx, rows):
    hi, ld = 50257, 51872
    lg, top = _case(hi, ld, rows, "random", seed=40 + rows)
    dev = torch.from_numpy(lg).cuda()
    for pattern in ("every_other", "all"):
        picks = [-1 if (pattern == "all" or r % 2 == 0) else top[r] for r in range(rows)]
        _, logp = WR.pick_probs_ref(lg, hi, picks)
        out = torch.full((rows,), SENTINEL, device="cuda")
        rc = _run(ccx_ctx, dev, ld, rows, hi, torch.tensor(picks, dtype=torch.int32, device="cuda"), out)
        ccx_ctx.check(rc, "ccx_dec_pick_probs")
        got = out.cpu().double().numpy()
        for r in range(rows):
            if picks[r] < 0:
                assert got[r] == SENTINEL, (pattern, r)
            else:
                within(N_PICK, abs(math.log(got[r]) - logp[r]), TOL_LOG, (pattern, r))


def test_strided_tables_write_only_their_own_column(ccx_ctx):
    """the model's call: column t of a [rows][T] pick table and of a [rows][T] output"""
    hi, ld, rows, Tp, To, cp, co = 50257, 51872, 5, 6, 9, 2, 4
    lg, top = _case(hi, ld, rows, "random", seed=77)
    table = np.full((rows, Tp), 12345, dtype=np.int32)              # the other columns: valid ids that must not be used
    col = [top[0], -1, 0, hi - 1, top[4]]
    table[:, cp] = col
    _, logp = WR.pick_probs_ref(lg, hi, col)
    picks = torch.from_numpy(table).cuda()
    out = torch.full((rows, To), SENTINEL, device="cuda")
    d_over = dict(picks=picks.data_ptr() + 4 * cp, picks_elems=picks.numel() - cp, out=out.data_ptr() + 4 * co, out_elems=out.numel() - co)
    rc = _run(ccx_ctx, torch.from_numpy(lg).cuda(), ld, rows, hi, picks, out, pick_stride=Tp, out_stride=To, override=d_over)
    ccx_ctx.check(rc, "ccx_dec_pick_probs")
    got = out.cpu().double().numpy()
    mask = np.ones((rows, To), dtype=bool)
    for r in range(rows):
        if col[r] >= 0:
            mask[r, co] = False
            within(N_PICK, abs(math.log(got[r, co]) - logp[r]), TOL_LOG, r)
    assert np.all(got[mask] == SENTINEL)
    # the same rows through unit strides carry the same bits
    out1 = torch.full((rows,), SENTINEL, device="cuda")
    rc = _run(ccx_ctx, torch.from_numpy(lg).cuda(), ld, rows, hi, torch.tensor(col, dtype=torch.int32, device="cuda"), out1)
    ccx_ctx.check(rc, "ccx_dec_pick_probs")
    assert torch.equal(out1, out[:, co])


def test_refusals_name_the_field_and_launch_nothing(ccx_ctx):
    hi, ld, rows = 50257, 51872, 3
    dev = torch.zeros(rows * ld + 4, device="cuda")
    base = dev[:rows * ld]
    picks = torch.tensor([0, -1, hi - 1, 7, 7, 7, 7], dtype=torch.int32, device="cuda")
    out = torch.full((7,), SENTINEL, device="cuda")
    badpick_hi = torch.tensor([0, hi, 1], dtype=torch.int32, device="cuda")
    badpick_neg = torch.tensor([0, 1, -2], dtype=torch.int32, device="cuda")
    # the phrase only the REQUIRE that should fire writes -> the descriptor fields that provoke it
    bad = {
        "rows = 0 out of range": dict(rows=0),
        "rows = 65537 out of range": dict(rows=65537),
        "hi = 0 out of range": dict(hi=0),
        "hi = 53249 out of range": dict(hi=53249, ld=53252),
        f"ld = {hi - 1} must be": dict(ld=hi - 1),
        f"ld = {ld + 2} must be": dict(ld=ld + 2),
        "logits null or not 16-byte aligned": dict(logits=dev.data_ptr() + 4),
        f"logits_elems = {(rows - 1) * ld + hi}": dict(logits_elems=(rows - 1) * ld + hi),   # the last float4 ends at hi rounded up to 4
        "pick_stride = 0 out of range": dict(pick_stride=0),
        "out_stride = 0 out of range": dict(out_stride=0),
        "out_stride = -1 out of range": dict(out_stride=-1),
        "picks_elems = 4": dict(pick_stride=2, picks_elems=4),
        "out_elems = 6": dict(out_stride=3, out_elems=6),
        "picks null": dict(picks=None),
        "out null": dict(out=None),
        f"picks of row 1 = {hi}": dict(picks=badpick_hi.data_ptr(), picks_elems=3),
        "picks of row 2 = -2": dict(picks=badpick_neg.data_ptr(), picks_elems=3),
    }
    ccx_ctx.prof_enable(True)
    try:
        n0 = ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle)
        for field, ov in bad.items():
            rc = _run(ccx_ctx, base, ld, rows, hi, picks, out, override=ov)
            msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
            assert rc == 1, (field, rc, msg)
            assert "ccx_dec_pick_probs: " in msg and field in msg, (field, msg)
            assert float(out.min()) == SENTINEL and float(out.max()) == SENTINEL, field      # nothing was written
        assert ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle) == n0                              # ... and nothing launched
        rc = _run(ccx_ctx, base, ld, rows, hi, picks, out)
        ccx_ctx.check(rc, "ccx_dec_pick_probs")
        assert ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle) == n0 + 1
        got = out.cpu().numpy()
        assert got[1] == SENTINEL and np.all(got[3:] == SENTINEL) and got[0] == got[2]
        assert abs(math.log(float(got[0])) + math.log(hi)) < TOL_LOG                          # all-zero logits: 1 / hi
    finally:
        ccx_ctx.prof_enable(False)
