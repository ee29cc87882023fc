"""GPU: the FP8 encoder-output stream of the decode cross attention (csrc/cross_x.hip, FL = 2; the format: include/ccx.h, restated in
tests/xa_fp8_reference.py), through the stand-alone operator ccx_cross_attention_xa_fp8.

No tolerance appears in this file.  The dequantised values xhat are exact in bf16, so two comparisons carry everything:
  * xhat, decoded FROM THE IMAGE by the read-back kernel with the stream's own conversion, equals the reference quantiser's bit for bit
    (codes, scales and the image layout's round trip at once);
  * the operator's output equals, bit for bit, ccx_cross_attention_xa (the bf16 stream) run on that xhat -- same MFMAs, same values,
    same order, same lanes.
How close the bf16 stream is to fp64 is tests/test_cross_x_gpu.py's business, whose cases and inputs are reused here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import xa_fp8_reference as R
from tests.test_cross_x_gpu import _bf16_round, _case, _run

pytestmark = pytest.mark.gpu


def _run_fp8(ccx_ctx, q, wk, wv, bv, xa, row_seq, H, rows_per_seq=0, null_xhat=False):
    from clearconverse_amd import _lib
    lib = _lib.load()
    rows, D = q.shape
    n_seq, S, _ = xa.shape
    qd = q.contiguous().cuda()
    xd = xa.to(torch.bfloat16).contiguous().cuda()
    keep = xd.clone()
    out = torch.empty(rows, D, device="cuda")
    xhat = torch.empty(n_seq, S, D, device="cuda", dtype=torch.bfloat16)
    wk_h, wv_h, bv_h = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (wk, wv, bv))
    rs = None if row_seq is None else (C.c_int * rows)(*[int(v) for v in row_seq])
    ccx_ctx.check(lib.ccx_cross_attention_xa_fp8(ccx_ctx.handle, qd.data_ptr(), wk_h.ctypes.data, wv_h.ctypes.data, bv_h.ctypes.data,
                                                 xd.data_ptr(), rs, rows_per_seq, rows, n_seq, H, S, out.data_ptr(),
                                                 None if null_xhat else xhat.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "ccx_cross_attention_xa_fp8")
    assert torch.equal(xd.view(torch.int16), keep.view(torch.int16)), "the operator must not modify xa_dev"
    return out.cpu(), xhat.cpu().to(torch.float32)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _both(ccx_ctx, q, wk, wv, bv, xa, row_seq, H, rows_per_seq=0):
    """the FP8 operator, and the bf16 operator on the xhat it returned"""
    got, xhat = _run_fp8(ccx_ctx, q, wk, wv, bv, xa, row_seq, H, rows_per_seq)
    want = _run(ccx_ctx, q, wk, wv, bv, xhat, row_seq, H, rows_per_seq)
    return got, want, xhat


@pytest.mark.parametrize("H,S", [(2, 16), (4, 37), (6, 100), (8, 1500), (12, 1499), (12, 1500)])
def test_xhat_from_the_image_is_the_reference_quantiser_bit_for_bit(ccx_ctx, H, S):
    """random rows over a wide range of row magnitudes, with every hand-worked block planted in the first and the last feature block, on
    the first and last key of the first, an interior and the ragged last tile (one sequence per hand block).  The query is zero: the
    planted 2^100 must not turn the scores into NaN, and the output comparison then holds here as well."""
    D, n_seq = 64 * H, len(R.HAND_BLOCKS)
    g = torch.Generator().manual_seed(900 + H + S)
    xa = _bf16_round(torch.randn(n_seq, S, D, generator=g) * torch.exp2(torch.randn(n_seq, S, 1, generator=g) * 4.0))
    R.plant(xa, R.hand_places(S, D))
    _, wk, wv, bv, _, _ = _case(3, H, 16, 1, 1)
    q = torch.zeros(n_seq, D)
    got, want, xhat = _both(ccx_ctx, q, wk, wv, bv, xa, None, H)
    ref = R.xhat_of(xa)
    bad = (xhat.view(torch.int32) != ref.view(torch.int32)).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:8].tolist(), [(float(xa[tuple(i)]), float(xhat[tuple(i)]), float(ref[tuple(i)])) for i in bad[:8]])
    for seq, key, blk, name in R.hand_places(S, D):           # and the planted blocks against the values worked by hand
        assert _same_bits(xhat[seq, key, 32 * blk:32 * blk + 32], torch.tensor(R.HAND_BLOCKS[name][1])), (seq, key, blk, name)
    assert torch.isfinite(got).all() and _same_bits(got, want)


@pytest.mark.parametrize("H,S,rows", [(12, 1500, 5), (2, 1500, 19), (6, 1500, 3), (12, 100, 2), (4, 37, 3), (8, 16, 2), (12, 1499, 1)])
def test_output_is_the_bf16_stream_on_xhat(ccx_ctx, H, S, rows):
    q, wk, wv, bv, xa, _ = _case(100 + H + S, H, S, rows, rows, q_gain=2.0)
    got, want, xhat = _both(ccx_ctx, q, wk, wv, bv, xa, None, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert not torch.equal(xhat, xa), "the quantiser changed nothing: the test would show nothing"
    assert _same_bits(xhat, R.xhat_of(xa))


def test_rows_mapped_to_sequences_and_launch_independence(ccx_ctx):
    """the row -> sequence map; a row alone equals the same row in its batch; a second run equals the first"""
    H, S = 12, 1500
    rs = [0, 0, 0, 1, 2, 2, 1]
    q, wk, wv, bv, xa, _ = _case(11, H, S, len(rs), 3, row_seq=rs)
    got, want, xhat = _both(ccx_ctx, q, wk, wv, bv, xa, rs, H)
    assert torch.equal(got, want)
    for r in (1, 3, 6):
        alone, _ = _run_fp8(ccx_ctx, q[r:r + 1], wk, wv, bv, xa, [rs[r]], H)
        assert torch.equal(alone[0], got[r]), r
    again, xhat2 = _run_fp8(ccx_ctx, q, wk, wv, bv, xa, rs, H)
    assert torch.equal(again, got) and _same_bits(xhat2, xhat)


@pytest.mark.parametrize("H,P", [(12, 9), (12, 16), (2, 5), (6, 4), (12, 1)])
def test_prefill_form(ccx_ctx, H, P):
    """groups of P rows per sequence, four rows of a group per streaming block (RB = 4): the bf16 prefill form on xhat, and the same rows
    taken one per block"""
    n_seq, S = 3, 1500
    rs = [s for s in range(n_seq) for _ in range(P)]
    q, wk, wv, bv, xa, _ = _case(300 + H + P, H, S, len(rs), n_seq, q_gain=1.5, row_seq=rs)
    got, want, _ = _both(ccx_ctx, q, wk, wv, bv, xa, rs, H, rows_per_seq=P)
    assert torch.equal(got, want)
    single, _ = _run_fp8(ccx_ctx, q, wk, wv, bv, xa, rs, H)
    assert torch.equal(single, got)


def test_peaked_scores_and_the_repeat_pass(ccx_ctx):
    """the two peaked cases of tests/test_cross_x_gpu.py: p up to ~2^60 against the fixed reference, and a key that makes the block
    repeat its key range -- the repeat pass reloads and converts the image again"""
    H, S = 12, 1500
    for boost in (6.0, 40.0):
        q, wk, wv, bv, xa, _ = _case(7, H, S, 3, 3)
        for seq, key, h in ((1, 1001, 5), (2, 777, 0)):
            qe = (q[seq, 64 * h:64 * h + 64] @ wk[64 * h:64 * h + 64, :])
            xa[seq, key] = _bf16_round(qe / qe.norm() * boost * 4.0)
        got, want, _ = _both(ccx_ctx, q, wk, wv, bv, xa, None, H)
        assert torch.isfinite(got).all(), boost
        assert torch.equal(got, want), boost


def test_argument_errors(ccx_ctx):
    from clearconverse_amd import _lib
    q, wk, wv, bv, xa, _ = _case(1, 2, 64, 2, 2)
    with pytest.raises(_lib.CcxError):
        _run_fp8(ccx_ctx, q, wk, wv, bv, xa, [0, 5], 2)               # a row mapped past n_seq
    q3, wk3, wv3, bv3, xa3, _ = _case(1, 3, 64, 1, 1)
    with pytest.raises(_lib.CcxError):
        _run_fp8(ccx_ctx, q3, wk3, wv3, bv3, xa3, None, 3)            # width 192 is not instantiated
    with pytest.raises(_lib.CcxError) as e:
        _run_fp8(ccx_ctx, q, wk, wv, bv, xa, None, 2, null_xhat=True)
    assert "xhat_out_dev" in str(e.value)
