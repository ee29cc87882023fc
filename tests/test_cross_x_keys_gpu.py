"""-m gpu: the decode cross attention against the encoder output with a key count PER SEQUENCE (csrc/cross_x.hip, XsParams::seq_S: the
reduced audio context), through the stand-alone operators ccx_cross_attention_xa_keys / ccx_cross_attention_xa_fp8_keys.

2 heads take the half-line stream (D = 128), 4 heads the full-line stream (D = 256); the FP8 sibling takes the FP8 stream at both.  At
n_ctx = 80 (five 16-key tiles) the counts 1, 15, 16, 17, 33, 48, 80 give: an empty first key half, one ragged tile, exactly one tile, a
ragged second tile (one tile per half), three tiles split 1 + 2 with a ragged last one, three whole tiles, everything.
  * against the explicit-K/V fp64 reference of tests/test_cross_x_gpu.py on the sequence's first `count` rows, with its TOL;
  * all counts full: the bits of ccx_cross_attention_xa;
  * count k: the bits of the same sequence run alone through ccx_cross_attention_xa at n_ctx = k;
  * row maps, and rows_per_seq = 5 (four rows of a group per streaming block, RB = 4, with a ragged second block);
  * the FP8 sibling: the bits of the bf16 sibling on the xhat it returns;
  * a second run: the same bits.
Measured on an MI355X: rel-L2 4.9e-3 (one row per sequence), 5.3e-3 (row maps), 5.8e-3 (prompt groups) under TOL = 1e-2;
profiles/audio_ctx_measured_deviations.json.  ccx_cross_attention_xa accepts windows of fewer than 16 keys since this operator exists
(an empty first key half is a case of the kernel's own merge), which is what the runs alone at n_ctx = 1 and 15 use."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import within
from tests.test_cross_x_gpu import TOL, _case, _reference, _run

pytestmark = pytest.mark.gpu

N_CTX = 80
COUNTS = [1, 15, 16, 17, 33, 48, 80]


def _run_keys(ccx_ctx, q, wk, wv, bv, xa, row_seq, H, counts, rows_per_seq=0, fp8=False):
    from clearconverse_amd import _lib
    lib = _lib.load()
    rows, D = q.shape
    n_seq, S, _ = xa.shape
    qd = q.contiguous().cuda()
    xd = xa.to(torch.bfloat16).contiguous().cuda()
    out = torch.empty(rows, D, device="cuda")
    wk_h, wv_h, bv_h = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (wk, wv, bv))
    rs = None if row_seq is None else (C.c_int * rows)(*[int(v) for v in row_seq])
    nk = None if counts is None else (C.c_int * n_seq)(*[int(v) for v in counts])
    st = torch.cuda.current_stream().cuda_stream
    if fp8:
        xhat = torch.empty(n_seq, S, D, device="cuda", dtype=torch.bfloat16)
        ccx_ctx.check(lib.ccx_cross_attention_xa_fp8_keys(ccx_ctx.handle, qd.data_ptr(), wk_h.ctypes.data, wv_h.ctypes.data, bv_h.ctypes.data,
                                                          xd.data_ptr(), rs, rows_per_seq, rows, n_seq, H, S, nk, out.data_ptr(), xhat.data_ptr(), st),
                      "ccx_cross_attention_xa_fp8_keys")
        return out.cpu(), xhat.cpu().to(torch.float32)
    ccx_ctx.check(lib.ccx_cross_attention_xa_keys(ccx_ctx.handle, qd.data_ptr(), wk_h.ctypes.data, wv_h.ctypes.data, bv_h.ctypes.data,
                                                  xd.data_ptr(), rs, rows_per_seq, rows, n_seq, H, S, nk, out.data_ptr(), st),
                  "ccx_cross_attention_xa_keys")
    return out.cpu()


def _check_fp64(got, q, wk, wv, bv, xa, rs, H, counts, name):
    want = _reference(q, wk, wv, bv, [xa[s, :counts[s]] for s in range(xa.shape[0])], rs, H)
    assert torch.isfinite(got).all()
    for r in range(q.shape[0]):
        within(f"cross attention against xa, keys per sequence ({name}): output rel-L2", float((got[r] - want[r]).norm() / want[r].norm()), TOL,
               (H, r, counts[rs[r]]))


@pytest.mark.parametrize("H", [2, 4])
def test_counts_against_explicit_kv_and_alone(ccx_ctx, H):
    n_seq = len(COUNTS)
    q, wk, wv, bv, xa, rs = _case(500 + H, H, N_CTX, n_seq, n_seq, q_gain=2.0)
    got = _run_keys(ccx_ctx, q, wk, wv, bv, xa, None, H, COUNTS)
    _check_fp64(got, q, wk, wv, bv, xa, rs, H, COUNTS, "one row per sequence")
    for s, k in enumerate(COUNTS):
        alone = _run(ccx_ctx, q[s:s + 1], wk, wv, bv, xa[s:s + 1, :k], None, H)
        assert torch.equal(alone[0], got[s]), (H, k)
    assert torch.equal(_run_keys(ccx_ctx, q, wk, wv, bv, xa, None, H, COUNTS), got), "a second run differs"
    # the counts follow the sequence, not the row: the same sequences in another order
    perm = [3, 0, 6, 1, 5, 2, 4]
    got_p = _run_keys(ccx_ctx, q[perm], wk, wv, bv, xa[perm], None, H, [COUNTS[i] for i in perm])
    assert torch.equal(got_p, got[perm])


@pytest.mark.parametrize("H", [2, 4])
def test_full_counts_are_the_plain_operator_bit_for_bit(ccx_ctx, H):
    q, wk, wv, bv, xa, _ = _case(510 + H, H, N_CTX, 3, 3, q_gain=2.0)
    assert torch.equal(_run_keys(ccx_ctx, q, wk, wv, bv, xa, None, H, [N_CTX] * 3), _run(ccx_ctx, q, wk, wv, bv, xa, None, H))


@pytest.mark.parametrize("H", [2, 4])
def test_row_maps_and_prompt_groups(ccx_ctx, H):
    """rows mapped to sequences in any order read their sequence's count; groups of 5 rows per sequence (RB = 4: a block of four rows and
    a ragged block of one) equal the same rows taken one per block"""
    n_seq = len(COUNTS)
    rs = [6, 0, 0, 3, 1, 5, 2, 2, 4, 1]
    q, wk, wv, bv, xa, _ = _case(520 + H, H, N_CTX, len(rs), n_seq, q_gain=1.5, row_seq=rs)
    got = _run_keys(ccx_ctx, q, wk, wv, bv, xa, rs, H, COUNTS)
    _check_fp64(got, q, wk, wv, bv, xa, rs, H, COUNTS, "rows mapped to sequences")
    for r in (0, 2, 7, 9):
        alone = _run(ccx_ctx, q[r:r + 1], wk, wv, bv, xa[rs[r]:rs[r] + 1, :COUNTS[rs[r]]], None, H)
        assert torch.equal(alone[0], got[r]), (H, r)
    P = 5
    rg = [s for s in range(n_seq) for _ in range(P)]
    q, wk, wv, bv, xa, _ = _case(530 + H, H, N_CTX, len(rg), n_seq, q_gain=1.5, row_seq=rg)
    grouped = _run_keys(ccx_ctx, q, wk, wv, bv, xa, rg, H, COUNTS, rows_per_seq=P)
    _check_fp64(grouped, q, wk, wv, bv, xa, rg, H, COUNTS, "prompt rows sharing a pass")
    assert torch.equal(_run_keys(ccx_ctx, q, wk, wv, bv, xa, rg, H, COUNTS), grouped)
    assert torch.equal(_run_keys(ccx_ctx, q, wk, wv, bv, xa, rg, H, COUNTS, rows_per_seq=P), grouped), "a second run differs"


@pytest.mark.parametrize("H", [2, 4])
def test_fp8_sibling_is_the_bf16_sibling_on_xhat(ccx_ctx, H):
    n_seq = len(COUNTS)
    q, wk, wv, bv, xa, _ = _case(540 + H, H, N_CTX, n_seq, n_seq, q_gain=2.0)
    got, xhat = _run_keys(ccx_ctx, q, wk, wv, bv, xa, None, H, COUNTS, fp8=True)
    assert torch.isfinite(got).all()
    assert not torch.equal(xhat, xa), "the quantiser changed nothing: the test would show nothing"
    assert torch.equal(got, _run_keys(ccx_ctx, q, wk, wv, bv, xhat, None, H, COUNTS))
    again, xhat2 = _run_keys(ccx_ctx, q, wk, wv, bv, xa, None, H, COUNTS, fp8=True)
    assert torch.equal(again, got) and torch.equal(xhat2, xhat)
    P = 5
    rg = [s for s in range(n_seq) for _ in range(P)]
    q, wk, wv, bv, xa, _ = _case(550 + H, H, N_CTX, len(rg), n_seq, q_gain=1.5, row_seq=rg)
    got, xhat = _run_keys(ccx_ctx, q, wk, wv, bv, xa, rg, H, COUNTS, rows_per_seq=P, fp8=True)
    assert torch.equal(got, _run_keys(ccx_ctx, q, wk, wv, bv, xhat, rg, H, COUNTS, rows_per_seq=P))


def test_argument_errors(ccx_ctx):
    from clearconverse_amd import _lib
    q, wk, wv, bv, xa, _ = _case(1, 2, N_CTX, 2, 2)
    for fp8 in (False, True):
        for bad in ([0, 5], [5, N_CTX + 1]):
            with pytest.raises(_lib.CcxError) as e:
                _run_keys(ccx_ctx, q, wk, wv, bv, xa, None, 2, bad, fp8=fp8)
            assert "outside [1, 80]" in str(e.value)
        with pytest.raises(_lib.CcxError) as e:
            _run_keys(ccx_ctx, q, wk, wv, bv, xa, None, 2, None, fp8=fp8)
        assert "n_keys_host is null" in str(e.value)
