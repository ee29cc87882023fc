"""GPU: the three word-alignment kernels (csrc/align.hip) away from the model, through ccx_align_op, against tests/align_reference.py.
Padding keys hold NaN bit patterns and every output is pre-filled with NaN, so a key read past n_keys or a cell never stored shows.

Bounds.  A priori (u = 2^-24):
  scores   a score is 64 fma and one multiply: |ds| <= 66 u S with S = sum |q_i k_i| / 8 < 200 in every case here (asserted); p =
           exp(s - max) / sum carries 2 |ds| + 2 u from the two scores and the exponential, the sum of <= 1500 terms in chains of
           <= 6 + a tree of 256 another ~20 u, the division 1 u: |dp| / max_j p <= 2 * 66 u * 200 + 25 u = 1.6e-3.
  matrix   z = (p - mean) / std with mean a sequential sum of T <= 226 terms: |d mean| <= T u mean, which the division by std turns
           into T u mean / std < 226 u * 10 (std / mean > 0.1 is asserted for every input column); std itself carries (T + 4) u / 2
           relative, times |z| <= sqrt(T) = 15: 226 u * 10 + 115 u * 15 + 4 u * 15 = 2.4e-4.  The median picks one of those values (it
           is 1-Lipschitz) and the mean over heads adds Hsel u |z|: 2.5e-4 absolute.
The first run on an MI355X measured 8.192e-07 (scores) and 4.953e-07 (matrix) as the worst values over this file
(profiles/align_kernels_measured_deviations.json); the bounds below are <= 2.5 x those, the project's rule.
  dtw      exact: costs are multiples of 1/64 in [-4, 4], every partial sum is exact in fp32, and the kernel's cells are single
           fp32 adds -- path, length and jump frames must equal the host loop.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import align_reference as AR
from tests.conftest import within

pytestmark = pytest.mark.gpu

TOL_SCORES = 2.0e-6       # a priori 1.6e-3; measured 8.192e-07
TOL_MATRIX = 1.2e-6       # a priori 2.5e-4; measured 4.953e-07
N_SCORES = "align scores: max |p - ref| / max_j ref"
N_MATRIX = "align matrix: max |A - ref| (standard deviations)"

SCORES, MATRIX, DTW = range(3)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, math.nan, device="cuda", dtype=dtype)


def _ints(vals):
    return (C.c_int * len(vals))(*[int(x) for x in vals])


def _call(ctx, op, d, labels=False):
    from clearconverse_amd import _lib
    lib = _lib.load()
    if labels:
        ctx.prof_enable(True)
    try:
        rc = lib.ccx_align_op(ctx.handle, op, C.byref(d), torch.cuda.current_stream().cuda_stream)
        names = [r[0] for r in ctx.prof_records()] if labels else []
    finally:
        if labels:
            ctx.prof_enable(False)
    torch.cuda.synchronize()
    return rc, lib.ccx_last_error(ctx.handle).decode(), names


# ---------------------------------------------------------------------------------------------------------------- scores
def _scores_desc(q, k, n_keys, Hsel, T, Mmax, t, heads=None, head0=0):
    """q [n_seq, H, 64] f32 CPU, k [n_seq, H, Spad, 64] CPU (bf16 values, NaN behind n_keys).  Returns (desc, P, keep-alive)."""
    from clearconverse_amd import _lib
    n_seq, H, Spad, _ = k.shape
    qd, kd = q.contiguous().cuda(), k.to(torch.bfloat16).cuda()
    P = _nan(n_seq, Hsel, T, Mmax)
    d = _lib.AlignDesc()
    d.q, d.q_elems, d.k, d.k_elems = qd.data_ptr(), qd.numel(), kd.data_ptr(), kd.numel()
    d.n_seq, d.H, d.Spad = n_seq, H, Spad
    heads = list(range(H)) if heads is None else heads
    hc, kc = _ints(heads), _ints(n_keys)
    d.heads, d.n_heads, d.head0, d.t = hc, len(heads), head0, t
    d.Hsel, d.T, d.Mmax, d.n_keys = Hsel, T, Mmax, kc
    d.P, d.P_elems = P.data_ptr(), P.numel()
    return d, P, (qd, kd, hc, kc)


def _scores_operands(seed, n_seq, n_keys, Spad, gain=1.0, H=2):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n_seq, H, 64, generator=g) * gain
    k = AR.bf16_round(torch.randn(n_seq, H, Spad, 64, generator=g))
    for s, n in enumerate(n_keys):
        k[s, :, n:] = math.nan
    return q, k


ALL_KEYS = [1, 7, 63, 64, 65, 1499, 1500]


@pytest.mark.parametrize("n_seq, n_keys, gain", [
    (1, [1500], 1.0),
    (3, [1, 7, 63], 1.0),
    (17, [ALL_KEYS[i % 7] for i in range(17)], 1.0),
    (3, [65, 1499, 1500], 16.0),        # the softmax range: scores of +-100, probabilities down to exp(-200) = 0
])
def test_scores(ccx_ctx, n_seq, n_keys, gain):
    Spad, Mmax, T, t = 1536, 1500, 2, 1
    q, k = _scores_operands(11 + n_seq, n_seq, n_keys, Spad, gain)
    assert AR.scores_abs_sum(q, k, n_keys) < 200.0            # the S of the bound
    d, P, keep = _scores_desc(q, k, n_keys, Hsel=2, T=T, Mmax=Mmax, t=t)
    rc, msg, names = _call(ccx_ctx, SCORES, d, labels=True)
    assert rc == 0, msg
    assert names == ["align_scores_kernel"]
    got = P.cpu()
    assert torch.isnan(got[:, :, 0]).all()                    # the other token row is not touched
    ref = AR.scores_ref(q, k, n_keys)
    for s, n in enumerate(n_keys):
        row = got[s, :, t]
        assert torch.isfinite(row).all(), (s, n)              # a padding key (NaN) never reached the result
        assert bool((row[:, n:] == 0).all()), (s, n)
        err = (row[:, :n].double() - ref[s, :, :n]).abs().amax(-1) / ref[s, :, :n].amax(-1)
        within(N_SCORES, float(err.max()), TOL_SCORES, (n_seq, s, n, gain))
        assert float((row[:, :n].double().sum(-1) - 1).abs().max()) < 1e-5


def test_scores_selected_heads_land_where_the_table_says(ccx_ctx):
    """heads = [1] of H = 2 written as head 2 of Hsel = 3: the other heads of P stay untouched"""
    q, k = _scores_operands(5, 2, [9, 70], 128)
    d, P, keep = _scores_desc(q, k, [9, 70], Hsel=3, T=1, Mmax=96, t=0, heads=[1], head0=2)
    rc, msg, _ = _call(ccx_ctx, SCORES, d)
    assert rc == 0, msg
    got = P.cpu()
    assert torch.isnan(got[:, :2]).all()
    ref = AR.scores_ref(q, k, [9, 70])
    for s, n in enumerate([9, 70]):
        within(N_SCORES, float((got[s, 2, 0, :n].double() - ref[s, 1, :n]).abs().max() / ref[s, 1, :n].max()), TOL_SCORES, s)


# ---------------------------------------------------------------------------------------------------------------- matrix
def _probs(seed, Hsel, T, M, gain=4.0):
    """[Hsel, T, M] probabilities: softmax rows of seeded scores with gain 4 over M + 1 keys, the last one dropped (over M = 1 key a
    softmax row is the constant 1, whose std over the tokens is 0).  Frames whose std / mean over the tokens is not above 0.12 are
    drawn again, so that no (head, frame) is a bad input."""
    g = torch.Generator().manual_seed(seed)
    s = gain * torch.randn(Hsel, T, M + 1, generator=g)
    for _ in range(200):
        p = torch.softmax(s, dim=-1)[..., :M]
        std, mean = torch.std_mean(p.double(), dim=1, unbiased=False)
        bad = (std / mean) <= 0.12
        if not bool(bad.any()):
            break
        idx = bad.nonzero()
        s[idx[:, 0], :, idx[:, 1]] = gain * torch.randn(len(idx), T, generator=g)
    return p.contiguous()


def _matrix_desc(Ps, Hsel, T, Mmax):
    """Ps: list of [Hsel, T_s, M_s] CPU tensors -> (desc, P device, A device, keep)"""
    from clearconverse_amd import _lib
    n_seq = len(Ps)
    P = torch.full((n_seq, Hsel, T, Mmax), math.nan)
    for s, p in enumerate(Ps):
        P[s, :, :p.shape[1], :p.shape[2]] = p
    Pd, A = P.cuda(), _nan(n_seq, T, Mmax)
    d = _lib.AlignDesc()
    rows, keys = _ints([p.shape[1] for p in Ps]), _ints([p.shape[2] for p in Ps])
    d.n_seq, d.Hsel, d.T, d.Mmax, d.n_keys, d.n_rows = n_seq, Hsel, T, Mmax, keys, rows
    d.P, d.P_elems, d.A, d.A_elems = Pd.data_ptr(), Pd.numel(), A.data_ptr(), A.numel()
    return d, Pd, A, (rows, keys)


def _check_matrix(ctx, Ps, Hsel, T, Mmax, what):
    for p in Ps:
        std, mean = torch.std_mean(p.double(), dim=1, unbiased=False)
        assert bool((std / mean > 0.1).all()), (what, tuple(p.shape))       # the input condition of the bound, on the CPU
    d, Pd, A, keep = _matrix_desc(Ps, Hsel, T, Mmax)
    rc, msg, names = _call(ctx, MATRIX, d, labels=True)
    assert rc == 0, msg
    assert names == ["align_matrix_kernel"]
    got = A.cpu()
    for s, p in enumerate(Ps):
        Ts, Ms = p.shape[1], p.shape[2]
        blk = got[s, :Ts, :Ms]
        assert torch.isfinite(blk).all(), (what, s)
        assert torch.isnan(got[s, Ts:]).all() and torch.isnan(got[s, :, Ms:]).all(), (what, s)     # nothing written outside the block
        within(N_MATRIX, float((blk.double() - AR.matrix_ref(p)).abs().max()), TOL_MATRIX, (what, s, Ts, Ms))


MS = [1, 3, 4, 7, 8, 750, 1500]


@pytest.mark.parametrize("Hsel, Ts", [(6, [2, 5, 226, 2, 5, 226, 226]), (1, [226, 2, 5, 226, 2, 5, 2])])
def test_matrix(ccx_ctx, Hsel, Ts):
    """every M with a T of each size, seven sequences of different shapes in one launch"""
    Ps = [_probs(100 * Hsel + i, Hsel, T, M) for i, (T, M) in enumerate(zip(Ts, MS))]
    _check_matrix(ccx_ctx, Ps, Hsel, 226, 1500, f"Hsel={Hsel}")


def test_matrix_median_with_equal_neighbours(ccx_ctx):
    """frames 4, 5 and 9, 10 carry the same column: their standardised values are equal bit for bit inside every median window that
    holds them -- the 4th of 7 must be an order statistic, not a selection that assumes distinct values"""
    p = _probs(7, 2, 5, 70)
    p[:, :, 5] = p[:, :, 4]
    p[:, :, 10] = p[:, :, 9]
    p[:, :, 66] = p[:, :, 64]          # across the boundary of the kernel's 64-frame tile
    _check_matrix(ccx_ctx, [p], 2, 5, 72, "equal neighbours")


# ---------------------------------------------------------------------------------------------------------------- dtw
def _grid_costs(seed, N, M):
    g = np.random.default_rng(seed)
    return (g.integers(-256, 257, (N, M)) / 64.0).astype(np.float32)


def _dtw_desc(xs, r0, T, Mmax):
    """xs: list of fp32 cost matrices [N_s, M_s]; A = -x in rows r0 .. r0 + N_s, NaN everywhere else"""
    from clearconverse_amd import _lib
    n_seq = len(xs)
    A = np.full((n_seq, T, Mmax), np.nan, dtype=np.float32)
    for s, x in enumerate(xs):
        A[s, r0:r0 + x.shape[0], :x.shape[1]] = -x
    Ad = torch.from_numpy(A).cuda()
    ti = torch.full((n_seq, T + Mmax), -7, device="cuda", dtype=torch.int32)
    tj, ln, jf = ti.clone(), torch.full((n_seq,), -7, device="cuda", dtype=torch.int32), torch.full((n_seq, T), -7, device="cuda", dtype=torch.int32)
    d = _lib.AlignDesc()
    rows, keys = _ints([r0 + x.shape[0] for x in xs]), _ints([x.shape[1] for x in xs])
    d.n_seq, d.Hsel, d.T, d.Mmax, d.n_keys, d.n_rows, d.r0 = n_seq, 1, T, Mmax, keys, rows, r0
    d.A, d.A_elems = Ad.data_ptr(), Ad.numel()
    d.text_idx, d.text_idx_elems, d.time_idx, d.time_idx_elems = ti.data_ptr(), ti.numel(), tj.data_ptr(), tj.numel()
    d.path_len, d.path_len_elems, d.jump_frame, d.jump_frame_elems = ln.data_ptr(), ln.numel(), jf.data_ptr(), jf.numel()
    return d, (Ad, ti, tj, ln, jf, rows, keys)


def _check_dtw(ctx, xs, r0, T, Mmax):
    d, (Ad, ti, tj, ln, jf, rows, keys) = _dtw_desc(xs, r0, T, Mmax)
    rc, msg, names = _call(ctx, DTW, d, labels=True)
    assert rc == 0, msg
    assert names == ["align_dtw_kernel"]
    ti, tj, ln, jf = ti.cpu().numpy(), tj.cpu().numpy(), ln.cpu().numpy(), jf.cpu().numpy()
    for s, x in enumerate(xs):
        N, M = x.shape
        ri, rj = AR.dtw_ref_fast(x) if N * M > 4096 else AR.dtw_ref(x)
        assert ln[s] == len(ri) <= N + M - 1, (s, N, M)
        assert np.array_equal(ti[s, :ln[s]], ri) and np.array_equal(tj[s, :ln[s]], rj), (s, N, M)
        assert np.array_equal(jf[s, :N], AR.jump_frames(ri, rj)) and bool((jf[s, N:] == -1).all()), (s, N, M)


def test_dtw_small_and_ragged(ccx_ctx):
    shapes = [(1, 1), (1, 9), (9, 1), (2, 3), (64, 64), (65, 63), (226, 1500)]
    _check_dtw(ccx_ctx, [_grid_costs(i, N, M) for i, (N, M) in enumerate(shapes)], r0=1, T=227, Mmax=1500)


def test_dtw_full_size_ties_and_planted_diagonal(ccx_ctx):
    flat = np.zeros((20, 30), dtype=np.float32)                   # all equal (0, so that costs tie too): every inner cell takes "left"
    diag = _grid_costs(3, 40, 40) * 0 + 1.0
    diag[np.arange(40), np.arange(40)] = -4.0                     # planted: the path must be the diagonal
    _check_dtw(ccx_ctx, [_grid_costs(9, 448, 1500), flat, diag], r0=0, T=448, Mmax=1500)
    ri, rj = AR.dtw_ref(diag)
    assert ri.tolist() == rj.tolist() == list(range(40))
    ri, rj = AR.dtw_ref(flat)
    assert ri.tolist() == list(range(20)) + [19] * 29 and rj.tolist() == [0] * 20 + list(range(1, 30))


# ---------------------------------------------------------------------------------------------------------------- descriptor violations
def _valid(op):
    if op == SCORES:
        q, k = _scores_operands(1, 2, [5, 40], 64)
        d, P, keep = _scores_desc(q, k, [5, 40], Hsel=2, T=3, Mmax=48, t=1)
        return d, [P], keep
    if op == MATRIX:
        d, Pd, A, keep = _matrix_desc([_probs(1, 2, 4, 9), _probs(2, 2, 3, 5)], 2, 4, 12)
        return d, [A], (Pd, keep)
    d, keep = _dtw_desc([_grid_costs(1, 3, 5), _grid_costs(2, 2, 7)], 1, 6, 8)
    return d, [keep[1], keep[2], keep[3], keep[4]], keep


def _set(**kw):
    def f(d):
        for n, v in kw.items():
            setattr(d, n, v(getattr(d, n)) if callable(v) else v)
    return f


def _arr(name, vals):
    def f(d):
        a = _ints(vals)
        f.keep = a
        setattr(d, name, a)
    return f


VIOLATIONS = [
    (SCORES, _set(n_seq=0), "n_seq"), (SCORES, _set(Hsel=97), "Hsel"), (SCORES, _set(T=449), "T ="), (SCORES, _set(Mmax=1501), "Mmax"),
    (SCORES, _set(n_keys=None), "n_keys is NULL"), (SCORES, _arr("n_keys", [0, 40]), "n_keys[0]"), (SCORES, _arr("n_keys", [5, 49]), "n_keys[1]"),
    (SCORES, _set(H=65), "H ="), (SCORES, _set(Spad=0), "Spad"), (SCORES, _set(Spad=32), "exceeds Spad"),
    (SCORES, _set(heads=None), "heads"), (SCORES, _set(n_heads=0), "n_heads"), (SCORES, _set(head0=1), "head0"),
    (SCORES, _arr("heads", [0, 2]), "heads[1]"), (SCORES, _set(t=3), "t ="), (SCORES, _set(t=-1), "t ="),
    (SCORES, _set(q=None), "q is NULL"), (SCORES, _set(q=lambda p: p + 4), "q is not 16-byte aligned"), (SCORES, _set(q_elems=lambda n: n - 1), "q_elems"),
    (SCORES, _set(k=None), "k is NULL"), (SCORES, _set(k=lambda p: p + 2), "k is not 16-byte aligned"), (SCORES, _set(k_elems=lambda n: n - 1), "k_elems"),
    (SCORES, _set(P=None), "P is NULL"), (SCORES, _set(P=lambda p: p + 4), "P is not 16-byte aligned"), (SCORES, _set(P_elems=lambda n: n - 1), "P_elems"),
    (MATRIX, _set(n_rows=None), "n_rows is NULL"), (MATRIX, _arr("n_rows", [1, 3]), "n_rows[0]"), (MATRIX, _arr("n_rows", [4, 5]), "n_rows[1]"),
    (MATRIX, _set(P=None), "P is NULL"), (MATRIX, _set(P=lambda p: p + 4), "P is not 16-byte aligned"),
    (MATRIX, _set(P_elems=lambda n: n - 1), "P_elems"), (MATRIX, _set(A=None), "A is NULL"), (MATRIX, _set(A=lambda p: p + 8), "A is not 16-byte aligned"),
    (MATRIX, _set(A_elems=lambda n: n - 1), "A_elems"), (MATRIX, lambda d: setattr(d, "A", d.P), "aliases"),
    (DTW, _set(r0=-1), "r0"), (DTW, _set(r0=3), "r0"), (DTW, _arr("n_rows", [4, 7]), "n_rows[1]"), (DTW, _set(A_elems=lambda n: n - 1), "A_elems"),
    (DTW, _set(A=None), "A is NULL"), (DTW, _set(A=lambda p: p + 4), "A is not 16-byte aligned"),
    (DTW, _set(text_idx=lambda p: p + 4), "text_idx is not 16-byte aligned"), (DTW, _set(time_idx=None), "time_idx is NULL"),
    (DTW, _set(path_len=lambda p: p + 4), "path_len is not 16-byte aligned"), (DTW, _set(jump_frame=lambda p: p + 8), "jump_frame is not 16-byte aligned"),
    (DTW, _set(text_idx=None), "text_idx is NULL"), (DTW, _set(text_idx_elems=lambda n: n - 1), "text_idx_elems"),
    (DTW, _set(time_idx=lambda p: p + 4), "time_idx is not 16-byte aligned"), (DTW, _set(time_idx_elems=lambda n: n - 1), "time_idx_elems"),
    (DTW, _set(path_len=None), "path_len is NULL"), (DTW, _set(path_len_elems=1), "path_len_elems"),
    (DTW, _set(jump_frame=None), "jump_frame is NULL"), (DTW, _set(jump_frame_elems=lambda n: n - 1), "jump_frame_elems"),
]


def test_descriptor_violations_return_err_arg_with_nothing_launched(ccx_ctx):
    from clearconverse_amd import _lib
    lib = _lib.load()
    rc = lib.ccx_align_op(ccx_ctx.handle, 3, C.byref(_valid(SCORES)[0]), None)
    assert rc == 1 and "ccx_align_op: unknown op" in lib.ccx_last_error(ccx_ctx.handle).decode()
    assert lib.ccx_align_op(ccx_ctx.handle, SCORES, None, None) == 1
    for i, (op, mutate, fragment) in enumerate(VIOLATIONS):
        d, outs, keep = _valid(op)
        before = [o.clone() for o in outs]
        mutate(d)
        rc, msg, names = _call(ccx_ctx, op, d, labels=True)
        assert rc == 1, (i, fragment, msg)
        assert "ccx_align_op" in msg and fragment in msg, (i, fragment, msg)
        assert names == [], (i, fragment)
        for o, b in zip(outs, before):
            assert torch.equal(o.view(torch.int32), b.view(torch.int32)), (i, fragment)      # bit patterns: NaN == NaN here
    # and each valid descriptor runs
    for op in (SCORES, MATRIX, DTW):
        rc, msg, _ = _call(ccx_ctx, op, _valid(op)[0])
        assert rc == 0, msg
