"""GPU: dec_linear_kernel (csrc/decoder.hip) on its own, one launch at a time through ccx_dec_linear_op -- the parameter block the
<= 16-row decode chain fills and the production launcher unchanged -- against the fp64 reference of tests/dec_linear_reference.py.

Shapes are the smallest at which each thing can go wrong: every LayerNorm width class (a float4 slot partly live, depths 6 / 8 / 10, the
5-slot form), ragged row counts around the two-rows-per-pass pairing, every pending-slab count, every K-slice layout, real cache
positions and row -> sequence maps, N tails.  Every output, cache and gap between strides starts as 0xFF bytes (NaN bit patterns in f32
and in bf16), so a quad never stored, a store outside its place and a read of a slab that is not pending all show.

Bounds (tests/dec_linear_reference.py bound()): 4 x the figure of an fp32 evaluation of the same computation on the CPU
(profiles/dec_linear_measured_deviations.json "yardstick", next to the values measured on an MI355X), never above 2^-8 + K 2^-24.  The
exact checks -- the resolved rows, the sentinels, the bit-equalities, the zero shifts -- have no tolerance.

The host matrices and the device vectors of a shape are made once and cached (LR.weights, _dev); the packed weight image is not: the
entry point takes the host matrix and packs and uploads it on every call."""
import ctypes as C

import pytest
import torch

from tests import dec_linear_reference as LR
from tests import dec_reference as DR
from tests.conftest import within

pytestmark = pytest.mark.gpu

GAP = 64                     # elements between two slabs
_dev_cache = {}


def _nan(shape, dtype=torch.float32):
    """a device buffer of 0xFF bytes"""
    return torch.full(shape, -1, dtype=torch.int32 if dtype == torch.float32 else torch.int16, device="cuda").view(dtype)


def _untouched(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16) == -1


def _dev(K, N):
    """the device vectors of a shape, uploaded once; the host matrix stays where LR.weights keeps it"""
    if (K, N) not in _dev_cache:
        w = LR.weights(K, N)
        _dev_cache[(K, N)] = {k: w[k].cuda() for k in ("bias", "ln_g", "ln_b")}
    return _dev_cache[(K, N)]


def _desc(act, epi, M, N, K, bias=True):
    from clearconverse_amd import _lib
    d = _lib.DecLinearDesc()
    d.act, d.epi, d.M, d.N, d.K = act, epi, M, N, K
    d.w_host = LR.weights(K, N)["w"].data_ptr()
    if bias:
        d.bias, d.bias_elems = _dev(K, N)["bias"].data_ptr(), N
    d.eps = LR.EPS
    return d


def _ln(d, pend_n, x_out=True, mean_out=True):
    """the ACT_LN operands of d's shape: rows 0 .. M - 1 of LR.ln_inputs, four slab places of which the first pend_n hold slabs (with
    pend_n == 0 the first one too: it is read with weight 0) and the others NaN, the slabs GAP apart"""
    M, K = d.M, d.K
    x, pend = LR.ln_inputs(K)
    dv = _dev(K, d.N)
    t = {"x": x[:M].contiguous().cuda(), "x_out": _nan((16, K)), "mean": _nan((16,))}
    stride = M * K + GAP
    t["pend"] = _nan((3 * stride + M * K,))
    for s in range(max(pend_n, 1)):
        t["pend"][s * stride:s * stride + M * K] = pend[s, :M].reshape(-1).cuda()
    d.x, d.x_elems = t["x"].data_ptr(), t["x"].numel()
    d.pend, d.pend_n, d.pend_stride, d.pend_elems = t["pend"].data_ptr(), pend_n, stride, t["pend"].numel()
    d.ln_g, d.ln_b, d.ln_elems = dv["ln_g"].data_ptr(), dv["ln_b"].data_ptr(), K
    if x_out:
        d.x_out, d.x_out_elems = t["x_out"].data_ptr(), t["x_out"].numel()
    if mean_out:
        d.ln_mean_out, d.ln_mean_out_elems = t["mean"].data_ptr(), 16
    return t


def _bf16(d, rows, lda=None):
    """ACT_BF16: the rows (values that are bf16 already) lda apart, the gap NaN.  -> the buffer, which the caller keeps bound until
    the call has returned"""
    lda = d.K if lda is None else lda
    a = _nan((d.M, lda), torch.bfloat16)
    a[:, :d.K] = rows.cuda().to(torch.bfloat16)
    d.act_rows, d.lda, d.act_elems = a.data_ptr(), lda, a.numel()
    return a


def _out(d, rows, ldo, dtype=torch.float32, slabs=1):
    """`out`: `slabs` slabs of rows x ldo, GAP apart, all NaN.  -> the buffer and its view [slabs][rows][ldo]"""
    stride = rows * ldo + GAP
    buf = _nan((slabs * stride,), dtype)
    d.out, d.ldo, d.out_elems = buf.data_ptr(), ldo, buf.numel()
    if d.epi == LR.PARTIAL:
        d.out_stride = stride
    return buf, buf.view(slabs, stride)[:, :rows * ldo].view(slabs, rows, ldo), buf.view(slabs, stride)[:, rows * ldo:]


def _call(ctx, d, what="ccx_dec_linear_op"):
    from clearconverse_amd import _lib
    lib = _lib.load()
    rc = lib.ccx_dec_linear_op(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, what)


def _check_side_outputs(t, xr, M, what):
    """x_out: the resolved rows bit for bit, nothing behind them.  ln_mean_out: exactly 0 below the threshold, the mean above it (an
    fp32 sum chain of depth <= 16: 2^-20 of the row's mean |x|), nothing behind row M."""
    assert torch.equal(t["x_out"][:M].cpu(), xr[:M]), what
    assert _untouched(t["x_out"][M:]).all(), what
    shift, ratio = LR.centre_shift(xr[:M])
    mean_abs = xr[:M].double().abs().mean(dim=1)
    mo = t["mean"].cpu()
    assert _untouched(t["mean"][M:]).all(), what
    lo, hi = ratio <= 0.8, ratio >= 1.25
    assert bool((lo | hi).all()) and bool((mo[:M][lo] == 0.0).all()), (what, mo[:M], ratio)
    assert bool(((mo[:M].double() - shift).abs()[hi] <= 2.0 ** -20 * mean_abs[hi]).all()), (what, mo[:M], shift)


# ---- ACT_LN prologue ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LR.LN_WIDTHS)
def test_layernorm_prologue(ccx_ctx, K):
    N = LR.N_SMALL
    x, pend = LR.ln_inputs(K)
    w = LR.weights(K, N)
    tol = LR.bound(LR.N_LN, K)
    row0 = {}
    for n in LR.LN_PEND:
        xr = LR.resolve(x, pend, n)
        ref = LR.linear(LR.layer_norm(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"])
        for M in LR.LN_ROWS:
            what = (K, M, n)
            d = _desc(LR.ACT_LN, LR.F32, M, N, K)
            t = _ln(d, n)
            _, out, _ = _out(d, 16, N)
            _call(ccx_ctx, d)
            got = out[0].cpu()
            assert torch.isfinite(got[:M]).all(), what                 # a slab that is not pending was not added
            assert _untouched(out[0, M:]).all(), what
            fig = LR.row_rel_l2(got[:M], ref[:M])
            print(f"K {K} M {M} pend_n {n}: rel-L2 {fig:.3e} (bound {tol:.3e})")
            within(LR.N_LN, fig, tol, what)
            _check_side_outputs(t, xr, M, what)
            row0[(M, n)] = got[0].clone()
        # a row's bits do not depend on the rows beside it
        assert torch.equal(row0[(1, n)], row0[(16, n)]), (K, n)
        assert torch.equal(row0[(5, n)], row0[(16, n)]), (K, n)


def test_layernorm_prologue_without_its_side_outputs(ccx_ctx):
    """x_out = NULL and ln_mean_out = NULL: the same rows, bit for bit"""
    K, N, M, n = 768, LR.N_SMALL, 9, 3
    outs = []
    for side in (True, False):
        d = _desc(LR.ACT_LN, LR.F32, M, N, K)
        t = _ln(d, n, x_out=side, mean_out=side)
        _, out, _ = _out(d, 16, N)
        _call(ccx_ctx, d)
        outs.append(out[0].cpu())
        assert side or (_untouched(t["x_out"]).all() and _untouched(t["mean"]).all())
    assert torch.isfinite(outs[0][:M]).all() and torch.equal(outs[0][:M], outs[1][:M])


def _ln_linear_pair(ctx, K, N, epi, rows, outs=None):
    """ccx_dec_ln_linear (dec_resolve_ln_kernel -> dec_linear<ACT_BF16>) on M = 17 rows: what the > 16-row chain computes.
    outs: a list that receives the device `out` before the call"""
    from clearconverse_amd import _lib
    lib = _lib.load()
    dv = _dev(K, N)
    x = rows.contiguous().cuda()
    M = x.shape[0]
    out = _nan((3, M, K) if epi == LR.SELF_QKV else (M, N))
    d = _lib.DecLnLinearDesc()
    d.M, d.K, d.F, d.N, d.epi, d.packed = M, K, 0, N, epi, 0
    d.x, d.x_elems, d.ln_g, d.ln_b, d.eps = x.data_ptr(), x.numel(), dv["ln_g"].data_ptr(), dv["ln_b"].data_ptr(), LR.EPS
    d.w_host, d.bias, d.out, d.out_elems = LR.weights(K, N)["w"].data_ptr(), dv["bias"].data_ptr(), out.data_ptr(), out.numel()
    if outs is not None:
        outs.append(out)
    rc = lib.ccx_dec_ln_linear(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_ln_linear")
    return out.cpu()


@pytest.mark.parametrize("K", (128, 768))
def test_rows_do_not_depend_on_which_kernel_normalised_them(ccx_ctx, K):
    """dec_ln.h and decoder.h promise it: the LayerNorm prologue (<= 16 rows) and dec_resolve_ln_kernel -> ACT_BF16 (> 16 rows) give a
    row the same bits"""
    x, _ = LR.ln_inputs(K)
    rows17 = torch.cat([x, x[3:4]])
    for epi, N in ((LR.F32, LR.N_SMALL), (LR.GELU, LR.N_SMALL), (LR.SELF_QKV, 3 * K)):
        pair = _ln_linear_pair(ccx_ctx, K, N, epi, rows17)
        d = _desc(LR.ACT_LN, epi, 16, N, K)
        ops = _ln(d, 0)                              # (bound until the call has returned, like every device buffer here)
        if epi == LR.SELF_QKV:
            ck, cv = _nan((16, K // 64, 1, 64), torch.bfloat16), _nan((16, K // 64, 1, 64), torch.bfloat16)
            pos = (C.c_int * 16)(*([0] * 16))
            d.cache_k, d.cache_v, d.cache_elems, d.cache_T, d.n_seq, d.pos = ck.data_ptr(), cv.data_ptr(), ck.numel(), 1, 16, pos
            _, out, _ = _out(d, 16, K)
            _call(ccx_ctx, d)
            assert torch.equal(out[0].cpu(), pair[0, :16]), (K, "q")
            assert torch.equal(ck.float().cpu().reshape(16, K), pair[1, :16]) and torch.equal(cv.float().cpu().reshape(16, K), pair[2, :16]), (K, "k / v")
        else:
            _, out, _ = _out(d, 16, N, torch.bfloat16 if epi == LR.GELU else torch.float32)
            _call(ccx_ctx, d)
            got = out[0].float().cpu()
            assert torch.isfinite(got).all() and torch.equal(got, pair[:16]), (K, epi, float((got - pair[:16]).abs().max()))


# ---- GELU epilogue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,ldo", LR.GELU_CASES)
def test_layernorm_gelu(ccx_ctx, K, N, ldo):
    x, pend = LR.ln_inputs(K)
    w = LR.weights(K, N)
    for M, n in zip((16, 5), LR.SIDE_PEND):
        xr = LR.resolve(x, pend, n)
        ref = LR.gelu(LR.linear(LR.layer_norm(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"]))
        d = _desc(LR.ACT_LN, LR.GELU, M, N, K)
        t = _ln(d, n)
        _, out, _ = _out(d, 16, ldo, torch.bfloat16)
        _call(ccx_ctx, d)
        assert _untouched(out[0, :, N:]).all() and _untouched(out[0, M:]).all(), (K, M)
        _check_side_outputs(t, xr, M, (K, N, M, n))
        got = out[0, :M, :N].float().cpu()
        assert torch.isfinite(got).all(), (K, M)
        fig = LR.bf16_excess(got, ref[:M])
        print(f"LN -> GELU K {K} N {N} M {M}: excess {fig:.3e}")
        within(LR.N_GELU, fig, LR.bound(LR.N_GELU, K), (K, N, M))


@pytest.mark.parametrize("K,N,ldo", LR.GELU_BF16_CASES)
def test_bf16_gelu(ccx_ctx, K, N, ldo):
    w = LR.weights(K, N)
    a = LR.bf16_rows(16, K)
    ref = LR.gelu(LR.linear(a, w["w"], w["bias"]))
    for M in (5, 16):
        d = _desc(LR.ACT_BF16, LR.GELU, M, N, K)
        rows = _bf16(d, a[:M], K + 8)                # (device buffers stay bound until the call has returned)
        _, out, _ = _out(d, 16, ldo, torch.bfloat16)
        _call(ccx_ctx, d)
        assert _untouched(out[0, :, N:]).all() and _untouched(out[0, M:]).all(), (K, M)
        got = out[0, :M, :N].float().cpu()
        assert torch.isfinite(got).all(), (K, M)
        fig = LR.bf16_excess(got, ref[:M])
        print(f"bf16 -> GELU K {K} N {N} M {M}: excess {fig:.3e}")
        within(LR.N_GELU_BF16, fig, LR.bound_gelu_bf16(K), (K, N, M))


# ---- SELF_QKV epilogue -------------------------------------------------------------------------------------------------------
_qkv_refs = {}


def _qkv_ref(K, act, n=0):
    """q | k | v of the 16 LayerNorm rows under n pending slabs, or of the 40 bf16 rows"""
    if (K, act, n) not in _qkv_refs:
        w = LR.weights(K, 3 * K)
        x, pend = LR.ln_inputs(K)
        a = LR.layer_norm(LR.resolve(x, pend, n), w["ln_g"], w["ln_b"]) if act == LR.ACT_LN else LR.bf16_rows(40, K)
        _qkv_refs[(K, act, n)] = LR.linear(a, w["w"], w["bias"])
    return _qkv_refs[(K, act, n)]


@pytest.mark.parametrize("cache_T", LR.QKV_CACHE_T)
@pytest.mark.parametrize("K", LR.QKV_WIDTHS)
def test_self_qkv_cache_append(ccx_ctx, K, cache_T):
    H = K // 64
    for act, cases in ((LR.ACT_LN, "ab"), (LR.ACT_BF16, "abc")):
        for case in cases:
            what = (K, cache_T, act, case)
            M, n_seq, pos, row_seq = LR.qkv_addressing(case, cache_T)
            n = LR.SIDE_PEND["ab".index(case)] if act == LR.ACT_LN else 0       # a: no pending slab, b: three
            ref = _qkv_ref(K, act, n)[:M]
            d = _desc(act, LR.SELF_QKV, M, 3 * K, K)
            ops = _ln(d, n) if act == LR.ACT_LN else _bf16(d, LR.bf16_rows(40, K)[:M])
            ck, cv = _nan((n_seq, H, cache_T, 64), torch.bfloat16), _nan((n_seq, H, cache_T, 64), torch.bfloat16)
            hpos = (C.c_int * M)(*pos)
            hseq = (C.c_int * M)(*row_seq) if row_seq is not None else None
            d.cache_k, d.cache_v, d.cache_elems, d.cache_T, d.n_seq, d.pos = ck.data_ptr(), cv.data_ptr(), ck.numel(), cache_T, n_seq, hpos
            if hseq is not None:
                d.row_seq = hseq
            _, out, _ = _out(d, M + 2, K)
            _call(ccx_ctx, d)
            q = out[0, :M].cpu()
            assert torch.isfinite(q).all() and _untouched(out[0, M:]).all(), what
            if act == LR.ACT_LN:
                _check_side_outputs(ops, LR.resolve(*LR.ln_inputs(K), n), M, what)
            name = LR.N_LN if act == LR.ACT_LN else LR.n_bf16(K)
            within(name, LR.row_rel_l2(q, ref[:, :K]), LR.bound(name, K), what)
            for cache, cols in ((ck, slice(K, 2 * K)), (cv, slice(2 * K, 3 * K))):
                exp, written = LR.cache_scatter(ref[:, cols], pos, row_seq, n_seq, cache_T)
                fig, clean = LR.cache_figures(cache.float().cpu(), exp, written, _untouched(cache).cpu())
                assert clean, what                                       # every element no row names still holds the sentinel
                print(f"cache K {K} T {cache_T} act {act} case {case}: excess {fig:.3e}")
                name = LR.N_CACHE_LN if act == LR.ACT_LN else LR.N_CACHE_BF16
                within(name, fig, LR.bound(name, K), what)


# ---- ACT_COMBINE prologue ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", LR.COMBINE_HEADS)
def test_combine_prologue(ccx_ctx, H):
    K = 64 * H
    for M, ns, T, spike, N in LR.combine_cases(H):
        what = (H, M, ns, T, spike, N)
        po, pml = LR.combine_inputs(H, M, ns, T, spike)
        w = LR.weights(K, N)
        ref = LR.partial_slabs(LR.combine(po, pml), w["w"], w["bias"])
        d = _desc(LR.ACT_COMBINE, LR.PARTIAL, M, N, K)
        dpo, dpml = po.cuda(), pml.cuda()
        d.part_o, d.part_ml, d.nsplit, d.part_o_elems, d.part_ml_elems = dpo.data_ptr(), dpml.data_ptr(), ns, dpo.numel(), dpml.numel()
        _, out, gaps = _out(d, M, N, slabs=ref.shape[0])
        _call(ccx_ctx, d)
        got = out.cpu()
        assert torch.isfinite(got).all() and _untouched(gaps).all(), what
        fig = LR.row_rel_l2(got, ref)
        print(f"combine H {H} M {M} nsplit {ns} T {T} spike {spike} N {N}: rel-L2 {fig:.3e}")
        within(LR.N_COMBINE, fig, LR.bound(LR.N_COMBINE, K), what)


# ---- PARTIAL epilogue, K slices ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LR.SLICE_WIDTHS)
def test_partial_k_slices(ccx_ctx, K):
    N = LR.N_SMALL
    w = LR.weights(K, N)
    a = LR.bf16_rows(16, K)
    ref = LR.partial_slabs(a, w["w"], w["bias"])
    name = LR.n_bf16(K)
    for M in LR.SLICE_ROWS:
        d = _desc(LR.ACT_BF16, LR.PARTIAL, M, N, K)
        rows = _bf16(d, a[:M])
        _, out, gaps = _out(d, M, N, slabs=ref.shape[0])
        _call(ccx_ctx, d)
        got = out.cpu()
        assert torch.isfinite(got).all() and _untouched(gaps).all(), (K, M)
        fig, fig_sum = LR.row_rel_l2(got, ref[:, :M]), LR.row_rel_l2(got.double().sum(0), ref[:, :M].sum(0))
        print(f"K slices K {K} M {M}: rel-L2 per slab {fig:.3e}, of the sum {fig_sum:.3e}")
        within(name, fig, LR.bound(name, K), (K, M, "slabs"))
        within(name, fig_sum, LR.bound(name, K), (K, M, "sum"))


# ---- F32 epilogue, N tails and strides ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LR.TAIL_WIDTHS)
def test_f32_tails_and_strides(ccx_ctx, K):
    M = 5
    a = LR.bf16_rows(5, K)
    name = LR.n_bf16(K)
    for N in LR.TAIL_N:
        w = LR.weights(K, N)
        ref = LR.linear(a, w["w"], w["bias"])
        d = _desc(LR.ACT_BF16, LR.F32, M, N, K)
        rows = _bf16(d, a, K + 8)
        _, out, _ = _out(d, M + 3, N + 8)
        _call(ccx_ctx, d)
        assert _untouched(out[0, :, N:]).all() and _untouched(out[0, M:]).all(), (K, N)
        got = out[0, :M, :N].cpu()
        assert torch.isfinite(got).all(), (K, N)
        within(name, LR.row_rel_l2(got, ref), LR.bound(name, K), (K, N))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _valid(kind):
    """a descriptor the entry point accepts, its `out` buffer and what must stay alive"""
    if kind == "ln":
        d = _desc(LR.ACT_LN, LR.F32, 5, LR.N_SMALL, 768)
        keep = [_ln(d, 3)]
        keep.append(_out(d, 16, LR.N_SMALL))
    elif kind == "gelu":
        d = _desc(LR.ACT_LN, LR.GELU, 5, 512, 128)
        keep = [_ln(d, 0)]
        keep.append(_out(d, 16, 520, torch.bfloat16))
    elif kind == "bf16":
        d = _desc(LR.ACT_BF16, LR.F32, 5, LR.N_SMALL, 768)
        keep = [_bf16(d, LR.bf16_rows(5, 768), 776)]
        keep.append(_out(d, 8, LR.N_SMALL + 8))
    elif kind == "partial":
        d = _desc(LR.ACT_BF16, LR.PARTIAL, 3, LR.N_SMALL, 1536)
        keep = [_bf16(d, LR.bf16_rows(16, 1536)[:3])]
        keep.append(_out(d, 3, LR.N_SMALL, slabs=2))
    elif kind == "combine":
        d = _desc(LR.ACT_COMBINE, LR.PARTIAL, 7, LR.N_SMALL, 128)
        po, pml = (t.cuda() for t in LR.combine_inputs(2, 7, 5))
        d.part_o, d.part_ml, d.nsplit, d.part_o_elems, d.part_ml_elems = po.data_ptr(), pml.data_ptr(), 5, po.numel(), pml.numel()
        keep = [po, pml]
        keep.append(_out(d, 7, LR.N_SMALL))
    else:
        assert kind == "qkv"
        M, n_seq, pos, row_seq = LR.qkv_addressing("b", 8)
        d = _desc(LR.ACT_LN, LR.SELF_QKV, M, 384, 128)
        ck, cv = _nan((n_seq, 2, 8, 64), torch.bfloat16), _nan((n_seq, 2, 8, 64), torch.bfloat16)
        hpos, hseq = (C.c_int * M)(*pos), (C.c_int * M)(*row_seq)
        d.cache_k, d.cache_v, d.cache_elems, d.cache_T, d.n_seq, d.pos, d.row_seq = ck.data_ptr(), cv.data_ptr(), ck.numel(), 8, n_seq, hpos, hseq
        keep = [_ln(d, 0), ck, cv, hpos, hseq]
        keep.append(_out(d, M, 128))
    return d, keep[-1][0], keep


def S(**kw):
    return lambda d: [setattr(d, k, v) for k, v in kw.items()]


def P(name, nbytes=4):
    """the pointer moved off its 16-byte alignment"""
    return lambda d: setattr(d, name, getattr(d, name) + nbytes)


def E(name):
    """one element fewer behind the pointer than the launch touches"""
    return lambda d: setattr(d, name, getattr(d, name) - 1)


def I(name, i, v):
    def f(d):
        getattr(d, name)[i] = v
    return f


REFUSALS = [
    # the pair, the shape
    ("ln", "unknown act", S(act=3)), ("ln", "unknown epi", S(epi=4)), ("ln", "not a pair", S(epi=LR.PARTIAL)),
    ("combine", "not a pair", S(epi=LR.F32)),
    ("ln", "M = 17", S(M=17)), ("ln", "M = 0", S(M=0)), ("combine", "M = 17", S(M=17)), ("bf16", "M = 4097", S(M=4097)),
    ("ln", "K = 1312", S(K=1312)), ("ln", "K = 100", S(K=100)), ("bf16", "K = 5152", S(K=5152)), ("bf16", "K = 0", S(K=0)),
    ("combine", "multiple of 64", S(K=416)), ("qkv", "multiple of 64", S(K=224, N=672)), ("qkv", "N == 3 K", S(N=256)),
    ("ln", "N = 6", S(N=6)), ("ln", "N = 0", S(N=0)),
    ("bf16", "needs the PARTIAL", S(K=1536)),
    # the launcher's rule: a K slice that leaves a wave without a k-step
    ("bf16", "K = 160 leaves K slice 0 of 1 with 5 k-steps", S(K=160)), ("bf16", "K = 288 leaves K slice 0 of 1 with 9 k-steps", S(K=288)),
    ("ln", "K = 64 leaves K slice 0 of 1 with 2 k-steps", S(K=64)), ("combine", "K = 192 leaves", S(K=192)),
    # strides
    ("bf16", "ldo = 92", S(ldo=92)), ("bf16", "ldo = 98", S(ldo=98)), ("qkv", "ldo = 124", S(ldo=124)), ("gelu", "ldo = 508", S(ldo=508)),
    ("bf16", "lda = 760", S(lda=760)), ("bf16", "lda = 772", S(lda=772)),
    ("partial", "out_stride = 284", S(out_stride=284)), ("partial", "out_stride = 290", S(out_stride=290)),
    # the LayerNorm operands
    ("ln", "pend_n = 5", S(pend_n=5)), ("ln", "pend_n = -1", S(pend_n=-1)),
    ("ln", "pend_stride = 3836", S(pend_stride=3836)), ("ln", "pend_stride = 3842", S(pend_stride=3842)),
    ("ln", "aliasing x", lambda d: setattr(d, "x_out", d.x)),
    ("combine", "nsplit = 0", S(nsplit=0)), ("combine", "nsplit = 9", S(nsplit=9)),
    # the cache addressing
    ("qkv", "pos[3] = 8", I("pos", 3, 8)), ("qkv", "pos[0] = -1", I("pos", 0, -1)),
    ("qkv", "row_seq[9] = 3", I("row_seq", 9, 3)), ("qkv", "row_seq[0] = -1", I("row_seq", 0, -1)),
    ("qkv", "a second time", I("pos", 1, 0)),
    ("qkv", "row_seq is NULL with more rows", S(row_seq=None)), ("qkv", "pos is NULL", S(pos=None)),
    ("qkv", "cache_T = 0", S(cache_T=0)), ("qkv", "n_seq = 0", S(n_seq=0)),
    # NULL and alignment
    ("ln", "w_host is NULL", S(w_host=None)), ("ln", "x, pend, ln_g or ln_b is NULL", S(x=None)), ("ln", "x, pend, ln_g or ln_b is NULL", S(pend=None)),
    ("ln", "out null", S(out=None)), ("bf16", "act_rows null", S(act_rows=None)), ("combine", "part_o / part_ml null", S(part_ml=None)),
    ("qkv", "cache_k / cache_v null", S(cache_v=None)),
    ("ln", "bias not 16-byte aligned", P("bias")), ("ln", "not 16-byte aligned", P("x")), ("ln", "not 16-byte aligned", P("pend")),
    ("ln", "not 16-byte aligned", P("ln_g")), ("ln", "not 16-byte aligned", P("ln_b")), ("ln", "x_out not 16-byte aligned", P("x_out")),
    ("ln", "out null or not 16-byte aligned", P("out")), ("gelu", "out null or not 16-byte aligned", P("out", 8)),
    ("bf16", "act_rows null or not 16-byte aligned", P("act_rows", 8)),
    ("combine", "part_o / part_ml null or not 16-byte aligned", P("part_o")), ("combine", "part_o / part_ml null or not 16-byte aligned", P("part_ml", 8)),
    ("qkv", "cache_k / cache_v null or not 16-byte aligned", P("cache_k", 8)), ("qkv", "cache_k / cache_v null or not 16-byte aligned", P("cache_v", 8)),
    # the extents
    ("ln", "bias_elems", S(bias_elems=95)), ("ln", "x_elems", S(x_elems=5 * 768 - 1)), ("ln", "pend_elems", S(pend_elems=2 * (5 * 768 + 64) + 5 * 768 - 1)),
    ("gelu", "pend_elems", S(pend_elems=5 * 128 - 1)),
    ("ln", "x_out_elems", S(x_out_elems=5 * 768 - 1)), ("ln", "ln_elems", S(ln_elems=767)), ("ln", "ln_mean_out_elems", S(ln_mean_out_elems=4)),
    ("bf16", "act_elems", S(act_elems=4 * 776 + 767)), ("combine", "part_o_elems", E("part_o_elems")), ("combine", "part_ml_elems", E("part_ml_elems")),
    ("bf16", "out_elems", S(out_elems=4 * 104 + 95)), ("gelu", "out_elems", S(out_elems=4 * 520 + 511)),
    ("partial", "out_elems", S(out_elems=(3 * 96 + 64) + 3 * 96 - 1)), ("qkv", "out_elems", S(out_elems=10 * 128 - 1)),
    ("qkv", "cache_elems", E("cache_elems")),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=[f"{i:02d}-{k}-" + "".join(c if c.isalnum() else "_" for c in w) for i, (k, w, _) in enumerate(REFUSALS)])
def test_refusals(ccx_ctx, i):
    from clearconverse_amd import _lib
    kind, what, change = REFUSALS[i]
    d, out, keep = _valid(kind)
    change(d)
    with pytest.raises(_lib.CcxError) as e:
        _call(ccx_ctx, d)
    msg = str(e.value)
    assert "failed (1)" in msg and "ccx_dec_linear_op" in msg and what in msg, msg
    assert _untouched(out).all()


def test_ln_linear_refuses_a_starved_slice(ccx_ctx):
    """the same rule through ccx_dec_ln_linear, before its LayerNorm kernel is launched"""
    from clearconverse_amd import _lib
    outs = []
    with pytest.raises(_lib.CcxError) as e:
        _ln_linear_pair(ccx_ctx, 64, LR.N_SMALL, LR.F32, torch.zeros(17, 64), outs)
    assert "failed (1)" in str(e.value) and "ccx_dec_ln_linear" in str(e.value) and "K = 64 leaves a K slice of 2 k-steps" in str(e.value), str(e.value)
    assert _untouched(outs[0]).all()
