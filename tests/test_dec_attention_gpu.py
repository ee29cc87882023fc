"""GPU: the five attention forms of the decode step (csrc/decoder.hip), run away from the model through ccx_dec_attention_desc, against
the fp64 reference of tests/dec_reference.py from the operands the kernels see.  Padding keys hold NaN bit patterns and every output
is pre-filled with NaN, so a key read past the end or a block that never stored shows as a non-finite output.  The profile labels
say which instantiation ran.

Bounds (profiles/dec_kernels_measured_deviations.json): to be 2x the worst value measured on an MI355X over this
file; until a GPU session has measured them, the a-priori figures derived below.
  bf16 outputs   excess of |got - ref| over half a bf16 ulp of ref, over the head's max |v|
  f32 partials   |merged in fp64 - ref| / max |v|
  query forms    the same for the forms that compute their query: the reference rounds the LayerNorm output to bf16 from fp64
                 statistics, the kernel from fp32 ones, so an activation may land on the other side of a rounding boundary
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests.conftest import within

pytestmark = pytest.mark.gpu

# A-PRIORI figures (DESIGN.md section 3 marks them as placeholders, to become 2 x measured):
# a score t = sum of 64 fma * log2(e) / 8 carries |dt| <= 66 u S with S = sum |q_i k_i| log2(e) / 8 <= 200 in every case of this file
# (gain 16 and the -100 shift reach ~150), p = 2^t carries dt ln 2 + 2 u, numerator and denominator each, and the <= 1537 probabilities
# of a head are added in chains of <= T / 32 + 14 terms: 2 (66 u 200 ln 2 + 2 u) + 62 u = 1.1e-3 with u = 2^-24.
TOL_BF16_OUT = 1.1e-3
TOL_PARTIALS = 1.1e-3
# ... plus the query's own error: 768-term fp32 dot products and LayerNorm outputs that round to the other bf16 neighbour
TOL_QUERY_FORMS = 5e-3
N_BF16 = "dec attention: bf16 output, excess over half an ulp / max|v|"
N_PART = "dec attention: f32 partials merged in fp64, |err| / max|v|"
N_QUERY = "dec attention: fused / two-launch query forms, merged partials |err| / max|v|"

SELF, SPLIT, STREAM, PREFILL, FUSED_Q, TWO_LAUNCH_Q = range(6)
STREAM_LABEL = {4: "dec_cross_stream_kernel<true,4,false>", 6: "dec_cross_stream_kernel<true,6,false>",
                12: "dec_cross_stream_kernel<true,12,false>", None: "dec_attention_kernel<true> (cross)"}


def _nan(*shape):
    return torch.full(shape, math.nan, device="cuda")


def _operands(seed, rows, n_seq, H, kv_T, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(rows, H, 64, generator=g) * gain
    k = DR.bf16_round(torch.randn(n_seq, H, kv_T, 64, generator=g))
    v = DR.bf16_round(torch.randn(n_seq, H, kv_T, 64, generator=g))
    return q, k, v


def _pad_nan(k, v, seq_keys):
    """keys at and behind seq_keys[s] of sequence s: NaN"""
    for s, n in enumerate(seq_keys):
        k[s, :, n:], v[s, :, n:] = math.nan, math.nan


def _ints(vals):
    return None if vals is None else (C.c_int * len(vals))(*[int(x) for x in vals])


def _run(ctx, form, k, v, q=None, T=0, pos=None, row_seq=None, rows_per_seq=0, nsplit=1, combine=0, lds_pad=0, fq=None, rows=None,
         override=None, labels=False):
    """One call of ccx_dec_attention_desc.  k / v: CPU float tensors [n_seq, H, kv_T, 64] (or bf16 CUDA tensors, reused between calls);
    fq: dict(x, pend, pend_n, ln_g, ln_b, wq, bq) of CPU tensors for the query forms.  Returns a dict of CPU tensors."""
    from clearconverse_amd import _lib
    lib = _lib.load()
    kd = k if k.is_cuda else k.to(torch.bfloat16).cuda()
    vd = v if v.is_cuda else v.to(torch.bfloat16).cuda()
    n_seq, H, kv_T, _ = kd.shape
    rows = rows if rows is not None else (q.shape[0] if q is not None else fq["x"].shape[0])
    d = _lib.DecAttnDesc()
    keep = [kd, vd]
    d.k, d.v, d.kv_elems = kd.data_ptr(), vd.data_ptr(), kd.numel()
    d.rows, d.n_seq, d.H, d.kv_T, d.T = rows, n_seq, H, kv_T, T
    if q is not None:
        qd = q.contiguous().cuda()
        keep.append(qd)
        d.q, d.q_elems = qd.data_ptr(), qd.numel()
    pos_c, rs_c = _ints(pos), _ints(row_seq)
    if pos_c is not None:
        d.pos = pos_c
    if rs_c is not None:
        d.row_seq = rs_c
    d.rows_per_seq, d.nsplit, d.combine, d.lds_pad = rows_per_seq, nsplit, combine, lds_pad
    out = _nan(rows, H, 64)
    d.out, d.out_elems = out.data_ptr(), out.numel()
    part_o, part_ml = _nan(rows, H, nsplit, 64), _nan(rows, H, nsplit, 2)
    d.part_o, d.part_o_elems, d.part_ml, d.part_ml_elems = part_o.data_ptr(), part_o.numel(), part_ml.data_ptr(), part_ml.numel()
    q_x_out = None
    if fq is not None:
        dev = {n: fq[n].contiguous().cuda() for n in ("x", "pend", "ln_g", "ln_b", "bq")}
        keep.append(dev)
        wq = np.ascontiguousarray(fq["wq"].numpy(), dtype=np.float32)
        keep.append(wq)
        q_x_out = _nan(rows, 768)
        d.x, d.x_elems, d.pend, d.pend_elems = dev["x"].data_ptr(), dev["x"].numel(), dev["pend"].data_ptr(), dev["pend"].numel()
        d.pend_n, d.pend_stride = fq["pend_n"], fq["pend"].shape[1] * 768
        d.ln_g, d.ln_b, d.eps, d.wq_host, d.bq = dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), 1e-5, wq.ctypes.data, dev["bq"].data_ptr()
        d.q_x_out, d.q_x_out_elems = q_x_out.data_ptr(), q_x_out.numel()
    for name, val in (override or {}).items():
        if callable(val):
            val = val(getattr(d, name))
        setattr(d, name, val)
    if labels:
        ctx.prof_enable(True)
    try:
        rc = lib.ccx_dec_attention_desc(ctx.handle, form, C.byref(d), torch.cuda.current_stream().cuda_stream)
        names = [r[0] for r in ctx.prof_records()] if labels else []
    finally:
        if labels:
            ctx.prof_enable(False)
    torch.cuda.synchronize()
    res = {"out": out.cpu(), "part_o": part_o.cpu(), "part_ml": part_ml.cpu(), "labels": names,
           "q_x_out": None if q_x_out is None else q_x_out.cpu()}
    ctx.check(rc, "ccx_dec_attention_desc")
    return res


def _check_out(res, ref, vmax, what):
    assert torch.isfinite(res["out"]).all(), what
    within(N_BF16, DR.bf16_out_excess(res["out"], ref, vmax), TOL_BF16_OUT, what)


def _check_partials(res, ref, vmax, parts, what, name=N_PART, tol=None):
    tol = TOL_PARTIALS if tol is None else tol
    po, pml = res["part_o"], res["part_ml"]
    assert torch.isfinite(po).all() and torch.isfinite(pml).all(), what
    within(name, DR.f32_rel_err(DR.merge_partials(po, pml), ref, vmax), tol, what)
    # per split: the normalised partial o / l, and the maximum the split saw; empty splits carry l = 0 and o = 0
    pm, pl, pov = parts
    live = pl > 0
    assert torch.equal(pml[..., 1] > 0, live), what
    assert bool((po[~live] == 0).all()), what
    got = po.double()[live] / pml[..., 1].double()[live][:, None]
    want = pov[live] / pl[live][:, None]
    vm = vmax[:, :, None].expand_as(pl)[live]
    within(name, float(((got - want).abs() / vm[:, None]).max()), tol, what)
    # the kernels leave the split's true maximum as the partial's reference (fp32 score arithmetic: a few ulp of |m|)
    assert float((pml[..., 0].double()[live] - pm[live]).abs().max()) < 1e-3 * max(1.0, float(pm[live].abs().max())), what


# ---------------------------------------------------------------------------------------------------------------------------------
# self attention: dec_attention_kernel<true>, keys [0, pos]
# ---------------------------------------------------------------------------------------------------------------------------------
POS_SET = (0, 7, 8, 63, 64, 255, 256, 257, 447)


@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("rows", [5, 17])
def test_self_mixed_positions(ccx_ctx, H, rows):
    kv_T = 448
    pos = [POS_SET[(2 * r + rows) % len(POS_SET)] for r in range(rows)]
    if rows == 17:
        assert set(pos) == set(POS_SET)
    q, k, v = _operands(10 + H + rows, rows, rows, H, kv_T, gain=2.0)
    _pad_nan(k, v, [p + 1 for p in pos])
    kd, vd = k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda()
    res = _run(ccx_ctx, SELF, kd, vd, q=q, pos=pos, labels=True)
    assert res["labels"] == ["dec_attention_kernel<true> (self)"]
    ref, vmax = DR.attention_ref(q, k, v, [p + 1 for p in pos])
    _check_out(res, ref, vmax, ("self", H, rows))
    # a row's bits do not depend on the other rows of the launch
    for r in sorted({0, rows // 2, rows - 1}):
        alone = _run(ccx_ctx, SELF, kd, vd, q=q[r:r + 1], pos=[pos[r]], row_seq=[r])
        assert torch.equal(alone["out"][0], res["out"][r]), r


@pytest.mark.parametrize("H", [2, 12])
def test_self_rows_of_a_sequence_at_positions_0_to_8(ccx_ctx, H):
    """the prompt prefill's self attention: 3 sequences x 9 rows through row_seq; row t sees keys 0 .. t of its sequence's cache, whose
    later rows hold the other rows' (finite) keys"""
    kv_T, P = 448, 9
    row_seq = [s for s in range(3) for _ in range(P)]
    pos = [t for _ in range(3) for t in range(P)]
    q, k, v = _operands(20 + H, 3 * P, 3, H, kv_T, gain=2.0)
    _pad_nan(k, v, [P] * 3)
    res = _run(ccx_ctx, SELF, k, v, q=q, pos=pos, row_seq=row_seq)
    ref, vmax = DR.attention_ref(q, k, v, [p + 1 for p in pos], row_seq=row_seq)
    _check_out(res, ref, vmax, ("self row_seq", H))


# ---------------------------------------------------------------------------------------------------------------------------------
# split-KV partials: dec_attention_kernel<false>, and dec_combine_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("T", [1, 5, 16, 37, 257, 1499, 1500])
def test_split_partials_and_combine(ccx_ctx, H, T):
    rows, kv_T = 3, (T + 127) // 128 * 128
    q, k, v = _operands(30 + H + T, rows, rows, H, kv_T, gain=2.0)
    _pad_nan(k, v, [T] * rows)
    kd, vd = k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda()
    seen = set()
    for nsplit in (1, 2, 6, 7, 8):
        ref, vmax, parts = DR.attention_ref(q, k, v, [T] * rows, nsplit=nsplit)
        res = _run(ccx_ctx, SPLIT, kd, vd, q=q, T=T, nsplit=nsplit, combine=1, labels=True)
        seen.update(res["labels"])
        assert res["labels"] == ["dec_attention_kernel<false> (cross)", "dec_combine_kernel"]
        _check_partials(res, ref, vmax, parts, ("split", H, T, nsplit))
        _check_out(res, ref, vmax, ("split + combine", H, T, nsplit))
        if T == 5 and nsplit == 8:
            assert bool((parts[1][:, :, 5:] == 0).all()) and bool((res["part_ml"][:, :, 5:, 1] == 0).all())      # empty splits
        padded = _run(ccx_ctx, SPLIT, kd, vd, q=q, T=T, nsplit=nsplit, lds_pad=98304)
        assert torch.equal(padded["part_o"], res["part_o"]) and torch.equal(padded["part_ml"], res["part_ml"]), nsplit
        assert torch.isnan(padded["out"]).all()                   # no combine asked for: out is not touched


# ---------------------------------------------------------------------------------------------------------------------------------
# lean streaming: dec_cross_stream_kernel<true, NP>, fallback behind 1536 keys
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("T", [16, 37, 500, 512, 513, 768, 769, 1499, 1500, 1536, 1537])
def test_stream_every_instantiation(ccx_ctx, H, T):
    rows, kv_T = 3, (T + 127) // 128 * 128
    q, k, v = _operands(40 + H + T, rows, rows, H, kv_T, gain=2.0)
    _pad_nan(k, v, [T] * rows)
    kd, vd = k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda()
    ref, vmax = DR.attention_ref(q, k, v, [T] * rows)
    res = _run(ccx_ctx, STREAM, kd, vd, q=q, T=T, labels=True)
    assert res["labels"] == [STREAM_LABEL[DR.np_pieces(T)]], (T, res["labels"])
    _check_out(res, ref, vmax, ("stream", H, T))
    padded = _run(ccx_ctx, STREAM, kd, vd, q=q, T=T, lds_pad=98304)
    assert torch.equal(padded["out"], res["out"])


# ---------------------------------------------------------------------------------------------------------------------------------
# prompt prefill: dec_cross_stream_kernel<.., true> (2 rows per sequence), dec_cross_prefill_kernel<NP, 4> (3 and more)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("T", [37, 600, 1500])
def test_prefill_rows_share_their_sequence(ccx_ctx, H, T):
    n_seq, kv_T = 3, (T + 127) // 128 * 128
    npc = DR.np_pieces(T)
    _, k, v = _operands(50 + H + T, 1, n_seq, H, kv_T)
    _pad_nan(k, v, [T] * n_seq)
    kd, vd = k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda()
    for P in (2, 3, 4, 5, 9, 16):
        rows = n_seq * P
        q = torch.randn(rows, H, 64, generator=torch.Generator().manual_seed(P)) * 2.0
        row_seq = [r // P for r in range(rows)]
        res = _run(ccx_ctx, PREFILL, kd, vd, q=q, T=T, row_seq=row_seq, rows_per_seq=P, labels=True)
        want = f"dec_cross_stream_kernel<true,{npc},true>" if P == 2 else f"dec_cross_prefill_kernel<{npc},4>"
        assert res["labels"] == [want], (P, res["labels"])
        ref, vmax = DR.attention_ref(q, k, v, [T] * rows, row_seq=row_seq)
        _check_out(res, ref, vmax, ("prefill", H, T, P))


# ---------------------------------------------------------------------------------------------------------------------------------
# the query inside the attention blocks: dec_cross_fused_q_kernel<EARLY_V> against dec_linear + dec_attention_kernel<false>
# ---------------------------------------------------------------------------------------------------------------------------------
def _query_operands(seed, rows, max_pend=4):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(rows, 768, generator=g) * 1.5 + 0.3, "pend": torch.randn(max_pend, rows, 768, generator=g) * 0.5,
            "ln_g": 1.0 + 0.1 * torch.randn(768, generator=g), "ln_b": 0.1 * torch.randn(768, generator=g),
            "wq": torch.randn(768, 768, generator=g) * (2.0 / math.sqrt(768)), "bq": 0.1 * torch.randn(768, generator=g), "pend_n": 0}


@pytest.fixture(scope="module")
def cross_kv():
    """K / V of 16 sequences x 12 heads for the query forms, per key count: (k, v on the CPU with NaN padding, their bf16 device copies)"""
    cache = {}

    def get(T):
        if T not in cache:
            _, k, v = _operands(60 + T, 1, 16, 12, (T + 127) // 128 * 128)
            _pad_nan(k, v, [T] * 16)
            cache[T] = (k, v, k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda())
        return cache[T]
    return get


@pytest.mark.parametrize("B", [1, 7, 8, 16])
@pytest.mark.parametrize("T", [37, 1500])
def test_fused_query_equals_two_launches_and_the_reference(ccx_ctx, cross_kv, B, T):
    k, v, kd, vd = cross_kv(T)
    kd, vd = kd[:B].contiguous(), vd[:B].contiguous()
    fq = _query_operands(70 + B + T, B)
    for pend_n in (0, 1, 4):
        fq["pend_n"] = pend_n
        qref, xres = DR.fused_q_ref(fq["x"], fq["pend"], pend_n, fq["ln_g"], fq["ln_b"], 1e-5, fq["wq"], fq["bq"])
        qref = qref.reshape(B, 12, 64)
        for nsplit in (6, 8):
            fused = _run(ccx_ctx, FUSED_Q, kd, vd, fq=fq, T=T, nsplit=nsplit, labels=True)
            two = _run(ccx_ctx, TWO_LAUNCH_Q, kd, vd, fq=fq, T=T, nsplit=nsplit, labels=True)
            assert fused["labels"] == ["dec_cross_fused_q_kernel"]
            assert two["labels"] == ["dec_linear_kernel<1, 1, 6, 0, 3>", "dec_attention_kernel<false> (cross)"]
            # which instantiation ran is inferred from the launcher's grid rule (<= 512 blocks: EARLY_V); the label does not tell them apart
            what = ("query forms", B, T, pend_n, nsplit, "EARLY_V" if B * 12 * nsplit <= 512 else "late V")
            for name in ("part_o", "part_ml", "q_x_out"):
                assert torch.equal(fused[name], two[name]), (name, what)
            # the resolved rows: x + the slabs, added in fp32 one after the other
            assert torch.equal(two["q_x_out"], xres), what
            ref, vmax, parts = DR.attention_ref(qref, k[:B], v[:B], [T] * B, nsplit=nsplit)
            assert torch.isfinite(two["part_o"]).all() and torch.isfinite(two["part_ml"]).all()
            within(N_QUERY, DR.f32_rel_err(DR.merge_partials(two["part_o"], two["part_ml"]), ref, vmax), TOL_QUERY_FORMS, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# score patterns: scores that dominate, at the keys where the rescale and the merges can go wrong
# ---------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("gain 1", "gain 4", "gain 16", "first", "last", "last_wave", "last_piece", "shifted")


def _patterned(pattern, q, k, v, T, row_of_seq, streaming, nsplit=1):
    """q [rows, H, 64] (the queries the kernel will use), k / v [n_seq, H, kv_T, 64]; row_of_seq[s]: the row whose query the pattern of
    sequence s is aligned with.  Returns (q, k) with the pattern applied (k bf16-rounded again)."""
    q, k = q.clone(), k.clone()
    if pattern.startswith("gain"):
        return q * float(pattern.split()[1]), k
    for s, r in enumerate(row_of_seq):
        qq = q[r]                                                     # [H, 64]
        unit = qq / (qq * qq).sum(dim=-1, keepdim=True) * 8.0         # q . unit / 8 == 1
        if pattern == "shifted":
            k[s, :, :T] = DR.bf16_round(k[s, :, :T] - 100.0 * unit[:, None, :])      # every score of the row moves by about -100
        else:
            key = DR.pattern_keys(T, streaming, nsplit)[pattern]
            k[s, :, key] = DR.bf16_round(40.0 * unit)                 # one key about 40 above the rest: a near one-hot softmax
    return q, k


@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_patterns_self(ccx_ctx, pattern):
    H, kv_T, pos = 2, 448, [447, 257, 63]
    q, k, v = _operands(80, 3, 3, H, kv_T)
    for r, p in enumerate(pos):
        qr, kr = _patterned(pattern, q[r:r + 1], k[r:r + 1], v, p + 1, [0], False)
        q[r], k[r] = qr[0], kr[0]
    _pad_nan(k, v, [p + 1 for p in pos])
    res = _run(ccx_ctx, SELF, k, v, q=q, pos=pos)
    ref, vmax = DR.attention_ref(q, k, v, [p + 1 for p in pos])
    _check_out(res, ref, vmax, ("self", pattern))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_patterns_split(ccx_ctx, pattern):
    H, T, kv_T = 2, 1500, 1536
    q, k, v = _operands(81, 3, 3, H, kv_T)
    for nsplit in (1, 6):
        qp, kp = _patterned(pattern, q, k, v, T, [0, 1, 2], False, nsplit)
        _pad_nan(kp, v, [T] * 3)
        res = _run(ccx_ctx, SPLIT, kp, v, q=qp, T=T, nsplit=nsplit, combine=1)
        ref, vmax, parts = DR.attention_ref(qp, kp, v, [T] * 3, nsplit=nsplit)
        _check_partials(res, ref, vmax, parts, ("split", pattern, nsplit))
        _check_out(res, ref, vmax, ("split + combine", pattern, nsplit))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_patterns_stream(ccx_ctx, pattern):
    H = 2
    for T in (500, 700, 1500):                                        # NP = 4, 6, 12
        kv_T = (T + 127) // 128 * 128
        q, k, v = _operands(82 + T, 3, 3, H, kv_T)
        qp, kp = _patterned(pattern, q, k, v, T, [0, 1, 2], True)
        _pad_nan(kp, v, [T] * 3)
        res = _run(ccx_ctx, STREAM, kp, v, q=qp, T=T)
        ref, vmax = DR.attention_ref(qp, kp, v, [T] * 3)
        _check_out(res, ref, vmax, ("stream", pattern, T))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_patterns_prefill(ccx_ctx, pattern):
    H, T, kv_T, n_seq = 2, 600, 640, 3
    for P in (2, 5):
        rows = n_seq * P
        q, k, v = _operands(83 + P, rows, n_seq, H, kv_T)
        row_seq = [r // P for r in range(rows)]
        qp, kp = _patterned(pattern, q, k, v, T, [s * P + (s % P) for s in range(n_seq)], True)
        _pad_nan(kp, v, [T] * n_seq)
        res = _run(ccx_ctx, PREFILL, kp, v, q=qp, T=T, row_seq=row_seq, rows_per_seq=P)
        ref, vmax = DR.attention_ref(qp, kp, v, [T] * rows, row_seq=row_seq)
        _check_out(res, ref, vmax, ("prefill", pattern, P))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_patterns_query_forms(ccx_ctx, pattern):
    B, T, kv_T, nsplit = 2, 1500, 1536, 6
    _, k, v = _operands(84, 1, B, 12, kv_T)
    fq = _query_operands(85, B)
    fq["pend_n"] = 1
    if pattern.startswith("gain"):
        fq["wq"] = fq["wq"] * float(pattern.split()[1]) / 2.0
        fq["bq"] = fq["bq"] * float(pattern.split()[1]) / 2.0
    qref = DR.fused_q_ref(fq["x"], fq["pend"], 1, fq["ln_g"], fq["ln_b"], 1e-5, fq["wq"], fq["bq"])[0].reshape(B, 12, 64)
    if not pattern.startswith("gain"):
        _, k = _patterned(pattern, qref.float(), k, v, T, [0, 1], False, nsplit)
    _pad_nan(k, v, [T] * B)
    fused = _run(ccx_ctx, FUSED_Q, k, v, fq=fq, T=T, nsplit=nsplit)
    two = _run(ccx_ctx, TWO_LAUNCH_Q, k, v, fq=fq, T=T, nsplit=nsplit)
    for name in ("part_o", "part_ml", "q_x_out"):
        assert torch.equal(fused[name], two[name]), (name, pattern)
    ref, vmax, parts = DR.attention_ref(qref, k, v, [T] * B, nsplit=nsplit)
    assert torch.isfinite(two["part_o"]).all() and torch.isfinite(two["part_ml"]).all()
    within(N_QUERY, DR.f32_rel_err(DR.merge_partials(two["part_o"], two["part_ml"]), ref, vmax), TOL_QUERY_FORMS, ("query forms", pattern))


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections: one per host check; nothing is launched
# ---------------------------------------------------------------------------------------------------------------------------------
def _base(form, kv_T=32):
    """a small valid call of each form, as the keyword arguments of _run"""
    H = 12 if form in (FUSED_Q, TWO_LAUNCH_Q) else 2
    n_seq = 17 if form in (FUSED_Q, TWO_LAUNCH_Q) else 4
    q, k, v = _operands(90 + form, 4, n_seq, H, kv_T)
    kw = {"k": k, "v": v, "q": q, "T": 16}
    if form == SELF:
        kw.update(T=0, pos=[0, 5, 31, 16])
    if form == SPLIT:
        kw.update(nsplit=2, combine=1)
    if form == PREFILL:
        kw.update(row_seq=[0, 0, 1, 1], rows_per_seq=2)
    if form in (FUSED_Q, TWO_LAUNCH_Q):
        kw.update(q=None, fq=_query_operands(91, 17), rows=2, nsplit=2)
        kw["fq"]["pend_n"] = 1
    return kw


def _bump(p):
    return p + 4


REJECTIONS = [
    ("unknown form", 6, SELF, {}, "unknown form"),
    ("pos at kv_T", SELF, SELF, {"pos": [0, 5, 32, 16]}, "pos[2]"),
    ("negative pos", SELF, SELF, {"pos": [0, -1, 3, 16]}, "pos[1]"),
    ("pos missing", SELF, SELF, {"pos": None}, "pos is NULL"),
    ("pos given to a cross form", SPLIT, SPLIT, {"pos": [0, 1, 2, 3]}, "pos is taken"),
    ("T behind kv_T", STREAM, STREAM, {"T": 33}, "T = 33"),
    ("T zero", SPLIT, SPLIT, {"T": 0}, "T = 0"),
    ("prefill: more than 1536 keys", PREFILL, PREFILL, {"kv_T": 1664, "T": 1537}, "at most 1536 keys"),
    ("row_seq out of range", SELF, SELF, {"row_seq": [0, 1, 4, 2]}, "row_seq[2]"),
    ("more rows than sequences without a map", SELF, SELF, {"override": {"n_seq": 3}}, "row_seq is NULL"),
    ("streaming: more rows than sequences", STREAM, STREAM, {"override": {"n_seq": 3}}, "more rows (4) than sequences (3)"),
    ("row_seq given to the streaming form", STREAM, STREAM, {"row_seq": [0, 1, 2, 3]}, "row_seq is not taken"),
    ("prefill: rows no multiple of rows_per_seq", PREFILL, PREFILL, {"rows_per_seq": 3}, "multiple"),
    ("prefill: one row per sequence", PREFILL, PREFILL, {"rows_per_seq": 1}, "rows_per_seq = 1"),
    ("prefill: a row outside its group's sequence", PREFILL, PREFILL, {"row_seq": [0, 1, 1, 1]}, "group's sequence"),
    ("prefill: groups not on their own sequences", PREFILL, PREFILL, {"row_seq": [1, 1, 0, 0]}, "group g on sequence g"),
    ("prefill: no map", PREFILL, PREFILL, {"row_seq": None}, "needs row_seq"),
    ("rows_per_seq given to another form", STREAM, STREAM, {"rows_per_seq": 2}, "prefill form only"),
    ("q_elems short", STREAM, STREAM, {"override": {"q_elems": 4 * 2 * 64 - 1}}, "q is read"),
    ("kv_elems short", SELF, SELF, {"override": {"kv_elems": 4 * 2 * 32 * 64 - 1}}, "k / v are read"),
    ("out_elems short", PREFILL, PREFILL, {"override": {"out_elems": 4 * 2 * 64 - 1}}, "out is written"),
    ("part_o_elems short", SPLIT, SPLIT, {"override": {"part_o_elems": 4 * 2 * 2 * 64 - 1}}, "part_o is written"),
    ("part_ml_elems short", SPLIT, SPLIT, {"override": {"part_ml_elems": 4 * 2 * 2 * 2 - 1}}, "part_ml is written"),
    ("q misaligned", SELF, SELF, {"override": {"q": _bump}}, "q null or not 16-byte"),
    ("k misaligned", STREAM, STREAM, {"override": {"k": _bump}}, "k / v null or not 16-byte"),
    ("v null", STREAM, STREAM, {"override": {"v": None}}, "k / v null"),
    ("part_ml misaligned", SPLIT, SPLIT, {"override": {"part_ml": _bump}}, "part_o / part_ml"),
    ("out null", STREAM, STREAM, {"override": {"out": None}}, "out is NULL"),
    ("nsplit 9", SPLIT, SPLIT, {"nsplit": 9}, "nsplit = 9"),
    ("nsplit 0", SPLIT, SPLIT, {"override": {"nsplit": 0}}, "nsplit = 0"),
    ("negative lds_pad", SPLIT, SPLIT, {"lds_pad": -16}, "lds_pad"),
    ("lds_pad given to the self form", SELF, SELF, {"lds_pad": 1024}, "lds_pad"),
    ("H zero", SELF, SELF, {"override": {"H": 0}}, "H=0"),
    ("fused query: 17 rows", FUSED_Q, FUSED_Q, {"rows": 17}, "rows <= 16"),
    ("fused query: pend_n 5", FUSED_Q, FUSED_Q, {"override": {"pend_n": 5}}, "pend_n = 5"),
    ("fused query: x_elems short", FUSED_Q, FUSED_Q, {"override": {"x_elems": 2 * 768 - 1}}, "x is read"),
    ("fused query: pend_elems short", TWO_LAUNCH_Q, TWO_LAUNCH_Q, {"override": {"pend_elems": 2 * 768 - 1}}, "pend is read"),
    ("fused query: pend_stride below a slab", FUSED_Q, FUSED_Q, {"override": {"pend_stride": 768}}, "pend_stride"),
    ("fused query: pend_stride no multiple of 4", FUSED_Q, FUSED_Q, {"override": {"pend_stride": 17 * 768 + 2}}, "pend_stride = 13058"),
    ("fused query: q_x_out aliases x", FUSED_Q, FUSED_Q, {"override": {"q_x_out": "x"}}, "aliasing x"),
    ("fused query: q_x_out_elems short", TWO_LAUNCH_Q, TWO_LAUNCH_Q, {"override": {"q_x_out_elems": 100}}, "q_x_out is written"),
    ("fused query: x misaligned", FUSED_Q, FUSED_Q, {"override": {"x": _bump}}, "not 16-byte aligned"),
    ("fused query: no weights", TWO_LAUNCH_Q, TWO_LAUNCH_Q, {"override": {"wq_host": None}}, "is NULL"),
    ("fused query: row_seq", FUSED_Q, FUSED_Q, {"row_seq": [0, 1]}, "row_seq is not taken"),
]


@pytest.mark.parametrize("name,form,base,change,fragment", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(ccx_ctx, name, form, base, change, fragment):
    from clearconverse_amd import _lib
    kw = _base(base, change.get("kv_T", 32))
    override = dict(change.get("override", {}))
    kw.update({k_: v_ for k_, v_ in change.items() if k_ not in ("override", "kv_T")})
    if override.get("q_x_out") == "x":
        # point q_x_out at x itself: the callables see the descriptor's fields in this order
        holder = {}
        override = {"x": lambda p: holder.setdefault("x", p), "q_x_out": lambda p: holder["x"]}
    with pytest.raises(_lib.CcxError) as e:
        _run(ccx_ctx, form, override=override, **kw)
    assert fragment in str(e.value), str(e.value)
    assert "(1)" in str(e.value)                      # CCX_ERR_ARG


def test_a_rejected_call_launches_nothing(ccx_ctx):
    from clearconverse_amd import _lib
    kw = _base(SPLIT)
    kw["T"] = 33
    ccx_ctx.prof_enable(True)
    try:
        with pytest.raises(_lib.CcxError):
            _run(ccx_ctx, SPLIT, **kw)
        assert ccx_ctx.prof_records() == []
    finally:
        ccx_ctx.prof_enable(False)
