"""GPU: the SepFormer layer kernels (csrc/sepformer.hip) one at a time through ccx_sep_op -- the production launchers of
csrc/sepformer.h, away from the model -- against the fp64 references of tests/sep_reference.py from the operands the kernels see.

Every buffer is larger than the rows in use; rows outside every sequence (and qkv / feats / fc rows past a length) hold NaN and every
output is pre-filled with NaN, so a read past a sequence or a row that was never stored shows as a non-finite value, and a store
outside a sequence as changed bits.  The profile labels say which kernel ran (the final norm and the decoder have no profile scope in
the product, so they have no label to check).

Comparators and bounds (tests/sep_reference.py, proven on the CPU in tests/test_sep_reference_cpu.py):
  fused attention, FFN   rel-L2 of the update, || got - ref || / || ref - h_in ||, per sequence / 32-token group (one bound per input
                         regime) and per row (one looser bound), against the bf16-mirrored reference
  split attention        excess of |got - ref| over half a bf16 ulp, over the head's max |v| (the inputs are bf16 already)
  final norm, decoder    fp32 only: a derived per-element allowance, |got - ref| / allowance < 1
The rel-L2 and excess bounds are 2 x the worst value measured on an MI355X (profiles/sep_kernels_measured_deviations.json); the CPU
suite rejects every mutation at them.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import sep_reference as SR
from tests.conftest import within

pytestmark = pytest.mark.gpu

ATTN_BLOCK, ATTENTION, FFN, FINAL_NORM, DECODER = range(5)
N_SEQ = "sep kernels: fused attention / FFN, update rel-L2 per sequence or 32-token group, regime "
N_ROW = "sep kernels: fused attention / FFN, update rel-L2 per row"
N_SPLIT = "sep kernels: split attention, excess over half a bf16 ulp / max|v|"
N_NORM = "sep kernels: final norm, |err| / derived allowance"
N_DEC = "sep kernels: decoder, |err| / derived allowance"

BUFFERS = ("h", "xin", "y", "qkv", "att", "feats", "fc", "out")
PARAM_COUNT = {"ln_g": "ln_elems", "ln_b": "ln_elems", "gln_g": "gln_elems", "gln_b": "gln_elems", "wqkv": "wqkv_elems",
               "bqkv": "bqkv_elems", "wo": "wo_elems", "bo": "bo_elems", "w1": "w1_elems", "b1": "b1_elems", "w2": "w2_elems",
               "b2": "b2_elems", "wdec": "wdec_elems"}
BF16_PARAMS = ("wqkv", "wo", "w1", "w2")


def _ints(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def _dev_params(P):
    return {k: (v.to(torch.bfloat16) if k in BF16_PARAMS else v.float()).contiguous().cuda() for k, v in P.items() if k in PARAM_COUNT}


def _call(ctx, op, tensors, rows, seqs=None, utts=None, n_tok=0, d_ffn=0, segment=150, out_stride=0, override=None, labels=True):
    """One ccx_sep_op.  tensors: name -> CUDA tensor for the buffers and parameters of the op.  Returns (rc, profile labels)."""
    from clearconverse_amd import _lib
    lib = _lib.load()
    d = _lib.SepDesc()
    for name, t in tensors.items():
        setattr(d, name, t.data_ptr())
        if name in BUFFERS:
            setattr(d, name + "_elems", t.numel())
        else:
            setattr(d, PARAM_COUNT[name], t.numel())
    d.rows, d.n_tok, d.d_ffn, d.segment, d.out_stride = rows, n_tok, d_ffn, segment, out_stride
    keep = []
    if seqs is not None:
        keep = [_ints([s for s, _ in seqs]), _ints([n for _, n in seqs])]
        d.seq_start, d.seq_len, d.n_seq = keep[0], keep[1], len(seqs)
    if utts is not None:
        keep = [_ints([u[i] for u in utts]) for i in range(3)]
        d.utt_tok0, d.utt_L, d.utt_T, d.n_utt = keep[0], keep[1], keep[2], len(utts)
    for name, val in (override or {}).items():
        setattr(d, name, val(getattr(d, name)) if callable(val) else val)
    if labels:
        ctx.prof_enable(True)
    try:
        rc = lib.ccx_sep_op(ctx.handle, op, C.byref(d), torch.cuda.current_stream().cuda_stream)
        names = [r[0] for r in ctx.prof_records()] if labels else []
    finally:
        if labels:
            ctx.prof_enable(False)
    torch.cuda.synchronize()
    return rc, names


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _nan_outside(t, mask):
    t = t.clone()
    t[~mask] = math.nan
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# fused attention block
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused(regime):
    h, seqs, rows, P, planted = SR.fused_case(regime, 0)
    return h, seqs, rows, P, SR.attn_block_op(h, seqs, P)


def _run_fused(ctx, h, seqs, rows, P, labels=True):
    mask = SR.in_sequence_mask(seqs, rows)
    h_in = _nan_outside(h, mask).cuda()
    h_dev = h_in.clone()
    T = dict(_dev_params({k: P[k] for k in ("ln_g", "ln_b", "wqkv", "bqkv", "wo", "bo")}), h=h_dev)
    rc, names = _call(ctx, ATTN_BLOCK, T, rows, seqs=seqs, labels=labels)
    ctx.check(rc, "ccx_sep_op")
    assert torch.equal(_bits(h_dev)[~mask.cuda()], _bits(h_in)[~mask.cuda()]), "a row outside every sequence changed"
    got = h_dev.cpu()
    assert torch.isfinite(got[mask]).all()
    return got, names


def _check_update(got, ref, h_in, regime, what):
    within(N_SEQ + regime, SR.update_rel_l2(got, ref, h_in), SR.BOUND_SEQ[regime], what)
    within(N_ROW, SR.update_rel_rows(got, ref, h_in), SR.BOUND_ROW, what)


@pytest.mark.parametrize("regime", SR.ALL_REGIMES)
def test_fused_attention_block(ccx_ctx, regime):
    """one launch over sequences of 1, 2, 15, 16, 17, 31, 33, 97, 150, 150, 159 and 160 tokens"""
    h, seqs, rows, P, ref = _fused(regime)
    got, names = _run_fused(ccx_ctx, h, seqs, rows, P)
    assert names == ["sep_attn_block_kernel"]
    for (s0, n), r in zip(seqs, ref):
        _check_update(got[s0:s0 + n], r, h[s0:s0 + n], regime, ("fused", regime, n))


def test_fused_attention_rows_do_not_depend_on_the_table_order(ccx_ctx):
    h, seqs, rows, P, _ = _fused("unit")
    a, _ = _run_fused(ccx_ctx, h, seqs, rows, P, labels=False)
    perm = [seqs[i] for i in (7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4, 6)]
    b, _ = _run_fused(ccx_ctx, h, perm, rows, P, labels=False)
    assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# split attention
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dominant", [None, "first", "last"])
def test_split_attention(ccx_ctx, dominant):
    """lengths 1 .. 335: the register-resident path (<= 160), the streaming path with one, two full and three key blocks; a dominant key
    in the first key block (alpha = 1 afterwards) and in the last (alpha << 1 when it arrives).  Both head groups run."""
    qkv, seqs, rows, planted = SR.split_case(0, dominant)
    mask = SR.in_sequence_mask(seqs, rows)
    qkv_dev = _nan_outside(qkv, mask).to(torch.bfloat16).cuda()
    att = torch.full((rows, SR.D), math.nan, dtype=torch.bfloat16, device="cuda")
    rc, names = _call(ccx_ctx, ATTENTION, {"qkv": qkv_dev, "att": att}, rows, seqs=seqs)
    ccx_ctx.check(rc, "ccx_sep_op")
    assert names == ["sep_attention_kernel"]
    got = att.float().cpu()
    assert torch.isnan(got[~mask]).all(), "a row outside every sequence was written"
    assert torch.isfinite(got[mask]).all()
    ref = SR.attention_op(qkv, seqs, round_out=False)
    for (s0, n), r in zip(seqs, ref):
        within(N_SPLIT, SR.bf16_out_excess(got[s0:s0 + n], r, SR.head_vmax(qkv, s0, n)), SR.BOUND_SPLIT, ("split", dominant, n))


# ---------------------------------------------------------------------------------------------------------------------------------
# FFN
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_ffn(ctx, h, n_tok, rows, P, d_ffn, labels=True, shift=0):
    """shift: rows the token buffer sits below the start of its allocation"""
    mask = torch.arange(rows) < n_tok
    h_in = torch.cat([torch.full((shift, SR.D), math.nan), _nan_outside(h, mask)]).cuda()
    h_dev = h_in.clone()
    T = dict(_dev_params({k: P[k] for k in ("ln_g", "ln_b", "w1", "b1", "w2", "b2")}), h=h_dev[shift:])
    rc, names = _call(ctx, FFN, T, rows, n_tok=n_tok, d_ffn=d_ffn, labels=labels)
    ctx.check(rc, "ccx_sep_op")
    keep = torch.cat([torch.ones(shift, dtype=torch.bool), ~mask]).cuda()
    assert torch.equal(_bits(h_dev)[keep], _bits(h_in)[keep]), "a row past n_tok changed"
    got = h_dev[shift:shift + n_tok].cpu()
    assert torch.isfinite(got).all()
    return got, names


def _check_ffn(got, ref, h, n_tok, regime, what):
    for a, b in SR.ffn_groups(n_tok):
        within(N_SEQ + regime, SR.update_rel_l2(got[a:b], ref[a:b], h[a:b]), SR.BOUND_SEQ[regime], what + (a,))
    within(N_ROW, SR.update_rel_rows(got, ref, h[:n_tok]), SR.BOUND_ROW, what)


@pytest.mark.parametrize("d_ffn", SR.FFN_WIDTHS)
@pytest.mark.parametrize("n_tok", SR.FFN_TOKENS)
def test_ffn_widths_and_token_counts(ccx_ctx, n_tok, d_ffn):
    """ring depths 1, 2, 3, 4 (first in-loop stage), 5 (first wrap to slot 0) and 16; one token, a last block with one valid token (257),
    three blocks"""
    h, rows, P = SR.ffn_case("unit", n_tok, d_ffn, 0)
    got, names = _run_ffn(ccx_ctx, h, n_tok, rows, P, d_ffn)
    assert names == ["sep_ffn_kernel"]
    _check_ffn(got, SR.ffn_op(h, n_tok, P), h, n_tok, "unit", ("ffn", n_tok, d_ffn))


@pytest.mark.parametrize("regime", ["offset", "lowvar", "special"])
@pytest.mark.parametrize("n_tok,d_ffn", [(257, 320), (600, 1024)])
def test_ffn_input_regimes(ccx_ctx, regime, n_tok, d_ffn):
    h, rows, P = SR.ffn_case(regime, n_tok, d_ffn, 0)
    got, _ = _run_ffn(ccx_ctx, h, n_tok, rows, P, d_ffn, labels=False)
    _check_ffn(got, SR.ffn_op(h, n_tok, P), h, n_tok, regime, ("ffn", regime, n_tok, d_ffn))


@pytest.mark.parametrize("case", ["b1_minus_100", "w2_zero", "w1_zero_b1_zero"])
def test_ffn_exact_cases(ccx_ctx, case):
    """the hidden activation or W2 is zero: the update is b2 alone and h' = fl(fl(0 + b2) + h) bit for bit"""
    n_tok, d_ffn = 257, 320
    h, rows, P = SR.ffn_case("unit", n_tok, d_ffn, 0)
    P = dict(P)
    if case == "b1_minus_100":
        P["b1"] = torch.full_like(P["b1"], -100.0)
    elif case == "w2_zero":
        P["w2"] = torch.zeros_like(P["w2"])
    else:
        P["w1"], P["b1"] = torch.zeros_like(P["w1"]), torch.zeros_like(P["b1"])
    got, _ = _run_ffn(ccx_ctx, h, n_tok, rows, P, d_ffn, labels=False)
    assert torch.equal(_bits(got), _bits((0.0 + P["b2"].float()) + h[:n_tok].float()))


def test_ffn_rows_do_not_depend_on_the_buffer_position(ccx_ctx):
    n_tok, d_ffn = 257, 1024
    h, rows, P = SR.ffn_case("unit", n_tok, d_ffn, 0)
    a, _ = _run_ffn(ccx_ctx, h, n_tok, rows, P, d_ffn, labels=False)
    b, _ = _run_ffn(ccx_ctx, h, n_tok, rows, P, d_ffn, labels=False, shift=1)
    assert torch.equal(_bits(a), _bits(b))
    c, _ = _run_ffn(ccx_ctx, h[1:], n_tok - 1, rows - 1, P, d_ffn, labels=False)      # the same tokens one slot earlier in their tiles
    assert torch.equal(_bits(a[1:]), _bits(c))


# ---------------------------------------------------------------------------------------------------------------------------------
# final norm, decoder
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["offset", "lowvar"])
def test_final_norm(ccx_ctx, regime):
    h, xin, seqs, rows, P = SR.norm_case(regime, 0)
    mask = SR.in_sequence_mask(seqs, rows)
    y = torch.full((rows, SR.D), math.nan, device="cuda")
    T = dict(_dev_params({k: P[k] for k in ("ln_g", "ln_b", "gln_g", "gln_b")}), h=_nan_outside(h, mask).cuda(),
             xin=_nan_outside(xin, mask).cuda(), y=y)
    rc, _ = _call(ccx_ctx, FINAL_NORM, T, rows, seqs=seqs, labels=False)
    ccx_ctx.check(rc, "ccx_sep_op")
    got = y.cpu()
    assert torch.isnan(got[~mask]).all(), "a row outside every sequence was written"
    assert torch.isfinite(got[mask]).all()
    ref = SR.final_norm_op(h, xin, seqs, P)
    for seq, r in zip(seqs, ref):
        s0, n = seq
        allow = SR.final_norm_allowance(h, xin, seq, P)
        within(N_NORM, float(((got[s0:s0 + n].double() - r).abs() / allow).max()), 1.0, ("final norm", regime, n))


def test_decoder(ccx_ctx):
    """three utterances in one launch: L = 1 (T = 16); T = 8 L + 13; L = 150 exactly (the whole following chunk is padding), trimmed to
    out_stride = 1003"""
    feats, fc, utts, rows, wdec, out_stride = SR.decoder_case(0)
    mask = torch.zeros(rows, dtype=torch.bool)
    for tok0, L, T in utts:
        mask[tok0:tok0 + L] = True
    out = torch.full((len(utts), out_stride, 2), math.nan, device="cuda")
    T_ = {"feats": _nan_outside(feats, mask).cuda(), "fc": _nan_outside(fc, mask).cuda(), "wdec": wdec.float().cuda(), "out": out}
    rc, _ = _call(ccx_ctx, DECODER, T_, rows, utts=utts, out_stride=out_stride, labels=False)
    ccx_ctx.check(rc, "ccx_sep_op")
    got = out.cpu()
    assert torch.isfinite(got).all()
    ref = SR.decoder_op(feats, fc, utts, wdec, out_stride)
    allow = SR.decoder_allowance(feats, fc, utts, wdec, out_stride)
    for u, (tok0, L, T) in enumerate(utts):
        n = min(T, 8 * (L + 1))
        assert bool((got[u, n:] == 0).all()), u                                     # past the frames' support and past T: exactly 0
        within(N_DEC, float(((got[u, :n].double() - ref[u, :n]).abs() / allow[u, :n].clamp_min(1e-30)).max()), 1.0, ("decoder", u))


# ---------------------------------------------------------------------------------------------------------------------------------
# repeatability: a wrong wait count of the FFN's DMA ring shows as a run-to-run difference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ffn_repeats_bit_identically(ccx_ctx):
    n_tok, d_ffn = 20000, 1024
    h, rows, P = SR.ffn_case("unit", n_tok, d_ffn, 1)
    T = _dev_params({k: P[k] for k in ("ln_g", "ln_b", "w1", "b1", "w2", "b2")})
    h_in = h.cuda()
    first = None
    for i in range(20):
        h_dev = h_in.clone()
        rc, _ = _call(ccx_ctx, FFN, dict(T, h=h_dev), rows, n_tok=n_tok, d_ffn=d_ffn, labels=False)
        ccx_ctx.check(rc, "ccx_sep_op")
        if first is None:
            first = h_dev
        else:
            assert torch.equal(_bits(first), _bits(h_dev)), i
    got = first[:n_tok].cpu()
    _check_ffn(got, SR.ffn_op(h, n_tok, P), h, n_tok, "unit", ("ffn repeat",))


def test_fused_attention_repeats_bit_identically(ccx_ctx):
    seqs, rows = SR.layout((150,) * 130, gap=0)
    P = SR.make_params(2)
    h = SR.make_rows("unit", rows, 2)
    T = _dev_params({k: P[k] for k in ("ln_g", "ln_b", "wqkv", "bqkv", "wo", "bo")})
    h_in = h.cuda()
    first = None
    for i in range(20):
        h_dev = h_in.clone()
        rc, _ = _call(ccx_ctx, ATTN_BLOCK, dict(T, h=h_dev), rows, seqs=seqs, labels=False)
        ccx_ctx.check(rc, "ccx_sep_op")
        if first is None:
            first = h_dev
        else:
            assert torch.equal(_bits(first), _bits(h_dev)), i
    got = first.cpu()
    for (s0, n), r in zip(seqs, SR.attn_block_op(h, seqs, P)):
        _check_update(got[s0:s0 + n], r, h[s0:s0 + n], "unit", ("fused repeat", s0))


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections: every host check of ccx_sep_op refuses with CCX_ERR_ARG, names its field and launches nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def _reject(ctx, op, tensors, rows, field, watch, **kw):
    before = {k: _bits(tensors[k]).clone() for k in watch}
    rc, names = _call(ctx, op, tensors, rows, **kw)
    msg = ctx.lib.ccx_last_error(ctx.handle).decode()
    assert rc == 1, (rc, msg)
    assert msg.startswith("ccx_sep_op:") and field in msg, msg
    assert names == []
    for k in watch:
        assert torch.equal(before[k], _bits(tensors[k])), k


def _fused_tensors(rows=40):
    P = SR.make_params(0)
    return dict(_dev_params({k: P[k] for k in ("ln_g", "ln_b", "wqkv", "bqkv", "wo", "bo")}), h=SR.make_rows("unit", rows, 0).cuda())


SEQ_REJECTIONS = {
    "start_negative": ([(-1, 5)], "seq_start"), "past_the_rows": ([(30, 11)], "seq_start"), "empty": ([(3, 0)], "seq_len"),
    "overlap": ([(20, 10), (3, 10), (12, 9)], "overlap")}


@pytest.mark.parametrize("case", sorted(SEQ_REJECTIONS))
def test_rejects_bad_sequence_tables(ccx_ctx, case):
    seqs, field = SEQ_REJECTIONS[case]
    _reject(ccx_ctx, ATTN_BLOCK, _fused_tensors(), 40, field, ["h"], seqs=seqs)


def test_rejects_a_sequence_too_long_for_the_fused_block(ccx_ctx):
    _reject(ccx_ctx, ATTN_BLOCK, _fused_tensors(200), 200, "seq_len[0] = 161", ["h"], seqs=[(0, 161)])
    # the split kernel takes it
    qkv = torch.zeros(200, 384, dtype=torch.bfloat16, device="cuda")
    att = torch.zeros(200, 128, dtype=torch.bfloat16, device="cuda")
    rc, _ = _call(ccx_ctx, ATTENTION, {"qkv": qkv, "att": att}, 200, seqs=[(0, 161)], labels=False)
    assert rc == 0
    for seqs, field in (([(190, 11)], "seq_start"), ([(0, 0)], "seq_len")):
        _reject(ccx_ctx, ATTENTION, {"qkv": qkv, "att": att}, 200, field, ["att"], seqs=seqs)
        norm = dict(_dev_params({k: SR.make_params(0)[k] for k in ("ln_g", "ln_b", "gln_g", "gln_b")}), h=torch.zeros(200, 128, device="cuda"),
                    xin=torch.zeros(200, 128, device="cuda"), y=torch.zeros(200, 128, device="cuda"))
        _reject(ccx_ctx, FINAL_NORM, norm, 200, field, ["y"], seqs=seqs)


@pytest.mark.parametrize("field,count", [("wqkv_elems", 384 * 128 - 1), ("wo_elems", 128 * 128 + 128), ("bqkv_elems", 128), ("h_elems", 40 * 128 - 1)])
def test_rejects_wrong_element_counts_fused(ccx_ctx, field, count):
    _reject(ccx_ctx, ATTN_BLOCK, _fused_tensors(), 40, field, ["h"], seqs=[(0, 10)], override={field: count})


def _ffn_tensors(d_ffn=128, rows=40):
    P = SR.make_params(0, d_ffn)
    return dict(_dev_params({k: P[k] for k in ("ln_g", "ln_b", "w1", "b1", "w2", "b2")}), h=SR.make_rows("unit", rows, 0).cuda())


@pytest.mark.parametrize("d_ffn", [0, 32, 96, 1088])
def test_rejects_d_ffn_the_kernel_cannot_stage(ccx_ctx, d_ffn):
    """stages of 64 hidden units and a 4096-byte bias region: multiples of 64 up to 1024 (192 and 320 run, see above)"""
    _reject(ccx_ctx, FFN, _ffn_tensors(), 40, "d_ffn", ["h"], n_tok=40, d_ffn=d_ffn)


@pytest.mark.parametrize("n_tok", [0, -3, 41])
def test_rejects_n_tok_out_of_range(ccx_ctx, n_tok):
    _reject(ccx_ctx, FFN, _ffn_tensors(), 40, "n_tok", ["h"], n_tok=n_tok, d_ffn=128)


@pytest.mark.parametrize("field,count", [("w1_elems", 64 * 128), ("w2_elems", 256 * 128), ("b1_elems", 64)])
def test_rejects_wrong_element_counts_ffn(ccx_ctx, field, count):
    _reject(ccx_ctx, FFN, _ffn_tensors(), 40, field, ["h"], n_tok=40, d_ffn=128, override={field: count})


DECODER_REJECTIONS = {
    "no_frames": ([(0, 0, 16)], "utt_L"), "too_few_samples": ([(0, 1, 15)], "utt_T"), "samples_past_the_stride": ([(0, 37, 401)], "utt_T"),
    "padded_frames_past_the_rows": ([(0, 150, 400)], "utt_tok0"), "second_utterance_past_the_rows": ([(0, 3, 40), (150, 2, 32)], "utt_tok0[1]")}


@pytest.mark.parametrize("case", sorted(DECODER_REJECTIONS))
def test_rejects_bad_utterance_tables(ccx_ctx, case):
    utts, field = DECODER_REJECTIONS[case]
    rows = 299                                             # 150 frames need 300 rows: a whole extra chunk
    T = {"feats": torch.zeros(rows, 128, device="cuda"), "fc": torch.zeros(rows, 256, device="cuda"),
         "wdec": torch.zeros(128, 16, device="cuda"), "out": torch.full((len(utts), 400, 2), math.nan, device="cuda")}
    _reject(ccx_ctx, DECODER, T, rows, field, ["out"], utts=utts, out_stride=400)


# every pointer and count of every op: the checks are shared macros, each op names its own fields
def _attention_tensors(rows=40):
    return {"qkv": torch.zeros(rows, 384, dtype=torch.bfloat16, device="cuda"), "att": torch.zeros(rows, 128, dtype=torch.bfloat16, device="cuda")}


def _norm_tensors(rows=40):
    P = SR.make_params(0)
    return dict(_dev_params({k: P[k] for k in ("ln_g", "ln_b", "gln_g", "gln_b")}), h=SR.make_rows("unit", rows, 0).cuda(),
                xin=torch.zeros(rows, 128, device="cuda"), y=torch.zeros(rows, 128, device="cuda"))


def _decoder_tensors(rows=299):
    return {"feats": torch.zeros(rows, 128, device="cuda"), "fc": torch.zeros(rows, 256, device="cuda"),
            "wdec": torch.zeros(128, 16, device="cuda"), "out": torch.full((1, 400, 2), math.nan, device="cuda")}


# op -> (op code, tensors, rows, arguments of a call that would run, the buffer the op writes)
OPS = {"fused": (ATTN_BLOCK, _fused_tensors, 40, dict(seqs=[(0, 10)]), "h"),
       "attention": (ATTENTION, _attention_tensors, 40, dict(seqs=[(0, 10)]), "att"),
       "ffn": (FFN, _ffn_tensors, 40, dict(n_tok=40, d_ffn=128), "h"),
       "final_norm": (FINAL_NORM, _norm_tensors, 40, dict(seqs=[(0, 10)]), "y"),
       "decoder": (DECODER, _decoder_tensors, 299, dict(utts=[(0, 3, 40)], out_stride=400), "out")}
OP_FIELDS = {"fused": ("h", "ln_g", "ln_b", "wqkv", "bqkv", "wo", "bo"), "attention": ("qkv", "att"),
             "ffn": ("h", "ln_g", "ln_b", "w1", "b1", "w2", "b2"), "final_norm": ("h", "xin", "y", "ln_g", "ln_b", "gln_g", "gln_b"),
             "decoder": ("feats", "fc", "wdec", "out")}
OP_POINTERS = [(op, f) for op, fields in OP_FIELDS.items() for f in fields]


def _reject_op(ctx, op, field, override, **extra):
    code, make, rows, kw, written = OPS[op]
    kw = dict(kw, **extra)
    rows = kw.pop("rows", rows)
    _reject(ctx, code, make(), rows, field, [written], override=override, **kw)


@pytest.mark.parametrize("op,field", OP_POINTERS)
def test_rejects_a_misaligned_pointer(ccx_ctx, op, field):
    _reject_op(ccx_ctx, op, field + " is not 16-byte aligned", {field: lambda p: p + 4})


@pytest.mark.parametrize("op,field", OP_POINTERS)
def test_rejects_a_null_pointer(ccx_ctx, op, field):
    _reject_op(ccx_ctx, op, field + " is NULL", {field: None})


@pytest.mark.parametrize("op,field", OP_POINTERS)
def test_rejects_a_wrong_element_count(ccx_ctx, op, field):
    """a buffer one element short of what the op touches; a parameter tensor of any other size than the kernel reads"""
    count = field + "_elems" if field in BUFFERS else PARAM_COUNT[field]
    _reject_op(ccx_ctx, op, count, {count: lambda n: n - 1})


def test_rejects_an_output_that_aliases_an_input(ccx_ctx):
    for src in ("h", "xin"):
        code, make, rows, kw, written = OPS["final_norm"]
        T = make()
        _reject(ccx_ctx, code, T, rows, "y aliases", [written], override={"y": T[src].data_ptr()}, **kw)


RANGE_REJECTIONS = {
    "unknown_op": ("fused", "unknown op", {}, dict(code=5)), "op_negative": ("fused", "unknown op", {}, dict(code=-1)),
    "no_rows": ("fused", "rows", {}, dict(rows=0)),
    "no_sequences": ("attention", "n_seq", {"n_seq": 0}, {}), "too_many_sequences": ("final_norm", "n_seq", {"n_seq": (1 << 20) + 1}, {}),
    "null_sequence_table": ("fused", "seq_start or seq_len is NULL", {"seq_len": None}, {}),
    "no_utterances": ("decoder", "n_utt", {"n_utt": 0}, {}), "too_many_utterances": ("decoder", "n_utt", {"n_utt": 65536}, {}),
    "null_utterance_table": ("decoder", "utt_tok0, utt_L or utt_T is NULL", {"utt_L": None}, {}),
    "segment_zero": ("decoder", "segment", {"segment": 0}, {}),
    "stride_under_a_frame": ("decoder", "out_stride", {"out_stride": 15}, {}),
    "final_norm_past_the_rows": ("final_norm", "seq_start", {}, dict(seqs=[(35, 6)])),
    "final_norm_empty": ("final_norm", "seq_len", {}, dict(seqs=[(0, 10), (20, 0)]))}


@pytest.mark.parametrize("case", sorted(RANGE_REJECTIONS))
def test_rejects_ranges(ccx_ctx, case):
    op, field, override, extra = RANGE_REJECTIONS[case]
    code, make, rows, kw, written = OPS[op]
    kw = dict(kw, **{k: v for k, v in extra.items() if k not in ("code", "rows")})
    _reject(ccx_ctx, extra.get("code", code), make(), extra.get("rows", rows), field, [written], override=override, **kw)
