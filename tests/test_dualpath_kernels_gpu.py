"""GPU: the dual-path SepFormer kernels (csrc/dualpath.hip) one at a time through ccx_dualpath_op -- the production launchers of
csrc/dualpath.h, away from the model -- against the fp64 references of tests/dualpath_reference.py from the operands the kernels see.

Rows outside every sequence hold NaN and every output is pre-filled with NaN: a read past a sequence shows as a non-finite value, a
row that was never stored stays NaN, a store outside the rows in use changes bits.  Bounds: copies and single fp32 additions are
compared bit for bit; one bf16 rounding of an fp64 value gets half a bf16 ulp (+ 2^-10 of it for the fp32 arithmetic in front);
fp32 sums get the derived (n + 3) u sum|terms|; attention and the GroupNorm get a measured bound (dualpath_reference.py)."""
import ctypes as C
import math

import pytest
import torch

from tests import dualpath_reference as R
from tests.conftest import within
from tests.sep_reference import half_ulp_bf16

pytestmark = pytest.mark.gpu
N_ATT = "dualpath kernels: attention, excess over half a bf16 ulp / max|v|"
N_GN = "dualpath kernels: group norm, max|err| / max|ref|"
N_SUM = "dualpath kernels: encoder / decoder, |err| / derived allowance"
N_GATE = "dualpath kernels: gate, |err| / (half a bf16 ulp (1 + 2^-10))"
D = 256


def _ints(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def _op(ctx, op, bufs, tables=None, expect_ok=True, **scalars):
    """One ccx_dualpath_op.  bufs: field -> CUDA tensor (or (tensor, stated elements)); tables: field -> list of ints."""
    from clearconverse_amd import _lib
    d = _lib.DualPathDesc()
    for name, t in bufs.items():
        t, n = t if isinstance(t, tuple) else (t, t.numel())
        setattr(d, name, t.data_ptr() if hasattr(t, "data_ptr") else t)
        setattr(d, name + "_elems", n)
    keep = []
    for name, vals in (tables or {}).items():
        keep.append(_ints(vals))
        setattr(d, name, keep[-1])
    for name, v in scalars.items():
        setattr(d, name, v)
    rc = _lib.load().ccx_dualpath_op(ctx.handle, op, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect_ok:
        ctx.check(rc, "ccx_dualpath_op")
    return rc


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- attention ----------------------------------------------------------------------------------------------------------------
# 64 and 65: on and one past the block of CCX_DP_KEY_BLOCK keys, contiguous and strided
ATT_LENS = ((1, 1), (15, 1), (16, 1), (17, 1), (250, 1), (257, 1), (10, 1), (2, 10), (37, 10), (2, 250), (19, 250), (64, 1), (65, 1),
            (65, 10))


def _att_run(ctx, qkv, seqs, rows, order=None):
    mask = torch.zeros(rows, dtype=torch.bool)
    for f, s, n in seqs:
        mask[f + s * torch.arange(n)] = True
    q = qkv.clone()
    q[~mask] = math.nan
    out = torch.full((rows, D), math.nan).to(torch.bfloat16).cuda()
    before = out.clone()
    sq = seqs if order is None else [seqs[i] for i in order]
    from clearconverse_amd import _lib
    _op(ctx, _lib.DP_ATTENTION, {"in": q.to(torch.bfloat16).cuda(), "out": out},
        {"seq_first": [s[0] for s in sq], "seq_stride": [s[1] for s in sq], "seq_len": [s[2] for s in sq]}, rows=rows, n_seq=len(sq))
    assert torch.equal(_bits(out)[~mask.cuda()], _bits(before)[~mask.cuda()]), "a row outside every sequence changed"
    return out.cpu()


@pytest.mark.parametrize("kind", ["random", "dominant", "flat"])
def test_attention(ccx_ctx, kind):
    qkv, seqs, rows = R.attention_case(ATT_LENS, 1)
    if kind == "dominant":
        for i, s in enumerate(seqs):
            R.plant_dominant(qkv, s, (0, s[2] - 1, (s[2] - 1) // 16 * 16)[i % 3])
    if kind == "flat":
        qkv[:, :D] = 0.0                                    # every score 0: the output is the plain mean of v
    got = _att_run(ccx_ctx, qkv, seqs, rows)
    refs = R.attention_op(qkv, seqs, round_out=False)
    for (f, s, n), ref in zip(seqs, refs):
        idx = f + s * torch.arange(n)
        g = got[idx].float()
        assert torch.isfinite(g).all(), (f, s, n)
        vmax = qkv[idx, 2 * D:].double().abs().view(n, 8, 32).amax(dim=(0, 2))
        within(N_ATT, R.att_excess(g, ref, vmax), R.BOUND_ATT_EXCESS, (kind, f, s, n))
        if kind == "flat":
            assert float((g.double() - qkv[idx, 2 * D:].double().mean(0)).abs().max()) < 2.0 ** -7 * float(vmax.max())
    again = _att_run(ccx_ctx, qkv, seqs, rows)
    assert torch.equal(_bits(again), _bits(got)), "a repeat differs"
    shuffled = _att_run(ccx_ctx, qkv, seqs, rows, order=list(reversed(range(len(seqs)))))
    assert torch.equal(_bits(shuffled), _bits(got)), "the result depends on the table's order"


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_group_norm_large_mean_tiny_variance_channel(ccx_ctx, mode):
    from clearconverse_amd import _lib
    g = torch.Generator().manual_seed(5)
    utts = [(2, 1), (5, 37), (45, 500), (547, 130)]          # (row0, rows): one row, fewer rows than slices, many rows
    rows = 680
    x = torch.randn(rows, D, generator=g)
    x[:, 7] = 100.0 + 1e-3 * torch.randn(rows, generator=g)
    x[45:545, :] = 30.0 + 1e-2 * torch.randn(500, D, generator=g)      # a whole utterance with a large mean and a tiny variance
    gamma, beta, skip = 1 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g), torch.randn(rows, D, generator=g)
    mask = torch.zeros(rows, dtype=torch.bool)
    for r0, n in utts:
        mask[r0:r0 + n] = True
    xin = x.clone()
    xin[~mask] = math.nan
    out = torch.full((rows, D), math.nan, dtype=torch.bfloat16 if mode else torch.float32).cuda()
    before = out.clone()
    bufs = {"in": xin.cuda(), "out": out, "w": gamma.cuda(), "w2": beta.cuda()}
    if mode == 0:
        bufs["in2"] = skip.cuda()
    _op(ccx_ctx, _lib.DP_GROUP_NORM, bufs, {"utt_row0": [u[0] for u in utts], "utt_rows": [u[1] for u in utts]}, rows=rows, n_utt=len(utts), mode=mode)
    assert torch.equal(_bits(out)[~mask.cuda()], _bits(before)[~mask.cuda()])
    for r0, n in utts:
        ref = R.group_norm(x[r0:r0 + n].double(), gamma.double(), beta.double())
        got = out[r0:r0 + n].cpu().double()
        if mode == 0:
            err = (got - (ref + skip[r0:r0 + n].double())).abs().max()
        else:                                                # one bf16 rounding of the fp32 value: the fp32 error + half a bf16 ulp
            err = ((got - ref).abs() - half_ulp_bf16(ref)).clamp_min(0).max()
        within(N_GN, float(err / ref.abs().max()), R.BOUND_GN, (mode, r0, n))


# ---- segmentation, overlap-add, PE add -------------------------------------------------------------------------------------------
def _utt_tables(Ls, K, gap_rows=2):
    tok0, frame0, gaps, Ss, t, f = [], [], [], [], gap_rows, 1
    for L in Ls:
        gap, S = R.geometry(L, K)
        tok0.append(t); frame0.append(f); gaps.append(gap); Ss.append(S)
        t += S * K + gap_rows
        f += L + 1
    return {"utt_tok0": tok0, "utt_frame0": frame0, "utt_L": list(Ls), "utt_gap": gaps, "utt_S": Ss}, t, f


@pytest.mark.parametrize("K,Ls", [(10, (1, 4, 5, 14, 15, 37)), (250, (1, 124, 125, 499))])
def test_segmentation_overlap_add_and_pe(ccx_ctx, K, Ls):
    """L % K == K / 2 - 1 gives gap = 1, L % K == K / 2 gives gap = K"""
    from clearconverse_amd import _lib
    tabs, rows, frames = _utt_tables(Ls, K)
    assert 1 in tabs["utt_gap"] and K in tabs["utt_gap"]
    g = torch.Generator().manual_seed(K)
    x = torch.randn(frames, D, generator=g)
    tok = torch.full((rows, D), math.nan).cuda()
    _op(ccx_ctx, _lib.DP_SEGMENT, {"in": x.cuda(), "out": tok}, tabs, rows=rows, frames=frames, n_utt=len(Ls), segment=K)
    want = torch.full((rows, D), math.nan)
    for t0, f0, L, S in zip(tabs["utt_tok0"], tabs["utt_frame0"], Ls, tabs["utt_S"]):
        want[t0:t0 + S * K] = R.segmentation(x[f0:f0 + L], K).reshape(S * K, D)
    assert torch.equal(_bits(tok.cpu()), _bits(want)), "segmentation is a copy with zeros: bit for bit"

    for mode in (0, 1):
        pe = R.positional_encoding(max(K, max(tabs["utt_S"])) + 1, D)
        xin = torch.randn(rows, D, generator=g)
        out = torch.full((rows, D), math.nan).cuda()
        _op(ccx_ctx, _lib.DP_PE_ADD, {"in": xin.cuda(), "out": out, "w": pe.cuda()}, tabs, rows=rows, n_utt=len(Ls), segment=K, mode=mode)
        want = torch.full((rows, D), math.nan)
        for t0, S in zip(tabs["utt_tok0"], tabs["utt_S"]):
            p = pe[:S, None].expand(S, K, D) if mode else pe[None, :K].expand(S, K, D)
            want[t0:t0 + S * K] = xin[t0:t0 + S * K] + p.reshape(S * K, D)
        assert torch.equal(_bits(out.cpu()), _bits(want)), ("PE add is one fp32 addition", mode)

    for n_spk in (1, 3):
        fc = torch.randn(rows, n_spk * D, generator=g)
        out = torch.full((frames * n_spk, D), math.nan).to(torch.bfloat16).cuda()
        _op(ccx_ctx, _lib.DP_OVERLAP_ADD, {"in": fc.cuda(), "out": out}, tabs, rows=rows, frames=frames, n_utt=len(Ls), segment=K, n_spk=n_spk)
        want = torch.full((frames * n_spk, D), math.nan).to(torch.bfloat16)
        for t0, f0, L, S in zip(tabs["utt_tok0"], tabs["utt_frame0"], Ls, tabs["utt_S"]):
            y = R.overlap_add(fc[t0:t0 + S * K].view(S, K, n_spk * D), L)          # fp32: one addition per value, exact to compare
            want[f0 * n_spk:(f0 + L) * n_spk] = y.view(L * n_spk, D).to(torch.bfloat16)
        assert torch.equal(_bits(out.cpu()), _bits(want)), ("overlap-add is one fp32 addition and one rounding", n_spk)


# ---- gate and PReLU -----------------------------------------------------------------------------------------------------------------
def test_gate_and_prelu(ccx_ctx):
    from clearconverse_amd import _lib
    vals = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 9.0, -9.0, 20.0, -20.0, 40.0, -40.0, 100.0, -100.0, 1e4, -1e4])
    rows = len(vals)
    a = vals[:, None].expand(rows, D).clone()
    b = vals[torch.arange(D) % rows][None].expand(rows, D).clone()
    g = torch.cat([a, b], 1).contiguous()
    out = torch.full((rows, D), math.nan).to(torch.bfloat16).cuda()
    _op(ccx_ctx, _lib.DP_GATE, {"in": g.cuda(), "out": out}, rows=rows)
    ref = R.gate_op(g.double())
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs() / (half_ulp_bf16(ref) * (1 + 2.0 ** -10))
    within(N_GATE, float(err.max()), 1.0 + 1e-9)
    assert float(got[16].abs().max()) <= 1.0 and torch.equal(got[17, :2], torch.tensor([-0.5, -0.5], dtype=torch.float64))   # tanh(-100) sigmoid(0)

    x = torch.cat([vals, torch.randn(4 * D - rows, generator=torch.Generator().manual_seed(2))]).view(4, D).contiguous()
    for slope in (0.25, -0.5):
        out = torch.full((4, D), math.nan).to(torch.bfloat16).cuda()
        _op(ccx_ctx, _lib.DP_PRELU, {"in": x.cuda(), "out": out, "w": torch.tensor([slope]).cuda()}, rows=4)
        want = torch.where(x >= 0, x, torch.tensor(slope) * x).to(torch.bfloat16)
        assert torch.equal(_bits(out.cpu()), _bits(want)), slope


# ---- encoder and decoder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n_spk", [(16, 3), (16, 1), (2, 2), (32, 2)])
def test_encoder_and_decoder(ccx_ctx, kernel, n_spk):
    from clearconverse_amd import _lib
    stride = kernel // 2
    Ts = (kernel, kernel + 1, 8 * kernel + 3 if kernel > 2 else 37)                   # T = kernel, an odd T, a longer odd T
    Ls = [(T - kernel) // stride + 1 for T in Ts]
    in_stride = max(Ts) + 5
    frame0 = [1, 3 + Ls[0], 5 + Ls[0] + Ls[1]]
    frames = frame0[-1] + Ls[-1] + 2
    g = torch.Generator().manual_seed(kernel + n_spk)
    mix = torch.randn(len(Ts), in_stride, generator=g)
    for i, T in enumerate(Ts):
        mix[i, T:] = math.nan                                                          # samples past T must not be read
    w = torch.randn(D, kernel, generator=g) / math.sqrt(kernel)
    feats = torch.full((frames, D), math.nan).cuda()
    tabs = {"utt_frame0": frame0, "utt_L": Ls, "utt_T": list(Ts)}
    _op(ccx_ctx, _lib.DP_ENCODER, {"in": mix.cuda(), "out": feats, "w": w.cuda()}, tabs, frames=frames, n_utt=len(Ts), kernel=kernel, in_stride=in_stride)
    feats = feats.cpu()
    used = torch.zeros(frames, dtype=torch.bool)
    for f0, L, T, i in zip(frame0, Ls, Ts, range(3)):
        used[f0:f0 + L] = True
        ref = R.encoder_op(mix[i, :T].double(), w.double(), stride)
        allow = (kernel + 3) * R.U32 * R.encoder_op(mix[i, :T].double().abs(), w.double().abs(), stride) + 1e-30
        within(N_SUM, float(((feats[f0:f0 + L].double() - ref).abs() / allow).max()), 1.0, ("encoder", kernel, T))
    assert torch.isnan(feats[~used]).all(), "a frame row outside every utterance was written"

    # decoder: its own operands; out sits inside a guard band of NaN
    fe = torch.relu(torch.randn(frames, D, generator=g))
    mk = torch.randn(frames * n_spk, D, generator=g)
    wdec = torch.randn(D, kernel, generator=g) / 16
    out_stride = max(Ts) + 3
    Td = (Ts[0], Ts[1], out_stride)                                                    # the last utterance trimmed at out_stride
    guard = 64
    buf = torch.full((guard + len(Ts) * out_stride * n_spk + guard,), math.nan).cuda()
    out = buf[guard:guard + len(Ts) * out_stride * n_spk]
    _op(ccx_ctx, _lib.DP_DECODER, {"in": fe.cuda(), "in2": mk.cuda(), "out": out, "w": wdec.cuda()}, {"utt_frame0": frame0, "utt_L": Ls, "utt_T": list(Td)},
        frames=frames, n_utt=len(Ts), kernel=kernel, n_spk=n_spk, out_stride=out_stride)
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all(), "the guard band around out was written"
    got = out.cpu().view(len(Ts), out_stride, n_spk).double()
    assert torch.isfinite(got).all()
    for i, (f0, L, T) in enumerate(zip(frame0, Ls, Td)):
        m = mk.view(frames, n_spk, D)[f0:f0 + L].double()
        ref = R.decoder_op(fe[f0:f0 + L].double(), m, wdec.double(), stride, T, out_stride)
        allow = (2 * D + 5) * R.U32 * R.decoder_op(fe[f0:f0 + L].double(), m.abs(), wdec.double().abs(), stride, T, out_stride) + 1e-30
        within(N_SUM, float(((got[i] - ref).abs() / allow).max()), 1.0, ("decoder", kernel, n_spk, T))
        assert float(got[i, T:].abs().max() if T < out_stride else 0.0) == 0.0


# ---- host refusals: CCX_ERR_ARG naming the entry point and the field, nothing launched --------------------------------------------------
def test_host_refusals(ccx_ctx):
    from clearconverse_amd import _lib
    lib = _lib.load()
    rows = 64
    qkv = torch.zeros(rows, 3 * D, dtype=torch.bfloat16).cuda()
    f32 = torch.zeros(rows, 3 * D).cuda()
    out = torch.full((rows, 3 * D), 7.0).cuda()
    out16 = torch.full((rows, D), 7.0).to(torch.bfloat16).cuda()
    vec = torch.ones(D).cuda()
    att = dict(bufs={"in": qkv, "out": out16}, tables={"seq_first": [0, 20], "seq_stride": [1, 2], "seq_len": [16, 10]}, rows=rows, n_seq=2)
    chunk = dict(tables={"utt_tok0": [0], "utt_frame0": [0], "utt_L": [14], "utt_gap": [1], "utt_S": [4]}, rows=rows, frames=20, n_utt=1, segment=10)
    fr = dict(tables={"utt_frame0": [0], "utt_L": [3], "utt_T": [32]}, frames=20, n_utt=1, kernel=16)

    def mod(base, **kw):
        c = {k: (dict(v) if isinstance(v, dict) else v) for k, v in base.items()}
        for k, v in kw.items():
            if k in ("bufs", "tables"):
                c.setdefault(k, {}).update(v)
            else:
                c[k] = v
        return c

    seg_bufs = {"in": f32, "out": out}
    cases = [
        (_lib.DP_ATTENTION, mod(att, tables={"seq_len": [0, 10]}), "seq_len[0]"),
        (_lib.DP_ATTENTION, mod(att, tables={"seq_stride": [1, 0]}), "seq_stride[1]"),
        (_lib.DP_ATTENTION, mod(att, tables={"seq_first": [0, 46]}), "seq_first[1]"),
        (_lib.DP_ATTENTION, mod(att, tables={"seq_first": [-1, 20]}), "seq_first[0]"),
        (_lib.DP_ATTENTION, mod(att, bufs={"in": (qkv, rows * 3 * D - 1)}), "in_elems"),
        (_lib.DP_ATTENTION, mod(att, bufs={"out": (out16.data_ptr() + 2, out16.numel())}), "out is not 16-byte aligned"),
        (_lib.DP_ATTENTION, mod(att, bufs={"out": qkv}), "aliases"),
        (_lib.DP_ATTENTION, mod(att, n_seq=0), "n_seq"),
        (_lib.DP_ATTENTION, mod(att, rows=0), "rows"),
        (_lib.DP_GROUP_NORM, dict(bufs={"in": f32, "in2": f32, "out": out, "w": vec, "w2": vec}, tables={"utt_row0": [0], "utt_rows": [65]}, rows=rows, n_utt=1), "utt_rows[0]"),
        (_lib.DP_GROUP_NORM, dict(bufs={"in": f32, "in2": f32, "out": out, "w": vec, "w2": vec}, tables={"utt_row0": [0], "utt_rows": [0]}, rows=rows, n_utt=1), "utt_rows[0]"),
        (_lib.DP_GROUP_NORM, dict(bufs={"in": f32, "in2": f32, "out": out, "w": (vec, 255), "w2": vec}, tables={"utt_row0": [0], "utt_rows": [4]}, rows=rows, n_utt=1), "w holds"),
        (_lib.DP_GROUP_NORM, dict(bufs={"in": f32, "out": out, "w": vec, "w2": vec}, tables={"utt_row0": [0], "utt_rows": [4]}, rows=rows, n_utt=1, mode=2), "mode"),
        (_lib.DP_GROUP_NORM, dict(bufs={"in": f32, "out": out, "w": vec, "w2": vec}, tables={"utt_row0": [0], "utt_rows": [4]}, rows=rows, n_utt=1, mode=0), "in2 is NULL"),
        (_lib.DP_SEGMENT, mod(chunk, bufs=seg_bufs, tables={"utt_gap": [6]}), "utt_gap[0]"),
        (_lib.DP_SEGMENT, mod(chunk, bufs=seg_bufs, tables={"utt_S": [5]}), "utt_S[0]"),
        (_lib.DP_SEGMENT, mod(chunk, bufs=seg_bufs, tables={"utt_tok0": [25]}), "utt_tok0[0]"),
        (_lib.DP_SEGMENT, mod(chunk, bufs=seg_bufs, tables={"utt_frame0": [7]}), "utt_frame0[0]"),
        (_lib.DP_SEGMENT, mod(chunk, bufs=seg_bufs, segment=9), "segment"),
        (_lib.DP_SEGMENT, mod(chunk, bufs=seg_bufs, tables={"utt_L": [0]}), "utt_L[0]"),
        (_lib.DP_OVERLAP_ADD, mod(chunk, bufs=seg_bufs, n_spk=4), "n_spk"),
        (_lib.DP_OVERLAP_ADD, mod(chunk, bufs={"in": (f32, rows * D * 2 - 1), "out": out}, n_spk=2), "in_elems"),
        (_lib.DP_PE_ADD, mod(chunk, bufs={"in": f32, "out": out, "w": (f32, 9 * D)}, mode=0), "w_elems"),
        (_lib.DP_PE_ADD, mod(chunk, bufs={"in": f32, "out": out, "w": (f32, 3 * D)}, mode=1), "w_elems"),
        (_lib.DP_GATE, dict(bufs={"in": (f32, rows * 2 * D - 1), "out": out16}, rows=rows), "in_elems"),
        (_lib.DP_PRELU, dict(bufs={"in": f32, "out": out16, "w": (vec, 2)}, rows=rows), "w holds"),
        (_lib.DP_ENCODER, mod(fr, bufs={"in": f32, "out": out, "w": (f32, D * 16)}, in_stride=40, tables={"utt_L": [4]}), "utt_L[0]"),
        (_lib.DP_ENCODER, mod(fr, bufs={"in": f32, "out": out, "w": (f32, D * 16)}, in_stride=40, tables={"utt_T": [41]}), "utt_T[0]"),
        (_lib.DP_ENCODER, mod(fr, bufs={"in": f32, "out": out, "w": (f32, D * 16)}, in_stride=40, kernel=34), "kernel"),
        (_lib.DP_ENCODER, mod(fr, bufs={"in": f32, "out": out, "w": (f32, D * 15)}, in_stride=40), "w holds"),
        (_lib.DP_DECODER, mod(fr, bufs={"in": f32, "in2": f32, "out": (out, 40 * 2 - 1), "w": (f32, D * 16)}, out_stride=40, n_spk=2), "out_elems"),
        (_lib.DP_DECODER, mod(fr, bufs={"in": f32, "in2": f32, "out": out, "w": (f32, D * 16)}, out_stride=8, n_spk=2), "out_stride"),
        (_lib.DP_DECODER, mod(fr, bufs={"in": f32, "in2": f32, "out": out, "w": (f32, D * 16)}, out_stride=40, n_spk=0), "n_spk"),
        (99, mod(att), "unknown op"),
    ]
    for op, kw, needle in cases:
        rc = _op(ccx_ctx, op, kw.pop("bufs"), kw.pop("tables", None), expect_ok=False, **kw)
        msg = lib.ccx_last_error(ccx_ctx.handle).decode()
        assert rc == 1 and "ccx_dualpath_op" in msg and needle in msg, (op, needle, rc, msg)
        assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(out16.float().min()) == 7.0, ("something was launched", needle)
