"""GPU: the middle of a > 16-row decode layer on the X-stream path, self attention .. cross-attention out projection, run away from the
model through ccx_dec_mid_chain (include/ccx.h): the production launchers, producers and consumers together.  What it is for:

  * CCX_DEC_PACKED_MID -- the chain's remaining bf16 rows (both attention outputs, the resolved rows xb) handed on as fragment images
    (csrc/decoder.h dec_frag_off).  An image puts the same 16 bytes into the same lane as the row-major load, so every output must be
    BIT-equal to the row-major chain.  Scratch rows and outputs start as NaN bit patterns and hold whole 16-row tiles, so a lane fed
    from a padding row or a store that never happened shows as a non-finite output.
  * the launch size: a row's bits do not depend on it.
  * that the chain computes what it says, stage by stage against fp64 (each stage's reference starts from the operands the GPU stage
    consumed, so a kernel answers for its own error only).

Shapes are the smallest at which each thing can go wrong.  Rows: 32 (two tiles), 48 (a ragged 64-row block), 272 (four full row blocks
and one tile: 32 columns per block, the decode lanes' instantiations); 40 and 16: the launcher must keep row-major rows by itself.
Encoder lengths: those of tests/test_xs_full_lines_gpu.py (1500, 1499, 40, 16, 100, 37)."""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests.conftest import within

pytestmark = pytest.mark.gpu

PARTS = ("attn_self", "x", "xb", "xb_stats", "xq", "attn_cross", "co")
MEASURED = Path(__file__).resolve().parent.parent / "profiles" / "dec_mid_chain_measured_deviations.json"
N_XQ = "dec mid chain: expanded query xq, rel-L2 against fp64"
N_CROSS = "dec mid chain: merged value projection, rel-L2 against fp64"

_cache = {}


def _weights(D):
    """host weights of a width, made once and left unchanged"""
    if ("w", D) not in _cache:
        g = torch.Generator().manual_seed(500 + D)
        mat = lambda: np.ascontiguousarray((torch.randn(D, D, generator=g) / math.sqrt(D)).numpy(), dtype=np.float32)
        vec = lambda s, o=0.0: np.ascontiguousarray((o + s * torch.randn(D, generator=g)).numpy(), dtype=np.float32)
        _cache[("w", D)] = {"wo": mat(), "bo": vec(0.1, 0.05), "lnc_g": vec(0.1, 1.0), "lnc_b": vec(0.1), "cq_w": mat(), "cq_b": vec(0.1),
                            "ck_w": mat(), "cv_w": mat(), "cv_b": vec(0.1), "co_w": mat(), "co_b": vec(0.1)}
    return _cache[("w", D)]


def _rows(D, kv_T, n=272):
    """device rows of a width and a cache length, shared by every row count (row r is the same row everywhere)"""
    key = ("rows", D, kv_T)
    if key not in _cache:
        H = D // 64
        g = torch.Generator(device="cuda").manual_seed(900 + D + kv_T)
        x = torch.randn(n, D, device="cuda", generator=g) + 0.5
        x[:, 3] *= 20.0
        shift = x.mean(1)
        shift[1::2] = 0.0                                   # every other row uncentred, as a near-zero-mean row is in the model
        _cache[key] = {"q": torch.randn(n, D, device="cuda", generator=g),
                       "k": torch.randn(n, H, kv_T, 64, device="cuda", generator=g).to(torch.bfloat16),
                       "v": torch.randn(n, H, kv_T, 64, device="cuda", generator=g).to(torch.bfloat16),
                       "x": x, "shift": shift.contiguous()}
    return _cache[key]


def _xa(D, S, n):
    key = ("xa", D, S, n)
    if key not in _cache:
        for k in [k for k in _cache if k[0] == "xa"]:       # one encoder output at a time
            del _cache[k]
        g = torch.Generator(device="cuda").manual_seed(300 + D + S)
        _cache[key] = torch.randn(n, S, D, device="cuda", generator=g).to(torch.bfloat16)
    return _cache[key]


def _pos(M, kv_T, edges=None):
    if edges is not None:
        return np.array([edges[r % len(edges)] - 1 for r in range(M)], dtype=np.int32)
    return np.array([(37 * r + 5) % kv_T for r in range(M)], dtype=np.int32)


def _desc(M, D, S, kv_T, pos, packed, out, used):
    from clearconverse_amd import _lib
    H = D // 64
    w, r = _weights(D), _rows(D, kv_T)
    xa = _xa(D, S, M)
    d = _lib.DecMidChainDesc()
    d.M, d.D, d.H, d.S, d.kv_T, d.packed = M, D, H, S, kv_T, packed
    d.q, d.self_k, d.self_v, d.x, d.shift, d.xa = (r["q"].data_ptr(), r["k"].data_ptr(), r["v"].data_ptr(), r["x"].data_ptr(),
                                                  r["shift"].data_ptr(), xa.data_ptr())
    d.pos = pos.ctypes.data
    for name in w:
        setattr(d, name, w[name].ctypes.data)
    d.out, d.packed_used = out.data_ptr(), C.pointer(used)
    d.q_elems, d.kv_elems, d.x_elems, d.xa_elems, d.out_elems = M * D, M * D * kv_T, M * D, xa.numel(), out.numel()
    return d


def _split(out, M, D):
    H = D // 64
    sizes = {"attn_self": (M, D), "x": (M, D), "xb": (M, D), "xb_stats": (M, D // 16, 2), "xq": (M, H, D), "attn_cross": (M, D), "co": (M, D)}
    res, o = {}, 0
    for name in PARTS:
        n = math.prod(sizes[name])
        res[name] = out[o:o + n].view(sizes[name])
        o += n
    assert o == out.numel()
    return res


def _run(ctx, M, D, S, kv_T=96, packed=0, pos=None):
    from clearconverse_amd import _lib
    lib = _lib.load()
    pos = _pos(M, kv_T) if pos is None else pos
    out = torch.full((lib.ccx_dec_mid_chain_out_elems(M, D, D // 64),), math.nan, device="cuda")
    used = C.c_int(-1)
    d = _desc(M, D, S, kv_T, pos, packed, out, used)
    rc = lib.ccx_dec_mid_chain(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_mid_chain")
    res = _split(out.cpu(), M, D)
    for name in PARTS:
        assert torch.isfinite(res[name]).all(), (name, M, D, S, packed)
    return res, used.value


def _same(a, b, what):
    for name in PARTS:
        assert torch.equal(a[name], b[name]), (what, name, float((a[name] - b[name]).abs().max()))


# (D, M, S): both widths at every row count, every encoder length once
IMAGE_CASES = [(768, 32, 1500), (768, 48, 1499), (768, 272, 40), (768, 32, 16), (256, 32, 100), (256, 48, 37), (256, 272, 40)]


@pytest.mark.parametrize("D,M,S", IMAGE_CASES)
def test_image_equals_row_major(ccx_ctx, D, M, S):
    rm, used0 = _run(ccx_ctx, M, D, S, packed=0)
    pk, used1 = _run(ccx_ctx, M, D, S, packed=1)
    assert (used0, used1) == (0, 1)
    _same(rm, pk, (D, M, S))


@pytest.mark.parametrize("M", [40, 16])
def test_launcher_keeps_row_major_rows_by_itself(ccx_ctx, M):
    """not whole tiles (40), a single tile (16): asked for images, the launcher takes row-major and says so"""
    rm, used0 = _run(ccx_ctx, M, 768, 40, packed=0)
    pk, used1 = _run(ccx_ctx, M, 768, 40, packed=1)
    assert (used0, used1) == (0, 0)
    _same(rm, pk, M)


@pytest.mark.parametrize("packed", [0, 1])
def test_rows_do_not_depend_on_the_launch(ccx_ctx, packed):
    """rows 0 .. 31 of a 272-row launch (four row tiles and 32 columns per block in the out projections) against a 32-row launch of
    the same rows (two row tiles, 16 columns per block)"""
    big = _run(ccx_ctx, 272, 768, 40, packed=packed)[0]
    small = _run(ccx_ctx, 32, 768, 40, packed=packed)[0]
    for name in PARTS:
        assert torch.equal(small[name], big[name][:32]), (packed, name)


# pos + 1: one key, a partial chunk, the 64-key chunk edges (waves 1, 2 and 3 of a block get their first key at 65, 129 and 193 .. 255),
# the end of the four waves' first round and the second trip of wave 0's key loop behind it, the cache edge
SELF_EDGES = [1, 8, 63, 64, 65, 128, 129, 255, 256, 257, 448]


def test_self_attention_image_at_the_chunk_edges(ccx_ctx):
    """32 rows x 12 heads at kv_T = 448 whose key counts take every value above: the self attention that stores the image
    (dec_attention_kernel<true, false, true>) against the row-major one, bit for bit through the whole chain, and its rows against fp64
    under tests/test_dec_attention_gpu.py's bound"""
    M, D, S, kv_T = 32, 768, 16, 448
    pos = _pos(M, kv_T, SELF_EDGES)
    assert set(int(v) + 1 for v in pos) == set(SELF_EDGES)
    rm, used0 = _run(ccx_ctx, M, D, S, kv_T=kv_T, packed=0, pos=pos)
    pk, used1 = _run(ccx_ctx, M, D, S, kv_T=kv_T, packed=1, pos=pos)
    assert (used0, used1) == (0, 1)
    _same(rm, pk, "self attention edges")
    H = D // 64
    r = _rows(D, kv_T)
    ref, vmax = DR.attention_ref(r["q"][:M].cpu().view(M, H, 64), r["k"][:M].float().cpu(), r["v"][:M].float().cpu(), pos + 1)
    ex = DR.bf16_out_excess(pk["attn_self"].view(M, H, 64), ref, vmax)
    print(f"self attention at the chunk edges, excess over half a bf16 ulp / max|v|: {ex:.3e}")
    within("dec attention: bf16 output, excess over half an ulp / max|v|", ex, 1.1e-3, "image, chunk edges")


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def _fp64_figures(res, M, D, S, kv_T, pos):
    """every stage against fp64 from the operands the GPU stage consumed; weights rounded to bf16 as the product rounds them"""
    H = D // 64
    w = {k: torch.from_numpy(v) for k, v in _weights(D).items()}
    r = {k: v[:M].cpu() for k, v in _rows(D, kv_T).items()}
    xa = _xa(D, S, M).cpu().double()
    bf = lambda t: DR.bf16_round(t.float()).double()
    fig = {}
    # self attention
    ref, vmax = DR.attention_ref(r["q"].view(M, H, 64), r["k"].float(), r["v"].float(), pos + 1)
    fig["attn_self"] = DR.bf16_out_excess(res["attn_self"].view(M, H, 64), ref, vmax)
    # out projection into the residual: the increment
    inc = res["attn_self"].double() @ bf(w["wo"]).T + w["bo"].double()
    fig["x"] = _rel(res["x"].double() - r["x"].double(), inc)
    # the centred bf16 copy and its tile statistics, from the resolved rows the GPU wrote
    # (the shift exactly as the product forms it: mean(bo) summed in double and rounded to f32, added in f32 where the row has one)
    bo_sum = 0.0
    for v in w["bo"].tolist():
        bo_sum += v
    bo_mean = torch.tensor(bo_sum / D, dtype=torch.float64).float()
    sh = torch.where(r["shift"] != 0, r["shift"] + bo_mean, r["shift"]).double()
    c = res["x"].double() - sh[:, None]
    fig["xb"] = float(((res["xb"].double() - c).abs() / c.abs().clamp_min(2.0 ** -126)).max())
    t = c.view(M, D // 16, 16)
    fig["xb_sum"] = float(((res["xb_stats"][..., 0].double() - t.sum(-1)).abs() / t.abs().sum(-1)).max())
    fig["xb_sumsq"] = float(((res["xb_stats"][..., 1].double() - (t * t).sum(-1)).abs() / (t * t).sum(-1)).max())
    # LayerNorm-free query + expansion from xb and its statistics' meaning: LayerNorm of the centred rows
    xbd = res["xb"].double()
    mean = c.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((c - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    wg = bf(w["lnc_g"][None, :] * w["cq_w"])
    cc = w["cq_w"].double() @ w["lnc_b"].double() + w["cq_b"].double()
    q = rstd * (xbd @ wg.T - mean * wg.sum(-1)[None, :]) + cc
    wk = bf(w["ck_w"]).view(H, 64, D)
    fig["xq"] = _rel(res["xq"], torch.einsum("mhd,hdf->mhf", q.view(M, H, 64), wk))
    # streaming kernel + merge + value projection from the expanded query the GPU wrote
    s = torch.einsum("mhf,msf->mhs", res["xq"].double(), xa) * 0.125
    p = torch.softmax(s, dim=-1)
    ctx = torch.einsum("mhs,msf->mhf", p, xa)
    wv = bf(w["cv_w"]).view(H, 64, D)
    cross = torch.einsum("mhf,hdf->mhd", ctx, wv).reshape(M, D) + w["cv_b"].double()
    fig["attn_cross"] = _rel(res["attn_cross"], cross)
    # cross-attention out projection
    fig["co"] = _rel(res["co"], res["attn_cross"].double() @ bf(w["co_w"]).T + w["co_b"].double())
    return fig


def test_against_fp64(ccx_ctx):
    """Bounds.  Self attention: tests/test_dec_attention_gpu.py's (excess over half a bf16 ulp, 1.1e-3 of the head's max |v|).  The two
    linears: tests/test_dec_full_lines_gpu.py::test_against_fp64's 2^-8 + 768 * 2^-24 = 4.0e-3 rel-L2.  xb: one f32 subtraction and a bf16
    rounding -- half a bf16 ulp is 2^-8 of a value at the bottom of its binade -- 2^-8 + 2^-23 relative.  Its statistics: fp32 sums of 16 terms, 16 * 2^-24 of the sum of magnitudes.  xq and the merged value
    projection have no earlier bound: twice what the parent's form (packed = 0) measures on these inputs on an MI355X,
    profiles/dec_mid_chain_measured_deviations.json.  The new forms must meet the same bounds."""
    M, D, S, kv_T = 48, 768, 100, 96
    pos = _pos(M, kv_T)
    measured = json.loads(MEASURED.read_text())
    for packed in (0, 1):
        res, _ = _run(ccx_ctx, M, D, S, kv_T=kv_T, packed=packed, pos=pos)
        fig = _fp64_figures(res, M, D, S, kv_T, pos)
        print(f"mid chain against fp64 (packed {packed}): " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
        what = packed
        within("dec attention: bf16 output, excess over half an ulp / max|v|", fig["attn_self"], 1.1e-3, what)
        assert fig["x"] < 4.0e-3 and fig["co"] < 4.0e-3, (what, fig)
        assert fig["xb"] <= 2.0 ** -8 + 2.0 ** -23, (what, fig)
        assert fig["xb_sum"] <= 2.0 ** -20 and fig["xb_sumsq"] <= 2.0 ** -20, (what, fig)
        within(N_XQ, fig["xq"], 2.0 * measured[N_XQ]["worst"], what)
        within(N_CROSS, fig["attn_cross"], 2.0 * measured[N_CROSS]["worst"], what)


@pytest.mark.parametrize("what,change", [
    ("M = 0", dict(M=0)),
    ("D = 100", dict(D=100)),
    ("H = 6", dict(H=6)),
    ("S = 8", dict(S=8)),
    ("not 16-byte aligned", dict(q_offset=4)),
    ("not 16-byte aligned", dict(x_offset=8)),
    ("not 16-byte aligned", dict(xa_offset=2)),
    ("not 16-byte aligned", dict(self_k_offset=4)),
    ("not 16-byte aligned", dict(shift_offset=4)),
    ("not 16-byte aligned", dict(out_offset=4)),
    ("q_elems", dict(q_elems=10)),
    ("x_elems", dict(x_elems=10)),
    ("kv_elems", dict(kv_elems=10)),
    ("xa_elems", dict(xa_elems=10)),
    ("out_elems", dict(out_elems=10)),
    ("packed = 2", dict(packed=2)),
    ("pos[0] = 96", dict(pos0=96)),
])
def test_rejections(ccx_ctx, what, change):
    from clearconverse_amd import _lib
    lib = _lib.load()
    M, D, S, kv_T = 32, 768, 40, 96
    pos = _pos(M, kv_T)
    out = torch.full((lib.ccx_dec_mid_chain_out_elems(M, D, D // 64),), math.nan, device="cuda")
    used = C.c_int(-1)
    d = _desc(M, D, S, kv_T, pos, 1, out, used)
    for name, val in change.items():
        if name.endswith("_offset"):
            setattr(d, name[:-7], getattr(d, name[:-7]) + val)
        elif name == "pos0":
            pos[0] = val
        else:
            setattr(d, name, val)
    rc = lib.ccx_dec_mid_chain(ccx_ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with pytest.raises(_lib.CcxError) as e:
        ccx_ctx.check(rc, "ccx_dec_mid_chain")
    assert "ccx_dec_mid_chain" in str(e.value) and what in str(e.value), str(e.value)
    assert torch.isnan(out).all() and used.value == -1
