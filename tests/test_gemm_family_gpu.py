"""-m gpu: every epilogue, tap, row-remap and operand-view path of csrc/gemm_bf16.hip, one descriptor feature at a time, through
ccx_gemm_bf16_desc against the fp64 reference of tests/gemm_reference.py (itself checked in tests/test_gemm_reference_cpu.py).

Per destination buffer the comparator asserts
  (a) every element the descriptor does not write (dropped rows, pad rows, columns >= ceil16(N), head rows s >= S, guard rows behind
      the last row) keeps its pre-launch bits;
  (b) every written element: |got - ref| <= ulp + L * E, with E = (Kt + 3) 2^-24 (|A| |W|^T + |bias| + |resid|) the worst-case error
      of an fp32 sum of exact bf16 x bf16 products in any order, L the epilogue's Lipschitz constant (1; max(1, slope) |scale[n]| for
      epilogue 7, plus three roundings of the affine; 1.13 for GELU) and ulp = 2^-8 |ref| for bf16 outputs, 0 for fp32.  Derived, not
      tuned.  The GELU epilogues add GELU_EXCESS (hardware rcp / exp2 and the Abramowitz-Stegun erf), the one measured term;
  (c) aggregate rel-L2 under the project's GEMM bounds: 2e-5 fp32 out, 6e-3 bf16 out.
Which kernel ran (256x64, 128x128, phased 256x256) is asserted from the CCX_PROF_SHAPES label of the launch, so a change of the
dispatcher cannot quietly empty a column of this matrix.
"""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import gemm_reference as R
from tests.conftest import within

pytestmark = pytest.mark.gpu

SENT = -7.0
G64, G128, PH = "256x64", "128x128", "256x256"
# The GELU epilogues' own error (gelu_erf: Abramowitz-Stegun 7.1.26 erf, |error| <= 1.5e-7, through the hardware rcp and exp2) beyond
# L * E.  The rule is 2 x the worst max(|got - ref| - L * E, 0) that epilogue 6 shows over the cases below on the MI355X.  NOT YET
# MEASURED: no GPU run of this file has been made.  Until one is, the bound is the a-priori figure |x| / 2 * (1.5e-7 + 4 * 2^-24) at
# |x| <= 8 (the largest pre-activation these cases produce is < 8): 1.6e-6.  The first GPU session replaces both numbers (every
# case prints its excess; `within` records the worst in measured_deviations.json).
GELU_EXCESS_MEASURED = None
GELU_EXCESS = 1.6e-6


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _bf(x):
    return x.to(torch.bfloat16)


class Case:
    """Host tensors and descriptor of one launch.  `pad` = leading elements in front of a pointer (pointer-offset views)."""

    def __init__(self, d, t, pad=None):
        self.d, self.t, self.pad = d, t, pad or {}


def make(epi, M, N, K, seed, ntaps=1, lda=None, ldw=None, ldo=None, tap_stride=None, remap=None, bias="aligned", a_off=0,
         resid=None, resid_mod=0, ldr=None, resid_bf16=False, ldrb=None, scale=False, shift=False, slope=0.0, guard=2):
    g = torch.Generator().manual_seed(seed)
    taps = max(ntaps, 1)
    lda = K if lda is None else lda
    ldw = taps * K if ldw is None else ldw
    ldo = R.ceil16(N) if ldo is None else ldo
    tap_stride = (lda if tap_stride is None else tap_stride) if ntaps > 1 else 0
    d = dict(epi=epi, M=M, N=N, K=K, lda=lda, ldw=ldw, ldo=ldo, ntaps=ntaps, a_tap_stride=tap_stride, resid_mod=resid_mod, slope=slope)
    d.update(remap or {})
    t = {}
    t["A"] = _bf(torch.randn((M - 1) * lda + (taps - 1) * tap_stride + K, generator=g))
    t["W"] = _bf(torch.randn((N - 1) * ldw + taps * K, generator=g) / math.sqrt(taps * K))
    t["bias"] = None if bias == "none" else torch.randn(N, generator=g)
    orow, keep = R.dest_rows(d)
    rows = int(orow[keep].max()) + 1 + guard                                   # guard rows behind the last destination row
    f32 = epi in R.F32_OUT
    if resid == "inplace":
        assert f32 and ldr in (None, ldo) and not resid_mod
        d["ldr"] = ldo
        t["out"] = torch.randn(rows * ldo, generator=g)
        t["resid"] = t["out"]
    else:
        t["out"] = torch.full((rows * ldo,), SENT, dtype=torch.float32 if f32 else torch.bfloat16)
        if resid == "separate":
            d["ldr"] = R.ceil16(N) if ldr is None else ldr
            t["resid"] = torch.randn((resid_mod if resid_mod > 0 else rows) * d["ldr"], generator=g)
    if resid_bf16:
        d["ldrb"] = R.ceil16(N) if ldrb is None else ldrb
        t["resid_bf16"] = _bf(torch.randn(rows * d["ldrb"], generator=g))
    if scale:
        t["scale"] = torch.randn(N, generator=g) * 1.5                        # both signs
    if shift:
        t["shift"] = torch.randn(N, generator=g)
    pad = {}
    if a_off:
        pad["A"] = a_off
    if bias == "offset":
        pad["bias"] = 1                                                        # 4 bytes off a 16-byte boundary: the scalar bias branch
    return Case(d, t, pad)


def make_heads(B, S, Spad, d_model, n_head, K, first_block, v_transposed, seed):
    g = torch.Generator().manual_seed(seed)
    nblk = 3 - first_block
    M, N = B * S, nblk * d_model
    d = dict(epi=R.EPI_HEADS, M=M, N=N, K=K, lda=K, ldw=K, d_model=d_model, n_head=n_head, S=S, Spad=Spad, first_block=first_block,
             v_transposed=v_transposed)
    t = dict(A=_bf(torch.randn(M * K, generator=g)), W=_bf(torch.randn(N * K, generator=g) / math.sqrt(K)), bias=torch.randn(N, generator=g))
    for name in ("hq", "hk", "hv")[first_block:]:
        t[name] = torch.full((B * n_head * Spad * 64 + 128,), SENT, dtype=torch.bfloat16)      # 128 guard elements
    return Case(d, t)


def fill_desc(case, dev):
    from clearconverse_amd._lib import GemmDesc
    d, t = case.d, case.t
    desc = GemmDesc()
    for f in R.FIELDS:
        setattr(desc, f, d.get(f, 0))

    def ptr(name):
        x = dev.get(name)
        return None if x is None else x.data_ptr() + case.pad.get(name, 0) * x.element_size()

    for name in ("A", "W", "bias", "out", "resid", "scale", "shift", "resid_bf16", "hq", "hk", "hv"):
        setattr(desc, name, ptr(name))
    n = lambda name: 0 if t.get(name) is None else t[name].numel()
    desc.a_elems, desc.w_elems, desc.out_elems = n("A"), n("W"), n("out")
    desc.resid_elems, desc.resid_bf16_elems = n("resid"), n("resid_bf16")
    desc.heads_elems = max(n("hq"), n("hk"), n("hv"))
    return desc


def upload(case):
    dev = {}
    for name, x in case.t.items():
        if x is None:
            continue
        if name == "resid" and x is case.t.get("out"):
            continue
        p = case.pad.get(name, 0)
        dev[name] = torch.cat([torch.zeros(p, dtype=x.dtype), x]).cuda() if p else x.cuda()
    if case.t.get("resid") is not None and case.t["resid"] is case.t.get("out"):
        dev["resid"] = dev["out"]                                               # in place
    return dev


def launch(ccx_ctx, case, dev):
    """-> the tile geometry that ran ("256x64" / "128x128" / "256x256")."""
    desc = fill_desc(case, dev)
    old = os.environ.get("CCX_PROF_SHAPES")
    os.environ["CCX_PROF_SHAPES"] = "1"
    ccx_ctx.prof_enable(True)
    try:
        ccx_ctx.check(ccx_ctx.lib.ccx_gemm_bf16_desc(ccx_ctx.handle, case.d["epi"], C.byref(desc), _stream()), "ccx_gemm_bf16_desc")
        torch.cuda.synchronize()
        recs = ccx_ctx.prof_records()
    finally:
        ccx_ctx.prof_enable(False)
        if old is None:
            del os.environ["CCX_PROF_SHAPES"]
        else:
            os.environ["CCX_PROF_SHAPES"] = old
    assert len(recs) == 1, recs
    m = re.match(r"gemm<epi(\d+),(\d+x\d+)> M=(\d+) N=(\d+) K=(\d+) taps=(\d+)", recs[0][0])
    assert m, recs[0][0]
    assert (int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5))) == (case.d["epi"], case.d["M"], case.d["N"], case.d["K"])
    return m.group(2)


def run(ccx_ctx, case, geometry, tag):
    exp = R.gemm_reference(case.d, case.t)
    dev = upload(case)
    geo = launch(ccx_ctx, case, dev)
    assert geo == geometry, f"{tag}: the dispatcher ran {geo}, this case is meant for {geometry}"
    epi = case.d["epi"]
    gelu = GELU_EXCESS if epi in (R.EPI_BF16_GELU, R.EPI_F32_GELU_POS) else 0.0
    for name, e in exp.items():
        p = case.pad.get(name, 0)
        got = dev[name].cpu()[p:]
        v = R.compare(e, got, gelu)
        print(f"{tag} [{name}] {geo}: rel-L2 {v.rel_l2:.3e}  worst error/allowance {v.worst_ratio:.3f}  excess over L*E {v.excess:.3e}")
        assert v.ok, (tag, name, v.reason)
        if epi == R.EPI_F32_GELU_POS:
            within("gemm epi6: gelu approximation excess", v.excess, GELU_EXCESS, tag)
        if e["bf16"]:
            within("gemm family (descriptor tests): bf16 out rel-L2", v.rel_l2, 6e-3, tag)
        else:
            within("gemm family (descriptor tests): fp32 out rel-L2", v.rel_l2, 2e-5, tag)
        within("gemm family (descriptor tests): worst element error / derived allowance", v.worst_ratio, 1.0, tag)


# geometry -> (M, N) that reaches it with the fewest rows
SHAPES = {G64: (300, 64), G128: (300, 192), PH: (14336, 1024)}
VIEWS = {
    "lda>K": dict(lda=104),
    "lda<K": dict(K=320, lda=64),                        # overlapping rows (the x-vector's TDNN input)
    "A+8": dict(a_off=8),
    "ldw>K": dict(ldw=136),
    "ldo>N": dict(ldo_extra=48),
    "null-bias": dict(bias="none"),
    "bias+1": dict(bias="offset"),
}


@pytest.mark.parametrize("epi", [0, 3])
@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("geometry", [G64, G128, PH])
def test_operand_views(ccx_ctx, geometry, view, epi):
    M, N = SHAPES[geometry]
    kw = dict(VIEWS[view])
    K = kw.pop("K", 64)
    if "ldo_extra" in kw:
        kw["ldo"] = N + kw.pop("ldo_extra")
    run(ccx_ctx, make(epi, M, N, K, seed=list(VIEWS).index(view) * 31 + epi + N, **kw), geometry, f"view {view} epi{epi}")


@pytest.mark.parametrize("epi", [0, 3])
@pytest.mark.parametrize("M,N,ldo,geometry", [(200, 3, 16, G64), (200, 7, 128, G64), (200, 60, 64, G64), (200, 72, 80, G128),
                                              (200, 1500, 1536, G128), (200, 1104, 1104, G128), (9728, 1500, 1536, PH),
                                              (11520, 1104, 1104, PH)])
def test_ragged_n(ccx_ctx, M, N, ldo, geometry, epi):
    run(ccx_ctx, make(epi, M, N, 64, seed=N + epi, ldo=ldo), geometry, f"ragged N={N} epi{epi}")


@pytest.mark.parametrize("epi", [0, 3])
@pytest.mark.parametrize("N,geometry", [(48, G64), (144, G128)])
@pytest.mark.parametrize("M", [1, 15, 17, 129, 255, 257])
def test_ragged_m(ccx_ctx, M, N, geometry, epi):
    run(ccx_ctx, make(epi, M, N, 128, seed=M + N + epi), geometry, f"ragged M={M} epi{epi}")


@pytest.mark.parametrize("epi", [0, 3])
def test_ragged_m_phased(ccx_ctx, epi):
    run(ccx_ctx, make(epi, 14336 + 37, 1024, 64, seed=37 + epi), PH, f"ragged M phased epi{epi}")


# level 1 alone: groups of 58 rows, 30 kept, written 32 apart from row 33; both levels: images of 31 groups, 30 kept, 32 apart
REMAP1 = dict(rpb_in=58, rpb_valid=30, rpb_out=32, roff=33)
REMAP2 = dict(REMAP1, img_rows_in=31, img_rows_valid=30, img_rows_out=32)
IMG = 31 * 58


def _taps_cases():
    out = []
    for geometry in (G64, G128):
        for K in (64, 192):
            for wide in (False, True):
                for remap in (False, True):
                    out.append((geometry, 3, K, wide, remap))
    out += [(G128, 5, 64, False, False), (G128, 5, 64, True, True)]
    out += [(PH, 3, 64, False, False), (PH, 3, 64, True, True), (PH, 3, 192, True, False), (PH, 3, 192, False, True)]
    return out


@pytest.mark.parametrize("geometry,ntaps,K,wide,remap", _taps_cases())
def test_taps(ccx_ctx, geometry, ntaps, K, wide, remap):
    """ntaps x K: one K tile per tap (K = 64) and three (K = 192); a_tap_stride equal to the row pitch and a whole group of rows (58
    rows, as a convolution's next image row); with and without the row remap behind it."""
    M, N = SHAPES[geometry]
    if remap:
        M = 5 * 58 + 13 if geometry != PH else 8 * IMG          # a ragged last group / whole images
    lda = K + 8 if wide else K
    stride = 58 * lda if wide else lda
    rm = None if not remap else (REMAP2 if geometry == PH else REMAP1)
    epi = 0 if remap else 3
    run(ccx_ctx, make(epi, M, N, K, seed=ntaps * K + wide + 2 * remap, ntaps=ntaps, lda=lda, tap_stride=stride, remap=rm), geometry,
        f"taps={ntaps} K={K} stride={'group' if wide else 'row'} remap={remap}")


@pytest.mark.parametrize("epi", [0, 1, 5, 8])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("geometry", [G64, G128])
def test_remap(ccx_ctx, geometry, levels, epi):
    _, N = SHAPES[geometry]
    N -= 4                                                      # ragged N under the remap: 60 and 188
    M = 5 * 58 + 13 if levels == 1 else 2 * IMG + 3 * 58 + 5    # a ragged last group / a ragged last image
    run(ccx_ctx, make(epi, M, N, 64, seed=levels * 10 + epi, remap=REMAP1 if levels == 1 else REMAP2, resid_bf16=epi == 8), geometry,
        f"remap levels={levels} epi{epi}")


def test_remap_taps_add_relu_phased(ccx_ctx):
    """A ResNet convolution's whole descriptor on the phased kernel: three taps a padded image row apart, both remap levels, bf16
    residual read at the destination row."""
    run(ccx_ctx, make(8, 16 * IMG, 1024, 64, seed=8, ntaps=3, tap_stride=58 * 64, remap=REMAP2, resid_bf16=True), PH, "conv-like phased epi8")


@pytest.mark.parametrize("geometry", [G64, G128, PH])
def test_resid_in_place(ccx_ctx, geometry):
    M, N = SHAPES[geometry]
    run(ccx_ctx, make(2, M, N, 64, seed=2 + N, resid="inplace"), geometry, "epi2 in place")


def test_resid_in_place_phased_ragged_m(ccx_ctx):
    """Full 256-row tiles fetch the residual through the LDS, the last (ragged) row tile through registers."""
    run(ccx_ctx, make(2, 14336 + 37, 1024, 128, seed=22, resid="inplace"), PH, "epi2 in place, ragged M")


def test_resid_mod_phased(ccx_ctx):
    """resid_mod > 0 on full tiles of the phased kernel: the LDS path (which fetches row m) must not be taken."""
    run(ccx_ctx, make(2, 14336, 1024, 64, seed=23, resid="separate", resid_mod=100), PH, "epi2 resid_mod=100 phased")


@pytest.mark.parametrize("geometry", [G64, G128])
@pytest.mark.parametrize("resid_mod", [30, 7])
def test_gelu_pos(ccx_ctx, resid_mod, geometry):
    """Epilogue 6 as Whisper's conv2 uses it: groups of 31 rows, the last of each dropped, residual row = destination row modulo
    resid_mod (the group length, and a length that divides nothing)."""
    _, N = SHAPES[geometry]
    rm = dict(rpb_in=31, rpb_valid=30, rpb_out=30, roff=0)
    run(ccx_ctx, make(6, 9 * 31, N, 192, seed=6 + resid_mod, lda=128, remap=rm, resid="separate", resid_mod=resid_mod), geometry,
        f"epi6 resid_mod={resid_mod}")


@pytest.mark.parametrize("slope", [0.01, 0.0])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("resid", ["separate", None])
def test_lrelu_affine(ccx_ctx, resid, affine, slope):
    run(ccx_ctx, make(7, 300, 144, 128, seed=7 + affine + 2 * (resid is None), resid=resid, scale=affine, shift=affine, slope=slope), G128,
        f"epi7 resid={resid} affine={affine} slope={slope}")


@pytest.mark.parametrize("geometry,M,N,ldo", [(G64, 300, 60, 64), (PH, 14336, 1024, 1024), (G128, 200, 1500, 1536)])
def test_lrelu_affine_geometries(ccx_ctx, geometry, M, N, ldo):
    run(ccx_ctx, make(7, M, N, 64, seed=70 + N, ldo=ldo, resid="separate", ldr=ldo, scale=True, shift=True, slope=0.01), geometry,
        f"epi7 all terms N={N}")


@pytest.mark.parametrize("geometry,N,ldo,ldrb", [(G64, 60, 64, 72), (G128, 72, 80, 96)])
@pytest.mark.parametrize("resid", [True, False])
def test_add_relu(ccx_ctx, resid, geometry, N, ldo, ldrb):
    run(ccx_ctx, make(8, 300, N, 64, seed=80 + N + resid, ldo=ldo, resid_bf16=resid, ldrb=ldrb), geometry, f"epi8 resid={resid} N={N}")


@pytest.mark.parametrize("first_block,v_transposed", [(0, 1), (1, 0)])
def test_heads(ccx_ctx, first_block, v_transposed):
    run(ccx_ctx, make_heads(3, 100, 128, 128, 2, 128, first_block, v_transposed, seed=40 + first_block), G128,
        f"heads first_block={first_block} v_transposed={v_transposed}")


def test_heads_phased(ccx_ctx):
    run(ccx_ctx, make_heads(13, 1500, 1536, 256, 4, 256, 0, 1, seed=44), PH, "heads phased")


# ---- rejections: return codes only, nothing is launched ---------------------------------------------------------------------------
def _refused(ccx_ctx, case, fragment, dev=None, edit=None):
    dev = dev or upload(case)
    desc = fill_desc(case, dev)
    if edit:
        edit(desc)
    rc = ccx_ctx.lib.ccx_gemm_bf16_desc(ccx_ctx.handle, case.d["epi"], C.byref(desc), _stream())
    msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
    assert rc != 0 and fragment in msg, (rc, msg)
    torch.cuda.synchronize()


def _small(epi, **kw):
    return make(epi, 40, 24, 64, seed=1, **kw)


def test_rejects_misaligned_resid(ccx_ctx):
    _refused(ccx_ctx, _small(2, resid="separate"), "resid must be 16-byte aligned", edit=lambda d: setattr(d, "resid", d.resid + 4))


def test_rejects_misaligned_resid_bf16(ccx_ctx):
    _refused(ccx_ctx, _small(8, resid_bf16=True), "resid_bf16 must be 16-byte aligned", edit=lambda d: setattr(d, "resid_bf16", d.resid_bf16 + 2))


def test_rejects_misaligned_out(ccx_ctx):
    _refused(ccx_ctx, _small(0), "out must be 16-byte aligned", edit=lambda d: setattr(d, "out", d.out + 2))


def test_rejects_misaligned_heads(ccx_ctx):
    _refused(ccx_ctx, make_heads(1, 8, 8, 128, 2, 64, 1, 0, seed=1), "not 16-byte aligned", edit=lambda d: setattr(d, "hv", d.hv + 8))


def test_rejects_ldr_not_multiple_of_4(ccx_ctx):
    _refused(ccx_ctx, _small(2, resid="separate", ldr=34), "ldr=34 must be a multiple of 4")


def test_rejects_ldr_short_of_ceil16_n(ccx_ctx):
    # N = 24: the epilogue loads float4s up to column 32; a tight ldr = 24 makes the last row read past the buffer
    for epi in (2, 6, 7):
        _refused(ccx_ctx, _small(epi, resid="separate", ldr=24), "ldr=24 must be a multiple of 4 and cover N rounded up to 16")


def test_rejects_ldrb_not_multiple_of_8(ccx_ctx):
    _refused(ccx_ctx, _small(8, resid_bf16=True, ldrb=36), "ldrb=36 must be a multiple of 8")


def test_rejects_ldrb_short_of_ceil16_n(ccx_ctx):
    _refused(ccx_ctx, _small(8, resid_bf16=True, ldrb=24), "ldrb=24 must be a multiple of 8 and cover N rounded up to 16")


def test_rejects_negative_resid_mod(ccx_ctx):
    _refused(ccx_ctx, _small(2, resid="separate"), "resid_mod", edit=lambda d: setattr(d, "resid_mod", -1))


def test_rejects_resid_mod_on_epilogues_that_ignore_it(ccx_ctx):
    _refused(ccx_ctx, _small(7, resid="separate"), "resid_mod is honoured by epilogues 2 and 6 only", edit=lambda d: setattr(d, "resid_mod", 8))


def test_rejects_missing_resid(ccx_ctx):
    _refused(ccx_ctx, _small(6, resid="separate"), "epilogue 6 needs resid", edit=lambda d: setattr(d, "resid", None))


@pytest.mark.parametrize("valid", [0, 59])
def test_rejects_bad_rpb_valid(ccx_ctx, valid):
    _refused(ccx_ctx, make(0, 116, 24, 64, seed=1, remap=REMAP1, guard=64), "0 < rpb_valid <= rpb_in", edit=lambda d: setattr(d, "rpb_valid", valid))


@pytest.mark.parametrize("valid", [0, 32])
def test_rejects_bad_img_rows_valid(ccx_ctx, valid):
    _refused(ccx_ctx, make(0, IMG, 24, 64, seed=1, remap=REMAP2, guard=64), "0 < img_rows_valid <= img_rows_in", edit=lambda d: setattr(d, "img_rows_valid", valid))


@pytest.mark.parametrize("field,buffer", [("a_elems", "A is read"), ("w_elems", "W is read"), ("out_elems", "out is written"),
                                          ("resid_elems", "resid is read"), ("resid_bf16_elems", "resid_bf16 is read")])
def test_rejects_descriptor_past_a_buffer(ccx_ctx, field, buffer):
    """The extent check of ccx_gemm_bf16_desc, tight to the element: the exact need passes (every other test), one less is refused."""
    if field == "resid_bf16_elems":
        case = make(8, 5 * 58, 24, 64, seed=1, ntaps=3, tap_stride=72, remap=REMAP1, resid_bf16=True)
    else:
        case = make(2, 5 * 58, 24, 64, seed=1, ntaps=3, tap_stride=72, remap=REMAP1, resid="separate", resid_mod=50)
    d = case.d
    orow, keep = R.dest_rows(d)
    last = int(orow[keep].max())
    need = {"a_elems": (d["M"] - 1) * d["lda"] + 2 * 72 + 64, "w_elems": 23 * d["ldw"] + 3 * 64, "out_elems": last * d["ldo"] + 32,
            "resid_elems": 49 * d.get("ldr", 0) + 32, "resid_bf16_elems": last * d.get("ldrb", 0) + 32}[field]
    _refused(ccx_ctx, case, buffer, edit=lambda x: setattr(x, field, need - 1))


def test_rejects_heads_past_the_destination(ccx_ctx):
    case = make_heads(2, 8, 16, 128, 2, 64, 0, 0, seed=1)
    _refused(ccx_ctx, case, "hq/hk/hv are written", edit=lambda d: setattr(d, "heads_elems", 2 * 2 * 16 * 64 - 1))
