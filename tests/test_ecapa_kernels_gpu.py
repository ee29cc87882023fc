"""GPU: the four ECAPA-TDNN kernels of csrc/ecapa.hip on their own (ccx_ecapa_op) against the fp64 statements of
tests/ecapa_reference.py, on inputs already rounded to bf16: what is measured is the kernel, not the rounding of its inputs.

Row layout (csrc/ecapa.h): crop i owns rows row_off[i] .. row_off[i] + T_i + 8 (4 halo rows, T_i frames, 4 halo rows).  The tests put
two rows of NaN between crops and around them: a read past a halo shows as a wrong value, a write past one as a lost NaN.

Bounds: 2.5 x the deviation measured on an MI355X (ECAPA-TDNN), asserted through tests.conftest.within."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ecapa_reference as R
from tests.conftest import within

pytestmark = pytest.mark.gpu

F = 128          # csrc/ecapa.h ECAPA_R2_TILE
HALO = 4
GAP = 2          # poisoned rows around every crop


def _lib():
    from clearconverse_amd import _lib
    return _lib


def layout(frames):
    """row_off of every crop and the row count, with GAP poisoned rows before, between and after the crops."""
    off, r = [], GAP
    for T in frames:
        off.append(r)
        r += T + 2 * HALO + GAP
    return off, r


def to_rows(crops, off, rows, C_):
    """[T_i, C] tensors -> bf16 [rows, C] device buffer with reflection halos; everything else NaN."""
    buf = torch.full((rows, C_), float("nan"), dtype=torch.float32)
    for x, o in zip(crops, off):
        T = x.shape[0]
        idx = R.reflect_index(torch.arange(-HALO, T + HALO), T)
        buf[o:o + T + 2 * HALO] = x[idx].float()
    return buf.to(torch.bfloat16).cuda()


def poison(rows, C_, dtype=torch.bfloat16):
    return torch.full((rows, C_), float("nan"), dtype=dtype, device="cuda")


def iarr(v):
    return (C.c_int * len(v))(*[int(a) for a in v])


def base_desc(frames, off, rows):
    L = _lib()
    d = L.EcapaDesc()
    d.n, d.rows = len(frames), rows
    d._keep = [iarr(off), iarr(frames)]
    d.row_off, d.frames = d._keep[0], d._keep[1]
    return d


def run(ctx, op, d):
    L = _lib()
    return ctx.lib.ccx_ecapa_op(ctx.handle, op, C.byref(d), L.current_stream_ptr())


def check_rows(y, off, frames, C_, what):
    """Every crop's halo rows mirror its valid rows bit for bit, and no row outside the crops was written."""
    yf = y.float().cpu()
    owned = torch.zeros(y.shape[0], dtype=torch.bool)
    for o, T in zip(off, frames):
        owned[o:o + T + 2 * HALO] = True
        v = yf[o + HALO:o + HALO + T, :C_]
        for j in range(1, HALO + 1):
            assert torch.equal(yf[o + HALO - j, :C_], v[j]), (what, "low halo", j, T)
            assert torch.equal(yf[o + HALO + T - 1 + j, :C_], v[T - 1 - j]), (what, "high halo", j, T)
    assert bool(torch.isnan(yf[~owned]).all()), (what, "a row outside the crops was written")


# ------------------------------------------------------------------------------------------------------------ Res2Net
R2_FRAMES = (5, 6, F - 1, F, F + 1, 2 * F + 3)


def r2_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    w = R.bf16_round(torch.randn(7, 128, 128, 3, generator=g, dtype=torch.float64) * (0.8 / np.sqrt(384)))
    aff = torch.stack([0.1 * torch.randn(7, 128, generator=g), 1 + 0.1 * torch.randn(7, 128, generator=g),
                       0.1 * torch.randn(7, 128, generator=g)], dim=1).float()            # [7][3][128]
    crops = []
    for T in R2_FRAMES:
        x = torch.randn(T, 1024, generator=g, dtype=torch.float64)
        x[0] *= 8.0                      # a large-magnitude row at each crop edge: a wrong reflection index shows
        x[T - 1] *= -8.0
        crops.append(R.bf16_round(x))
    return w, aff, crops


def r2_run(ctx, crops, w, aff, dil):
    L = _lib()
    frames = [c.shape[0] for c in crops]
    off, rows = layout(frames)
    x = to_rows(crops, off, rows, 1024)
    y = poison(rows, 1024)
    d = base_desc(frames, off, rows)
    wf = np.ascontiguousarray(w.float().numpy())
    af = np.ascontiguousarray(aff.numpy())
    d.x, d.x_elems, d.ldx = x.data_ptr(), x.numel(), 1024
    d.y, d.y_elems, d.ldy = y.data_ptr(), y.numel(), 1024
    d.dilation = dil
    d.w_host = wf.ctypes.data_as(C.POINTER(C.c_float))
    d.aff_host = af.ctypes.data_as(C.POINTER(C.c_float))
    ctx.check(run(ctx, L.ECAPA_RES2NET, d), "ccx_ecapa_op(RES2NET)")
    return y, off, frames


@pytest.mark.parametrize("dil", [2, 3, 4])
def test_res2net_against_fp64_batched_and_alone(ccx_ctx, dil):
    w, aff, crops = r2_inputs(100 + dil)
    y, off, frames = r2_run(ccx_ctx, crops, w, aff, dil)
    check_rows(y, off, frames, 1024, f"res2net d{dil}")
    for i, (c, o) in enumerate(zip(crops, off)):
        T = c.shape[0]
        got = y[o + HALO:o + HALO + T].double().cpu()
        ref = R.res2net_ref(c, w, aff, dil)
        assert torch.equal(got[:, :128], c[:, :128]), "chunk 0 is copied through"
        for s in range(1, 8):
            e = R.rel_l2(got[:, 128 * s:128 * (s + 1)], ref[:, 128 * s:128 * (s + 1)])
            print(f"res2net d{dil} T={T} stage {s}: rel-L2 {e:.3e}")
            within(f"ecapa res2net stage {s} rel-L2", e, 2.5 * R2_MEASURED[s], (dil, T))
        # alone: bit for bit what the crop got among its launch mates
        y1, o1, _ = r2_run(ccx_ctx, [c], w, aff, dil)
        assert torch.equal(y1[o1[0]:o1[0] + T + 2 * HALO].view(torch.int16), y[o:o + T + 2 * HALO].view(torch.int16)), (dil, T)


# measured worst rel-L2 per stage over the dilations and crop lengths above (MI355X); the chain rounds each stage's input to bf16
R2_MEASURED = {1: 2.03e-3, 2: 2.56e-3, 3: 2.86e-3, 4: 2.82e-3, 5: 2.66e-3, 6: 2.80e-3, 7: 2.75e-3}


# ------------------------------------------------------------------------------------------------------------ ASP pool
ASP_FRAMES = (15, 17, 16, 33, 200)       # one frame short of and one frame past the 16-frame tiles
ASP_C = 128
ASP_MEASURED = {"mean": 2.94e-3, "std": 1.86e-3}        # MI355X; the output is bf16 (half an ulp: 2^-9 = 1.95e-3)


def test_asp_pool_against_fp64(ccx_ctx):
    L = _lib()
    g = torch.Generator().manual_seed(7)
    hid = [R.bf16_round(torch.rand(T, 128, generator=g, dtype=torch.float64) * 2 - 1) for T in ASP_FRAMES]
    xs = [R.bf16_round(torch.randn(T, ASP_C, generator=g, dtype=torch.float64)) for T in ASP_FRAMES]
    wa = torch.randn(ASP_C, 128, generator=g, dtype=torch.float64) * 1.2          # logits spread over about +-20
    wa[0] = 30.0 * hid[3][7]             # channel 0 of crop 3: one-hot attention on frame 7, the std clamp engages
    wa = R.bf16_round(wa)
    for x in xs:                          # channel 1: large mean, tiny variance (both values exact in bf16): the cancellation case
        x[:, 1] = 1000.0 + 4.0 * (torch.arange(x.shape[0]) % 2)
    ba = torch.randn(ASP_C, generator=g).float()
    sc, sh = (1 + 0.1 * torch.randn(2 * ASP_C, generator=g)).float(), (0.1 * torch.randn(2 * ASP_C, generator=g)).float()
    sc[ASP_C + 1], sh[ASP_C + 1] = 1.0, 0.0
    off, rows = layout(ASP_FRAMES)
    xb, hb = to_rows(xs, off, rows, ASP_C), to_rows(hid, off, rows, 128)
    out = torch.full((len(ASP_FRAMES), 2 * ASP_C), float("nan"), dtype=torch.bfloat16, device="cuda")
    wab, bad, scd, shd = wa.to(torch.bfloat16).cuda(), ba.cuda(), sc.cuda(), sh.cuda()
    d = base_desc(ASP_FRAMES, off, rows)
    d.x, d.x_elems, d.ldx = xb.data_ptr(), xb.numel(), ASP_C
    d.channels, d.hidden, d.hidden_elems = ASP_C, hb.data_ptr(), hb.numel()
    d.wa, d.ba, d.bn_scale, d.bn_shift = wab.data_ptr(), bad.data_ptr(), scd.data_ptr(), shd.data_ptr()
    d.wa_elems, d.ba_elems, d.bn_elems = wab.numel(), ASP_C, 2 * ASP_C
    d.pooled, d.pooled_elems = out.data_ptr(), out.numel()
    ccx_ctx.check(run(ccx_ctx, L.ECAPA_ASP_POOL, d), "ccx_ecapa_op(ASP_POOL)")
    got = out.double().cpu()
    spread = []
    for i, T in enumerate(ASP_FRAMES):
        ref, att = R.asp_pool_ref(hid[i], xs[i], wa, ba, sc, sh, return_attention=True)
        spread.append(float((hid[i] @ wa.T).abs().max()))
        # the output is bf16: the error is taken relative to |ref| + 1 (half an ulp is 2^-9 of it at most)
        em = float(((got[i, :ASP_C] - ref[:ASP_C]).abs() / (ref[:ASP_C].abs() + 1)).max())
        es = float(((got[i, ASP_C:] - ref[ASP_C:]).abs() / (ref[ASP_C:].abs() + 1)).max())
        print(f"asp_pool T={T}: mean err {em:.3e}, std err {es:.3e}")
        within("ecapa asp_pool mean err / (|ref| + 1)", em, 2.5 * ASP_MEASURED["mean"], T)
        within("ecapa asp_pool std err / (|ref| + 1)", es, 2.5 * ASP_MEASURED["std"], T)
        if i == 3:
            assert float(att[:, 0].max()) > 1 - 1e-9                                   # one-hot in the reference
            assert abs(float(got[i, ASP_C]) - float(1e-6 * sc[ASP_C] + sh[ASP_C])) <= 2 ** -8 * abs(float(sh[ASP_C])) + 1e-6
        # cancellation channel: the values are 1000 and 1004, std 2 (up to the attention's weighting)
        rel = abs(float(got[i, ASP_C + 1]) - float(ref[ASP_C + 1])) / float(ref[ASP_C + 1])
        print(f"asp_pool T={T}: cancellation channel std {float(got[i, ASP_C + 1]):.4f} (ref {float(ref[ASP_C + 1]):.4f})")
        assert rel < 2 ** -7, (T, rel)                                                  # one bf16 ulp: nothing is lost to x^2 - mean^2
    assert max(spread) > 20.0


# ------------------------------------------------------------------------------------------------------------ SE
SE_FRAMES = (5, 37, 130)
SE_MEASURED = {"gates": 2.14e-7, "y": 1.69e-3}         # MI355X; gates are fp32, y is bf16


def test_se_against_fp64_ragged(ccx_ctx):
    L = _lib()
    g = torch.Generator().manual_seed(11)
    xs = [R.bf16_round(torch.randn(T, 1024, generator=g, dtype=torch.float64) + 0.5) for T in SE_FRAMES]
    rs = [R.bf16_round(torch.randn(T, 1024, generator=g, dtype=torch.float64)) for T in SE_FRAMES]
    w1 = (torch.randn(128, 1024, generator=g) * (2.0 / 32)).float()
    b1 = (0.1 * torch.randn(128, generator=g)).float()
    w2 = (torch.randn(1024, 128, generator=g) * (1.5 / np.sqrt(128))).float()
    b2 = (0.5 * torch.randn(1024, generator=g)).float()
    off, rows = layout(SE_FRAMES)
    xb, rb = to_rows(xs, off, rows, 1024), to_rows(rs, off, rows, 1024)
    y = poison(rows, 1024)
    gates = torch.full((len(SE_FRAMES), 1024), float("nan"), device="cuda")
    dev = [t.cuda() for t in (w1, b1, w2, b2)]
    d = base_desc(SE_FRAMES, off, rows)
    d.x, d.x_elems, d.ldx = xb.data_ptr(), xb.numel(), 1024
    d.y, d.y_elems, d.ldy = y.data_ptr(), y.numel(), 1024
    d.resid, d.resid_elems, d.ld_resid = rb.data_ptr(), rb.numel(), 1024
    d.w1, d.b1, d.w2, d.b2 = [t.data_ptr() for t in dev]
    d.w1_elems, d.b1_elems, d.w2_elems, d.b2_elems = [t.numel() for t in dev]
    d.gates, d.gates_elems = gates.data_ptr(), gates.numel()
    ccx_ctx.check(run(ccx_ctx, L.ECAPA_SE, d), "ccx_ecapa_op(SE)")
    check_rows(y, off, SE_FRAMES, 1024, "se")
    lo, hi = 1.0, 0.0
    for i, (T, o) in enumerate(zip(SE_FRAMES, off)):
        ref, e = R.se_ref(xs[i], rs[i], w1, b1, w2, b2)
        lo, hi = min(lo, float(e.min())), max(hi, float(e.max()))
        eg = float((gates[i].double().cpu() - e).abs().max())
        ey = R.rel_l2(y[o + HALO:o + HALO + T].double().cpu(), ref)
        print(f"se T={T}: gates max abs err {eg:.3e}, y rel-L2 {ey:.3e}")
        within("ecapa se gates max abs err", eg, 2.5 * SE_MEASURED["gates"], T)
        within("ecapa se y rel-L2", ey, 2.5 * SE_MEASURED["y"], T)
    assert lo < 0.2 and hi > 0.8


# ------------------------------------------------------------------------------------------------------------ front end
FB_MEASURED = {"abs": 3.68e-3}                        # MI355X; fp32 DFT + log10, bf16 output


def test_fbank_against_fp64_ragged_zero_and_minimum(ccx_ctx):
    L = _lib()
    from clearconverse_amd.weights import ecapa_fbank_tables
    tb = ecapa_fbank_tables()
    crops = [R.speechlike(8000, 0), R.speechlike(12345, 1), torch.zeros(9000), R.speechlike(31234, 2)]
    lens = [int(c.numel()) for c in crops]
    frames = [1 + n // 160 for n in lens]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    wav = torch.cat(crops).float().cuda()
    off, rows = layout(frames)
    feats = poison(rows, 80)
    win, fil = tb["fbank.window"].cuda(), tb["fbank.filters"].contiguous().cuda()
    d = base_desc(frames, off, rows)
    ns = iarr(lens)
    d.wav, d.wav_elems = wav.data_ptr(), wav.numel()
    d.offsets, d.n_samples = offs.ctypes.data_as(C.POINTER(C.c_int64)), ns
    d.window, d.window_elems, d.filters, d.filters_elems = win.data_ptr(), 400, fil.data_ptr(), 80 * 201
    d.feats, d.feats_elems = feats.data_ptr(), feats.numel()
    ccx_ctx.check(run(ccx_ctx, L.ECAPA_FBANK, d), "ccx_ecapa_op(FBANK)")
    check_rows(feats, off, frames, 80, "fbank")
    for i, (T, o) in enumerate(zip(frames, off)):
        got = feats[o + HALO:o + HALO + T].double().cpu()
        ref, clamped = R.fbank(crops[i], tb["fbank.window"], tb["fbank.filters"], return_clamped=True)
        if i == 2:
            assert bool((got == 0).all()), "an all-zero crop sits on the 1e-10 floor everywhere: every feature is exactly 0"
            continue
        frac = float(clamped.double().mean())
        assert 0.05 <= frac <= 0.95, frac
        # dB values of tens, stored as bf16: the error is taken relative to |ref| + 1
        e = float(((got - ref).abs() / (ref.abs() + 1)).max())
        print(f"fbank n={lens[i]} T={T}: max err / (|ref| + 1) {e:.3e}, clamped {frac:.2f}")
        within("ecapa fbank max err / (|ref| + 1)", e, 2.5 * FB_MEASURED["abs"], lens[i])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_descriptor_refusals_launch_nothing(ccx_ctx):
    L = _lib()
    w, aff, crops = r2_inputs(5)
    crops = crops[:2]
    frames = [c.shape[0] for c in crops]
    off, rows = layout(frames)
    x = to_rows(crops, off, rows, 1024)
    y = poison(rows, 1024)
    wf, af = np.ascontiguousarray(w.float().numpy()), np.ascontiguousarray(aff.numpy())

    def good():
        d = base_desc(frames, off, rows)
        d.x, d.x_elems, d.ldx = x.data_ptr(), x.numel(), 1024
        d.y, d.y_elems, d.ldy = y.data_ptr(), y.numel(), 1024
        d.dilation = 2
        d.w_host, d.aff_host = wf.ctypes.data_as(C.POINTER(C.c_float)), af.ctypes.data_as(C.POINTER(C.c_float))
        return d

    def refused(d, field, op=None):
        rc = run(ccx_ctx, L.ECAPA_RES2NET if op is None else op, d)
        msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
        assert rc == 1 and "ccx_ecapa_op" in msg and field in msg, (field, rc, msg)
        assert bool(torch.isnan(y.float()).all()), (field, "something was launched")

    d = good(); d._keep[1][0] = 4; refused(d, "frames[0]")
    d = good(); d._keep[0][1] = off[0] + 3; refused(d, "overlap")
    d = good(); d.rows = off[1] + frames[1] + 7; refused(d, "row_off[1]")
    d = good(); d.n = 0; refused(d, "n =")
    d = good(); d.row_off = None; refused(d, "row_off")
    d = good(); d.dilation = 5; refused(d, "dilation")
    d = good(); d.ldx = 1020; refused(d, "ldx")
    d = good(); d.ldy = 512; refused(d, "ldy")
    d = good(); d.x_elems = x.numel() - 1; refused(d, "x_elems")
    d = good(); d.y_elems = y.numel() - 1; refused(d, "y_elems")
    d = good(); d.x = x.data_ptr() + 2; refused(d, "x is not 16-byte aligned")
    d = good(); d.y = None; refused(d, "y is NULL")
    d = good(); d.y = x.data_ptr(); refused(d, "aliases")
    d = good(); d.w_host = None; refused(d, "w_host")
    d = good(); refused(d, "unknown op", op=9)
    # the other ops' own fields
    d = good(); d.ld_resid = 1024; refused(d, "resid", op=L.ECAPA_SE)
    d = good(); d.channels = 65; refused(d, "channels", op=L.ECAPA_ASP_POOL)
    d = good(); d.channels = 64; refused(d, "hidden", op=L.ECAPA_ASP_POOL)
    d = good(); refused(d, "offsets", op=L.ECAPA_FBANK)
    wav = torch.zeros(20000, device="cuda")
    offs = np.zeros(2, dtype=np.int64)
    d = good(); d.wav, d.wav_elems = wav.data_ptr(), wav.numel()
    d.offsets = offs.ctypes.data_as(C.POINTER(C.c_int64))
    ns = iarr([7999, 8000]); d.n_samples = ns; refused(d, "n_samples[0]", op=L.ECAPA_FBANK)
    ns = iarr([8000, 8000]); d.n_samples = ns; refused(d, "frames[0]", op=L.ECAPA_FBANK)      # 5 frames stated, 51 computed
    offs[0] = 12001; refused(d, "offsets[0]", op=L.ECAPA_FBANK)                               # 12001 + 8000 > 20000 samples
