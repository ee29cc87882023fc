"""GPU: the kernels of csrc/speaker.hip on their own (ccx_speaker_op) against the fp64 statements of tests/speaker_reference.py, on
inputs already rounded the way the kernels see them: what is measured is the kernel, not the rounding of its inputs.

Poison.  Every output buffer is pre-filled with a NaN bit pattern and must come back with exactly those bits outside what the op may
write (rows between crops, columns past the live ones).  Every input is NaN outside what the op may read: samples after a crop's end
and between crops, rows between crops, input rows past 3 n_out of a crop for pool = 3, columns past C, gx rows past a sequence,
weights between weight rows.  A read of any of them shows as a NaN in the output.  All ragged cases run batched and alone, and the
results must be bit-equal.

Bounds.  The sinc bound is derived (speaker_reference.sinc_bound) and asserted elementwise as a ratio < 1; the LSTM conditions are
set, not measured.  The other bounds are 2 x the deviation measured on an MI355X, as literals below.  Every
parity assertion goes through tests.conftest.within."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import speaker_reference as S
from tests.conftest import within

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = 0x7FC1                    # a quiet-NaN bf16 bit pattern (fits int16)
NAN = float("nan")


def _lib():
    from clearconverse_amd import _lib
    return _lib


def run(ctx, op, d):
    return ctx.lib.ccx_speaker_op(ctx.handle, op, C.byref(d), _lib().current_stream_ptr())


def iarr(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def larr(v):
    return (C.c_int64 * len(v))(*[int(x) for x in v])


def fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def sentinel_bf16(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def f32_bits(t):
    return t.contiguous().view(torch.int32).cpu()


def rows_layout(counts, gap=3, first=2):
    """Row offsets of crops with `counts` rows each, `gap` unused rows between them -> (offsets, total rows)."""
    off, pos = [], first
    for c in counts:
        off.append(pos)
        pos += c + gap
    return off, pos


def wav_layout(waves):
    """The crops at odd sample positions of one NaN-filled buffer, NaN between them and after the last -> (wav cuda, offsets)."""
    off, pos = [], 1
    for w in waves:
        off.append(pos)
        pos += w.numel() + 12
        pos += 1 - pos % 2
    buf = torch.full((pos + 64,), NAN)
    for o, w in zip(off, waves):
        assert o % 2 == 1
        buf[o:o + w.numel()] = w
    return buf.cuda(), off


# ------------------------------------------------------------------------------------------------------------ waveform statistics
# Worst relative error of a and c against fp64 over the lengths below, measured on an MI355X.  Bounds: 2 x these.
WAV_MEASURED = {"plain": {"a": 7.862e-8, "c": 3.108e-7}, "dc": {"a": 4.919e-8, "c": 9.377e-8}}
WAV_LENGTHS = (251, 255, 256, 257, 2047, 2048, 2049, 4099, 31234)


def wav_stats_run(ctx, waves, sel=None):
    L = _lib()
    sel = list(range(len(waves))) if sel is None else sel
    wav, off = wav_layout(waves)
    out = torch.full((len(sel) + 1, 4), NAN, device="cuda")
    d = L.SpeakerDesc()
    d.n, d.wav, d.wav_elems = len(sel), wav.data_ptr(), wav.numel()
    d.crop_off, d.crop_len = larr([off[i] for i in sel]), iarr([waves[i].numel() for i in sel])
    d.norm_w, d.norm_b = S.NORM_W, S.NORM_B
    d.out, d.out_elems = out.data_ptr(), 4 * len(sel)
    ctx.check(run(ctx, L.SPEAKER_WAV_STATS, d), "ccx_speaker_op(WAV_STATS)")
    assert bool(torch.isnan(out[-1]).all()), "a row past the last crop was written"
    return out[:-1]


@pytest.mark.parametrize("variant", ["plain", "dc", "zeros"])
def test_wav_stats_against_fp64(ccx_ctx, variant):
    kind = {"plain": "zero-mean", "dc": "dc 0.5 std 1e-3", "zeros": "silence"}[variant]
    waves = [S.sinc_wave(kind, n, n) for n in WAV_LENGTHS]
    got = wav_stats_run(ccx_ctx, waves)
    assert bool(torch.isfinite(got).all())
    for i, w in enumerate(waves):
        alone = wav_stats_run(ccx_ctx, waves, [i])
        assert torch.equal(f32_bits(alone[0]), f32_bits(got[i])), (variant, w.numel(), "a crop's result depends on its launch mates")
    g = got.double().cpu()
    for i, w in enumerate(waves):
        a, c, mean = S.wav_stats(w, S.NORM_W, S.NORM_B)
        if variant == "zeros":
            want = S.NORM_W / math.sqrt(float(np.float32(1e-5)))                # a = w rsqrt(0 + 1e-5), c = b - 0 a
            assert abs(float(g[i, 0]) / want - 1) <= 3 * 2.0 ** -23            # rsqrtf within 2 ulp, one product
            assert float(g[i, 1]) == float(np.float32(S.NORM_B)) and float(g[i, 2]) == 0.0 and float(g[i, 3]) == 0.0
            continue
        ea, ec = abs(float(g[i, 0]) / a - 1), abs(float(g[i, 1]) / c - 1)
        em = abs(float(g[i, 2]) + float(g[i, 3]) - mean)                     # the mean is carried as mean_hi + mean_lo
        print(f"wav stats {variant} n={w.numel()}: rel err a {ea:.3e}, c {ec:.3e}, mean abs err {em:.3e}")
        within(f"speaker wav stats rel err of a ({variant})", ea, 2 * WAV_MEASURED[variant]["a"], w.numel())
        within(f"speaker wav stats rel err of c ({variant})", ec, 2 * WAV_MEASURED[variant]["c"], w.numel())
        # mean_lo is a sum of deviations d = x - mean_hi (each rounded once) in 8 x 256 partials of at most 16 terms, 11 more additions
        # and a division: under 32 roundings of at most 2^-24 mean |d| each
        assert em <= 2.0 ** -19 * float((w.double() - float(g[i, 2])).abs().mean())


# ------------------------------------------------------------------------------------------------------------ sinc stage
def sinc_run(ctx, crops, filt, sel=None):
    """-> [out rows of crop i] (device f32 [n_pool][80]) for the crops in `sel`, launched together."""
    L = _lib()
    sel = list(range(len(crops))) if sel is None else sel
    waves, frames = [crops[i][0] for i in sel], [crops[i][1] for i in sel]
    wav, off = wav_layout(waves)
    row_off, rows = rows_layout(frames)
    out = torch.full((rows, S.NF), NAN, device="cuda")
    fh = np.ascontiguousarray(filt.numpy(), dtype=np.float32)
    d = L.SpeakerDesc()
    d.n, d.wav, d.wav_elems = len(sel), wav.data_ptr(), wav.numel()
    d.crop_off, d.crop_len = larr(off), iarr([w.numel() for w in waves])
    d.norm_w, d.norm_b, d.filters_host = S.NORM_W, S.NORM_B, fptr(fh)
    d.frames, d.out_off, d.out, d.out_elems = iarr(frames), iarr(row_off), out.data_ptr(), out.numel()
    ctx.check(run(ctx, L.SPEAKER_SINC_POOL, d), "ccx_speaker_op(SINC_POOL)")
    written = torch.zeros(rows, dtype=torch.bool)
    for o, f in zip(row_off, frames):
        written[o:o + f] = True
    host = out.cpu()
    assert bool(torch.isnan(host[~written]).all()), "a row outside the crops was written"
    assert bool(torch.isfinite(host[written]).all()), "a value outside a crop was read, or a row was not written"
    return [out[o:o + f] for o, f in zip(row_off, frames)]


_SINC = {}


def sinc_result(ctx, filters, inputs):
    """(got, ref, bound) per crop of the ragged batch, fp64; batched and alone runs are compared on the way."""
    key = (filters, inputs)
    if key not in _SINC:
        filt = S.sinc_filter_bank(filters)
        crops = S.sinc_crops(inputs)
        got = sinc_run(ctx, crops, filt)
        for i in range(len(crops)):
            alone = sinc_run(ctx, crops, filt, [i])[0]
            assert torch.equal(f32_bits(alone), f32_bits(got[i])), (key, crops[i][1], "a crop's result depends on its launch mates")
        refs = [S.sinc_stage(x, filt, S.NORM_W, S.NORM_B, p) for x, p in crops]
        _SINC[key] = ([g.double().cpu() for g in got], [r[0] for r in refs], [r[1] for r in refs])
    return _SINC[key]


@pytest.mark.parametrize("inputs", S.SINC_INPUTS)
@pytest.mark.parametrize("filters", S.SINC_FILTERS)
def test_sinc_pool_against_fp64(ccx_ctx, filters, inputs):
    """|got - ref| <= |a| (3 2^-18 + 272 2^-24) sum |x_k w_k| + 2^-22 (|a conv| + |c sum w|) per position (derivation:
    speaker_reference.sinc_bound), carried through |.| and the max-pool; pooled frames 1 .. 257 per crop cover the 16-frame wave and the
    128-frame work item boundaries, the sample counts leave 0, 1 and 2 unpooled positions and a ragged tail."""
    got, ref, bound = sinc_result(ccx_ctx, filters, inputs)
    for g, r, b, p in zip(got, ref, bound, S.SINC_FRAMES):
        ratio = (g - r).abs() / b
        print(f"sinc {filters} / {inputs}, {p} frames: worst err / bound {float(ratio.max()):.3f}, last frame {float(ratio[-1].max()):.3f}")
        within(f"speaker sinc err / bound ({filters} filters)", float(ratio.max()), 1.0, (filters, inputs, p))


def test_sinc_tap_locator_pins_every_k_step(ccx_ctx):
    """Filter f is a unit impulse at tap k_f: the output is max_r |a x[10 (3 i + r) + k_f] + c|, gathered here without a convolution.
    Taps 0, 29 | 30, 31 (the two zero-weight k slots follow tap 29 of every step), 239 | 240 and 250 (the last live tap of the ninth
    step) sit in every 16-filter tile."""
    got, _, bound = sinc_result(ccx_ctx, "tap locator", "zero-mean")
    taps = torch.tensor([S.locator_tap(f) for f in range(S.NF)])
    assert all(set(S.LOCATOR_TAPS) <= set(taps[16 * t:16 * t + 16].tolist()) for t in range(5))
    for (x, p), g, b in zip(S.sinc_crops("zero-mean"), got, bound):
        a, c, _ = S.wav_stats(x, S.NORM_W, S.NORM_B)
        pos = 10 * torch.arange(3 * p)[:, None] + taps[None, :]                     # [positions][80]
        want = (a * x.double()[pos] + c).abs().reshape(p, 3, S.NF).max(dim=1).values
        ratio = (g - want).abs() / b
        within("speaker sinc err / bound (tap locator, gathered)", float(ratio.max()), 1.0, p)


def test_sinc_pool_grid_stride_loop(ccx_ctx):
    """130 crops of 129 frames are 260 work items for 256 persistent blocks: four blocks restage their samples for a second item."""
    filt = S.sinc_filter_bank("mel")
    crops = S.sinc_grid_crops()
    assert len(crops) * -(-129 // 128) > 256
    got = sinc_run(ccx_ctx, crops, filt)
    for i in (0, 127, 128, 129):
        alone = sinc_run(ccx_ctx, crops, filt, [i])[0]
        assert torch.equal(f32_bits(alone), f32_bits(got[i])), (i, "a crop's result depends on its launch mates")
    worst = 0.0
    for (x, p), g in zip(crops, got):
        r, b = S.sinc_stage(x, filt, S.NORM_W, S.NORM_B, p)
        worst = max(worst, float(((g.double().cpu() - r).abs() / b).max()))
    print(f"sinc, 130 crops of 129 frames: worst err / bound {worst:.3f}")
    within("speaker sinc err / bound (mel filters)", worst, 1.0, "260 work items")


@pytest.mark.parametrize("filters", S.SINC_FILTERS)
def test_sinc_dc_offset_costs_no_precision(ccx_ctx, filters):
    """Worst error over output rms under a DC offset stays within 4 x the zero-mean case's of the same run on the same filters."""
    rel = {}
    for inputs in S.SINC_INPUTS[:3]:
        got, ref, _ = sinc_result(ccx_ctx, filters, inputs)
        rel[inputs] = max(float((g - r).abs().max() / r.pow(2).mean().sqrt()) for g, r in zip(got, ref))
    print(f"sinc {filters}: worst err / output rms {rel}")
    # zero-mean: the split arithmetic in torch (tests/test_speaker_reference_cpu.py) gives 1.5e-5 to 2.1e-5; 1e-4 is 5 x that
    within(f"speaker sinc worst err / output rms ({filters} filters, zero-mean)", rel["zero-mean"], 1e-4)
    for inputs in S.SINC_INPUTS[1:3]:
        within(f"speaker sinc worst err / output rms ({filters} filters, {inputs}), bound 4 x zero-mean's", rel[inputs], 4 * rel["zero-mean"])
        within(f"speaker sinc err / rms under DC over zero-mean's ({filters} filters)", rel[inputs] / rel["zero-mean"], 4.0, inputs)


# ------------------------------------------------------------------------------------------------------------ instance norm
# Worst |err| / (|ref| + 1) over every case below, measured on an MI355X; the output is bf16, whose rounding (2^-9 relative) is most of
# it.  "offset": the channel with mean 100 and spread 0.1.  Bounds: 2 x these.
INORM_MEASURED = {"plain": 2.972e-3, "offset": 2.489e-3}
INORM_N = (1, 2, 5, 15, 16, 17, 33, 127, 129, 1000)
INORM_CONST = 3.0


def inorm_inputs(pool, Cn, ld_in):
    """[(rows f32 [pool n + pool - 1][ld_in], n)]: channel 1 has mean 100 and spread 0.1, channel 2 is constant, columns past C are NaN,
    the last pool - 1 rows (which a pool reading one frame too many would touch) are NaN."""
    g = torch.Generator().manual_seed(10 * pool + Cn)
    out = []
    for n in INORM_N:
        x = torch.randn(pool * n, Cn, generator=g) * (0.5 + torch.rand(Cn, generator=g)) + torch.randn(Cn, generator=g)
        x[:, 1] = 100.0 + 0.1 * torch.randn(pool * n, generator=g)
        x[:, 2] = INORM_CONST
        full = torch.full((pool * n + pool - 1, ld_in), NAN)
        full[:pool * n, :Cn] = x
        out.append((full, n))
    return out


def inorm_run(ctx, crops, pool, Cn, ld_in, ld_out, gamma, beta, sel=None):
    L = _lib()
    sel = list(range(len(crops))) if sel is None else sel
    frames = [crops[i][1] for i in sel]
    in_off, in_rows = rows_layout([crops[i][0].shape[0] for i in sel], gap=2)
    out_off, out_rows = rows_layout(frames, gap=2, first=1)
    xin = torch.full((in_rows, ld_in), NAN)
    for o, i in zip(in_off, sel):
        xin[o:o + crops[i][0].shape[0]] = crops[i][0]
    xin = xin.cuda()
    out = sentinel_bf16(out_rows, ld_out)
    gd, bd = gamma.cuda(), beta.cuda()
    d = L.SpeakerDesc()
    d.n, d.pool, d.C, d.frames = len(sel), pool, Cn, iarr(frames)
    d.in_, d.in_elems, d.ld_in, d.in_off = xin.data_ptr(), xin.numel(), ld_in, iarr(in_off)
    d.out, d.out_elems, d.ld_out, d.out_off = out.data_ptr(), out.numel(), ld_out, iarr(out_off)
    d.gamma, d.gamma_elems, d.beta, d.beta_elems = gd.data_ptr(), Cn, bd.data_ptr(), Cn
    ctx.check(run(ctx, L.SPEAKER_INORM, d), "ccx_speaker_op(INORM)")
    written = torch.zeros(out_rows, dtype=torch.bool)
    for o, f in zip(out_off, frames):
        written[o:o + f] = True
    assert bool((bits(out)[~written] == SENTINEL).all()), "a row outside the crops was written"
    return [out[o:o + f] for o, f in zip(out_off, frames)]


@pytest.mark.parametrize("pool,Cn,ld_in,ld_out", [(1, 80, 80, 80), (3, 60, 128, 64)])
def test_inorm_against_fp64(ccx_ctx, pool, Cn, ld_in, ld_out):
    g = torch.Generator().manual_seed(Cn)
    gamma, beta = (1 + 0.1 * torch.randn(Cn, generator=g)).float(), (0.1 * torch.randn(Cn, generator=g)).float()
    beta[2] = -0.3                                                          # the constant channel shows the negative slope
    crops = inorm_inputs(pool, Cn, ld_in)
    got = inorm_run(ccx_ctx, crops, pool, Cn, ld_in, ld_out, gamma, beta)
    const = S.bf16_round((torch.tensor(0.01) * beta[2]).double())               # fp32 product, then bf16
    for i, ((x, n), o) in enumerate(zip(crops, got)):
        alone = inorm_run(ccx_ctx, crops, pool, Cn, ld_in, ld_out, gamma, beta, [i])[0]
        assert torch.equal(bits(alone), bits(o)), (pool, n, "a crop's result depends on its launch mates")
        h = o.double().cpu()
        assert bool(torch.isfinite(h).all()), (pool, n, "a value outside the crop was read")
        assert bool((bits(o)[:, Cn:] == 0).all()), (pool, n, "pad channels must be exact zeros")
        ref = S.inorm(x[:, :Cn], gamma, beta, pool, n)
        dev = (h[:, :Cn] - ref).abs() / (ref.abs() + 1)
        plain = torch.ones(Cn, dtype=torch.bool)
        plain[1] = False
        print(f"inorm pool {pool} n_out={n}: plain {float(dev[:, plain].max()):.3e}, offset channel {float(dev[:, 1].max()):.3e}")
        within("speaker inorm |err| / (|ref| + 1)", float(dev[:, plain].max()), 2 * INORM_MEASURED["plain"], (pool, n))
        within("speaker inorm |err| / (|ref| + 1), channel with mean 100, spread 0.1", float(dev[:, 1].max()), 2 * INORM_MEASURED["offset"], (pool, n))
        assert bool((h[:, 2] == const).all()), (pool, n, "a constant channel must give LeakyReLU(beta) exactly")
        if n == 1:                                                          # one frame: every channel is constant
            want = S.bf16_round(torch.nn.functional.leaky_relu(beta, 0.01).double())
            assert torch.equal(h[0, :Cn], want), pool


# ------------------------------------------------------------------------------------------------------------ statistics pooling
# Worst distance of the fp64 mean / std from the values that round to the kernel's bf16 output (speaker_reference.bf16_excess: what
# the one output rounding, at most 2^-8 |ref|, does not explain), measured on an MI355X.  Bounds: 2 x these.
POOL_MEASURED = {"mean": 2.109e-8, "std": 1.469e-7}
POOL_C, POOL_LD, POOL_LDO = 1500, 1536, 3072
POOL_N = (2, 3, 14, 133)


def pool_inputs():
    """{n: x bf16-valued fp64 [n][1500]}"""
    g = torch.Generator().manual_seed(15)
    return {n: S.bf16_round(torch.randn(n, POOL_C, generator=g, dtype=F64) + 0.5 * torch.randn(1, POOL_C, generator=g, dtype=F64)) for n in POOL_N}


def pool_run(ctx, xs, cases, sel=None):
    """cases: [(n, weights fp32 [n_w] or None)] -> out rows bf16 [len(sel)][3072]."""
    L = _lib()
    sel = list(range(len(cases))) if sel is None else sel
    off, rows = rows_layout([n for n in POOL_N])
    xin = torch.full((rows, POOL_LD), NAN, dtype=F64)
    for o, n in zip(off, POOL_N):
        xin[o:o + n, :POOL_C] = xs[n]
    xin = xin.to(torch.bfloat16).cuda()
    where = dict(zip(POOL_N, off))
    out = sentinel_bf16(len(sel) + 1, POOL_LDO)
    d = L.SpeakerDesc()
    d.n, d.C, d.frames = len(sel), POOL_C, iarr([cases[i][0] for i in sel])
    d.in_, d.in_elems, d.ld_in, d.in_off = xin.data_ptr(), xin.numel(), POOL_LD, iarr([where[cases[i][0]] for i in sel])
    d.out, d.out_elems, d.ld_out = out.data_ptr(), len(sel) * POOL_LDO, POOL_LDO
    if cases[sel[0]][1] is not None:
        w_off, pos = [], 3
        for i in sel:
            w_off.append(pos)
            pos += cases[i][1].numel() + 5
        wbuf = torch.full((pos,), NAN)
        for o, i in zip(w_off, sel):
            wbuf[o:o + cases[i][1].numel()] = cases[i][1]
        wd = wbuf.cuda()
        d.weights, d.weights_elems, d.w_off, d.w_len = wd.data_ptr(), wd.numel(), larr(w_off), iarr([cases[i][1].numel() for i in sel])
    ctx.check(run(ctx, L.SPEAKER_STATS_POOL, d), "ccx_speaker_op(STATS_POOL)")
    b = bits(out)
    assert bool((b[-1] == SENTINEL).all()) and bool((b[:, 2 * POOL_C:] == SENTINEL).all()), "a cell outside mean || std was written"
    return out[:-1]


def pool_check(ctx, xs, cases, names):
    got = pool_run(ctx, xs, cases)
    for i, ((n, w), name) in enumerate(zip(cases, names)):
        alone = pool_run(ctx, xs, cases, [i])
        assert torch.equal(bits(alone[0]), bits(got[i])), (name, "a crop's result depends on its launch mates")
    h = got.double().cpu()[:, :2 * POOL_C]
    assert bool(torch.isfinite(h).all()), "a value outside a crop was read"
    for i, ((n, w), name) in enumerate(zip(cases, names)):
        ref = S.pool_stats(xs[n], w)
        ex = S.bf16_excess(h[i], ref)
        em, es = float(ex[:POOL_C].max()), float(ex[POOL_C:].max())
        print(f"stats pool {name}: beyond the output rounding, mean {em:.3e}, std {es:.3e}")
        within("speaker stats pool mean, beyond the output rounding", em, 2 * POOL_MEASURED["mean"], name)
        within("speaker stats pool std, beyond the output rounding", es, 2 * POOL_MEASURED["std"], name)
    return h


def test_stats_pool_unweighted_is_the_unbiased_std(ccx_ctx):
    xs = pool_inputs()
    pool_check(ccx_ctx, xs, [(n, None) for n in POOL_N], [f"unweighted n={n}" for n in POOL_N])


def test_stats_pool_weighted_against_fp64(ccx_ctx):
    from tests.resnet_reference import nearest_index_exact
    assert not np.array_equal(nearest_index_exact(14, 62), S.nearest_index(14, 62).numpy())      # the two index maps differ here
    xs = pool_inputs()
    g = torch.Generator().manual_seed(16)
    cases, names = [], []
    for n in POOL_N:
        for nw in sorted({1, n, 2 * n, 589, 62}):
            idx = S.nearest_index(n, nw)
            binary = (torch.rand(nw, generator=g) > 0.5).float()
            binary[idx[0]] = binary[idx[n - 1]] = 1.0
            cases += [(n, binary), (n, 0.05 + 0.95 * torch.rand(nw, generator=g))]
            names += [f"binary n={n} n_w={nw}", f"soft n={n} n_w={nw}"]
    h = pool_check(ccx_ctx, xs, cases, names)
    assert h.shape[0] == 2 * sum(len({1, n, 2 * n, 589, 62}) for n in POOL_N)
    # all-zero weights: mean 0 and std 0; one live weight read by one frame: that frame's value and std 0 (1 + 1e-8 is 1 in fp32)
    cases, names = [], []
    for n in POOL_N:
        onehot = torch.zeros(2 * n)
        onehot[2 * (n // 2)] = 1.0                                          # frame t reads weight 2 t
        assert (S.nearest_index(n, 2 * n) == 2 * (n // 2)).nonzero().flatten().tolist() == [n // 2]
        cases += [(n, torch.zeros(n)), (n, onehot)]
        names += [f"zero weights n={n}", f"one live frame n={n}"]
    got = pool_run(ccx_ctx, xs, cases).double().cpu()[:, :2 * POOL_C]
    for i, (n, _) in enumerate(cases):
        if i % 2 == 0:
            assert bool((got[i] == 0).all()), names[i]
        else:
            assert torch.equal(got[i, :POOL_C], xs[n][n // 2]) and bool((got[i, POOL_C:] == 0).all()), names[i]


# ------------------------------------------------------------------------------------------------------------ LSTM
# Regime (a), W_hh = 0: worst distance of the fp64 h from the values that round to the kernel's bf16 output (bf16_excess), measured on an
# MI355X: the gate arithmetic (exp2 / rcp builtins over common denominators) alone.  Bound: 2 x this.
LSTM_GATES_MEASURED = 2.796e-8
LSTM_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 37)


def lstm_batches():
    """Lists of (sequence id, length).  Crop counts 1, 15, 16, 17 and 37; in the 16-crop batches the longest sequence sits in each of the
    four accumulator row groups (rows 4 q .. 4 q + 3) in turn, among shorter ones."""
    cyc = lambda n, s: [(k + s, LSTM_LENGTHS[(k + s) % len(LSTM_LENGTHS)]) for k in range(n)]
    out = [[(k, L)] for k, L in enumerate(LSTM_LENGTHS)] + [cyc(15, 0), cyc(17, 3), cyc(37, 5)]
    for q in range(4):
        b = [(100 + 16 * q + k, LSTM_LENGTHS[k % 8]) for k in range(16)]        # lengths 1 .. 9
        b[4 * q + 1] = (100 + 16 * q + 4 * q + 1, 37)
        out.append(b)
    return out


def lstm_gx(regime, sid, length):
    g = torch.Generator().manual_seed(1000 * sid + length)
    if regime == "saturated":
        return 40.0 * torch.sign(torch.randn(length, 1024, generator=g))
    return (2.0 if regime == "gates" else 1.0) * torch.randn(length, 1024, generator=g)


def lstm_whh(regime):
    if regime != "recurrent":
        return torch.zeros(2, 512, 128)
    return (0.8 / math.sqrt(128)) * torch.randn(2, 512, 128, generator=torch.Generator().manual_seed(77))


def lstm_run(ctx, regime, batch):
    """-> [h bf16 [length][256]] (device) per sequence of the batch."""
    L = _lib()
    lens = [b[1] for b in batch]
    off, rows = rows_layout(lens, gap=2)
    gx = torch.full((rows, 1024), NAN)
    for o, (sid, n) in zip(off, batch):
        gx[o:o + n] = lstm_gx(regime, sid, n)
    gxd = gx.cuda()
    out = sentinel_bf16(rows, 256)
    wh = np.ascontiguousarray(lstm_whh(regime).numpy(), dtype=np.float32)
    d = L.SpeakerDesc()
    d.n, d.frames, d.whh_host = len(batch), iarr(lens), fptr(wh)
    d.in_, d.in_elems, d.in_off = gxd.data_ptr(), gxd.numel(), iarr(off)
    d.out, d.out_elems, d.out_off = out.data_ptr(), out.numel(), iarr(off)
    ctx.check(run(ctx, L.SPEAKER_LSTM, d), "ccx_speaker_op(LSTM)")
    written = torch.zeros(rows, dtype=torch.bool)
    for o, n in zip(off, lens):
        written[o:o + n] = True
    assert bool((bits(out)[~written] == SENTINEL).all()), "a row outside the sequences was written"
    return [out[o:o + n] for o, n in zip(off, lens)]


_LSTM_ALONE, _LSTM_REF = {}, {}


def lstm_results(ctx, regime, batches):
    """Yields (got fp64 [length][256], ref) per sequence of every batch; a sequence's bits must not depend on its batch."""
    whh = lstm_whh(regime)
    for batch in batches:
        got = lstm_run(ctx, regime, batch)
        for (sid, n), h in zip(batch, got):
            key = (regime, sid, n)
            if key not in _LSTM_ALONE:
                _LSTM_ALONE[key] = bits(h) if len(batch) == 1 else bits(lstm_run(ctx, regime, [(sid, n)])[0])
                _LSTM_REF[key] = S.lstm(lstm_gx(regime, sid, n), whh, round_h=regime == "recurrent")
            assert torch.equal(bits(h), _LSTM_ALONE[key]), (key, len(batch), "a sequence's result depends on its block mates")
            hd = h.double().cpu()
            assert bool(torch.isfinite(hd).all()), (key, "a gx row outside the sequence was read")
            yield key, hd, _LSTM_REF[key]


def test_lstm_gate_arithmetic(ccx_ctx):
    """(a) W_hh = 0: h follows from gx alone (c' = s(f) c + s(i) tanh(g), h = s(o) tanh(c')), both directions, every length and batch."""
    for key, got, ref in lstm_results(ccx_ctx, "gates", lstm_batches()):
        within("speaker lstm gates (W_hh = 0): |h - fp64| beyond the output rounding", float(S.bf16_excess(got, ref).max()), 2 * LSTM_GATES_MEASURED, key)


def test_lstm_saturated_gates(ccx_ctx):
    """(b) gx = +-40, W_hh = 0: the clamp of the exponents at +-25 costs less than 1e-9 (stated in fp64 here, the bf16 output cannot
    show it), and the kernel stays within the bound of (a)."""
    batch = lstm_batches()[-1]
    for key, got, ref in lstm_results(ccx_ctx, "saturated", [batch]):
        _, sid, n = key
        clamped = S.lstm(lstm_gx("saturated", sid, n), lstm_whh("saturated"), round_h=False, clamp=25.0)
        assert float((clamped - ref).abs().max()) < 1e-9
        within("speaker lstm gates (W_hh = 0): |h - fp64| beyond the output rounding", float(S.bf16_excess(got, ref).max()), 2 * LSTM_GATES_MEASURED, key)


def test_lstm_recurrence_against_fp64_contract(ccx_ctx):
    """(c) W_hh ~ N(0, 0.8^2 / 128), gx ~ N(0, 1): every output within two bf16 spacings of the fp64 run of the kernel's contract
    (speaker_reference.bf16_ulps), at most 1 % of the outputs different from it at all.  An fp32 run of the contract differs from the
    fp64 one in 0.09 % of the outputs at 37 steps (tests/test_speaker_reference_cpu.py).  Measured on an MI355X: worst distance 1 spacing,
    0.044 % of the outputs differ."""
    differ = total = 0
    for key, got, ref in lstm_results(ccx_ctx, "recurrent", lstm_batches()):
        within("speaker lstm: worst |h - contract| in bf16 spacings", float(S.bf16_ulps(got, ref).max()), 2.0 + 1e-9, key)
        differ, total = differ + int((S.bf16_order(got) != S.bf16_order(ref)).sum()), total + got.numel()
    print(f"lstm recurrence: {differ} of {total} outputs differ from the fp64 contract")
    within("speaker lstm: share of outputs that differ from the fp64 contract", differ / total, 0.01)


# ------------------------------------------------------------------------------------------------------------ activation
# Worst abs error against fp64 (log-softmax of logits up to +-100, sigmoid), measured on an MI355X.  Bounds: 2 x these.
ACT_MEASURED = {"log-softmax": 1.142e-5, "sigmoid": 8.848e-8}


@pytest.mark.parametrize("powerset", [True, False])
def test_activation_against_fp64(ccx_ctx, powerset):
    L = _lib()
    name = "log-softmax" if powerset else "sigmoid"
    for Cn in (1, 3, 7, 64):
        for rows in (1, 255, 256, 257):
            g = torch.Generator().manual_seed(100 * Cn + rows)
            x = torch.full((rows, 128), NAN)
            x[:, :Cn] = 3.0 * torch.randn(rows, Cn, generator=g)
            big = torch.rand(rows, Cn, generator=g)
            x[:, :Cn][big < 0.05] = 100.0
            x[:, :Cn][big > 0.95] = -100.0
            x[0, 0], x[rows - 1, Cn - 1] = 100.0, -100.0
            xd = x.cuda()
            out = torch.full((rows + 1, Cn), NAN, device="cuda")
            d = L.SpeakerDesc()
            d.rows, d.C, d.powerset = rows, Cn, 1 if powerset else 0
            d.in_, d.in_elems, d.ld_in, d.out, d.out_elems = xd.data_ptr(), xd.numel(), 128, out.data_ptr(), rows * Cn
            ccx_ctx.check(run(ccx_ctx, L.SPEAKER_ACTIVATION, d), "ccx_speaker_op(ACTIVATION)")
            assert bool(torch.isnan(out[-1]).all()), "a row past the last was written"
            got = out[:-1].double().cpu()
            assert bool(torch.isfinite(got).all()), (Cn, rows)
            e = float((got - S.activation(x[:, :Cn], powerset)).abs().max())
            print(f"activation {name} C={Cn} rows={rows}: max abs err {e:.3e}")
            within(f"speaker activation max abs err ({name})", e, 2 * ACT_MEASURED[name], (Cn, rows))
            if not powerset:
                assert bool((got[x[:, :Cn] == 100.0] == 1.0).all()) and bool((got[x[:, :Cn] == -100.0] == 0.0).all())


# ------------------------------------------------------------------------------------------------------------ refusals
def test_descriptor_refusals_launch_nothing(ccx_ctx):
    L = _lib()
    keep = []

    def dev(t):
        keep.append(t.cuda())
        return keep[-1]

    def refused(op, d, field, outs):
        rc = run(ccx_ctx, op, d)
        msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
        assert rc == 1 and "ccx_speaker_op" in msg and field in msg, (field, rc, msg)
        for o in outs:
            poison = torch.isnan(o).all() if o.dtype == torch.float32 else (bits(o) == SENTINEL).all()
            assert bool(poison), (field, "something was launched")

    wav = dev(0.1 * torch.randn(5000))
    filt = np.ascontiguousarray(S.sinc_filter_bank("dense").numpy())
    whh = np.zeros(2 * 512 * 128, dtype=np.float32)
    out32 = dev(torch.full((4096,), NAN))
    out16 = sentinel_bf16(1 << 16)
    rows32 = dev(torch.randn(64, 128))
    rows16 = dev(torch.randn(64, 1536).to(torch.bfloat16))
    gx = dev(torch.randn(16, 1024))
    gb = dev(torch.ones(128))
    wts = dev(torch.ones(64))

    def sinc_desc():
        d = L.SpeakerDesc()
        d.n, d.wav, d.wav_elems, d.crop_off, d.crop_len = 2, wav.data_ptr(), wav.numel(), larr([1, 2001]), iarr([1000, 2999])
        d.norm_w, d.norm_b, d.filters_host = 1.0, 0.0, fptr(filt)
        d.frames, d.out_off, d.out, d.out_elems = iarr([25, 91]), iarr([0, 25]), out32.data_ptr(), 116 * 80
        return d

    def inorm_desc():
        d = L.SpeakerDesc()
        d.n, d.pool, d.C, d.frames = 2, 3, 60, iarr([5, 4])
        d.in_, d.in_elems, d.ld_in, d.in_off = rows32.data_ptr(), rows32.numel(), 128, iarr([0, 20])
        d.out, d.out_elems, d.ld_out, d.out_off = out16.data_ptr(), 9 * 64, 64, iarr([0, 5])
        d.gamma, d.gamma_elems, d.beta, d.beta_elems = gb.data_ptr(), 60, gb.data_ptr(), 60
        return d

    def pool_desc():
        d = L.SpeakerDesc()
        d.n, d.C, d.frames = 2, 1500, iarr([14, 20])
        d.in_, d.in_elems, d.ld_in, d.in_off = rows16.data_ptr(), rows16.numel(), 1536, iarr([0, 30])
        d.out, d.out_elems, d.ld_out = out16.data_ptr(), 2 * 3072, 3072
        d.weights, d.weights_elems, d.w_off, d.w_len = wts.data_ptr(), 64, larr([0, 2]), iarr([2, 62])
        return d

    def lstm_desc():
        d = L.SpeakerDesc()
        d.n, d.frames, d.whh_host = 2, iarr([7, 5]), fptr(whh)
        d.in_, d.in_elems, d.in_off = gx.data_ptr(), gx.numel(), iarr([0, 9])
        d.out, d.out_elems, d.out_off = out16.data_ptr(), 16 * 256, iarr([0, 9])
        return d

    def act_desc():
        d = L.SpeakerDesc()
        d.rows, d.C, d.powerset = 64, 7, 1
        d.in_, d.in_elems, d.ld_in, d.out, d.out_elems = rows32.data_ptr(), rows32.numel(), 128, out32.data_ptr(), 64 * 7
        return d

    makers = {L.SPEAKER_SINC_POOL: sinc_desc, L.SPEAKER_INORM: inorm_desc, L.SPEAKER_STATS_POOL: pool_desc, L.SPEAKER_LSTM: lstm_desc,
              L.SPEAKER_ACTIVATION: act_desc}
    for op, make in makers.items():                                          # the descriptors the refusals below vary are accepted
        ccx_ctx.check(run(ccx_ctx, op, make()), f"ccx_speaker_op({op})")
    d = sinc_desc(); d.out_elems = 8
    ccx_ctx.check(run(ccx_ctx, L.SPEAKER_WAV_STATS, d), "ccx_speaker_op(WAV_STATS)")
    out32.fill_(NAN)
    out16.view(torch.int16).fill_(SENTINEL)
    outs = [out32, out16]

    def vary(op, field, change):
        d = makers[op]()
        change(d)
        refused(op, d, field, outs)

    S_, I_, P_, R_, A_ = L.SPEAKER_SINC_POOL, L.SPEAKER_INORM, L.SPEAKER_STATS_POOL, L.SPEAKER_LSTM, L.SPEAKER_ACTIVATION
    # the waveform ops
    for op in (L.SPEAKER_WAV_STATS, S_):
        d = sinc_desc(); d.wav = None; refused(op, d, "wav is NULL", outs)
        d = sinc_desc(); d.wav = wav.data_ptr() + 2; refused(op, d, "wav is NULL or not 4-byte aligned", outs)
        d = sinc_desc(); d.wav_elems = 4999; refused(op, d, "wav_elems", outs)
        d = sinc_desc(); d.crop_len = iarr([250, 2999]); refused(op, d, "crop_len[0]", outs)
        d = sinc_desc(); d.crop_off = larr([-1, 2001]); refused(op, d, "crop 0", outs)
        d = sinc_desc(); d.crop_off = None; refused(op, d, "crop_off", outs)
        d = sinc_desc(); d.n = 0; refused(op, d, "n = 0", outs)
        d = sinc_desc(); d.out = None; refused(op, d, "out is NULL", outs)
        d = sinc_desc(); d.out = out32.data_ptr() + 4; refused(op, d, "out is not 16-byte aligned", outs)
    d = sinc_desc(); d.out_elems = 7; refused(L.SPEAKER_WAV_STATS, d, "out_elems", outs)
    vary(S_, "out_elems", lambda d: setattr(d, "out_elems", 116 * 80 - 1))
    vary(S_, "filters_host", lambda d: setattr(d, "filters_host", None))
    vary(S_, "frames is NULL", lambda d: setattr(d, "frames", None))
    vary(S_, "frames[0]", lambda d: setattr(d, "frames", iarr([26, 91])))       # 1000 samples hold 25 pooled frames
    vary(S_, "frames[1]", lambda d: setattr(d, "frames", iarr([25, 0])))
    vary(S_, "out_off is NULL", lambda d: setattr(d, "out_off", None))
    vary(S_, "out_off[1]", lambda d: setattr(d, "out_off", iarr([0, -1])))
    # instance norm
    vary(I_, "pool = 2", lambda d: setattr(d, "pool", 2))
    vary(I_, "C = 62", lambda d: setattr(d, "C", 62))
    vary(I_, "C = 132", lambda d: setattr(d, "C", 132))
    vary(I_, "ld_in", lambda d: setattr(d, "ld_in", 56))                        # C > ld
    vary(I_, "ld_out", lambda d: setattr(d, "ld_out", 56))
    vary(I_, "ld_out", lambda d: setattr(d, "ld_out", 132))
    vary(I_, "frames[1]", lambda d: setattr(d, "frames", iarr([5, 0])))         # n_out = 0
    vary(I_, "in_elems", lambda d: setattr(d, "in_elems", 32 * 128 - 1))        # crop 1 reads rows 20 .. 31
    vary(I_, "out_elems", lambda d: setattr(d, "out_elems", 9 * 64 - 1))
    vary(I_, "in is NULL", lambda d: setattr(d, "in_", None))
    vary(I_, "in is not 16-byte aligned", lambda d: setattr(d, "in_", rows32.data_ptr() + 4))
    vary(I_, "out is not 16-byte aligned", lambda d: setattr(d, "out", out16.data_ptr() + 2))
    vary(I_, "gamma is NULL", lambda d: setattr(d, "gamma", None))
    vary(I_, "beta_elems", lambda d: setattr(d, "beta_elems", 59))
    vary(I_, "in_off is NULL", lambda d: setattr(d, "in_off", None))
    vary(I_, "in_off[0]", lambda d: setattr(d, "in_off", iarr([-3, 20])))
    # statistics pooling
    vary(P_, "C = 0", lambda d: setattr(d, "C", 0))
    vary(P_, "ld_in", lambda d: setattr(d, "ld_in", 1499))
    vary(P_, "ld_out", lambda d: setattr(d, "ld_out", 2999))
    vary(P_, "in_elems", lambda d: setattr(d, "in_elems", 49 * 1536 + 1499))
    vary(P_, "out_elems", lambda d: setattr(d, "out_elems", 3072 + 2999))
    vary(P_, "weights_elems", lambda d: setattr(d, "weights_elems", 63))
    vary(P_, "w_len[0]", lambda d: setattr(d, "w_len", iarr([0, 62])))
    vary(P_, "w_off[1]", lambda d: setattr(d, "w_off", larr([0, -2])))
    vary(P_, "without w_off or w_len", lambda d: setattr(d, "w_len", None))
    vary(P_, "weights is not 16-byte aligned", lambda d: setattr(d, "weights", wts.data_ptr() + 4))

    def unweighted_one_frame(d):
        d.weights, d.frames = None, iarr([14, 1])
    vary(P_, "frames[1]", unweighted_one_frame)
    # LSTM
    vary(R_, "whh_host", lambda d: setattr(d, "whh_host", None))
    vary(R_, "in_elems", lambda d: setattr(d, "in_elems", 14 * 1024 - 1))
    vary(R_, "out_elems", lambda d: setattr(d, "out_elems", 14 * 256 - 1))
    vary(R_, "out_off[1]", lambda d: setattr(d, "out_off", iarr([0, 8])))
    vary(R_, "frames[0]", lambda d: setattr(d, "frames", iarr([0, 5])))
    vary(R_, "n = 70000", lambda d: setattr(d, "n", 70000))
    # activation
    vary(A_, "rows = 0", lambda d: setattr(d, "rows", 0))
    vary(A_, "C = 0", lambda d: setattr(d, "C", 0))
    vary(A_, "ld_in", lambda d: setattr(d, "ld_in", 6))
    vary(A_, "in_elems", lambda d: setattr(d, "in_elems", 63 * 128 + 6))
    vary(A_, "out_elems", lambda d: setattr(d, "out_elems", 64 * 7 - 1))
    # an unknown op, no descriptor
    refused(6, act_desc(), "unknown op 6", outs)
    refused(-1, act_desc(), "unknown op -1", outs)
    rc = ccx_ctx.lib.ccx_speaker_op(ccx_ctx.handle, 0, None, L.current_stream_ptr())
    assert rc == 1 and "desc is NULL" in ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
