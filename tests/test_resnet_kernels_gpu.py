"""GPU: the kernels of csrc/resnet.hip on their own (ccx_resnet_op) against the fp64 statements of tests/resnet_reference.py, on
inputs already rounded the way the kernels see them: what is measured is the kernel, not the rounding of its inputs.

Layout: activations are padded NHWC bf16 [chunk][H + 2][W + 2][C].  Outputs are pre-filled with a NaN bit pattern (SENTINEL): the
kernels write interior cells only, so every halo cell must come back with exactly those bits.  Convolution inputs carry the read
slack of the strided GEMM view behind the last chunk, filled with large finite values: the rows that read it are dropped, so the
result must not depend on it (NaN would poison a dropped row's products with zero weights, which is the test's fault, not the
kernel's).

Bounds.  The convolution, conv1 and linear bounds are derived (bf16 output rounding + fp32 accumulation, see
resnet_reference.conv_bound) and asserted elementwise as a ratio < 1.  The fbank and pooling bounds are <= 2 x the deviation
measured on an MI355X.  Every parity assertion goes through tests.conftest.within."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import resnet_reference as R
from tests.conftest import within

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1                    # a quiet-NaN bf16 bit pattern (fits int16)
SENTINEL_F32 = float("nan")
BIG = 3.0e4


def _lib():
    from clearconverse_amd import _lib
    return _lib


def run(ctx, op, d):
    L = _lib()
    return ctx.lib.ccx_resnet_op(ctx.handle, op, C.byref(d), L.current_stream_ptr())


def fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def sentinel_bf16(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


# ------------------------------------------------------------------------------------------------------------ fbank
# Worst |log mel - fp64| and |fmean - fp64| over every T below, measured on an MI355X: the "dc" variant (samples near 16384 after
# scaling: the rounding of the fp32 frame mean leaks into the lowest bins) and the other three variants.  A CPU float32 emulation of
# the same pipeline (fp32 framing, torch.fft.rfft in fp32, fp32 mel sum and log) gave 4.8e-4 / 9.7e-5 ("dc") and 6.8e-6 / 4.1e-6 ("plain") on the
# same inputs.  Bounds: 2 x the measured values.
FB_MEASURED = {"dc": {"logmel": 3.958e-4, "fmean": 4.672e-5}, "other": {"logmel": 1.545e-5, "fmean": 5.187e-6}}
FB_T = (1, 3, 4, 33, 130)


@pytest.mark.parametrize("variant", R.FBANK_VARIANTS)
def test_fbank_against_fp64(ccx_ctx, variant):
    L = _lib()
    log_eps = math.log(R.FLT_EPSILON)
    for T in FB_T:
        waves = R.fbank_test_waves(T, variant)
        n = waves.shape[1]
        stride = n + 123                                               # stride > n_samples: the gap is never read
        buf = torch.full((2, stride), 1.0e3)
        buf[:, :n] = waves
        wav = buf.cuda()
        feats = torch.full((2, 80, T), SENTINEL_F32, device="cuda")
        fmean = torch.full((2, 80), SENTINEL_F32, device="cuda")
        d = L.ResnetDesc()
        d.n_chunks, d.wav, d.wav_elems, d.stride, d.n_samples = 2, wav.data_ptr(), wav.numel(), stride, n
        d.feats_t, d.feats_t_elems, d.fmean, d.fmean_elems = feats.data_ptr(), feats.numel(), fmean.data_ptr(), fmean.numel()
        ccx_ctx.check(run(ccx_ctx, L.RESNET_FBANK, d), "ccx_resnet_op(FBANK)")
        got, gm = feats.double().cpu(), fmean.double().cpu()
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gm).all())
        for c in range(2):
            E = R.mel_energies(waves[c])
            assert bool((E >= 1e-5 * E.max(dim=1, keepdim=True).values).all()), "a compared value would be FFT leakage"
            ref = R.fbank(waves[c]).T                                  # [80][T]
            e = float((got[c] - ref).abs().max())
            em = float((gm[c] - ref.mean(dim=1)).abs().max())
            print(f"fbank {variant} T={T} chunk {c}: log-mel max abs err {e:.3e}, fmean max abs err {em:.3e}")
            kind = "dc" if variant == "dc" else "other"
            within(f"resnet fbank log-mel max abs err ({kind})", e, 2 * FB_MEASURED[kind]["logmel"], (variant, T, c))
            within(f"resnet fbank fmean max abs err ({kind})", em, 2 * FB_MEASURED[kind]["fmean"], (variant, T, c))
            if variant == "leading zeros":
                zero = [t for t in range(T) if 160 * t + 400 <= int(0.4 * n)]   # frames wholly inside the zeros
                assert (len(zero) > 0) == (T >= 33)
                for t in zero:
                    assert float((got[c, :, t] - log_eps).abs().max()) <= 1e-6, (T, c, t)


# ------------------------------------------------------------------------------------------------------------ conv1
@pytest.mark.parametrize("T", [2, 255, 256, 300])
def test_conv1_against_fp64(ccx_ctx, T):
    """9 multiply-adds, the mean subtraction and the bias per output, in fp32, then bf16: 2^-8 |ref| + 11 2^-23 abs_sum."""
    L = _lib()
    g = torch.Generator().manual_seed(T)
    feats = (3.0 * torch.randn(2, 80, T, generator=g) - 8.0).float()
    fmean = (feats.mean(dim=2) + 0.37 * torch.randn(2, 80, generator=g)).float()        # nonzero, and not the rows' own mean
    w = (0.3 * torch.randn(32, 9, generator=g)).float()
    b = (0.2 * torch.randn(32, generator=g)).float()
    ref, a = R.conv1(feats, fmean, w, b)
    for edge in (ref[:, :, 0, :], ref[:, :, 79, :], ref[:, :, :, 0], ref[:, :, :, T - 1]):
        assert float((edge > 0).double().mean()) > 0.2                  # f = 0, f = 79, t = 0, t = T - 1 carry live values
    out = sentinel_bf16(2, 82, T + 2, 32)
    dev = [t.cuda() for t in (feats, fmean, w, b)]
    d = L.ResnetDesc()
    d.n_chunks, d.T = 2, T
    d.feats_t, d.feats_t_elems, d.fmean, d.fmean_elems = dev[0].data_ptr(), dev[0].numel(), dev[1].data_ptr(), dev[1].numel()
    d.c1w, d.c1w_elems, d.c1b, d.c1b_elems = dev[2].data_ptr(), 288, dev[3].data_ptr(), 32
    d.out, d.out_elems = out.data_ptr(), out.numel()
    ccx_ctx.check(run(ccx_ctx, L.RESNET_CONV1, d), "ccx_resnet_op(CONV1)")
    halo = R.halo_mask(2, 80, T, 32)
    assert bool((bits(out)[halo] == SENTINEL).all()), "a halo cell was written"
    got = R.from_padded(out.cpu().double())
    assert bool(torch.isfinite(got).all())
    ratio = (got - ref).abs() / (2.0 ** -8 * ref.abs() + 11 * 2.0 ** -23 * a)
    for name, r in (("interior", ratio), ("f=0", ratio[:, :, 0]), ("f=79", ratio[:, :, 79]), ("t=0", ratio[..., 0]), ("t=T-1", ratio[..., T - 1])):
        print(f"conv1 T={T} {name}: worst err / bound {float(r.max()):.3f}")
        within("resnet conv1 err / (2^-8 |ref| + 11 2^-23 abs-sum)", float(r.max()), 1.0, (T, name))


# ------------------------------------------------------------------------------------------------------------ conv
def conv_in_need(n, H, W, cin, k, s):
    """Elements of the input a convolution may read (include/ccx.h): the padded layout, or where the strided view of the GEMM ends.
    The view has one row per padded pixel (every second one with stride 2), rows of align(k cin, 64) elements, one tap per kernel
    row a padded row apart; the 1x1 convolution starts at padded pixel (1, 1)."""
    Wp = W + 2
    layout = n * (H + 2) * Wp * cin
    M = n * ((H + 2) // s) * Wp
    view = ((Wp + 1) * cin if k == 1 else 0) + (M - 1) * s * cin + (k - 1) * Wp * cin + -(-k * cin // 64) * 64
    return max(view, layout)


class ConvCase:
    def __init__(self, cin, cout, k, s, epi, H, W, n=2, seed=0):
        L = _lib()
        self.geo = (cin, cout, k, s, epi, H, W, n)
        self.Ho, self.Wo = (H, W) if s == 1 else (H // 2, (W - 1) // 2 + 1)
        g = torch.Generator().manual_seed(1000 * cin + 100 * k + 10 * s + W + seed)
        self.x = R.bf16_round(torch.randn(n, cin, H, W, generator=g, dtype=torch.float64))
        self.w = (torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)).float()
        self.scale = (1 + 0.1 * torch.randn(cout, generator=g)).float()
        self.shift = (0.1 * torch.randn(cout, generator=g)).float()
        self.resid = None
        if epi == L.RESNET_EPI_ADD_RELU:
            self.resid = R.bf16_round(torch.randn(n, cout, self.Ho, self.Wo, generator=g, dtype=torch.float64))

    def reference(self):
        L = _lib()
        cin, cout, k, s, epi, H, W, n = self.geo
        return R.conv(self.x, R.fold_weight(self.w, self.scale), self.shift, s, epi != L.RESNET_EPI_PLAIN, self.resid)

    def launch(self, ctx, chunks=None, slack=BIG, in_elems=None, expect_ok=True):
        """-> out bf16 [n][Ho + 2][Wo + 2][cout] (device), computed for `chunks` (default: all) with `slack` behind the last chunk."""
        L = _lib()
        cin, cout, k, s, epi, H, W, n = self.geo
        sel = list(range(n)) if chunks is None else chunks
        m = len(sel)
        need = conv_in_need(m, H, W, cin, k, s)
        layout = m * (H + 2) * (W + 2) * cin
        buf = torch.empty(need, dtype=torch.float64)
        buf[:layout] = R.to_padded(self.x[sel]).reshape(-1)              # zero halo
        sign = 1.0 - 2.0 * (torch.arange(need - layout) % 2)
        buf[layout:] = slack * sign
        xin = buf.to(torch.bfloat16).cuda()
        out = sentinel_bf16(m, self.Ho + 2, self.Wo + 2, cout)
        wf, sc, sh = (np.ascontiguousarray(t.numpy()) for t in (self.w, self.scale, self.shift))
        d = L.ResnetDesc()
        d.n_chunks, d.cin, d.cout, d.k, d.conv_stride, d.H, d.W, d.epi = m, cin, cout, k, s, H, W, epi
        d.w_host, d.scale_host, d.shift_host = fptr(wf), fptr(sc), fptr(sh)
        d.in_, d.in_elems = xin.data_ptr(), need if in_elems is None else in_elems
        d.out, d.out_elems = out.data_ptr(), out.numel()
        if self.resid is not None:
            rp = R.to_padded(self.resid[sel], halo=BIG).to(torch.bfloat16).cuda()   # the residual's halo is never read
            d.resid, d.resid_elems = rp.data_ptr(), rp.numel()
        rc = run(ctx, L.RESNET_CONV, d)
        if expect_ok:
            ctx.check(rc, "ccx_resnet_op(CONV)")
        return out, rc


def check_conv(ctx, case, mate=True):
    L = _lib()
    cin, cout, k, s, epi, H, W, n = case.geo
    ref, a = case.reference()
    out, _ = case.launch(ctx)
    halo = R.halo_mask(n, case.Ho, case.Wo, cout)
    assert bool((bits(out)[halo] == SENTINEL).all()), (case.geo, "a halo cell was written")
    got = R.from_padded(out.cpu().double())
    assert bool(torch.isfinite(got).all()), case.geo
    ratio = (got - ref).abs() / R.conv_bound(ref, a, k * k * cin)
    worst = float(ratio.max())
    print(f"conv {case.geo}: worst err / bound {worst:.3f} at {np.unravel_index(int(ratio.argmax()), ratio.shape)}, "
          f"last column {float(ratio[..., -1].max()):.3f}")
    within("resnet conv err / (2^-8 |ref| + K 2^-23 abs-sum)", worst, 1.0, case.geo)
    if epi != L.RESNET_EPI_PLAIN:
        assert 0.2 < float((ref > 0).double().mean()) < 0.8          # ReLU is live on both sides
    out2, _ = case.launch(ctx, slack=-7.0e3)
    assert torch.equal(bits(out2), bits(out)), (case.geo, "the result depends on the read slack")
    if mate:
        alone, _ = case.launch(ctx, chunks=[1])
        assert torch.equal(bits(alone)[0], bits(out)[1]), (case.geo, "a chunk's result depends on its launch mate")


EPI = {"plain": 0, "relu": 1, "add_relu": 2}
CONV_CASES = (
    [(32, 32, 3, 1, e, 8, W) for W in (5, 63, 64, 65, 130) for e in ("relu", "add_relu")]           # direct kernel: H % 4 == 0
    + [(32, 32, 3, 1, e, 6, 65) for e in ("relu", "add_relu")]                                          # GEMM: H % 4 != 0
    + [(32, 64, 3, 2, "relu", 8, W) for W in (33, 34)] + [(32, 64, 1, 2, "plain", 8, W) for W in (33, 34)]
    + [(64, 64, 3, 1, "add_relu", 8, 17), (64, 128, 3, 2, "relu", 8, 17), (64, 128, 1, 2, "plain", 8, 17)]
    + [(128, 128, 3, 1, "relu", 4, 9), (128, 128, 3, 1, "add_relu", 4, 9), (128, 256, 3, 2, "relu", 4, 9), (128, 256, 1, 2, "plain", 4, 9)]
    + [(256, 256, 3, 1, "add_relu", 2, 5)])


@pytest.mark.parametrize("cin,cout,k,s,epi,H,W", CONV_CASES)
def test_conv_against_fp64(ccx_ctx, cin, cout, k, s, epi, H, W):
    check_conv(ccx_ctx, ConvCase(cin, cout, k, s, EPI[epi], H, W))


@pytest.mark.parametrize("epi", ["relu", "add_relu"])
def test_conv_product_geometry(ccx_ctx, epi):
    check_conv(ccx_ctx, ConvCase(32, 32, 3, 1, EPI[epi], 80, 130, n=1), mate=False)


@pytest.mark.parametrize("cin,cout,k,stride", R.NETWORK_CONVS)
def test_conv_bound_sees_near_miss_convolutions(cin, cout, k, stride):
    """On the CPU reference: a shift by one pixel in x or in y, a swap of two taps and dropping the last column each move the
    reference by more than the bound above on at least a quarter of the pixels they touch (ReLU hides the rest)."""
    seen = R.fault_visibility(cin, cout, k, stride)
    assert set(seen) == {"shift x", "shift y", "last column dropped"} | ({"tap swap"} if k == 3 else set())
    for name, frac in seen.items():
        assert frac > 0.25, (name, frac)


# ------------------------------------------------------------------------------------------------------------ halo zero
@pytest.mark.parametrize("H,W,Cn", [(80, 33, 32), (10, 5, 256)])
def test_halo_zero_touches_halo_cells_of_its_chunks_only(ccx_ctx, H, W, Cn):
    L = _lib()
    bufs = [sentinel_bf16(4, H + 2, W + 2, Cn) for _ in range(3)]
    d = L.ResnetDesc()
    d.halo0, d.halo1, d.halo2, d.halo0_elems = bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[0].numel()
    d.c0, d.n, d.H, d.Wp, d.C = 1, 2, H, W + 2, Cn
    ccx_ctx.check(run(ccx_ctx, L.RESNET_HALO_ZERO, d), "ccx_resnet_op(HALO_ZERO)")
    zeroed = torch.zeros(4, H + 2, W + 2, Cn, dtype=torch.bool)
    zeroed[1:3] = R.halo_mask(2, H, W, Cn)
    for b in bufs:
        v = bits(b)
        assert bool((v[zeroed] == 0).all()), "a halo cell of chunks 1, 2 was not zeroed"
        assert bool((v[~zeroed] == SENTINEL).all()), "an interior cell or another chunk was written"


# ------------------------------------------------------------------------------------------------------------ pooling
# Worst |mean - fp64| and |std - fp64| over the cases below, measured on an MI355X (fp32 sums over at most 133 frames of values of
# order 1).  Bounds: 2 x these.
TSTP_MEASURED = {"mean": 2.051e-6, "std": 8.888e-7}
TSTP_CASES = [(W4, nw) for W4 in (2, 5, 125) for nw in sorted({1, W4, 2 * W4, 589})] + [(14, 62), (133, 589)]


def tstp_act(W4, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, 256, 10, W4, generator=g, dtype=torch.float64) + 0.5 * torch.randn(1, 256, 10, 1, generator=g, dtype=torch.float64)
    return R.bf16_round(x)


def tstp_run(ctx, x, weights, mask_chunk, n_masks):
    L = _lib()
    W4 = x.shape[-1]
    act = R.to_padded(x, halo=BIG).to(torch.bfloat16).cuda()            # a read of a halo cell shows
    pooled = torch.full((n_masks, 5120), SENTINEL_F32, device="cuda")
    d = L.ResnetDesc()
    d.n_chunks, d.act, d.act_elems, d.W4, d.n_masks = 3, act.data_ptr(), act.numel(), W4, n_masks
    d.pooled, d.pooled_elems = pooled.data_ptr(), pooled.numel()
    keep = []
    if weights is not None:
        wd = weights.float().cuda()
        keep.append(wd)
        d.weights, d.weights_elems, d.n_w = wd.data_ptr(), wd.numel(), weights.shape[1]
    if mask_chunk is not None:
        mc = (C.c_int * len(mask_chunk))(*mask_chunk)
        keep.append(mc)
        d.mask_chunk = mc
    ctx.check(run(ctx, L.RESNET_TSTP, d), "ccx_resnet_op(TSTP)")
    return pooled.double().cpu()


@pytest.mark.parametrize("W4,nw", TSTP_CASES)
def test_tstp_weighted_against_fp64(ccx_ctx, W4, nw):
    if (W4, nw) in ((14, 62), (133, 589)):
        assert not np.array_equal(R.nearest_index_exact(W4, nw), R.nearest_index(W4, nw).numpy())      # the two maps differ here
    x = tstp_act(W4, 7 * W4 + nw)
    idx = R.nearest_index(W4, nw)
    g = torch.Generator().manual_seed(nw)
    binary = (torch.rand(nw, generator=g) > 0.5).float()
    binary[idx[0]] = binary[idx[W4 - 1]] = 1.0                          # at least two frames (W4 >= 2): the variance is defined
    soft = 0.05 + 0.95 * torch.rand(2, nw, generator=g)
    t0 = W4 // 2
    onehot = torch.zeros(nw)
    onehot[idx[t0]] = 1.0
    hit = (idx == idx[t0]).nonzero().flatten().tolist()                 # the frames that read the one live weight
    weights = torch.stack([binary, soft[0], torch.zeros(nw), onehot, soft[1]])
    mask_chunk = [0, 0, 2, 2, 0]                                        # chunk 0 serves three masks, chunk 1 none
    got = tstp_run(ccx_ctx, x, weights, mask_chunk, 5)
    assert bool(torch.isfinite(got).all())
    ref = R.tstp(x, weights.double(), mask_chunk)
    for j, name in ((0, "binary"), (1, "soft"), (4, "soft")):
        em, es = float((got[j, :2560] - ref[j, :2560]).abs().max()), float((got[j, 2560:] - ref[j, 2560:]).abs().max())
        print(f"tstp W4={W4} n_w={nw} {name}: mean max abs err {em:.3e}, std max abs err {es:.3e}")
        within("resnet tstp mean max abs err", em, 2 * TSTP_MEASURED["mean"], (W4, nw, name))
        within("resnet tstp std max abs err", es, 2 * TSTP_MEASURED["std"], (W4, nw, name))
    assert bool((got[2] == 0).all()), "all-zero weights: mean 0 and std 0"
    if len(hit) == 1:                                                   # one frame: its value, std 0 (1 + 1e-8 is 1 in fp32)
        want = x[2, :, :, hit[0]].reshape(-1)
        assert torch.equal(got[3, :2560], want) and bool((got[3, 2560:] == 0).all())
    else:
        within("resnet tstp mean max abs err", float((got[3, :2560] - ref[3, :2560]).abs().max()), 2 * TSTP_MEASURED["mean"], (W4, nw, "one weight"))
        within("resnet tstp std max abs err", float((got[3, 2560:] - ref[3, 2560:]).abs().max()), 2 * TSTP_MEASURED["std"], (W4, nw, "one weight"))


@pytest.mark.parametrize("W4", [2, 5, 125])
def test_tstp_unweighted_is_the_unbiased_std(ccx_ctx, W4):
    x = tstp_act(W4, W4)
    ref = R.tstp(x)
    for mask_chunk, sel in ((None, [0, 1, 2]), ([2, 0, 0], [2, 0, 0])):
        got = tstp_run(ccx_ctx, x, None, mask_chunk, 3)
        em, es = float((got[:, :2560] - ref[sel, :2560]).abs().max()), float((got[:, 2560:] - ref[sel, 2560:]).abs().max())
        print(f"tstp W4={W4} unweighted mask_chunk={mask_chunk}: mean max abs err {em:.3e}, std max abs err {es:.3e}")
        within("resnet tstp mean max abs err", em, 2 * TSTP_MEASURED["mean"], (W4, "unweighted"))
        within("resnet tstp std max abs err", es, 2 * TSTP_MEASURED["std"], (W4, "unweighted"))


def test_linear_against_fp64(ccx_ctx):
    """5120 products accumulated in fp32 in any order: 5120 2^-24 sum |p w| elementwise."""
    L = _lib()
    g = torch.Generator().manual_seed(4)
    p = torch.randn(3, 5120, generator=g)
    w = torch.randn(256, 5120, generator=g) / math.sqrt(5120)
    b = 0.1 * torch.randn(256, generator=g)
    emb = torch.full((3, 256), SENTINEL_F32, device="cuda")
    dev = [t.cuda() for t in (p, w, b)]
    d = L.ResnetDesc()
    d.n_masks, d.pooled, d.pooled_elems = 3, dev[0].data_ptr(), dev[0].numel()
    d.lin_w, d.lin_w_elems, d.lin_b, d.lin_b_elems = dev[1].data_ptr(), dev[1].numel(), dev[2].data_ptr(), 256
    d.emb, d.emb_elems = emb.data_ptr(), emb.numel()
    ccx_ctx.check(run(ccx_ctx, L.RESNET_LINEAR, d), "ccx_resnet_op(LINEAR)")
    ref, _ = R.linear(p, w, b)
    a = p.double().abs() @ w.double().abs().T
    ratio = float(((emb.double().cpu() - ref).abs() / (5120 * 2.0 ** -24 * a)).max())
    print(f"linear: worst err / bound {ratio:.4f}")
    within("resnet linear err / (5120 2^-24 sum |p w|)", ratio, 1.0)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_descriptor_refusals_launch_nothing(ccx_ctx):
    L = _lib()

    def refused(rc, field, outs):
        msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
        assert rc == 1 and "ccx_resnet_op" in msg and field in msg, (field, rc, msg)
        for o in outs:
            assert bool((bits(o) == SENTINEL).all()), (field, "something was launched")

    # a buffer shorter than the layout plus slack
    for geo in ((32, 32, 3, 1, 1, 6, 9), (32, 64, 3, 2, 1, 6, 9), (64, 128, 1, 2, 0, 6, 9)):
        case = ConvCase(*geo)
        need, layout = conv_in_need(2, 6, 9, geo[0], geo[2], geo[3]), 2 * 8 * 11 * geo[0]
        assert need > layout
        for short in (layout, need - 1):
            out, rc = case.launch(ccx_ctx, in_elems=short, expect_ok=False)
            refused(rc, "in_elems", [out])
    # geometry checks come before any buffer arithmetic: generous buffers, so that only the named field is at fault
    xin = torch.zeros(1 << 18, dtype=torch.bfloat16, device="cuda")
    out = sentinel_bf16(1 << 18)
    res = torch.zeros(1 << 18, dtype=torch.bfloat16, device="cuda")
    host = np.zeros(512 * 256 * 9, dtype=np.float32)

    def conv_desc(cin, cout, k, s, epi, H, W, resid=False):
        d = L.ResnetDesc()
        d.n_chunks, d.cin, d.cout, d.k, d.conv_stride, d.H, d.W, d.epi = 2, cin, cout, k, s, H, W, epi
        d.w_host, d.scale_host, d.shift_host = fptr(host), fptr(host), fptr(host)
        d.in_, d.in_elems, d.out, d.out_elems = xin.data_ptr(), xin.numel(), out.data_ptr(), out.numel()
        if resid:
            d.resid, d.resid_elems = res.data_ptr(), res.numel()
        return d

    assert run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 32, 3, 1, 1, 4, 5)) == 0      # the descriptor the refusals below vary
    out.view(torch.int16).fill_(SENTINEL)
    # a (cin, cout, k, stride) combination the network does not have
    for geo in ((32, 128, 3, 1), (32, 32, 3, 2), (64, 64, 1, 1), (256, 512, 3, 2), (48, 48, 3, 1), (32, 64, 5, 2), (64, 32, 3, 2)):
        refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(*geo, 1, 4, 5)), "(cin, cout, k, conv_stride)", [out])
    # odd H, W below 2, an unknown epilogue, a residual nobody adds, a missing one, aliasing, a short output
    refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 32, 3, 1, 1, 3, 5)), "H =", [out])
    refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 64, 3, 2, 1, 5, 5)), "H =", [out])
    refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 32, 3, 1, 1, 4, 1)), "W =", [out])
    refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 32, 3, 1, 3, 4, 5)), "epi =", [out])
    refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 32, 3, 1, 1, 4, 5, resid=True)), "resid", [out])
    refused(run(ccx_ctx, L.RESNET_CONV, conv_desc(32, 32, 3, 1, 2, 4, 5)), "resid is NULL", [out])
    d = conv_desc(32, 32, 3, 1, 1, 4, 5); d.out = xin.data_ptr() + 64; refused(run(ccx_ctx, L.RESNET_CONV, d), "overlaps", [out])
    d = conv_desc(32, 32, 3, 1, 1, 4, 5); d.out_elems = 2 * 6 * 7 * 32 - 1; refused(run(ccx_ctx, L.RESNET_CONV, d), "out_elems", [out])
    d = conv_desc(32, 32, 3, 1, 1, 4, 5); d.w_host = None; refused(run(ccx_ctx, L.RESNET_CONV, d), "w_host", [out])
    d = conv_desc(32, 32, 3, 1, 1, 4, 5); d.n_chunks = 0; refused(run(ccx_ctx, L.RESNET_CONV, d), "n_chunks", [out])
    # halo zero: a buffer too short for c0 + n chunks, a channel count the network does not have
    d = L.ResnetDesc()
    d.halo0, d.halo1, d.halo2, d.halo0_elems = out.data_ptr(), out.data_ptr(), out.data_ptr(), 4 * 6 * 7 * 32 - 1
    d.c0, d.n, d.H, d.Wp, d.C = 1, 3, 4, 7, 32
    refused(run(ccx_ctx, L.RESNET_HALO_ZERO, d), "halo0_elems", [out])
    d.halo0_elems, d.C = out.numel(), 48
    refused(run(ccx_ctx, L.RESNET_HALO_ZERO, d), "C =", [out])
    # pooling: mask_chunk out of range, weights without mask_chunk, too short a buffer
    x = tstp_act(5, 1)
    act = R.to_padded(x).to(torch.bfloat16).cuda()
    wd = torch.ones(2, 7, device="cuda")
    pooled = torch.full((2, 5120), SENTINEL_F32, device="cuda")

    def pool_desc():
        d = L.ResnetDesc()
        d.n_chunks, d.act, d.act_elems, d.W4, d.n_masks = 3, act.data_ptr(), act.numel(), 5, 2
        d.pooled, d.pooled_elems = pooled.data_ptr(), pooled.numel()
        d.weights, d.weights_elems, d.n_w = wd.data_ptr(), wd.numel(), 7
        d._mc = (C.c_int * 2)(0, 2)
        d.mask_chunk = d._mc
        return d

    def pool_refused(d, field):
        msg_rc = run(ccx_ctx, L.RESNET_TSTP, d)
        msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
        assert msg_rc == 1 and "ccx_resnet_op" in msg and field in msg, (field, msg_rc, msg)
        assert bool(torch.isnan(pooled).all()), (field, "something was launched")

    d = pool_desc(); d._mc[1] = 3; pool_refused(d, "mask_chunk[1]")
    d = pool_desc(); d._mc[0] = -1; pool_refused(d, "mask_chunk[0]")
    d = pool_desc(); d.mask_chunk = None; pool_refused(d, "without mask_chunk")
    d = pool_desc(); d.weights = None; d.mask_chunk = None; pool_refused(d, "n_masks")           # 2 masks, 3 chunks, no map
    d = pool_desc(); d.act_elems = act.numel() - 1; pool_refused(d, "act_elems")
    d = pool_desc(); d.weights_elems = 13; pool_refused(d, "weights_elems")
    d = pool_desc(); d.W4 = 1; pool_refused(d, "W4")
    d = pool_desc(); d.pooled = pooled.data_ptr() + 4; pool_refused(d, "pooled is not 16-byte aligned")
    d = pool_desc()
    rc = run(ccx_ctx, 6, d)
    assert rc == 1 and "unknown op" in ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
    assert bool(torch.isnan(pooled).all())
