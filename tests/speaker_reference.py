"""fp64 restatement of the operators behind ccx_speaker_op (csrc/speaker.hip): the waveform statistics, the sinc stage, InstanceNorm
with its max-pool and LeakyReLU, statistics pooling, the LSTM recurrence and the frame activation, each written from its definition
(F.conv1d, max_pool1d, var(unbiased=False), a plain time loop) and not from the kernels' algorithms (no hi/lo split, no fragment
layout, no pieces, no common denominators).

The references run on the inputs the kernels see: fp32 waveforms and filters, fp32 rows, bf16 activations.  What a GPU test measures
is then the kernel, not the rounding of its inputs.  tests/test_speaker_reference_cpu.py checks these statements against second ones
built from other parts and against oracle/pyannote_ref.py, and shows what the sinc bound sees.

This file also holds the inputs of the sinc GPU tests (sinc_cases), so that the CPU suite can check the derived bound on them."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.resnet_reference import bf16_round, nearest_index, rel_l2, stats_pool  # noqa: F401  (re-exported)

F64 = torch.float64
K, STRIDE, NF = 251, 10, 80
EPS = 1e-5
SLOPE = 0.01


# ---------------------------------------------------------------------------------------------- bf16 as numbers
def bf16_order(x: torch.Tensor) -> torch.Tensor:
    """Values that are exactly bf16 -> integers in value order (adjacent bf16 values differ by 1; +0 and -0 both map to 0)."""
    b = x.to(torch.float32).to(torch.bfloat16).view(torch.int16).to(torch.int64)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def bf16_half_ulp(x: torch.Tensor) -> torch.Tensor:
    """Half the spacing of bf16 at each (bf16-valued, fp64-typed) x: a fp32 result within this distance of x may round to x."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return 2.0 ** (e - 8)


LSTM_ULP_FLOOR = 2.0 ** -4


def bf16_ulps(got: torch.Tensor, ref: torch.Tensor, floor: float = LSTM_ULP_FLOOR) -> torch.Tensor:
    """|got - ref| in units of the bf16 spacing at max(|ref|, floor).
    The floor is for outputs of a recurrence that feeds bf16-rounded values back: when two correct runs round one fed-back h_j
    differently (one spacing, at most 2^-8 for |h| < 1), a gate pre-activation moves by |W_hh| 2^-8 (up to 0.21 2^-8 = 8e-4 for the
    N(0, 0.8^2 / 128) weights of the tests at 3 sigma) and the next outputs by a like ABSOLUTE amount whatever their own size, so
    outputs below 2^-4 (spacing 2^-11 = 4.9e-4) cannot be held to their own spacing."""
    e = torch.floor(torch.log2(ref.abs().clamp(min=floor)))
    return (got - ref).abs() / 2.0 ** (e - 7)


def bf16_excess(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """How far the fp64 value `ref` lies outside the set of values that round to the bf16 `got`: the part of |got - ref| that the one
    output rounding (at most half a bf16 spacing, <= 2^-8 |got|) does not explain.  0 where `got` is a correct rounding of ref."""
    return ((got - ref).abs() - bf16_half_ulp(got)).clamp(min=0.0)


# ---------------------------------------------------------------------------------------------- waveform statistics, sinc stage
def wav_stats(x: torch.Tensor, w: float, b: float):
    """x [T] -> (a, c, mean) in fp64: InstanceNorm1d(1, affine) is a x + c with a = w / sqrt(var + eps), c = b - mean a."""
    x = x.to(F64)
    mean = x.mean()
    a = w / torch.sqrt(x.var(unbiased=False) + EPS)
    return float(a), float(b - mean * a), float(mean)


def sinc_positions(x: torch.Tensor, filt: torch.Tensor, w: float, b: float):
    """x [T] fp32, filt [80][251] fp32 -> (y, bound) fp64 [positions][80]: y = conv1d(instance_norm(x), filt, stride 10) before the
    absolute value, and the elementwise bound of sinc_bound() for it."""
    a, c, _ = wav_stats(x, w, b)
    xd, fd = x.to(F64), filt.to(F64)
    y = F.conv1d((a * xd + c)[None, None], fd[:, None, :], stride=STRIDE)[0].T
    conv = F.conv1d(xd[None, None], fd[:, None, :], stride=STRIDE)[0].T
    asum = F.conv1d(xd.abs()[None, None], fd.abs()[:, None, :], stride=STRIDE)[0].T
    return y, sinc_bound(a, c, conv, asum, fd.sum(dim=1), fd.abs().sum(dim=1))


SINC_K1 = 3.0


def sinc_bound(a: float, c: float, conv: torch.Tensor, asum: torch.Tensor, wsum: torch.Tensor, wabs: torch.Tensor) -> torch.Tensor:
    """|got - ref| <= |a| (k1 2^-18 + 272 2^-24) sum |x_k w_k| + 2^-22 (|a conv| + |c sum w|), elementwise per position and filter.

    The kernel splits each operand into two bf16: v = vh + vl + ev with |vl| <= 2^-9 |v| and |ev| <= 2^-18 |v|, and adds the three
    products xh wh + xl wh + xh wl, each exact in fp32.  Against x w that leaves the dropped xl wl (<= 2^-18 |x w|) and the two
    residual roundings ex w and x ew (<= 2^-18 |x w| each): k1 = 3.  272 = 9 steps x 30 taps + 2 zero slots products enter one
    fp32 accumulator, each addition rounding by at most 2^-24 of a partial sum that sum |x w| bounds.  The last term covers the fp32
    statistics (a, the mean inside c) and the fused multiply-add of the fold, a few units of 2^-24 of the two terms it adds.

    To this the reference adds its own error: `conv` and `wsum` are fp64 sums of 251 terms (as is the loader's filter sum), off by up
    to 251 2^-53 of the sum of magnitudes, which matters only where the taps cancel to (nearly) nothing: wabs = sum |w_k|."""
    kernel = abs(a) * (SINC_K1 * 2.0 ** -18 + 272 * 2.0 ** -24) * asum + 2.0 ** -22 * ((a * conv).abs() + (c * wsum).abs()[None, :])
    return kernel + 2 * 251 * 2.0 ** -53 * (abs(a) * asum + abs(c) * wabs[None, :])


def pool3(y: torch.Tensor, n_pool: int, first: int = 0) -> torch.Tensor:
    """[positions][80] -> [n_pool][80]: max over positions first + 3 i .. first + 3 i + 2."""
    return F.max_pool1d(y[first:first + 3 * n_pool].T[None], 3, stride=3)[0].T


def sinc_stage(x: torch.Tensor, filt: torch.Tensor, w: float, b: float, n_pool: int):
    """-> (out, bound) fp64 [n_pool][80]: max_pool1d(|conv1d(instance_norm(x))|, 3) and its elementwise bound (|.| and max are
    1-Lipschitz: a pooled value moves by at most the largest bound of its three positions)."""
    y, bound = sinc_positions(x, filt, w, b)
    return pool3(y.abs(), n_pool), pool3(bound, n_pool)


def sinc_split_emulation(x: torch.Tensor, filt: torch.Tensor, w: float, b: float, n_pool: int, centre: bool = True) -> torch.Tensor:
    """The kernel's arithmetic in torch, for validating bounds on the CPU: fp32 statistics, operands split into hi / lo bf16, three
    products accumulated in fp32, the norm folded around the convolution, |.|, max-pool.  centre = True is what the kernel does
    (x - mean is split, with the mean held as two floats, and the bias is folded: a conv(x - mean) + b sum w); centre = False
    splits the raw samples and folds a conv(x) + c sum w, which is what it did before."""
    x = x.float()
    mean = x.mean()
    lo = (x - mean).mean()                                                  # the kernel carries the mean as mean + lo
    a = torch.tensor(w) * torch.rsqrt(((x - mean) ** 2).mean() - lo * lo + EPS)
    v = (x - mean) - lo if centre else x
    shift = torch.tensor(b) if centre else torch.tensor(b) - (mean + lo) * a

    def split(t):
        hi = t.to(torch.bfloat16).float()
        return hi, (t - hi).to(torch.bfloat16).float()

    (xh, xl), (wh, wl) = split(v), split(filt.float())
    conv = lambda s, f: F.conv1d(s[None, None], f[:, None, :], stride=STRIDE)[0].T     # fp32
    acc = (conv(xl, wh) + conv(xh, wl)) + conv(xh, wh)
    y = a * acc + shift * filt.double().sum(dim=1).float()[None, :]        # the loader sums the taps in fp64 and rounds once
    return pool3(y.abs(), n_pool).to(F64)


def sinc_near_misses(x: torch.Tensor, filt: torch.Tensor, w: float, b: float, n_pool: int) -> dict:
    """What four near-misses of the sinc kernel would compute, {name: [n_pool][80]}; each keeps the statistics of the true input."""
    a, c, _ = wav_stats(x, w, b)
    xn = a * x.to(F64) + c
    conv = lambda s, f: F.conv1d(s[None, None], f.to(F64)[:, None, :], stride=STRIDE)[0].T.abs()
    out = {"input shifted by one sample": pool3(conv(torch.roll(xn, -1), filt), n_pool)}
    f = filt.clone()
    f[:, 249], f[:, 250] = filt[:, 250], filt[:, 249]
    out["taps 249 and 250 swapped"] = pool3(conv(xn, f), n_pool)
    f = filt.clone()
    f[:, 250] = 0.0
    out["tap 250 dropped"] = pool3(conv(xn, f), n_pool)
    out["pool over 3 i + 1 .. 3 i + 3"] = pool3(conv(xn, filt), n_pool, first=1)
    return out


# ---- the inputs of the sinc tests
SINC_FRAMES = (1, 5, 15, 16, 17, 127, 128, 129, 257)
SINC_FILTERS = ("mel", "dense", "tap locator")
SINC_INPUTS = ("zero-mean", "dc 0.3 std 0.01", "dc 0.5 std 1e-3", "silence")
LOCATOR_TAPS = (0, 29, 30, 31, 239, 240, 250)
NORM_W, NORM_B = float(torch.tensor(1.1)), float(torch.tensor(0.05))      # the synthetic checkpoints' waveform norm, as fp32 holds it


def sinc_samples(n_pool: int, k: int) -> int:
    """Samples of test crop k with n_pool pooled frames: 3 n_pool positions, k % 3 further positions the pool drops, and a ragged
    tail of (3 k + 1) % 10 samples no position reads."""
    return K + STRIDE * (3 * n_pool - 1 + k % 3) + (3 * k + 1) % 10


def locator_tap(f: int) -> int:
    """Tap of the unit impulse of filter f: each 16-filter tile holds the seven taps at the edges of the kernel's k steps."""
    return LOCATOR_TAPS[f % 16] if f % 16 < len(LOCATOR_TAPS) else (53 * f + 7) % K


def sinc_filter_bank(kind: str) -> torch.Tensor:
    if kind == "mel":
        from clearconverse_amd.weights import sinc_filters, synthetic_xvector_state_dict
        sd = synthetic_xvector_state_dict(1)
        return sinc_filters(sd["sincnet.conv1d.0.filterbank.low_hz_"], sd["sincnet.conv1d.0.filterbank.band_hz_"])
    if kind == "dense":
        return (torch.randn(NF, K, generator=torch.Generator().manual_seed(80)) / math.sqrt(K)).float()
    assert kind == "tap locator"
    f = torch.zeros(NF, K)
    for i in range(NF):
        f[i, locator_tap(i)] = 1.0
    return f


def sinc_wave(kind: str, n: int, seed: int) -> torch.Tensor:
    noise = torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=F64)
    if kind == "zero-mean":
        return (0.1 * noise).float()
    if kind == "dc 0.3 std 0.01":
        return (0.3 + 0.01 * noise).float()
    if kind == "dc 0.5 std 1e-3":
        return (0.5 + 1e-3 * noise).float()
    assert kind == "silence"
    return torch.zeros(n)


def sinc_crops(kind: str, frames=SINC_FRAMES):
    """-> [(wave [T] fp32, n_pool)] for the ragged batch of the sinc tests."""
    return [(sinc_wave(kind, sinc_samples(p, k), 100 * p + k), p) for k, p in enumerate(frames)]


def sinc_grid_crops():
    """130 crops of 129 frames: 260 work items (two per crop) for the kernel's 256 persistent blocks."""
    return [(sinc_wave("zero-mean", sinc_samples(129, k), 9000 + k), 129) for k in range(130)]


# ---------------------------------------------------------------------------------------------- instance norm
def inorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, pool: int, n_out: int) -> torch.Tensor:
    """x [rows][C] (the first pool n_out rows are used) -> LeakyReLU(InstanceNorm1d(max_pool1d(x, pool))) [n_out][C] in fp64:
    biased variance over the crop's frames, eps 1e-5, affine, slope 0.01."""
    v = x[:pool * n_out].to(F64)
    if pool > 1:
        v = F.max_pool1d(v.T[None], pool, stride=pool)[0].T
    mean = v.mean(dim=0, keepdim=True)
    var = v.var(dim=0, unbiased=False, keepdim=True)
    return F.leaky_relu((v - mean) / torch.sqrt(var + EPS) * gamma.to(F64) + beta.to(F64), SLOPE)


# ---------------------------------------------------------------------------------------------- pooling
def pool_stats(x: torch.Tensor, weights: torch.Tensor = None) -> torch.Tensor:
    """x [frames][C] -> [2 C] (mean || std) in fp64: unbiased std without weights; with weights [n_w], pyannote's StatsPool on the
    weights gathered at torch's nearest index map (tests/resnet_reference.py)."""
    return stats_pool(x.to(F64).T[None], None if weights is None else weights[None])[0]


# ---------------------------------------------------------------------------------------------- LSTM
def lstm(gx: torch.Tensor, whh: torch.Tensor, round_h: bool = True, dtype=F64, clamp: float = None) -> torch.Tensor:
    """One sequence, both directions.  gx [T][1024] (x W_ih^T + b_ih + b_hh: fwd 0..511 | rev 512..1023, gates i|f|g|o of 128 units
    each), whh [2][512][128] -> h [T][256] (fwd | rev, the reverse direction runs from the last row to the first).
    The kernel's contract (round_h): W_hh is rounded to bf16, h is rounded to bf16 after every step for the feedback and for the
    output; the cell state and the gates are not rounded.  Everything else in `dtype`.  clamp: gate pre-activations limited to
    +-clamp (2 g and 2 c for the tanh arguments), for stating what the kernel's clamp costs."""
    T = gx.shape[0]
    out = torch.zeros(T, 256, dtype=dtype)
    rnd = (lambda t: bf16_round(t)) if round_h else (lambda t: t)
    lim = (lambda t, s=1.0: t) if clamp is None else (lambda t, s=1.0: torch.clamp(t, -clamp / s, clamp / s))
    for d in range(2):
        W = rnd(whh[d].to(dtype))
        h = torch.zeros(128, dtype=dtype)
        c = torch.zeros(128, dtype=dtype)
        for step in range(T):
            t = step if d == 0 else T - 1 - step
            i, f, g, o = (gx[t, 512 * d:512 * (d + 1)].to(dtype) + W @ h).chunk(4)
            c = torch.sigmoid(lim(f)) * c + torch.sigmoid(lim(i)) * torch.tanh(lim(g, 2.0))
            h = rnd(torch.sigmoid(lim(o)) * torch.tanh(lim(c, 2.0)))
            out[t, 128 * d:128 * (d + 1)] = h
    return out


# ---------------------------------------------------------------------------------------------- activation
def activation(logits: torch.Tensor, powerset: bool) -> torch.Tensor:
    x = logits.to(F64)
    return F.log_softmax(x, dim=-1) if powerset else torch.sigmoid(x)
