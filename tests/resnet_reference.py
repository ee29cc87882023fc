"""fp64 restatement of the operators behind ccx_resnet_op (csrc/resnet.hip): Kaldi fbank, the first convolution, one folded
convolution of the trunk, weighted statistics pooling and the embedding layer, each written from its definition (framing and rfft,
F.conv2d, F.interpolate, the StatsPool formulas) and not from the kernels' algorithms (no radix-2 FFT, no taps, no strided views).

The references run on the inputs the kernels see: fp32 waveforms, bf16-rounded activations, weights folded in fp32 and rounded to
bf16 the way the loader does it.  What a GPU test measures is then the kernel, not the rounding of its inputs.
tests/test_resnet_reference_cpu.py checks these statements against oracle/wespeaker_ref.py (fp32) and pins the index-map facts."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
FRAME_LEN, FRAME_SHIFT, N_FFT, N_MELS = 400, 160, 512, 80
SAMPLE_RATE, LOW_FREQ, PREEMPH = 16000.0, 20.0, 0.97
FLT_EPSILON = float(np.finfo(np.float32).eps)
# (cin, cout, k, stride) of every convolution of the trunk after the first
NETWORK_CONVS = ([(c, c, 3, 1) for c in (32, 64, 128, 256)]
                 + [(c, 2 * c, k, 2) for c in (32, 64, 128) for k in (3, 1)])


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


# ---------------------------------------------------------------------------------------------- fbank
def num_frames(n_samples: int) -> int:
    return 0 if n_samples < FRAME_LEN else 1 + (n_samples - FRAME_LEN) // FRAME_SHIFT


def mel_banks() -> torch.Tensor:
    """Kaldi get_mel_banks in fp64: [80][257] triangles linear in mel between 20 Hz and Nyquist; bin 256 carries no weight."""
    def mel(f):
        return 1127.0 * torch.log(1.0 + f / 700.0)
    lo, hi = mel(torch.tensor(LOW_FREQ, dtype=F64)), mel(torch.tensor(SAMPLE_RATE / 2, dtype=F64))
    delta = (hi - lo) / (N_MELS + 1)
    left = lo + torch.arange(N_MELS, dtype=F64)[:, None] * delta
    center, right = left + delta, left + 2 * delta
    m = mel(torch.arange(N_FFT // 2, dtype=F64) * (SAMPLE_RATE / N_FFT))[None, :]
    banks = torch.clamp(torch.minimum((m - left) / (center - left), (right - m) / (right - center)), min=0.0)
    return F.pad(banks, (0, 1))


def spectrum(wave: torch.Tensor) -> torch.Tensor:
    """wave [n] (fp32 values in [-1, 1]) -> complex spectrum [T][257] of the windowed frames, fp64."""
    x = wave.to(F64) * 32768.0
    T = num_frames(x.numel())
    idx = torch.arange(T)[:, None] * FRAME_SHIFT + torch.arange(FRAME_LEN)[None, :]
    fr = x[idx]
    fr = fr - fr.mean(dim=1, keepdim=True)                                        # remove_dc_offset
    fr = fr - PREEMPH * torch.cat([fr[:, :1], fr[:, :-1]], dim=1)                 # replicate padding on the left
    win = 0.54 - 0.46 * torch.cos(2.0 * math.pi * torch.arange(FRAME_LEN, dtype=F64) / (FRAME_LEN - 1))
    return torch.fft.rfft(F.pad(fr * win, (0, N_FFT - FRAME_LEN)), dim=1)


def mel_energies(wave: torch.Tensor) -> torch.Tensor:
    """wave [n] -> mel energies [T][80] in fp64, before the floor and the logarithm."""
    spec = spectrum(wave)
    return (spec.real ** 2 + spec.imag ** 2) @ mel_banks().T


def fbank(wave: torch.Tensor) -> torch.Tensor:
    """wave [n] -> log mel energies [T][80] in fp64 (before the mean normalisation)."""
    return torch.log(torch.clamp(mel_energies(wave), min=FLT_EPSILON))


FBANK_VARIANTS = ("plain", "dc", "full scale", "leading zeros")


def fbank_test_waves(T: int, variant: str, n_chunks: int = 2) -> torch.Tensor:
    """The GPU test's input: [n_chunks][n] fp32 with n = 400 + 160 (T - 1) + 37 samples (T frames and a tail no frame uses).
    A synthetic two-speaker clip plus noise whose spectrum is flat AFTER pre-emphasis, so that every mel bin of every frame carries
    signal.  Variants: "dc" = 0.5 + 1e-3 of that; "full scale" = peak exactly 1; "leading zeros" = the first 40 % exact zeros."""
    from clearconverse_amd.audio import synthetic_clip
    n = FRAME_LEN + FRAME_SHIFT * (T - 1) + 37
    rows = []
    for c in range(n_chunks):
        g = np.random.default_rng(1000 * T + c)
        noise = np.convolve(g.standard_normal(n + 400), PREEMPH ** np.arange(400))[400:400 + n]
        noise /= np.sqrt(np.mean(noise ** 2))
        clip = np.asarray(synthetic_clip(5 + c, 10.0), dtype=np.float64)[3000 + 977 * c:3000 + 977 * c + n]
        x = 0.25 * clip + 0.12 * noise
        if variant == "dc":
            x = 0.5 + 1e-3 * (0.5 * clip + noise)
        elif variant == "full scale":
            x = x / np.abs(x).max()
        elif variant == "leading zeros":
            x[:int(0.4 * n)] = 0.0
        elif variant != "plain":
            raise ValueError(variant)
        rows.append(x.astype(np.float32))
    return torch.from_numpy(np.stack(rows))


# ---------------------------------------------------------------------------------------------- layouts
def to_padded(x: torch.Tensor, halo: float = 0.0) -> torch.Tensor:
    """NCHW [n][C][H][W] -> the kernels' padded NHWC [n][H + 2][W + 2][C] with `halo` in the one-pixel border."""
    n, C, H, W = x.shape
    out = torch.full((n, H + 2, W + 2, C), halo, dtype=x.dtype)
    out[:, 1:H + 1, 1:W + 1, :] = x.permute(0, 2, 3, 1)
    return out


def from_padded(p: torch.Tensor) -> torch.Tensor:
    """padded NHWC [n][H + 2][W + 2][C] -> NCHW interior [n][C][H][W]."""
    return p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous()


def halo_mask(n: int, H: int, W: int, C: int) -> torch.Tensor:
    """bool [n][H + 2][W + 2][C]: True on the halo cells."""
    m = torch.ones((n, H + 2, W + 2, C), dtype=torch.bool)
    m[:, 1:H + 1, 1:W + 1, :] = False
    return m


# ---------------------------------------------------------------------------------------------- convolutions
def bn_fold(sd, name: str):
    """BatchNorm (eval, eps 1e-5) as a per-channel (scale, shift), fp64."""
    scale = sd[name + ".weight"].to(F64) / torch.sqrt(sd[name + ".running_var"].to(F64) + 1e-5)
    return scale, sd[name + ".bias"].to(F64) - sd[name + ".running_mean"].to(F64) * scale


def fold_weight(w: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The loader's weight: w[o] * scale[o] in fp32, rounded to bf16; returned in fp64."""
    return (w.float() * scale.float()[:, None, None, None]).to(torch.bfloat16).to(F64)


def conv(x: torch.Tensor, w: torch.Tensor, shift: torch.Tensor, stride: int, relu: bool, resid: torch.Tensor = None):
    """x NCHW fp64, w [cout][cin][k][k] fp64 (folded), padding k // 2 -> (out, abs_sum): out = [relu](conv + shift [+ resid]) and
    abs_sum = sum |a w| + |shift| [+ |resid|], the scale the accumulation's rounding errors are proportional to."""
    pad = w.shape[-1] // 2
    y = F.conv2d(x, w, stride=stride, padding=pad) + shift.to(F64)[None, :, None, None]
    a = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad) + shift.to(F64).abs()[None, :, None, None]
    if resid is not None:
        y, a = y + resid, a + resid.abs()
    return (torch.relu(y) if relu else y), a


def conv1(feats_t: torch.Tensor, fmean: torch.Tensor, w: torch.Tensor, b: torch.Tensor):
    """feats_t [n][80][T], fmean [n][80], w [32][9] (BatchNorm folded), b [32] -> (relu(conv3x3(feats - mean) + b), abs_sum), NCHW."""
    x = (feats_t.to(F64) - fmean.to(F64)[:, :, None])[:, None]
    return conv(x, w.to(F64).reshape(32, 1, 3, 3), b, 1, True)


# ---------------------------------------------------------------------------------------------- pooling
def nearest_index(n_out: int, n_in: int) -> torch.Tensor:
    """Source index of each of n_out destination elements under F.interpolate(mode="nearest"), asked of torch itself."""
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, -1)
    return F.interpolate(src, size=n_out, mode="nearest").view(-1).long()


def nearest_index_fp32(n_out: int, n_in: int) -> np.ndarray:
    """The kernels' map (ccx_common.h ccx_nearest_src): min(floor(t * (float(n_in) / float(n_out))), n_in - 1), all in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    t = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(t * scale).astype(np.int64), n_in - 1)


def nearest_index_exact(n_out: int, n_in: int) -> np.ndarray:
    """The exact rational map (t * n_in) // n_out that stats_pool_kernel used to apply."""
    return (np.arange(n_out, dtype=np.int64) * n_in) // n_out


def stats_pool(x: torch.Tensor, weights: torch.Tensor = None, index: torch.Tensor = None) -> torch.Tensor:
    """x [B][D][T] fp64, weights [B][n_w] or None -> [B][2 D] (mean || std): the formulas of oracle/wespeaker_ref.py stats_pool in
    fp64, the weights gathered at nearest_index (or at `index`, to state what another map would give)."""
    x = x.to(F64)
    if weights is None:
        return torch.cat([x.mean(dim=-1), x.std(dim=-1, unbiased=True)], dim=-1)
    idx = nearest_index(x.shape[-1], weights.shape[-1]) if index is None else torch.as_tensor(index).long()
    w = weights.to(F64)[:, idx].unsqueeze(1)                                      # [B][1][T]
    v1 = w.sum(dim=2) + 1e-8
    mean = torch.sum(x * w, dim=2) / v1
    v2 = torch.square(w).sum(dim=2)
    var = torch.sum(torch.square(x - mean.unsqueeze(2)) * w, dim=2) / (v1 - v2 / v1 + 1e-8)
    return torch.cat([mean, torch.sqrt(var)], dim=-1)


def tstp(x: torch.Tensor, weights: torch.Tensor = None, mask_chunk=None) -> torch.Tensor:
    """x NCHW [n][256][10][W4] -> pooled [n_masks][5120]: mean at c * 10 + h, std at 2560 + c * 10 + h."""
    n, C, H, W = x.shape
    flat = x.reshape(n, C * H, W)
    if mask_chunk is not None:
        flat = flat[torch.as_tensor(mask_chunk).long()]
    return stats_pool(flat, weights)


def linear(pooled: torch.Tensor, w: torch.Tensor, b: torch.Tensor):
    """-> (pooled @ w^T + b, sum |p w| + |b|) in fp64."""
    p, w, b = pooled.to(F64), w.to(F64), b.to(F64)
    return p @ w.T + b, p.abs() @ w.abs().T + b.abs()


# ---------------------------------------------------------------------------------------------- the convolution bound and what it sees
def conv_bound(ref: torch.Tensor, abs_sum: torch.Tensor, K: int) -> torch.Tensor:
    """Elementwise bound of a bf16-output, fp32-accumulated convolution with K products per output: 2^-8 |ref| for the output
    rounding (bf16 keeps 8 significant bits: round-to-nearest moves a value by less than 2^-8 of it) plus K 2^-23 abs_sum for K
    fp32 multiply-adds in any order (each rounds by at most 2^-24 of a partial sum, which abs_sum bounds; the factor 2 also covers
    the output rounding acting on the accumulated value instead of on ref).  ReLU is 1-Lipschitz, so the bound carries through it."""
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * abs_sum


def conv_faults(x: torch.Tensor, w: torch.Tensor, shift: torch.Tensor, stride: int, relu: bool, resid: torch.Tensor = None):
    """What four near-misses of a convolution kernel would compute, as {name: (output, region)}; region is a bool mask of the output
    pixels the fault touches.  A test shows that each differs from conv(...) by more than conv_bound somewhere in its region."""
    out = {}
    W = x.shape[-1]
    out["shift x"] = (conv(torch.roll(x, 1, dims=3), w, shift, stride, relu, resid)[0], None)
    out["shift y"] = (conv(torch.roll(x, 1, dims=2), w, shift, stride, relu, resid)[0], None)
    if w.shape[-1] == 3:
        ws = w.clone()
        ws[:, :, 0, 0], ws[:, :, 0, 1] = w[:, :, 0, 1], w[:, :, 0, 0]
        out["tap swap"] = (conv(x, ws, shift, stride, relu, resid)[0], None)
    xd = x.clone()
    last = W - 1 if w.shape[-1] == 3 else stride * ((W - 1) // stride)          # the last input column the convolution reads
    xd[..., last] = 0.0
    y = conv(xd, w, shift, stride, relu, resid)[0]
    ind = torch.zeros_like(x[:1, :1])
    ind[..., last] = 1.0
    reads = F.conv2d(ind, torch.ones(1, 1, *w.shape[2:], dtype=x.dtype), stride=stride, padding=w.shape[-1] // 2) > 0
    out["last column dropped"] = (y, reads.expand_as(y))                          # the output pixels that read the column
    return out


def fault_visibility(cin: int, cout: int, k: int, stride: int, H: int = 4, W: int = 9) -> dict:
    """{fault: fraction of the affected output pixels where it moves the fp64 reference by more than conv_bound}, on one random case
    of the given geometry.  Outside its region a fault must not exceed the bound at all (asserted here)."""
    g = torch.Generator().manual_seed(cin + k + stride)
    x = bf16_round(torch.randn(1, cin, H, W, generator=g, dtype=F64))
    w = fold_weight(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k), 1 + 0.1 * torch.randn(cout, generator=g))
    shift = 0.1 * torch.randn(cout, generator=g)
    ref, a = conv(x, w, shift, stride, True)
    bound = conv_bound(ref, a, k * k * cin)
    seen = {}
    for name, (y, region) in conv_faults(x, w, shift, stride, True).items():
        over = (y - ref).abs() > bound
        if region is not None:
            assert not bool(over[~region].any()), name
            over = over[region]
        seen[name] = float(over.double().mean())
    return seen
