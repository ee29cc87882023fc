"""CPU restatement of `noisereduce.reduce_noise` beyond the corner oracle/spectral_gate_ref.py covers: the non-stationary mode
(`stationary=False`, the package default) with its tunables, and the stationary mode with a separate noise clip (`y_noise`).

TEST INFRASTRUCTURE ONLY.  Follows noisereduce's `SpectralGateNonStationary.spectral_gating_nonstationary`,
`get_time_smoothed_representation` and `sigmoid` from recollection [UPSTREAM-RECALL]; the package is not installed and no fixture
exists, so this is **parity unpinned** exactly as the stationary restatement is.  The time smoothing is `scipy.signal.filtfilt`
itself, NOT the closed-form recursion the kernels implement (`smooth_time_closed_form` below restates that one for the CPU tests).

Per padded chunk (chunking, padding and STFT are those of the stationary path):
    A = |X|;  t = time_constant_s * sr / hop;  b = (sqrt(1 + 4 t^2) - 1) / (2 t^2)
    S = filtfilt([b], [1, b - 1], A, axis=time, padtype=None)
    M = sigmoid(((A - S) / S - thresh_n_mult_nonstationary) * sigmoid_slope_nonstationary)
    M = fftconvolve(M, smoothing_filter, "same");  M = M * prop_decrease + (1 - prop_decrease);  out = istft(X * M)
`variant` selects one deliberately WRONG rule (the non-degeneracy tests show that each lands far from the right one).
"""
from __future__ import annotations

import numpy as np
from scipy.signal import fftconvolve, filtfilt, istft, stft

from oracle.spectral_gate_ref import CHUNK, HOP, N_FFT, PADDING, _filter_chunk, _thresholds, smoothing_filter

VARIANTS = (None, "forward_only", "zero_init", "scale_before", "no_smoothing")

# Bounds of the GPU parity tests: at most 2.5 x the worst value measured on the MI355X against THIS restatement
# (profiles/specgate_nonstationary_measured_deviations.json).  The CPU non-degeneracy test needs the waveform one too.
GPU_WAVEFORM_BOUND = 6.5e-7    # rel-L2 of the denoised waveform, non-stationary mode, one chunk     (measured 2.65e-7)
GPU_CHUNKED_BOUND = 2.9e-7     # the same over a signal of several chunks                              (measured 1.16e-7)
GPU_SEAM_BOUND = 2.9e-7        # rel-L2 of the 4000 samples around a chunk seam                        (measured 1.19e-7)
GPU_SMOOTH_BOUND = 4.9e-6      # max |S - ref| / max(ref) per row, time smoothing alone                (measured 1.99e-6)


def time_coefficient(time_constant_s: float, sr: int = 16000) -> float:
    t = time_constant_s * sr / HOP
    return float((np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t))


def smooth_time(A: np.ndarray, b: float) -> np.ndarray:
    """[..., T] -> forward-backward first-order smoothing along the last axis: scipy's filtfilt, no edge padding."""
    return filtfilt([b], [1.0, b - 1.0], np.asarray(A, dtype=np.float64), axis=-1, padtype=None)


def smooth_time_closed_form(A: np.ndarray, b: float, forward_only: bool = False, zero_init: bool = False) -> np.ndarray:
    """What filtfilt computes for this filter, written out: f[0] = A[0], f[t] = b A[t] + (1 - b) f[t-1]; S[T-1] = f[T-1],
    S[t] = b f[t] + (1 - b) S[t+1].  forward_only / zero_init are the wrong rules of the non-degeneracy tests."""
    A = np.asarray(A, dtype=np.float64)
    T = A.shape[-1]
    f = np.empty_like(A)
    f[..., 0] = b * A[..., 0] if zero_init else A[..., 0]
    for t in range(1, T):
        f[..., t] = b * A[..., t] + (1.0 - b) * f[..., t - 1]
    if forward_only:
        return f
    S = np.empty_like(A)
    S[..., T - 1] = b * f[..., T - 1] if zero_init else f[..., T - 1]
    for t in range(T - 2, -1, -1):
        S[..., t] = b * f[..., t] + (1.0 - b) * S[..., t + 1]
    return S


def sigmoid_mask(A: np.ndarray, S: np.ndarray, thresh_n_mult: float = 2.0, sigmoid_slope: float = 10.0) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return 1.0 / (1.0 + np.exp(-((A - S) / S - thresh_n_mult) * sigmoid_slope))


def _padded(y: np.ndarray, start: int, end: int) -> np.ndarray:
    n = y.shape[0]
    i1, i2 = start - PADDING, end + PADDING
    padded = np.zeros(i2 - i1, dtype=np.float32)
    a, b = max(i1, 0), min(i2, n)
    padded[a - i1:b - i1] = y[a:b]
    return padded


def _filter_chunk_nonstationary(y, start, end, sr, prop_decrease, b, thresh_n_mult, sigmoid_slope, variant=None) -> np.ndarray:
    padded = _padded(y, start, end)
    _, _, X = stft(padded, nfft=N_FFT, noverlap=N_FFT - HOP, nperseg=N_FFT, padded=False)
    A = np.abs(X)
    if variant in ("forward_only", "zero_init"):
        S = smooth_time_closed_form(A, b, forward_only=variant == "forward_only", zero_init=variant == "zero_init")
    else:
        S = smooth_time(A, b)
    M = sigmoid_mask(A, S, thresh_n_mult, sigmoid_slope)
    if variant is not None:      # a wrong rule as a kernel would realise it: S == 0 cells (the zero padding, forward only) take mask 0
        M = np.nan_to_num(M, nan=0.0)
    filt, _, _ = smoothing_filter(sr)
    if variant == "scale_before":
        M = fftconvolve(M * prop_decrease + (1.0 - prop_decrease), filt, mode="same")
    elif variant == "no_smoothing":
        M = M * prop_decrease + (1.0 - prop_decrease)
    else:
        M = fftconvolve(M, filt, mode="same")
        M = M * prop_decrease + (1.0 - prop_decrease)
    _, den = istft(X * M, nfft=N_FFT, noverlap=N_FFT - HOP, nperseg=N_FFT)
    out = np.zeros(padded.shape[0], dtype=np.float64)
    m = min(out.shape[0], den.shape[0])
    out[:m] = den[:m]
    return out[PADDING:PADDING + (end - start)]


def reduce_noise_nonstationary(y, sr: int = 16000, prop_decrease: float = 1.0, time_constant_s: float = 2.0,
                               thresh_n_mult_nonstationary: float = 2.0, sigmoid_slope_nonstationary: float = 10.0,
                               variant=None) -> np.ndarray:
    """reduce_noise(y, sr, stationary=False, ...): any length, chunk by chunk; a noise clip would be ignored."""
    assert variant in VARIANTS
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    n = y.shape[0]
    b = time_coefficient(time_constant_s, sr)
    out = np.zeros(n, dtype=np.float32)
    for start in range(0, n, CHUNK):
        end = min(start + CHUNK, n)
        out[start:end] = _filter_chunk_nonstationary(y, start, end, sr, prop_decrease, b, thresh_n_mult_nonstationary,
                                                     sigmoid_slope_nonstationary, variant).astype(np.float32)
    return out


def noise_thresholds(y_noise, n_std: float = 1.5, clip_noise_stationary: bool = True) -> np.ndarray:
    """Per-bin mean + n_std * std of the dB spectrogram of the noise clip (unpadded STFT, 80 dB floor under ITS per-bin maximum)."""
    y_noise = np.asarray(y_noise, dtype=np.float32).reshape(-1)
    return _thresholds(y_noise[:CHUNK] if clip_noise_stationary else y_noise, n_std)


def reduce_noise_stationary(y, y_noise=None, sr: int = 16000, prop_decrease: float = 1.0, n_std_thresh_stationary: float = 1.5,
                            clip_noise_stationary: bool = True) -> np.ndarray:
    """reduce_noise(y, sr, stationary=True, y_noise=, n_std_thresh_stationary=): the threshold from the noise clip (the signal when
    None), everything after the threshold as in oracle.spectral_gate_ref."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    n = y.shape[0]
    thresh = noise_thresholds(y if y_noise is None else y_noise, n_std_thresh_stationary, clip_noise_stationary)
    out = np.zeros(n, dtype=np.float32)
    for start in range(0, n, CHUNK):
        end = min(start + CHUNK, n)
        out[start:end] = _filter_chunk(y, start, end, thresh, sr, prop_decrease).astype(np.float32)
    return out
