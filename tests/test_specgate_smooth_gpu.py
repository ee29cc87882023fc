"""-m gpu: the time-smoothing kernels of the non-stationary spectral gate (csrc/spectral_gate.hip: forward-backward first-order
recursion over 64-frame segments, three launches) on their own through ccx_specgate_time_smooth, against scipy.signal.filtfilt in
fp64 (tests/nonstationary_gate_reference.smooth_time) on matrices the test chooses.  A "row" is one bin's time series; the bins of
one launch hold every row kind.  The coefficient handed to the kernel is an fp32 number, and the reference runs on that number.
Error measure: max |S - ref| / max(ref) per row."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import within
from tests import nonstationary_gate_reference as R

pytestmark = pytest.mark.gpu

LD, BINS, SEG, CAP = 520, 513, 64, 2580
SENTINEL = -7.25


@pytest.fixture(scope="module")
def gate(ccx_ctx):
    from clearconverse_amd.denoise import SpectralGate
    g = SpectralGate(max_samples=16000, max_clips=4, ctx=ccx_ctx)
    yield g
    g.close()


def _rows(T: int, seed: int) -> np.ndarray:
    """[513 bins, T]: 0 constant, 1 / 2 / 3 impulse at the first / a middle / the last frame, 4 step, 5 all zero, the rest random
    magnitudes over six decades."""
    rng = np.random.default_rng(seed)
    A = 10.0 ** rng.uniform(-5, 1, (BINS, T))
    A[0] = 0.37
    A[1:6] = 0.0
    A[1, 0] = 1.0
    A[2, T // 2] = 1.0
    A[3, T - 1] = 1.0
    A[4, T // 3:] = 2.5
    return A.astype(np.float32)


def _smooth(gate, mats, b32: float, stride_rows: int):
    """mats: list of [513, T_i] f32 -> (list of S [513, T_i], the untouched tail rows of every clip)."""
    B = len(mats)
    a = torch.zeros((B, stride_rows, LD), dtype=torch.float32)
    for i, m in enumerate(mats):
        a[i, : m.shape[1], :BINS] = torch.from_numpy(np.ascontiguousarray(m.T))
    a = a.cuda()
    s = torch.full((B, stride_rows, LD), SENTINEL, dtype=torch.float32, device="cuda")
    nf = (C.c_int * B)(*[m.shape[1] for m in mats])
    rc = gate.lib.ccx_specgate_time_smooth(gate.handle, a.data_ptr(), s.data_ptr(), nf, B, stride_rows, float(b32),
                                           torch.cuda.current_stream().cuda_stream)
    gate.ctx.check(rc, "ccx_specgate_time_smooth")
    s = s.cpu().numpy()
    return [s[i, : m.shape[1], :BINS].T for i, m in enumerate(mats)], [s[i, m.shape[1]:] for i, m in enumerate(mats)]


def _check(name, S, A, b32):
    ref = R.smooth_time(A.astype(np.float64), float(b32))
    assert np.isfinite(S).all()
    zero = ref.max(axis=1) == 0
    assert zero[5] and np.all(S[zero] == 0)                    # the all-zero row comes out exactly zero
    err = np.abs(S[~zero] - ref[~zero]).max(axis=1) / ref[~zero].max(axis=1)
    within(name, err.max(), R.GPU_SMOOTH_BOUND, ctx=int(np.argmax(err)))


@pytest.mark.parametrize("tc", [2.0, 0.05, 10.0])
@pytest.mark.parametrize("T", [1, 2, 3, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 235, CAP])
def test_smoothing_against_filtfilt(gate, T, tc):
    b32 = np.float32(R.time_coefficient(tc))
    A = _rows(T, seed=T)
    (S,), (tail,) = _smooth(gate, [A], b32, stride_rows=T + 2)
    assert np.all(tail == SENTINEL)                            # rows past n_frames are left alone
    _check("specgate time smoothing: max |S - filtfilt| / max(filtfilt) per row", S, A, b32)


def test_three_clips_of_different_length_in_one_launch(gate):
    b32 = np.float32(R.time_coefficient(2.0))
    mats = [_rows(T, seed=100 + T) for T in (300, 1, 131)]
    Ss, tails = _smooth(gate, mats, b32, stride_rows=320)
    for A, S, tail in zip(mats, Ss, tails):
        assert np.all(tail == SENTINEL)
        _check("specgate time smoothing: max |S - filtfilt| / max(filtfilt) per row", S, A, b32)
        (alone,), _ = _smooth(gate, [A], b32, stride_rows=A.shape[1])
        assert np.array_equal(alone, S)                        # a clip does not depend on its neighbours in the launch


def test_refusals(gate):
    lib, h = gate.lib, gate.handle
    a = torch.zeros((1, 4, LD), device="cuda"); s = torch.zeros_like(a)

    def call(nf, B=1, stride=4, b=0.1, s_=s):
        arr = (C.c_int * len(nf))(*nf)
        rc = lib.ccx_specgate_time_smooth(h, a.data_ptr(), s_.data_ptr(), arr, B, stride, b, None)
        return rc, lib.ccx_last_error(gate.ctx.handle).decode()

    for kw, field in ((dict(nf=[0]), "n_frames[0]"), (dict(nf=[5]), "n_frames[0]"), (dict(nf=[CAP + 1], stride=CAP + 1), "n_frames[0]"),
                      (dict(nf=[1] * 5, B=5), "B = 5"), (dict(nf=[2], b=0.0), "b = 0"), (dict(nf=[2], b=1.5), "b = 1.5"),
                      (dict(nf=[2], s_=a), "aliases")):
        rc, msg = call(**kw)
        assert rc == 1 and "ccx_specgate_time_smooth" in msg and field in msg, (kw, msg)
