"""-m gpu: the kernels the 1280-wide, 128-mel Whisper checkpoints added, on their own.

* ccx_layernorm in its 5-slot form (1024 < D <= 1280: layernorm_kernel<5>, a lane keeps five float4 of the row) against float64
  F.layer_norm of the same float32 inputs.  Shapes: (5, 1280) a ragged row block with all 64 lanes live in the fifth slot;
  (33, 1028) ONE live lane in it; (4, 1276) a ragged tail inside it (63 lanes); (7, 1152) a partly filled slot (32 lanes).
  Rows: the plain rows of tests/test_kernels_gpu.py::test_layernorm, rows offset by tests/stressed_whisper.py's MU levels (10, 35,
  both signs) and rows whose OUTLIER_CHANNELS carry +-OUTLIER_SCALE["full"] (alternating signs, as outlier_state_dict sets them).
  Bounds: LN_F32_ABS = 3e-6 and LN_BF16_ABS = 0.03 are the literals of tests/test_kernels_gpu.py::test_layernorm (restated: a
  literal cannot be imported).  The bf16 figure is taken relative to max(1, |y|): that test's rows normalise to |y| < 5, an outlier
  channel here to |y| ~ 20, where the one bf16 rounding alone is 0.04.
  Measured on an MI355X: 8.65e-7 at the worst (an outlier row of (33, 1028)); offset rows 1.2e-7 .. 1.5e-7.  With float statistics,
  as the 4-slot form keeps them, the offset-35 rows of (33, 1028) came out at 5.93e-6 -- the float mean's own rounding, ~ulp(35),
  divided by a row std of 1 -- which is why the 5-slot form computes in double (csrc/elementwise.hip).
* the 128-bin log-mel (logmel_power_kernel<128>, logmel_finalize_kernel<128>, mel_to_im2col_kernel<128>) against
  oracle.whisper_ref.log_mel_spectrogram(..., n_mels=128).  Bound: LOGMEL_ABS = 1e-4, the literal of
  tests/test_whisper_gpu.py::test_logmel_matches_oracle (the DFT is the same code; 128-bin filters are narrower, so a mel value sums
  fewer power bins than an 80-bin one).
"""
import numpy as np
import pytest
import torch

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R
from tests.conftest import within
from tests.stressed_whisper import MU, OUTLIER_CHANNELS, OUTLIER_SCALE

pytestmark = pytest.mark.gpu

LN_F32_ABS = 3e-6      # tests/test_kernels_gpu.py::test_layernorm, fp32 output
LN_BF16_ABS = 0.03     # tests/test_kernels_gpu.py::test_layernorm, bf16 output
LOGMEL_ABS = 1e-4      # tests/test_whisper_gpu.py::test_logmel_matches_oracle


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _layernorm(ccx_ctx, x, gamma, beta):
    M, D = x.shape
    ob = torch.empty(M, D, dtype=torch.bfloat16, device="cuda")
    of = torch.empty(M, D, dtype=torch.float32, device="cuda")
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    ccx_ctx.check(ccx_ctx.lib.ccx_layernorm(ccx_ctx.handle, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), ob.data_ptr(), of.data_ptr(),
                                            M, D, 1e-5, _stream()), "layernorm")
    torch.cuda.synchronize()
    return of.cpu(), ob.cpu()


def _stressed_rows(M, D, g):
    """row r: kind r % 4 -- plain, offset MU[10], offset MU[40] (signs alternate), outlier channels"""
    x = torch.randn(M, D, generator=g)
    for r in range(M):
        kind = r % 4
        if kind == 0:
            x[r] = x[r] * 3 + 0.5
        elif kind == 1:
            x[r] += MU[10] * (1.0 if r % 8 < 4 else -1.0)
        elif kind == 2:
            x[r] += MU[40] * (1.0 if r % 8 < 4 else -1.0)
        else:
            for i, c in enumerate(OUTLIER_CHANNELS):
                x[r, c] += OUTLIER_SCALE["full"] * (1.0 if i % 2 == 0 else -1.0)
    return x.contiguous()


@pytest.mark.parametrize("M,D", [(5, 1280), (33, 1028), (4, 1276), (7, 1152)])
def test_layernorm_five_slots(ccx_ctx, M, D):
    g = torch.Generator().manual_seed(M + D)
    x = _stressed_rows(M, D, g)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    of, ob = _layernorm(ccx_ctx, x, gamma, beta)
    assert torch.isfinite(of).all()
    err = (of.double() - ref).abs().max(1).values
    for kind, name in enumerate(("plain", "offset 10", "offset 35", "outlier channels")):
        rows = list(range(kind, M, 4))
        print(f"layernorm 5-slot ({M}, {D}) {name}: max abs error {float(err[rows].max()):.3e}")
    within("layernorm_kernel<5>: fp32 output max abs error, stressed rows", float(err.max()), LN_F32_ABS, (M, D, int(err.argmax())))
    within("layernorm_kernel<5>: bf16 output max abs error / max(1, |y|)",
           float(((ob.double() - ref).abs() / ref.abs().clamp(min=1.0)).max()), LN_BF16_ABS, (M, D))
    # the last column of every row comes from the last live lane of the fifth slot; nothing behind a row is touched (ld == D: the next
    # row's first columns would show it)
    assert float((of[:, -4:].double() - ref[:, -4:]).abs().max()) < LN_F32_ABS


@pytest.mark.parametrize("M,D", [(33, 1024), (1500, 768)])
def test_layernorm_four_slot_widths_still_take_the_four_slot_form(ccx_ctx, M, D):
    """D <= 1024 dispatches to the unchanged 4-slot instantiation: the figures of tests/test_kernels_gpu.py hold, and a second call
    returns the same bits"""
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 3 + 0.5
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    of1, ob1 = _layernorm(ccx_ctx, x, gamma, beta)
    of2, ob2 = _layernorm(ccx_ctx, x, gamma, beta)
    assert torch.equal(of1, of2) and torch.equal(ob1.view(torch.int16), ob2.view(torch.int16))
    ref = torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-5)
    within("layernorm_kernel: fp32 output max abs error", float((of1 - ref).abs().max()), LN_F32_ABS, (M, D))


def test_layernorm_refuses_more_than_five_slots(ccx_ctx):
    x = torch.zeros(4, 1284, device="cuda")
    w = torch.ones(1284, device="cuda")
    of = torch.empty(4, 1284, device="cuda")
    rc = ccx_ctx.lib.ccx_layernorm(ccx_ctx.handle, x.data_ptr(), w.data_ptr(), w.data_ptr(), None, of.data_ptr(), 4, 1284, 1e-5, _stream())
    assert rc != 0 and b"1280" in ccx_ctx.lib.ccx_last_error(ccx_ctx.handle)


# ---------------------------------------------------------------------------------------------------------------- log-mel, 128 bins
@pytest.fixture(scope="module")
def mel128(ccx_ctx):
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=1, n_state=128, n_mels=128)
    sd = synthetic_whisper_state_dict(dims, seed=3)
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx)
    yield dims, sd, m
    m.close()


def _clips(lengths_s, seed0=0):
    clips = [synthetic_clip(seed0 + i, 30.0)[: int(s * 16000)] for i, s in enumerate(lengths_s)]
    n = [len(c) for c in clips]
    host = np.zeros((len(clips), max(n)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return clips, n, torch.from_numpy(host).cuda()


def test_logmel_128_matches_oracle(mel128):
    dims, sd, m = mel128
    clips, n, dev = _clips([30.0, 9.0, 0.7, 2.013])
    mel = m.log_mel(dev, n, return_mel=True).cpu()
    assert mel.shape == (4, 128, 3000) and torch.isfinite(mel).all()
    for b, c in enumerate(clips):
        full = R.log_mel_spectrogram(torch.from_numpy(c), n_mels=128)
        content = len(c) // 160
        ref = R.pad_or_trim(full[:, : min(3000, content)], 3000)
        assert ref.shape == (128, 3000)
        within("whisper: 128-bin log-mel max abs error", float((mel[b] - ref).abs().max()), LOGMEL_ABS, b)


def test_logmel_128_seek_window(mel128):
    dims, sd, m = mel128
    clips, n, dev = _clips([12.0])
    seek = 500
    mel = m.log_mel(dev, n, seek=[seek], return_mel=True).cpu()
    full = R.log_mel_spectrogram(torch.from_numpy(clips[0]), n_mels=128)
    content = len(clips[0]) // 160
    ref = R.pad_or_trim(full[:, seek: seek + min(3000, content - seek)], 3000)
    within("whisper: 128-bin log-mel max abs error", float((mel[0] - ref).abs().max()), LOGMEL_ABS, "seek")


def test_set_mel_128_equals_the_logmel_path(mel128):
    dims, sd, m = mel128
    clips, n, dev = _clips([8.0, 30.0])
    mel = m.log_mel(dev, n, return_mel=True)
    xa1 = m.encode(2, return_xa=True).clone()
    m.log_mel(dev[:1].contiguous(), n[:1])          # something else in the staging buffer in between
    m.set_mel(mel.contiguous())
    xa2 = m.encode(2, return_xa=True)
    assert torch.isfinite(xa1).all() and torch.equal(xa1, xa2)   # same im2col bits -> same kernels -> bit-identical
    ref = R.WhisperRef(R.Dims(**dims.__dict__), sd).encode(mel.cpu())
    rel = float((xa1.cpu().double() - ref.double()).norm() / ref.double().norm())
    within("whisper mini: encoder output rel-L2", rel, 8e-3, "128 mels")     # the bound of tests/test_whisper_gpu.py::test_encoder_mini
