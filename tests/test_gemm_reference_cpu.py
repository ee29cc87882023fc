"""CPU: the fp64 reference of the GEMM family's descriptor semantics (tests/gemm_reference.py) checked on its own.

1. Convolution equivalence: descriptors built the way csrc/resnet.hip run_conv and csrc/whisper.hip (conv1, conv2) build them --
   the padded-NHWC and the (T + 2)-row layouts restated here at small sizes -- give torch's conv2d / conv1d in fp64 on the valid
   pixels (< 1e-12) and leave every pad position untouched.
2. Discriminating power: the comparator rejects the output of a descriptor that differs from the right one by ONE unit in one
   field.  Subtly wrong kernel output cannot pass a comparator that rejects these.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_reference as R

SENT = -7.0


def _bf(x):
    return x.to(torch.bfloat16)


def _pad_to(n, m):
    return (n + m - 1) // m * m


# ---- ResNet: one convolution as a GEMM over a strided view of the padded NHWC input (run_conv) ----------------------------------
def _resnet_case(k, stride, n_img=2, H=6, W=7, cin=16, cout=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    Wp = W + 2
    x = _bf(torch.randn(n_img, cin, H, W, generator=g))
    w = _bf(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5)
    bias = torch.randn(cout, generator=g)
    Kpad = _pad_to(k * cin, 64)
    packed = torch.zeros(cout, k, Kpad, dtype=torch.bfloat16)                  # [o][kh][kw * cin + c], a kh row padded to Kpad
    packed[:, :, :k * cin] = w.permute(0, 2, 3, 1).reshape(cout, k, k * cin)
    xin = torch.zeros(n_img, H + 2, Wp, cin, dtype=torch.bfloat16)             # padded NHWC, zero halo
    xin[:, 1:H + 1, 1:W + 1] = x.permute(0, 2, 3, 1)
    Ho, Wo = H // stride, (W - 1) // stride + 1
    Wpo = Wo + 2
    RI = (H + 2) // stride
    M = n_img * RI * Wp
    a_off = (Wp + 1) * cin if k == 1 else 0
    d = dict(epi=R.EPI_BF16_ADD_RELU, lda=stride * cin, K=Kpad, ntaps=k, a_tap_stride=Wp * cin, ldw=k * Kpad, M=M, N=cout, ldo=_pad_to(cout, 16),
             rpb_in=Wp, rpb_valid=Wo, rpb_out=Wpo, roff=Wpo + 1, img_rows_in=RI, img_rows_valid=Ho, img_rows_out=Ho + 2, ldrb=_pad_to(cout, 16))
    need = (M - 1) * d["lda"] + (k - 1) * d["a_tap_stride"] + Kpad
    A = torch.zeros(max(need, xin.numel() - a_off) + 64, dtype=torch.bfloat16)  # the last rows' windows run past the image (dropped rows)
    A[:xin.numel() - a_off] = xin.flatten()[a_off:]
    resid = _bf(torch.randn(n_img, Ho + 2, Wpo, d["ldrb"], generator=g))
    out = torch.full((n_img * (Ho + 2) * Wpo * d["ldo"],), SENT, dtype=torch.bfloat16)
    t = dict(A=A, W=packed.flatten(), bias=bias, out=out, resid_bf16=resid.flatten())
    conv = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=1 if k == 3 else 0)   # [n, cout, Ho, Wo]
    want = torch.relu(conv.permute(0, 2, 3, 1) + resid[:, 1:Ho + 1, 1:Wo + 1, :cout].double())
    return d, t, want, (n_img, Ho, Wo, Wpo)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 2)])
def test_reference_is_the_resnet_convolution(k, stride):
    d, t, want, (n, Ho, Wo, Wpo) = _resnet_case(k, stride)
    e = R.gemm_reference(d, t)["out"]
    ldo, N = d["ldo"], d["N"]
    ref = e["ref"].view(n, Ho + 2, Wpo, ldo)
    assert float((ref[:, 1:Ho + 1, 1:Wo + 1, :N] - want).abs().max()) < 1e-12
    interior = torch.zeros(n, Ho + 2, Wpo, ldo, dtype=torch.bool)
    interior[:, 1:Ho + 1, 1:Wo + 1, :N] = True
    assert torch.equal(e["checked"].view_as(interior), interior)               # exactly the valid pixels carry asserted values
    scratch = torch.zeros_like(interior)
    scratch[:, 1:Ho + 1, 1:Wo + 1, :R.ceil16(N)] = True
    assert torch.equal(e["writable"].view_as(interior), scratch)               # the halo (pad rows and columns) is never writable
    assert bool((ref[~interior] == SENT).all())


# ---- Whisper conv stem at T = 40 (the model: T = 3000, rows 3000 -> 3002) -------------------------------------------------------
def _whisper_stem(T=40, B=2, n_mels=20, D=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    mel = _bf(torch.randn(B, n_mels, T, generator=g))
    w1 = _bf(torch.randn(D, n_mels, 3, generator=g) / (3 * n_mels) ** 0.5)
    b1 = torch.randn(D, generator=g)
    w2 = _bf(torch.randn(D, D, 3, generator=g) / (3 * D) ** 0.5)
    b2 = torch.randn(D, generator=g)
    pos = torch.randn(T // 2, D, generator=g)
    return mel, w1, b1, w2, b2, pos


def test_reference_is_whisper_conv1():
    T, B, n_mels, D = 40, 2, 20, 16
    mel, w1, b1, _, _, _ = _whisper_stem(T, B, n_mels, D)
    K = _pad_to(3 * n_mels, 64)
    melp = F.pad(mel, (1, 1))
    im2col = torch.zeros(B * T, K, dtype=torch.bfloat16)                       # row (b, t): mel[b, c, t - 1 + kk] at column c * 3 + kk
    im2col[:, :3 * n_mels] = melp.unfold(2, 3, 1).permute(0, 2, 1, 3).reshape(B * T, 3 * n_mels)
    Wm = torch.zeros(D, K, dtype=torch.bfloat16)
    Wm[:, :3 * n_mels] = w1.reshape(D, 3 * n_mels)
    d = dict(epi=R.EPI_BF16_GELU, lda=K, ldw=K, M=B * T, N=D, K=K, ldo=D, rpb_in=T, rpb_out=T + 2, roff=1, rpb_valid=T)
    out = torch.full((B * (T + 2) * D,), SENT, dtype=torch.bfloat16)
    e = R.gemm_reference(d, dict(A=im2col.flatten(), W=Wm.flatten(), bias=b1, out=out))["out"]
    want = F.gelu(F.conv1d(mel.double(), w1.double(), b1.double(), padding=1)).permute(0, 2, 1)     # [B, T, D]
    ref = e["ref"].view(B, T + 2, D)
    assert float((ref[:, 1:T + 1] - want).abs().max()) < 1e-12
    assert bool((ref[:, 0] == SENT).all()) and bool((ref[:, T + 1] == SENT).all())
    w = e["writable"].view(B, T + 2, D)
    assert not bool(w[:, 0].any()) and not bool(w[:, T + 1].any()) and bool(w[:, 1:T + 1].all())


def test_reference_is_whisper_conv2():
    T, B, n_mels, D = 40, 2, 20, 16
    _, _, _, w2, b2, pos = _whisper_stem(T, B, n_mels, D)
    g = torch.Generator().manual_seed(2)
    h = _bf(torch.randn(B, T, D, generator=g))                                  # conv1's output, time-major
    h1 = torch.zeros(B, T + 2, D, dtype=torch.bfloat16)                         # rows 0 and T + 1 of every sequence are the zero padding
    h1[:, 1:T + 1] = h
    S = T // 2
    M = B * (S + 1)
    A = torch.zeros((M - 1) * 2 * D + 3 * D, dtype=torch.bfloat16)              # the last (dropped) row reads one row past h1
    A[:h1.numel()] = h1.flatten()
    Wm = w2.permute(0, 2, 1).reshape(D, 3 * D)                                  # [o][kk * D + c]
    d = dict(epi=R.EPI_F32_GELU_POS, lda=2 * D, ldw=3 * D, M=M, N=D, K=3 * D, ldo=D, ldr=D, resid_mod=S, rpb_in=S + 1, rpb_out=S, roff=0,
             rpb_valid=S)
    out = torch.full((B * S * D,), SENT, dtype=torch.float32)
    e = R.gemm_reference(d, dict(A=A, W=Wm.contiguous().flatten(), bias=b2, out=out, resid=pos.flatten()))["out"]
    want = F.gelu(F.conv1d(h.permute(0, 2, 1).double(), w2.double(), b2.double(), stride=2, padding=1)).permute(0, 2, 1) + pos.double()
    assert float((e["ref"].view(B, S, D) - want).abs().max()) < 1e-12
    assert bool(e["checked"].all())                                             # every row of x is written: B * S rows out of B * (S + 1)


# ---- discriminating power -------------------------------------------------------------------------------------------------------
def _remap_case():
    """taps + both remap levels + ragged N + fp32 residual modulo resid_mod, small."""
    g = torch.Generator().manual_seed(3)
    d = dict(epi=R.EPI_F32_RESID, lda=64, ldw=192, M=2 * 5 * 10, N=20, K=64, ntaps=3, a_tap_stride=640, ldo=32, ldr=32, resid_mod=13,
             rpb_in=10, rpb_valid=7, rpb_out=9, roff=10, img_rows_in=5, img_rows_valid=4, img_rows_out=6)
    t = dict(A=_bf(torch.randn(99 * 64 + 2 * 640 + 64 + 64, generator=g)), W=_bf(torch.randn(20 * 192, generator=g) / 192 ** 0.5),
             bias=torch.randn(20, generator=g), resid=torch.randn(16 * 32, generator=g),
             out=torch.full((160 * 32,), SENT, dtype=torch.float32))
    return d, t


def _heads_case():
    g = torch.Generator().manual_seed(4)
    d = dict(epi=R.EPI_HEADS, lda=64, ldw=64, M=24, N=256, K=64, d_model=128, n_head=2, S=12, Spad=16, v_transposed=0, first_block=0)
    n = 2 * 2 * 16 * 64
    t = dict(A=_bf(torch.randn(24 * 64, generator=g)), W=_bf(torch.randn(256 * 64, generator=g) / 8), bias=torch.randn(256, generator=g))
    for k in ("hq", "hk", "hv"):
        t[k] = torch.full((n,), SENT, dtype=torch.bfloat16)
    return d, t


def _rejected(d, t, d2, t2):
    exp = R.gemm_reference(d, t)
    other = R.gemm_reference(d2, t2)
    for name, e in exp.items():
        assert R.compare(e, R.round_like(e)).ok                                 # the right answer passes ...
    verdicts = [R.compare(e, R.round_like(other[name])) if name in other else None for name, e in exp.items()]
    return any(v is None or not v.ok for v in verdicts) or set(other) != set(exp)


MUTATIONS = [("roff", +1), ("roff", -1), ("rpb_valid", -1), ("rpb_valid", +1), ("img_rows_valid", -1), ("img_rows_valid", +1),
             ("resid_mod", +1), ("resid_mod", -1), ("a_tap_stride", +8), ("a_tap_stride", -8), ("ntaps", -1), ("rpb_out", +1),
             ("img_rows_out", +1)]


@pytest.mark.parametrize("field,delta", MUTATIONS)
def test_comparator_rejects_one_unit_descriptor_mutations(field, delta):
    d, t = _remap_case()
    d2 = dict(d)
    d2[field] += delta
    assert _rejected(d, t, d2, t), (field, delta)


def test_comparator_rejects_a_skipped_middle_tap_and_a_shifted_bias():
    d, t = _remap_case()
    t2 = dict(t)
    W = t["W"].clone().view(20, 192)
    W[:, 64:128] = 0                                                             # the middle tap contributes nothing
    t2["W"] = W.flatten()
    assert _rejected(d, t, d, t2)
    t3 = dict(t)
    t3["bias"] = torch.roll(t["bias"], 1)                                        # bias[n - 1] in column n
    assert _rejected(d, t, d, t3)


def test_comparator_rejects_first_block_and_v_layout():
    d, t = _heads_case()
    d2 = dict(d, first_block=1)
    assert _rejected(d, t, d2, t)
    d3, t3 = dict(d, first_block=1), t
    d4 = dict(d3, v_transposed=1)                                                # k, v  against  k, V^T
    assert _rejected(d3, t3, d4, t3)


@pytest.mark.parametrize("epi", [R.EPI_BF16, R.EPI_BF16_GELU, R.EPI_BF16_RELU, R.EPI_BF16_LRELU_AFFINE, R.EPI_BF16_ADD_RELU])
def test_comparator_rejects_mutations_at_bf16_precision(epi):
    """The bf16 allowance (one rounding) is wide next to fp32's: the same one-unit mutations must still be rejected under it."""
    g = torch.Generator().manual_seed(5 + epi)
    d, t = _remap_case()
    d = dict(d, epi=epi, resid_mod=0, ldrb=32, slope=0.01)
    t = dict(t, out=torch.full((160 * 32,), SENT, dtype=torch.bfloat16), resid=torch.randn(160 * 32, generator=g),
             resid_bf16=_bf(torch.randn(160 * 32, generator=g)), scale=torch.randn(20, generator=g), shift=torch.randn(20, generator=g))
    for field, delta in [("roff", 1), ("rpb_valid", -1), ("img_rows_valid", -1), ("a_tap_stride", 8), ("ntaps", -1)]:
        d2 = dict(d)
        d2[field] += delta
        assert _rejected(d, t, d2, t), (field, delta)
    if epi in (R.EPI_BF16_LRELU_AFFINE, R.EPI_BF16_ADD_RELU):
        key = "resid" if epi == R.EPI_BF16_LRELU_AFFINE else "resid_bf16"
        t2 = dict(t)
        t2[key] = torch.roll(t[key], 32)                                         # the residual one row off
        assert _rejected(d, t, d, t2)


def test_comparator_rejects_a_touched_pad_element_and_a_one_ulp_error():
    d, t = _remap_case()
    e = R.gemm_reference(d, t)["out"]
    good = R.round_like(e)
    bad = good.clone()
    pad = int(torch.nonzero(~e["writable"]).flatten()[5])
    bad[pad] = 0.0                                                               # a pad element that stopped being the sentinel
    assert not R.compare(e, bad).ok
    bad = good.clone()
    k = int(torch.nonzero(e["checked"]).flatten()[7])
    bad[k] = bad[k] + 4e-4                                                       # far inside any rel-L2 bound, far outside the element budget
    v = R.compare(e, bad)
    assert not v.ok and v.rel_l2 < 2e-5
    scratch = good.clone()
    scratch[e["writable"] & ~e["checked"]] = 123.0                               # columns N .. ceil16(N): free
    assert R.compare(e, scratch).ok
