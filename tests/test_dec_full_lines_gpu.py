"""GPU: the > 16-row decode chain's bf16 rows as fragment images between its kernels (csrc/decoder.h dec_frag_off, switch
CCX_DEC_PACKED_ACT), run away from the model through ccx_dec_ln_linear: the production launchers, producer and consumer as a pair --
dec_resolve_ln_kernel -> dec_linear<ACT_BF16, epi>, and dec_resolve_ln_kernel -> dec_linear<ACT_BF16, GELU> -> dec_linear<ACT_BF16,
PARTIAL> for the 3072-wide rows only the GELU epilogue produces.  The image puts the same 16 bytes into the same lane as the
row-major load, so every output must be BIT-equal to the row-major path; the row buffers and the outputs start as NaN bit patterns and
hold whole 16-row tiles, so a lane fed from a padding row or a quad never stored shows as a non-finite output.

Self attention has no case here: dec_attention_kernel<true> already asks for 8 keys x 128 B per wave instruction (lane = key l / 8,
chunk l % 8), there is no half-line form of it to compare with (profiles/dec_full_lines_experiment.txt, section 1).

Row counts: 17 and 32 (two row tiles, 16 columns per block), 65 (four row tiles per block, a second block row with one live row and
three tiles behind the image), 256 (32 columns per block: the decode lanes' instantiations)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARTIAL, F32, SELF_QKV, GELU = range(4)
EPI_NAME = {PARTIAL: "partial", F32: "f32", SELF_QKV: "self_qkv", GELU: "gelu"}

# (K, F, N, epi): every epilogue that reads or writes the two converted buffers in the > 16-row chain.  The LayerNorm rows feed q|k|v
# (SELF_QKV), fc1 (GELU) and the query of its own launch (F32); the GELU rows (K = 3072 = F) feed fc2 (PARTIAL, three K slices).
CASES_EVERY_M = [
    (768, 0, 2304, SELF_QKV), (768, 0, 96, F32), (768, 0, 96, GELU), (768, 0, 96, PARTIAL),
    (768, 3072, 96, PARTIAL),
    (128, 0, 384, SELF_QKV), (128, 0, 96, F32), (128, 0, 96, GELU), (128, 512, 96, PARTIAL),     # the mini width
]
CASES_WIDE = [(768, 0, 2304, F32), (768, 0, 2304, GELU), (768, 3072, 2304, PARTIAL)]              # M = 17 and 256 only
ROWS = (17, 32, 65, 256)

_cache = {}


def _weights(K, F, N):
    """host weights and device vectors of a shape, made once and left unchanged"""
    key = (K, F, N)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 + K + 7 * F + 13 * N)
        kin = F if F else K
        w = {"w": np.ascontiguousarray((torch.randn(N, kin, generator=g) / math.sqrt(kin)).numpy(), dtype=np.float32),
             "bias": (0.1 * torch.randn(N, generator=g)).cuda(),
             "ln_g": (1.0 + 0.1 * torch.randn(K, generator=g)).cuda(), "ln_b": (0.1 * torch.randn(K, generator=g)).cuda()}
        if F:
            w["w1"] = np.ascontiguousarray((torch.randn(F, K, generator=g) / math.sqrt(K)).numpy(), dtype=np.float32)
            w["b1"] = (0.1 * torch.randn(F, generator=g)).cuda()
        _cache[key] = w
    return _cache[key]


def _rows(K):
    """256 residual rows of width K with an offset and an outlier column, shared by every row count (row r is the same row everywhere)"""
    key = ("x", K)
    if key not in _cache:
        g = torch.Generator().manual_seed(77 + K)
        x = torch.randn(256, K, generator=g) + 0.5
        x[:, 3] *= 20.0
        _cache[key] = x.cuda()
    return _cache[key]


def _out_shape(M, K, F, N, epi):
    if epi == PARTIAL:
        kin = F if F else K
        return ((kin + 1023) // 1024, M, N)
    if epi == SELF_QKV:
        return (3, M, K)
    return (M, N)


def _run(ctx, M, K, F, N, epi, packed):
    from clearconverse_amd import _lib
    lib = _lib.load()
    w = _weights(K, F, N)
    x = _rows(K)[:M].contiguous()
    out = torch.full(_out_shape(M, K, F, N, epi), math.nan, device="cuda")
    d = _lib.DecLnLinearDesc()
    d.M, d.K, d.F, d.N, d.epi, d.packed = M, K, F, N, epi, packed
    d.x, d.x_elems, d.ln_g, d.ln_b, d.eps = x.data_ptr(), x.numel(), w["ln_g"].data_ptr(), w["ln_b"].data_ptr(), 1e-5
    if F:
        d.w1_host, d.b1 = w["w1"].ctypes.data, w["b1"].data_ptr()
    d.w_host, d.bias = w["w"].ctypes.data, w["bias"].data_ptr()
    d.out, d.out_elems = out.data_ptr(), out.numel()
    rc = lib.ccx_dec_ln_linear(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_ln_linear")
    return out.cpu()


def _both(ctx, M, case):
    K, F, N, epi = case
    rm = _run(ctx, M, K, F, N, epi, 0)
    pk = _run(ctx, M, K, F, N, epi, 1)
    what = (M, K, F, N, EPI_NAME[epi])
    assert torch.isfinite(rm).all() and torch.isfinite(pk).all(), what
    assert torch.equal(rm, pk), (what, float((rm - pk).abs().max()))
    return pk


@pytest.mark.parametrize("M", ROWS)
def test_packed_equals_row_major(ccx_ctx, M):
    for case in CASES_EVERY_M + (CASES_WIDE if M in (17, 256) else []):
        _both(ccx_ctx, M, case)


def test_rows_do_not_depend_on_the_launch_size(ccx_ctx):
    """a row's bits are the same in a 17-row and in a 256-row launch (other row tiles per block, other columns per block), in both
    layouts"""
    for K, F, N, epi in [(768, 0, 96, F32), (768, 0, 2304, SELF_QKV), (768, 3072, 96, PARTIAL), (768, 0, 96, GELU)]:
        for packed in (0, 1):
            small = _run(ccx_ctx, 17, K, F, N, epi, packed)
            big = _run(ccx_ctx, 256, K, F, N, epi, packed)
            assert torch.equal(small, big[..., :17, :]), (K, F, N, EPI_NAME[epi], packed)


def test_against_fp64(ccx_ctx):
    """that the pair computes LayerNorm -> linear at all.  Bound: both operands of every product are rounded to bf16 (relative error
    2^-9 each, 2^-8 per product at worst); over a row of independent terms the rel-L2 error stays below that figure, the fp32 sums add
    K 2^-24 at the most: 2^-8 + 768 * 2^-24 = 4.0e-3."""
    K, N, M = 768, 96, 65
    w = _weights(K, 0, N)
    got = _both(ccx_ctx, M, (K, 0, N, F32)).double()
    x = _rows(K)[:M].cpu().double()
    xn = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    xn = xn * w["ln_g"].cpu().double() + w["ln_b"].cpu().double()
    ref = xn @ torch.from_numpy(w["w"]).double().T + w["bias"].cpu().double()
    rel = float((got - ref).norm() / ref.norm())
    print(f"ln -> linear rel-L2 against fp64: {rel:.3e}")
    assert rel < 4.0e-3, rel


@pytest.mark.parametrize("what,change", [
    ("K = 100", dict(K=100)),
    ("SELF_QKV needs", dict(epi=SELF_QKV)),
    ("packed = 2", dict(packed=2)),
    ("out_elems", dict(out_elems=10)),
])
def test_rejections(ccx_ctx, what, change):
    from clearconverse_amd import _lib
    lib = _lib.load()
    w = _weights(768, 0, 96)
    x = _rows(768)[:17].contiguous()
    out = torch.full((17, 96), math.nan, device="cuda")
    d = _lib.DecLnLinearDesc()
    d.M, d.K, d.F, d.N, d.epi, d.packed = 17, 768, 0, 96, F32, 1
    d.x, d.x_elems, d.ln_g, d.ln_b, d.eps = x.data_ptr(), x.numel(), w["ln_g"].data_ptr(), w["ln_b"].data_ptr(), 1e-5
    d.w_host, d.bias, d.out, d.out_elems = w["w"].ctypes.data, w["bias"].data_ptr(), out.data_ptr(), out.numel()
    for name, val in change.items():
        setattr(d, name, val)
    rc = lib.ccx_dec_ln_linear(ccx_ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.CcxError) as e:
        ccx_ctx.check(rc, "ccx_dec_ln_linear")
    assert "ccx_dec_ln_linear" in str(e.value) and what in str(e.value), str(e.value)
    assert torch.isnan(out).all()
