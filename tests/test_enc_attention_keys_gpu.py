"""-m gpu: enc_attention_kernel with a key count PER SEQUENCE (csrc/attention.hip `n_keys`, the reduced audio context of the Whisper
encoder), through the C ABI (ccx_enc_attention_keys):
  * rows below a sequence's count against fp64 softmax attention over its first `count` keys, from the same bf16 inputs, with the
    bounds of tests/test_kernels_gpu.py::test_enc_attention (P is rounded to bf16 before P.V and the output is bf16: ~2^-8 relative);
  * all counts equal to S: the bits of ccx_enc_attention;
  * a sequence with count k: the bits of the same sequence run alone through ccx_enc_attention at S = k;
  * rows at or beyond the count: zeros (finite, deterministic);
  * counts outside [1, S] and a null count array are refused.
Counts 1, 63, 64, 65, 128, 129, 200 at S = 200: one key, one key short of a key tile, exactly one, one more (a ragged second tile), a
whole query tile (the second query tile of the block row is then skipped), one more, all.
Measured on an MI355X: rel-L2 1.79e-3 (bound 4e-3), max abs 1.51e-2 (bound 0.06); profiles/audio_ctx_measured_deviations.json."""
import ctypes as C

import pytest
import torch

from tests.conftest import within

pytestmark = pytest.mark.gpu

REL_BOUND, ABS_BOUND = 4e-3, 0.06          # test_enc_attention's


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _inputs(B, H, S, Spad, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16)
    k = torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16)
    v = torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16)
    k[:, :, ::37] *= 4.0                     # a few large scores in every key tile: the running maximum moves late as well
    return q, k, v


def _padded(q, k, v, Spad, keep=None):
    """the kernel's layouts; keep: rows at or beyond it are zero (what a run at S = keep is given)"""
    B, H, S, _ = q.shape
    n = S if keep is None else keep
    qp = torch.zeros(B, H, Spad, 64, dtype=torch.bfloat16); qp[:, :, :n] = q[:, :, :n]
    kp = torch.zeros(B, H, Spad, 64, dtype=torch.bfloat16); kp[:, :, :n] = k[:, :, :n]
    vt = torch.zeros(B, H, 64, Spad, dtype=torch.bfloat16); vt[:, :, :, :n] = v[:, :, :n].transpose(-1, -2)
    return qp.cuda(), kp.cuda(), vt.cuda()


def _run_keys(ccx_ctx, dev, B, H, S, Spad, counts):
    qd, kd, vd = dev
    o = torch.full((B * S, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    nk = None if counts is None else (C.c_int * B)(*counts)
    rc = ccx_ctx.lib.ccx_enc_attention_keys(ccx_ctx.handle, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), B, H, S, Spad, nk, _stream())
    ccx_ctx.check(rc, "ccx_enc_attention_keys")
    torch.cuda.synchronize()
    return o.cpu().view(B, S, H * 64)


def _run_plain(ccx_ctx, dev, B, H, S, Spad):
    qd, kd, vd = dev
    o = torch.full((B * S, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    ccx_ctx.check(ccx_ctx.lib.ccx_enc_attention(ccx_ctx.handle, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), B, H, S, Spad, _stream()),
                  "ccx_enc_attention")
    torch.cuda.synchronize()
    return o.cpu().view(B, S, H * 64)


def _fp64(q, k, v, b, n):
    """sequence b over its first n positions: [n, H * 64]"""
    qq, kk, vv = q[b, :, :n].double(), k[b, :, :n].double(), v[b, :, :n].double()
    o = torch.softmax(qq @ kk.transpose(-1, -2) * 0.125, dim=-1) @ vv          # [H, n, 64]
    return o.permute(1, 0, 2).reshape(n, -1)


def _bits(t):
    return t.contiguous().view(torch.int16)


B, H, S, SPAD = 4, 2, 200, 256


@pytest.fixture(scope="module")
def small():
    q, k, v = _inputs(B, H, S, SPAD, 41)
    return q, k, v, _padded(q, k, v, SPAD)


@pytest.mark.parametrize("counts", [(1, 63, 64, 65), (128, 129, 200, 1), (65, 200, 129, 63)])
def test_counts_per_sequence_against_fp64_and_alone(ccx_ctx, small, counts):
    q, k, v, dev = small
    got = _run_keys(ccx_ctx, dev, B, H, S, SPAD, counts)
    assert torch.isfinite(got.float()).all()
    for b, n in enumerate(counts):
        ref = _fp64(q, k, v, b, n)
        g = got[b, :n].double()
        within("enc_attention_kernel, keys per sequence: output rel-L2", float((g - ref).norm() / ref.norm()), REL_BOUND, (counts, b))
        within("enc_attention_kernel, keys per sequence: output max abs error", float((g - ref).abs().max()), ABS_BOUND, (counts, b))
        assert not bool(got[b, n:].float().abs().any()), (counts, b, "rows at or beyond the count are zeros")
        # the same sequence alone at S = n, as the plain entry point wants it (rows >= S zero)
        alone = _run_plain(ccx_ctx, _padded(q[b:b + 1], k[b:b + 1], v[b:b + 1], SPAD, keep=n), 1, H, n, SPAD)
        assert torch.equal(_bits(alone[0]), _bits(got[b, :n])), (counts, b)
    assert torch.equal(_bits(_run_keys(ccx_ctx, dev, B, H, S, SPAD, counts)), _bits(got)), "a second run differs"


def test_full_counts_are_the_plain_kernel_bit_for_bit(ccx_ctx, small):
    q, k, v, dev = small
    got = _run_keys(ccx_ctx, dev, B, H, S, SPAD, (S,) * B)
    assert torch.equal(_bits(got), _bits(_run_plain(ccx_ctx, dev, B, H, S, SPAD)))


def test_one_key_short_of_the_whole_window(ccx_ctx):
    """S = 1500, count 1499: twelve query tiles, a ragged 24th key tile whose mask drops one more key than S does"""
    S2, SPAD2, n = 1500, 1536, 1499
    q, k, v = _inputs(1, 1, S2, SPAD2, 43)
    got = _run_keys(ccx_ctx, _padded(q, k, v, SPAD2), 1, 1, S2, SPAD2, (n,))
    assert torch.isfinite(got.float()).all()
    ref = _fp64(q, k, v, 0, n)
    g = got[0, :n].double()
    within("enc_attention_kernel, keys per sequence: output rel-L2", float((g - ref).norm() / ref.norm()), REL_BOUND, n)
    within("enc_attention_kernel, keys per sequence: output max abs error", float((g - ref).abs().max()), ABS_BOUND, n)
    assert not bool(got[0, n:].float().abs().any())
    alone = _run_plain(ccx_ctx, _padded(q, k, v, SPAD2, keep=n), 1, 1, n, SPAD2)
    assert torch.equal(_bits(alone[0]), _bits(got[0, :n]))


def test_argument_errors(ccx_ctx, small):
    from clearconverse_amd import _lib
    q, k, v, dev = small
    for bad in ((0, 5, 5, 5), (5, 5, 5, S + 1), (-3, 5, 5, 5)):
        with pytest.raises(_lib.CcxError) as e:
            _run_keys(ccx_ctx, dev, B, H, S, SPAD, bad)
        assert "outside [1, 200]" in str(e.value)
    with pytest.raises(_lib.CcxError) as e:
        _run_keys(ccx_ctx, dev, B, H, S, SPAD, None)
    assert "n_keys_host is null" in str(e.value)
