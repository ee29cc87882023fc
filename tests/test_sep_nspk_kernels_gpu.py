"""GPU: sep_decoder_kernel<NSPK> (csrc/sepformer.hip) for 1, 2, 3 and 4 sources through ccx_sep_op (op 4, ccx_sep_desc.n_spk)
against the fp64 reference and the derived allowance of tests/sep_nspk_reference.py (proven in tests/test_sep_nspk_reference_cpu.py).

feats / fc rows outside every utterance hold NaN; `out` is pre-filled with NaN and followed, inside the same tensor, by a guard band of
64 floats holding a bit pattern: a read past an utterance shows as a non-finite value, a sample never stored as NaN, a store past the
last utterance as changed guard bits.  out_stride = 1003 is odd, so with three sources utterance 1 begins at an odd float offset:
nothing wider than a float store is valid there.  out_stride = 16 is one sample group per utterance.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import sep_nspk_reference as NR
from tests.conftest import within

pytestmark = pytest.mark.gpu

DECODER = 4
N_DEC = "sep n_spk kernels: decoder, |err| / derived allowance"
GUARD = 64
GUARD_BITS = 0x5EEDBEEF


def _ints(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


@functools.lru_cache(maxsize=None)
def _case(n_spk, out_stride):
    feats, fc, utts, rows, wdec, _ = NR.decoder_case(n_spk, out_stride=out_stride)
    ref = NR.decoder_op(feats, fc, utts, wdec, out_stride, n_spk)
    allow = NR.decoder_allowance(feats, fc, utts, wdec, out_stride, n_spk)
    return feats, fc, utts, rows, wdec, ref, allow


def _device_inputs(n_spk, out_stride):
    feats, fc, utts, rows, wdec, _, _ = _case(n_spk, out_stride)
    mask = NR.used_rows(utts, rows)
    feats, fc = feats.clone(), fc.clone()
    feats[~mask] = math.nan
    fc[~mask] = math.nan
    return feats.cuda(), fc.cuda(), wdec.float().contiguous().cuda()


def _out_buffer(n_utt, out_stride, n_spk):
    """NaN where the kernel must store, the guard pattern behind it; returns (whole tensor, elements that belong to `out`)"""
    n = n_utt * out_stride * n_spk
    buf = torch.full((n + GUARD,), math.nan, device="cuda")
    buf[n:].view(torch.int32).fill_(GUARD_BITS)
    return buf, n


def _launch(ctx, feats, fc, wdec, buf, n_out, utts, rows, out_stride, field, override=None):
    """One ccx_sep_op(op 4) with ccx_sep_desc.n_spk = field.  Returns rc."""
    from clearconverse_amd import _lib
    lib = _lib.load()
    d = _lib.SepDesc()
    d.feats, d.feats_elems, d.fc, d.fc_elems = feats.data_ptr(), feats.numel(), fc.data_ptr(), fc.numel()
    d.wdec, d.wdec_elems, d.out, d.out_elems = wdec.data_ptr(), wdec.numel(), buf.data_ptr(), n_out
    d.rows, d.segment, d.out_stride, d.n_spk = rows, 150, out_stride, field
    keep = [_ints([u[i] for u in utts]) for i in range(3)]
    d.utt_tok0, d.utt_L, d.utt_T, d.n_utt = keep[0], keep[1], keep[2], len(utts)
    for name, val in (override or {}).items():
        setattr(d, name, val)
    rc = lib.ccx_sep_op(ctx.handle, DECODER, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _run(ctx, n_spk, out_stride, field=None):
    feats, fc, wdec = _device_inputs(n_spk, out_stride)
    _, _, utts, rows, _, _, _ = _case(n_spk, out_stride)
    buf, n = _out_buffer(len(utts), out_stride, n_spk)
    ctx.check(_launch(ctx, feats, fc, wdec, buf, n, utts, rows, out_stride, n_spk if field is None else field), "ccx_sep_op")
    assert bool((buf[n:].view(torch.int32) == GUARD_BITS).all()), "the guard band behind out changed"
    return buf[:n].view(len(utts), out_stride, n_spk)


@pytest.mark.parametrize("out_stride", NR.STRIDES)
@pytest.mark.parametrize("n_spk", NR.N_SPK)
def test_decoder_n_sources(ccx_ctx, n_spk, out_stride):
    """three utterances in one launch: L = 1 (T = 16); L = 37 (T = 8 L + 13, or 16); L = 150 exactly, trimmed to out_stride"""
    _, _, utts, _, _, ref, allow = _case(n_spk, out_stride)
    got = _run(ccx_ctx, n_spk, out_stride).cpu()
    assert got.shape == (3, out_stride, n_spk) and bool(torch.isfinite(got).all())
    for u, (tok0, L, T) in enumerate(utts):
        n = min(T, 8 * (L + 1))
        assert bool((got[u, T:] == 0).all()) and bool((got[u, n:] == 0).all()), u       # from T on (and past the frames' support): exactly 0
        ratio = (got[u, :n].double() - ref[u, :n]).abs() / allow[u, :n].clamp_min(1e-30)
        for s in range(n_spk):
            within(N_DEC, float(ratio[:, s].max()), 1.0, ("decoder", n_spk, out_stride, u, s))


@pytest.mark.parametrize("out_stride", NR.STRIDES)
def test_field_zero_means_two_sources(ccx_ctx, out_stride):
    a = _run(ccx_ctx, 2, out_stride, field=0)
    b = _run(ccx_ctx, 2, out_stride, field=2)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n_spk", NR.N_SPK)
def test_repeat_launch_is_bit_identical(ccx_ctx, n_spk):
    a = _run(ccx_ctx, n_spk, 1003)
    b = _run(ccx_ctx, n_spk, 1003)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# name: (n_spk the buffers are sized for, n_spk field, descriptor override, the field the message names)
REJECTIONS = {
    "n_spk_5": (4, 5, {}, "n_spk"),
    "n_spk_minus_1": (2, -1, {}, "n_spk"),
    "fc_sized_for_two_of_three": (3, 3, {"fc_elems": "two"}, "fc_elems"),
    "out_sized_for_two_of_three": (3, 3, {"out_elems": "two"}, "out_elems"),
    "fc_sized_for_three_of_four": (4, 4, {"fc_elems": "three"}, "fc_elems"),
    "out_sized_for_one_of_default": (2, 0, {"out_elems": "one"}, "out_elems"),
}


@pytest.mark.parametrize("case", sorted(REJECTIONS))
def test_bad_descriptors_are_refused_before_any_launch(ccx_ctx, case):
    sized, field, over, named = REJECTIONS[case]
    out_stride = 1003
    feats, fc, wdec = _device_inputs(sized, out_stride)
    _, _, utts, rows, _, _, _ = _case(sized, out_stride)
    buf, n = _out_buffer(len(utts), out_stride, sized)
    count = {"one": 1, "two": 2, "three": 3}
    o = {}
    if "fc_elems" in over:
        o["fc_elems"] = rows * 128 * count[over["fc_elems"]]
    if "out_elems" in over:
        o["out_elems"] = len(utts) * out_stride * count[over["out_elems"]]
    before = buf.clone()
    rc = _launch(ccx_ctx, feats, fc, wdec, buf, n, utts, rows, out_stride, field, override=o)
    msg = ccx_ctx.lib.ccx_last_error(ccx_ctx.handle).decode()
    assert rc == 1, (case, rc, msg)                                                     # CCX_ERR_ARG
    assert msg.startswith("ccx_sep_op:") and named in msg, (case, msg)
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "a refused call wrote to out"
