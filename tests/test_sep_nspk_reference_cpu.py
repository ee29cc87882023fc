"""CPU: the N-source decoder reference of tests/sep_nspk_reference.py is what the GPU test may trust.
  - at n_spk = 2 it IS tests/sep_reference.decoder_op (exact equality, allowance included);
  - at every n_spk it agrees to fp64 rounding with oracle/sepformer_ref.py's own statement -- `relu(fc.view(-1, 128, n_spk))`, one
    conv_transpose1d per source, pad / trim to T -- run through the oracle's `separate` with the mask logits handed in;
  - the generator's inputs tell the three misreadings (speaker-major layout, rotated sources, swapped tap halves) from the reference
    by more than 100 x the allowance the GPU test asserts at;
  - the ctypes SepDesc has the size and the n_spk offset of ccx_sep_desc (a host program compiled against include/ccx.h).
"""
import ctypes as C
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from clearconverse_amd import _lib
from clearconverse_amd.build import _hipcc
from oracle import sepformer_ref as O
from tests import sep_nspk_reference as NR
from tests import sep_reference as SR

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("out_stride", NR.STRIDES)
def test_two_sources_are_the_existing_reference(out_stride):
    feats, fc, utts, rows, wdec, _ = NR.decoder_case(2, out_stride=out_stride)
    assert torch.equal(NR.decoder_op(feats, fc, utts, wdec, out_stride, 2), SR.decoder_op(feats, fc, utts, wdec, out_stride))
    assert torch.equal(NR.decoder_allowance(feats, fc, utts, wdec, out_stride, 2), SR.decoder_allowance(feats, fc, utts, wdec, out_stride))
    for ours, theirs in (("swap_taps", "swap_taps"), ("rotate_spk", "swap_spk")):
        assert torch.equal(NR.decoder_op(feats, fc, utts, wdec, out_stride, 2, mut=ours),
                           SR.decoder_op(feats, fc, utts, wdec, out_stride, mut=theirs))


def test_case_geometry():
    for n_spk in NR.N_SPK:
        for out_stride in NR.STRIDES:
            feats, fc, utts, rows, wdec, st = NR.decoder_case(n_spk, out_stride=out_stride)
            assert st == out_stride and fc.shape == (rows, 128 * n_spk) and feats.shape == (rows, 128)
            assert [L for _, L, _ in utts] == [1, 37, 150] and all(16 <= T <= out_stride for _, _, T in utts)
            for (t0, L, _), nxt in zip(utts, [u[0] for u in utts[1:]] + [rows]):
                assert t0 + L + (150 - L % 150) <= nxt                     # chunk padding owned, 150 frames -> a whole extra chunk
    utts = NR.decoder_case(3)[2]
    assert utts[1][2] == 8 * 37 + 13 and utts[2][2] == 1003
    assert [(u * 1003 * 3) % 2 for u in (1, 2)] == [1, 0] and (1003 * 3) % 4 != 0     # float offsets no 8- or 16-byte store survives


@pytest.mark.parametrize("n_spk", NR.N_SPK)
def test_agrees_with_the_oracles_statement(n_spk):
    dims = O.SepDims(n_spk=n_spk)
    g = torch.Generator().manual_seed(77 + n_spk)
    enc = torch.randn(128, 1, 16, generator=g) / 2.0
    dec = torch.randn(128, 1, 16, generator=g, dtype=torch.float64) / 8.0
    ref = O.SepformerRef(dims, {"encoder.conv1d.weight": enc, "decoder.weight": dec})
    ref.sd["decoder.weight"] = dec                                           # the constructor made it fp32: keep the statement in fp64
    for L, T in ((1, 16), (37, 8 * 37 + 13), (150, 1003), (150, 16)):
        n_mix = max(T, 8 * (L - 1) + 16)                                     # the oracle takes L from the mixture's length
        mix = torch.randn(1, n_mix, generator=g)
        feats = F.relu(F.conv1d(mix[:, None, :], enc, None, stride=8))[0].transpose(0, 1)      # what `separate` computes itself
        assert feats.shape == (L, 128)
        fc = torch.randn(L, 128 * n_spk, generator=g, dtype=torch.float64)
        ref._pipeline = lambda f, fc=fc: fc
        theirs = ref.separate(mix)[0][:T]                                    # [T, n_spk]
        ours = NR.decoder_op(feats, fc, [(0, L, T)], dec[:, 0, :], T, n_spk)[0]
        scale = NR.decoder_op(feats.abs(), fc.abs(), [(0, L, T)], dec[:, 0, :].abs(), T, n_spk)[0]
        assert theirs.dtype == torch.float64 and theirs.shape == ours.shape == (T, n_spk)
        assert bool(((theirs - ours).abs() <= 300 * 2.0 ** -53 * scale).all()), (L, T)       # 256 terms each, either order


@pytest.mark.parametrize("out_stride", NR.STRIDES)
@pytest.mark.parametrize("n_spk", NR.N_SPK)
def test_misreadings_stand_out(n_spk, out_stride):
    feats, fc, utts, rows, wdec, _ = NR.decoder_case(n_spk, out_stride=out_stride)
    ref = NR.decoder_op(feats, fc, utts, wdec, out_stride, n_spk)
    allow = NR.decoder_allowance(feats, fc, utts, wdec, out_stride, n_spk)
    for u, (_, L, T) in enumerate(utts):
        n = min(T, 8 * (L + 1))
        assert bool((ref[u, n:] == 0).all()) and bool((allow[u, :n] > 0).all())
    for mut in NR.MUTATIONS:
        if n_spk == 1 and mut != "swap_taps":
            continue                                                         # one source has one layout
        bad = NR.decoder_op(feats, fc, utts, wdec, out_stride, n_spk, mut=mut)
        for u, (_, L, T) in enumerate(utts):
            n = min(T, 8 * (L + 1))
            for s in range(n_spk):                                           # every source on its own shows it
                assert float(((bad[u, :n, s] - ref[u, :n, s]).abs() / allow[u, :n, s]).max()) > 100.0, (mut, u, s)


PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "ccx.h"
int main() {
  printf("size %zu\n", sizeof(ccx_sep_desc));
  printf("out_elems %zu\n", offsetof(ccx_sep_desc, out_elems));
  printf("n_spk %zu\n", offsetof(ccx_sep_desc, n_spk));
  printf("fc_elems %zu\n", offsetof(ccx_sep_desc, fc_elems));
  printf("utt_tok0 %zu\n", offsetof(ccx_sep_desc, utt_tok0));
  return 0;
}
"""


def test_ctypes_sep_desc_has_the_c_layout(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert C.sizeof(_lib.SepDesc) == c.pop("size")
    for field, off in c.items():
        assert getattr(_lib.SepDesc, field).offset == off, field
    # appended: a descriptor written before the field existed ends where n_spk begins, and a zeroed one asks for two sources
    assert _lib.SepDesc.n_spk.offset == _lib.SepDesc.out_elems.offset + 8 and _lib.SepDesc().n_spk == 0
