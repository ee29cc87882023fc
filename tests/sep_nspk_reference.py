"""fp64 reference of the N-source SepFormer decoder (CCX_SEP_DECODER with ccx_sep_desc.n_spk, csrc/sepformer.hip:
sep_decoder_kernel<NSPK>), its derived allowance and the cases of tests/test_sep_nspk_kernels_gpu.py.  No GPU, no library: plain
torch on the CPU.  tests/sep_reference.py keeps the two-source statement; tests/test_sep_nspk_reference_cpu.py proves that this one
equals it at n_spk = 2 and equals oracle/sepformer_ref.py's mask / conv_transpose1d statement at every n_spk.

Layout of the mask logits: fc [rows, 128 * n_spk], channel-major and source-minor -- column c * n_spk + s is channel c of source s,
the meaning of the oracle's `fc.view(-1, 128, n_spk)`.  `mut` switches on ONE misreading (MUTATIONS); the CPU suite shows that the
cases can tell each of them from the reference by more than 100 x the allowance the GPU test asserts at.
"""
from __future__ import annotations

import torch

from tests import sep_reference as SR

D = SR.D
N_SPK = (1, 2, 3, 4)
STRIDES = (1003, 16)      # odd: with n_spk = 3 utterances 1 and 2 start at odd float offsets; 16: one sample group per utterance
MUTATIONS = ("speaker_major", "rotate_spk", "swap_taps")


def decoder_op(feats, fc, utts, wdec, out_stride, n_spk, mut=None, dtype=torch.float64):
    """feats [rows, 128], fc [rows, 128 * n_spk], utts [(tok0, L, T)], wdec [128, 16] -> [n_utt, out_stride, n_spk]:
    est[t][s] = sum_l sum_c feats[l][c] relu(fc[l][c * n_spk + s]) wdec[c][t - 8 l], zero from T on.
    mut: speaker_major reads fc as [L, n_spk, 128]; rotate_spk hands source s the mask of source s + 1 (both are the identity for
    one source: there they are no misreading); swap_taps exchanges the tap halves 0..7 and 8..15."""
    w = wdec.to(dtype)
    if mut == "swap_taps":
        w = torch.cat([w[:, 8:], w[:, :8]], dim=1)
    out = torch.zeros(len(utts), out_stride, n_spk, dtype=dtype)
    for u, (tok0, L, T) in enumerate(utts):
        f = feats[tok0:tok0 + L].to(dtype)
        m = torch.relu(fc[tok0:tok0 + L].to(dtype))
        if mut == "speaker_major":
            m = m.view(L, n_spk, D).transpose(1, 2)
        elif mut == "rotate_spk":
            m = m.view(L, D, n_spk).roll(-1, dims=2)
        else:
            m = m.view(L, D, n_spk)
        g = f[:, :, None] * m                                   # [L, 128, n_spk]
        frames = torch.einsum("lcs,ck->lks", g, w)              # [L, 16, n_spk]
        est = torch.zeros(8 * (L - 1) + 16, n_spk, dtype=dtype)
        for l in range(L):
            est[8 * l:8 * l + 16] += frames[l]
        n = min(T, est.shape[0], out_stride)
        out[u, :n] = est[:n]
    return out


def decoder_allowance(feats, fc, utts, wdec, out_stride, n_spk):
    """|est - ref| <= (n + 3) u sum |terms| with n = 256 products per sample (two token rows x 128 channels, whatever n_spk is: the
    sources do not share a sum) and two factors rounded per product (+ 2): the formula of tests/sep_reference.decoder_allowance"""
    return (256 + 3 + 2) * SR.U32 * decoder_op(feats.abs(), fc.abs(), utts, wdec.abs(), out_stride, n_spk)


def decoder_case(n_spk, seed=0, segment=150, out_stride=1003):
    """after tests/sep_reference.decoder_case: three utterances, L = 1 (T = 16); L = 37 (T = 8 L + 13: samples past 8 (L + 1) are
    zero); L = segment exactly (a whole chunk of padding), trimmed to T = out_stride.  No T exceeds out_stride: at out_stride = 16
    every utterance is trimmed to its first 16 samples and its later frames must not show."""
    L = (1, 37, segment)
    T = tuple(min(t, out_stride) for t in (16, 8 * 37 + 13, out_stride))
    utts, r = [], 0
    for l, t in zip(L, T):
        utts.append((r, l, t))
        r += l + (segment - l % segment)
    rows = r + 2
    g = torch.Generator().manual_seed(4100 + 10 * seed + n_spk)
    feats = torch.relu(torch.randn(rows, D, generator=g))
    fc = torch.randn(rows, n_spk * D, generator=g)
    wdec = SR.make_params(seed)["wdec"]
    return feats, fc, utts, rows, wdec, out_stride


def used_rows(utts, rows):
    m = torch.zeros(rows, dtype=torch.bool)
    for tok0, L, _ in utts:
        m[tok0:tok0 + L] = True
    return m
