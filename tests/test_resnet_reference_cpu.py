"""CPU: tests/resnet_reference.py (fp64, written from the definitions) against oracle/wespeaker_ref.py (fp32) on fp32 inputs, its
layout helpers, the conditions the GPU tests' inputs must meet, and the facts about the nearest-neighbour index map that
csrc/ccx_common.h ccx_nearest_src rests on.

u = 2^-24 is the unit roundoff of fp32.  Every bound below is first order in u, computed from the fp64 quantities, and doubled."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clearconverse_amd.weights import synthetic_resnet34_state_dict
from oracle import wespeaker_ref as O
from tests import resnet_reference as R

U = 2.0 ** -24


def test_fbank_matches_the_fp32_oracle():
    """The oracle rounds the frame to fp32 after DC removal, pre-emphasis and windowing (three operations on values of at most
    2 max|x|, so at most 6 u max|x| per sample), transforms in fp64, then rounds the power and accumulates the mel sum in fp32.
    A per-sample error e moves a spectrum bin by at most 400 e =: d, the power |X|^2 by 2 |X| d + d^2, and the mel energy E by
    dE = sum_k w_k (2 |X_k| d + d^2) + (L + 2) u E for a filter of L <= 64 bins.  log(E) moves by dE / E to first order (asserted
    small), and its fp32 result is rounded: 2 u |log E|.  The bound is twice the sum."""
    wave = R.fbank_test_waves(33, "plain")[0]
    got = torch.from_numpy(O.kaldi_fbank(wave.numpy())).double()
    ref = R.fbank(wave)
    assert got.shape == ref.shape == (33, 80)
    spec = R.spectrum(wave).abs()
    idx = torch.arange(33)[:, None] * 160 + torch.arange(400)[None, :]
    xmax = (wave.double() * 32768.0)[idx].abs().max(dim=1, keepdim=True).values        # [T][1]
    d = 400 * 6 * U * xmax
    E = R.mel_energies(wave)
    dE = (2 * spec * d + d ** 2) @ R.mel_banks().T + 66 * U * E
    assert float((dE / E).max()) < 0.05
    bound = 2 * (dE / E + 2 * U * ref.abs())
    err = (got - ref).abs()
    print(f"fbank vs oracle: worst err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


def test_mel_banks_and_window_match_the_oracle_tables():
    assert float((R.mel_banks() - torch.from_numpy(O.kaldi_mel_banks()).double()).abs().max()) <= U
    assert R.num_frames(399) == 0 and R.num_frames(400) == 1 and R.num_frames(559) == 1 and R.num_frames(560) == 2


def _oracle_block(sd, p, x, stride):
    """One basic block, the lines of oracle/wespeaker_ref.py resnet_trunk's loop body (fp32, BatchNorm unfolded)."""
    out = F.relu(O._bn(F.conv2d(x, sd[p + "conv1.weight"].float(), stride=stride, padding=1), sd, p + "bn1"))
    out = O._bn(F.conv2d(out, sd[p + "conv2.weight"].float(), padding=1), sd, p + "bn2")
    sc = O._bn(F.conv2d(x, sd[p + "shortcut.0.weight"].float(), stride=stride), sd, p + "shortcut.1") if (p + "shortcut.0.weight") in sd else x
    return F.relu(out + sc)


@pytest.mark.parametrize("p,stride", [("resnet.layer1.1.", 1), ("resnet.layer2.0.", 2)])
def test_one_block_matches_the_fp32_oracle_with_the_references_own_fold(p, stride):
    """Reference: three calls of R.conv with weights w * scale folded in fp64 (R.bn_fold).  Oracle: fp32 convolution, then fp32
    batch norm.  Each of the K additions of an fp32 accumulation rounds a partial sum by at most u of its magnitude.  The worst
    case, K u sum |a w|, overstates that K-fold for terms of mixed sign (it would not tell fp32 from bf16 here); the partial sums
    of such terms are of the order of Q = sqrt(sum (a w)^2), and 4 Q is allowed for each: one convolution is off by
    4 K u Q.  The batch norm adds a handful of roundings of scale (|conv| + |running_mean|) + |beta| <= B: 8 u B.  The second
    convolution also carries the first one's error e1 through w2, again as a root sum of squares (ReLU is 1-Lipschitz), and
    the residual add rounds twice more.  The bound is twice the total."""
    sd = synthetic_resnet34_state_dict(0)
    cin = sd[p + "conv1.weight"].shape[1]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, cin, 8, 9, generator=g)
    got = _oracle_block(sd, p, x, stride).double()

    def layer(inp, wname, bn, s, relu, resid=None):
        scale, shift = R.bn_fold(sd, p + bn)
        w = sd[p + wname].double() * scale[:, None, None, None]
        y, a = R.conv(inp, w, shift, s, relu, resid)
        K = w.shape[1] * w.shape[2] * w.shape[3]
        Q = torch.sqrt(F.conv2d(inp ** 2, w ** 2, stride=s, padding=w.shape[-1] // 2))
        lin = F.conv2d(inp, w, stride=s, padding=w.shape[-1] // 2).abs()
        B = lin + ((sd[p + bn + ".running_mean"].double() * scale).abs() + shift.abs())[None, :, None, None]
        if resid is not None:
            B = B + resid.abs()
        return y, w, 4 * K * U * Q + 8 * U * B

    xd = x.double()
    t, _, e1 = layer(xd, "conv1.weight", "bn1", stride, True)
    if (p + "shortcut.0.weight") in sd:
        sc, _, esc = layer(xd, "shortcut.0.weight", "shortcut.1", stride, False)
    else:
        sc, esc = xd, torch.zeros_like(t)
    ref, w2, e2 = layer(t, "conv2.weight", "bn2", 1, True, sc)
    bound = 2 * (e2 + torch.sqrt(F.conv2d(e1 ** 2, w2 ** 2, padding=1)) + esc)
    err = (got - ref).abs()
    print(f"block {p}: worst err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}, "
          f"worst bound / (|ref| + 1) {float((bound / (ref.abs() + 1)).max()):.3e}")
    assert got.shape == ref.shape
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((bound / (ref.abs() + 1)).max()) < 2.0 ** -10          # half of the unit roundoff of bf16


@pytest.mark.parametrize("weighted", [False, True])
def test_stats_pool_matches_the_fp32_oracle(weighted):
    """T = 37 frames of N(0.3, 1) data, soft weights in [0.1, 1].  fp32 sums of T terms: the weighted mean is off by
    dm = (T + 3) u sum |w x| / v1.  d = x - mean is off by u (|x| + |mean|) + dm, the weighted sum of squares S by
    (T + 4) u S + 2 sum w |d| dd, the denominator D = v1 - v2 / v1 by (T + 4) u (v1 + v2 / v1); var = S / D, std = sqrt(var)
    is off by dvar / (2 std) + u std.  Unweighted, torch's own mean / std: the same with w = 1 and D = T - 1.  Twice that."""
    g = torch.Generator().manual_seed(9)
    T = 37
    x = torch.randn(3, 40, T, generator=g) + 0.3
    w = (0.1 + 0.9 * torch.rand(3, 23, generator=g)) if weighted else None
    got = O.stats_pool(x, w).double()
    ref = R.stats_pool(x, w)
    xd = x.double()
    wt = w.double()[:, R.nearest_index(T, 23)].unsqueeze(1) if weighted else torch.ones(3, 1, T, dtype=torch.float64)
    v1, v2 = wt.sum(2), (wt ** 2).sum(2)
    mean, std = ref[:, :40], ref[:, 40:]
    dm = (T + 3) * U * (wt * xd.abs()).sum(2) / v1
    dd = U * (xd.abs() + mean.abs().unsqueeze(2)) + dm.unsqueeze(2)
    dabs = (xd - mean.unsqueeze(2)).abs()
    D = v1 - v2 / v1
    S = std ** 2 * D
    dvar = ((T + 4) * U * S + 2 * (wt * dabs * dd).sum(2)) / D + std ** 2 * (T + 4) * U * (v1 + v2 / v1) / D
    bound = 2 * torch.cat([dm + U * mean.abs(), dvar / (2 * std) + U * std], dim=1)
    err = (got - ref).abs()
    print(f"stats_pool weighted={weighted}: worst err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(bound.max()) < 1e-4


def test_tstp_and_linear_layouts():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 256, 10, 5, generator=g, dtype=torch.float64)
    p = R.tstp(x)
    assert p.shape == (2, 5120)
    assert float((p[1, 7 * 10 + 3] - x[1, 7, 3].mean()).abs()) < 1e-12
    assert float((p[1, 2560 + 7 * 10 + 3] - x[1, 7, 3].std(unbiased=True)).abs()) < 1e-12
    # all-ones weights: the weighted formulas give the unbiased std up to the 1e-8 regularisers
    q = R.tstp(x, torch.ones(3, 11, dtype=torch.float64), [1, 1, 0])
    assert float((q[0] - p[1]).abs().max()) < 1e-7 and float((q[2] - p[0]).abs().max()) < 1e-7
    y, a = R.linear(p, torch.ones(256, 5120), torch.zeros(256))
    assert float((y[:, 0] - p.sum(1)).abs().max()) < 1e-9 and bool((a >= y.abs()).all())


def test_layout_helpers_round_trip():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 32, 6, 5, generator=g, dtype=torch.float64)
    p = R.to_padded(x, halo=7.0)
    assert p.shape == (2, 8, 7, 32)
    assert torch.equal(R.from_padded(p), x)
    m = R.halo_mask(2, 6, 5, 32)
    assert bool((p[m] == 7.0).all()) and int(m.sum()) == 2 * 32 * (8 * 7 - 6 * 5)
    assert float(p[1, 3, 2, 9]) == float(x[1, 9, 2, 1])                  # padded (y + 1, x + 1, c)  <-  (c, y, x)
    assert torch.equal(R.to_padded(R.from_padded(p), halo=7.0), p)


# ------------------------------------------------------------------------------------------------------------ the index map
def test_fp32_index_map_is_torchs_and_the_exact_rational_map_is_not():
    """F.interpolate(mode="nearest") takes floor(t * (float)(n_in / n_out)) in fp32.  Where t n_in / n_out is an exact integer the fp32
    product can fall just below it, and torch (and pyannote's StatsPool through it) then reads the element before."""
    assert R.nearest_index(14, 62)[7] == 30 and R.nearest_index_exact(14, 62)[7] == 31 and R.nearest_index_fp32(14, 62)[7] == 30
    for n, nw in [(14, 62), (133, 589), (266, 589)]:
        t = R.nearest_index(n, nw).numpy()
        assert np.array_equal(R.nearest_index_fp32(n, nw), t), (n, nw)
        assert not np.array_equal(R.nearest_index_exact(n, nw), t), (n, nw)
    # the pipeline's own shape and the shapes of tests/test_speaker_gpu.py: the maps agree
    for n, nw in [(575, 589), (575, 293)]:
        assert np.array_equal(R.nearest_index_exact(n, nw), R.nearest_index(n, nw).numpy()), (n, nw)
    # torch against the fp32 formula: every pair of a dense corner, and every frame count against a set of weight counts
    pairs = [(n, nw) for n in range(2, 65) for nw in range(1, 129)]
    pairs += [(n, nw) for n in range(65, 700) for nw in (1, 2, 62, 117, 293, 589, 1178, 1299, n, 2 * n, n - 1, n + 1)]
    for n, nw in pairs:
        assert np.array_equal(R.nearest_index_fp32(n, nw), R.nearest_index(n, nw).numpy()), (n, nw)


def test_count_of_pairs_where_the_two_maps_differ():
    """Over n = 2..699 frames and n_w = 1..1299 weights, the exact rational map differs from the fp32 map at 20 928 pairs."""
    nw = np.arange(1, 1300, dtype=np.int64)[None, :]
    differ = 0
    for n in range(2, 700):
        t = np.arange(n, dtype=np.int64)[:, None]
        scale = (nw.astype(np.float32) / np.float32(n))
        f = np.minimum(np.floor(t.astype(np.float32) * scale).astype(np.int64), nw - 1)
        differ += int(((t * nw) // n != f).any(axis=0).sum())
    assert differ == 20928, differ


# ------------------------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("variant", R.FBANK_VARIANTS)
def test_fbank_test_inputs_are_broadband(variant):
    """tests/test_resnet_kernels_gpu.py compares log mel energies elementwise: none may be spectral leakage of a louder bin."""
    for T in (1, 3, 4, 33, 130):
        waves = R.fbank_test_waves(T, variant)
        assert waves.dtype == torch.float32 and waves.shape == (2, 400 + 160 * (T - 1) + 37)
        for wv in waves:
            E = R.mel_energies(wv)
            assert bool((E >= 1e-5 * E.max(dim=1, keepdim=True).values).all()), (variant, T)
    if variant == "full scale":
        assert float(waves.abs().max()) == 1.0
    if variant == "dc":
        assert abs(float(waves.mean()) - 0.5) < 1e-3


@pytest.mark.parametrize("cin,cout,k,stride", R.NETWORK_CONVS)
def test_conv_bound_sees_near_miss_convolutions(cin, cout, k, stride):
    """The elementwise bound of the GPU convolution tests is tight enough to tell a convolution from a nearly correct one: a shift by
    one pixel in x or y, two taps swapped, the last column dropped each exceed it on at least a quarter of the pixels they touch
    (ReLU hides the rest)."""
    seen = R.fault_visibility(cin, cout, k, stride)
    assert set(seen) == {"shift x", "shift y", "last column dropped"} | ({"tap swap"} if k == 3 else set())
    for name, frac in seen.items():
        assert frac > 0.25, (name, frac)
