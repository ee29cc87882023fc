"""CPU: the fp64 statements of tests/speaker_reference.py against second statements built from other parts (nn.LSTM, F.instance_norm,
nn.Conv1d, F.interpolate) and, chained, against oracle/pyannote_ref.py; the derived sinc bound on every input of the GPU test, and
what that bound and the LSTM conditions see."""
import math

import pytest
import torch
import torch.nn.functional as F

from clearconverse_amd.weights import sinc_filters, synthetic_pyannet_state_dict
from oracle import pyannote_ref as P
from tests import speaker_reference as S

F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- each statement, a second way
def test_wav_stats_and_sinc_stage_against_conv1d_module():
    g = _gen(1)
    x = (0.2 + 0.1 * torch.randn(251 + 10 * 50 + 7, generator=g)).float()
    filt = S.sinc_filter_bank("dense")
    a, c, mean = S.wav_stats(x, 1.3, -0.2)
    xn = F.instance_norm(x.double()[None, None], weight=torch.tensor([1.3], dtype=F64), bias=torch.tensor([-0.2], dtype=F64), eps=1e-5)[0, 0]
    assert float((a * x.double() + c - xn).abs().max()) < 1e-12 and abs(mean - float(x.double().mean())) < 1e-15
    conv = torch.nn.Conv1d(1, 80, 251, stride=10, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(filt.double()[:, None, :])
        y = conv(xn[None, None])[0].abs()                                   # [80][51]
    want = torch.stack([y[:, 3 * i:3 * i + 3].max(dim=1).values for i in range(17)])
    got, bound = S.sinc_stage(x, filt, 1.3, -0.2, 17)
    assert got.shape == (17, 80) and float((got - want).abs().max()) < 1e-12
    assert bound.shape == (17, 80) and bool((bound > 0).all())


@pytest.mark.parametrize("pool,C", [(1, 80), (3, 60)])
def test_inorm_against_functional_instance_norm(pool, C):
    g = _gen(pool)
    x = torch.randn(3 * 40 + 5, C, generator=g) + 3.0
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    v = x[:pool * 40].double()
    if pool == 3:
        v = v.reshape(40, 3, C).max(dim=1).values
    want = F.leaky_relu(F.instance_norm(v.T[None], weight=gamma.double(), bias=beta.double(), eps=1e-5), 0.01)[0].T
    assert float((S.inorm(x, gamma, beta, pool, 40) - want).abs().max()) < 1e-12


def test_pool_stats_against_interpolate():
    g = _gen(3)
    x = torch.randn(14, 20, generator=g, dtype=F64)
    w = torch.rand(62, generator=g)
    wt = F.interpolate(w.view(1, 1, -1), size=14, mode="nearest").view(-1).double()
    v1 = wt.sum() + 1e-8
    mean = (x * wt[:, None]).sum(dim=0) / v1
    var = ((x - mean) ** 2 * wt[:, None]).sum(dim=0) / (v1 - (wt ** 2).sum() / v1 + 1e-8)
    got = S.pool_stats(x, w)
    assert float((got[:20] - mean).abs().max()) < 1e-12 and float((got[20:] - var.sqrt()).abs().max()) < 1e-12
    plain = S.pool_stats(x)
    assert float((plain[:20] - x.mean(dim=0)).abs().max()) < 1e-14 and float((plain[20:] - x.std(dim=0)).abs().max()) < 1e-14


def _lstm_case(T, seed):
    g = _gen(seed)
    return torch.randn(T, 1024, generator=g), 0.8 / math.sqrt(128) * torch.randn(2, 512, 128, generator=g)


def test_lstm_against_nn_lstm():
    """Rounding off, the statement is torch's bidirectional LSTM with W_ih = I on the gx rows (input size 1024 is avoided: each
    direction gets its own 512 pre-activations through an identity W_ih)."""
    gx, whh = _lstm_case(23, 5)
    got = S.lstm(gx, whh, round_h=False)
    for d in range(2):
        m = torch.nn.LSTM(512, 128, batch_first=True).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(torch.eye(512, dtype=F64)); m.weight_hh_l0.copy_(whh[d].double())
            m.bias_ih_l0.zero_(); m.bias_hh_l0.zero_()
            seq = gx[:, 512 * d:512 * (d + 1)].double()
            seq = seq if d == 0 else torch.flip(seq, dims=[0])
            h = m(seq[None])[0][0]
        h = h if d == 0 else torch.flip(h, dims=[0])
        assert float((got[:, 128 * d:128 * (d + 1)] - h).abs().max()) < 1e-12, d


def test_lstm_fp32_run_of_the_contract_meets_the_gpu_conditions():
    """The conditions the GPU test sets for the kernel (every output within two bf16 ulps of the fp64 contract, at most 1 % different
    at all) hold with a wide margin for an fp32 run of the same contract, so they leave room for the kernel's exp2 / rcp builtins."""
    differ = total = 0
    for seed in range(4):
        gx, whh = _lstm_case(37, 10 + seed)
        a, b = S.lstm(gx, whh), S.lstm(gx, whh, dtype=torch.float32).double()
        assert float(S.bf16_ulps(b, a).max()) <= 2.0
        differ, total = differ + int((S.bf16_order(a) != S.bf16_order(b)).sum()), total + a.numel()
    print(f"fp32 against fp64 run of the LSTM contract: {differ} of {total} outputs differ")
    assert differ / total < 0.002


def test_lstm_clamp_costs_less_than_1e9():
    g = _gen(7)
    gx = 40.0 * torch.sign(torch.randn(9, 1024, generator=g))
    whh = torch.zeros(2, 512, 128)
    assert float((S.lstm(gx, whh, round_h=False) - S.lstm(gx, whh, round_h=False, clamp=25.0)).abs().max()) < 1e-9
    gx, whh = _lstm_case(9, 8)
    assert float((S.lstm(gx, whh, round_h=False) - S.lstm(gx, whh, round_h=False, clamp=25.0)).abs().max()) < 1e-9


def test_activation_against_definitions():
    x = torch.randn(5, 7, generator=_gen(9))
    lse = torch.log(torch.exp(x.double()).sum(dim=1, keepdim=True))
    assert float((S.activation(x, True) - (x.double() - lse)).abs().max()) < 1e-12
    assert float((S.activation(x, False) - 1 / (1 + torch.exp(-x.double()))).abs().max()) < 1e-15


def test_bf16_helpers():
    v = torch.tensor([1.0, 1.0078125, -1.0, 0.0, 0.99609375, 2.0 ** -130], dtype=F64)
    o = S.bf16_order(v)
    assert int(o[1] - o[0]) == 1 and int(o[0] - o[4]) == 1 and int(o[2]) == -int(o[0]) and int(o[3]) == 0
    assert float(S.bf16_half_ulp(torch.tensor([1.5], dtype=F64))) == 2.0 ** -8
    got, ref = torch.tensor([1.0, 1.0], dtype=F64), torch.tensor([1.003, 1.01], dtype=F64)
    ex = S.bf16_excess(got, ref)
    assert float(ex[0]) == 0.0 and abs(float(ex[1]) - (0.01 - 2.0 ** -8)) < 1e-15


# ---------------------------------------------------------------------------------------------- chained, against the oracle
@pytest.fixture(scope="module")
def pyannet():
    from clearconverse_amd.audio import synthetic_clip
    sd = synthetic_pyannet_state_dict(7, seed=3)
    wav = torch.from_numpy(synthetic_clip(3, 30.0)[1000:1000 + 12000].copy())
    return sd, wav


def _sincnet_chain(sd, wav):
    """SincNet from the statements: [frames][60] fp64."""
    g = lambda k: sd["sincnet." + k]
    filt = sinc_filters(g("conv1d.0.filterbank.low_hz_"), g("conv1d.0.filterbank.band_hz_"))
    n1 = ((wav.numel() - 251) // 10 + 1) // 3
    x, _ = S.sinc_stage(wav, filt, float(g("wav_norm1d.weight")), float(g("wav_norm1d.bias")), n1)
    x = S.inorm(x, g("norm1d.0.weight"), g("norm1d.0.bias"), 1, n1)
    for i in (1, 2):
        x = F.conv1d(x.T[None], g(f"conv1d.{i}.weight").double(), g(f"conv1d.{i}.bias").double())[0].T
        x = S.inorm(x, g(f"norm1d.{i}.weight"), g(f"norm1d.{i}.bias"), 3, x.shape[0] // 3)
    return x


# The oracle is fp32: a 251-term and two 300..400-term sums, three normalisations and (PyanNet) four recurrent layers.  Each fp32
# operation rounds by 6e-8; a few hundred of them per value, not all aligned, leave a relative L2 of a few 1e-7 to 1e-6.
ORACLE_FP32_FLOOR = 5e-6


def test_sincnet_chain_against_oracle(pyannet):
    sd, wav = pyannet
    ref = P.sincnet_forward(sd, wav[None, None])[0].T
    got = _sincnet_chain(sd, wav)
    assert got.shape == ref.shape
    e = S.rel_l2(got, ref)
    print(f"SincNet from the fp64 statements against the fp32 oracle: rel-L2 {e:.2e}")
    assert e < ORACLE_FP32_FLOOR


@pytest.mark.parametrize("powerset", [True, False])
def test_pyannet_chain_against_oracle(pyannet, powerset):
    sd, wav = pyannet
    x = _sincnet_chain(sd, wav)
    for l in range(4):
        wih = torch.cat([sd[f"lstm.weight_ih_l{l}{s}"] for s in ("", "_reverse")]).double()
        b = torch.cat([sd[f"lstm.bias_ih_l{l}{s}"] + sd[f"lstm.bias_hh_l{l}{s}"] for s in ("", "_reverse")]).double()
        whh = torch.stack([sd[f"lstm.weight_hh_l{l}{s}"] for s in ("", "_reverse")])
        x = S.lstm(x @ wih.T + b, whh, round_h=False)
    for i in range(2):
        x = F.leaky_relu(x @ sd[f"linear.{i}.weight"].double().T + sd[f"linear.{i}.bias"].double(), 0.01)
    got = S.activation(x @ sd["classifier.weight"].double().T + sd["classifier.bias"].double(), powerset)
    osd = dict(sd); osd["powerset"] = torch.tensor(1 if powerset else 0)
    ref = P.pyannet_forward(osd, wav[None, None])[0]
    e = S.rel_l2(got, ref)
    print(f"PyanNet from the fp64 statements against the fp32 oracle (powerset {powerset}): rel-L2 {e:.2e}")
    assert got.shape == ref.shape and e < ORACLE_FP32_FLOOR


# ---------------------------------------------------------------------------------------------- the sinc bound
@pytest.mark.parametrize("filters", S.SINC_FILTERS)
@pytest.mark.parametrize("inputs", S.SINC_INPUTS)
def test_sinc_bound_holds_for_the_split_arithmetic_on_every_gpu_input(filters, inputs):
    filt = S.sinc_filter_bank(filters)
    worst = 0.0
    crops = S.sinc_crops(inputs) + (S.sinc_grid_crops() if (filters, inputs) == ("mel", "zero-mean") else [])
    for x, n_pool in crops:
        ref, bound = S.sinc_stage(x, filt, S.NORM_W, S.NORM_B, n_pool)
        emu = S.sinc_split_emulation(x, filt, S.NORM_W, S.NORM_B, n_pool)
        assert bool((bound > 0).all())
        worst = max(worst, float(((emu - ref).abs() / bound).max()))
    print(f"sinc split emulation, {filters} filters, {inputs}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("filters", ["mel", "dense"])
def test_sinc_bound_sees_near_miss_convolutions(filters):
    """Each near miss moves the fp64 reference by more than the bound on more than a quarter of the outputs it touches (all of them:
    every output reads every tap and every sample of its window)."""
    filt = S.sinc_filter_bank(filters)
    n_pool = 129
    x = S.sinc_wave("zero-mean", S.sinc_samples(n_pool, 1), 7)          # one position beyond the pooled ones, for the shifted pool
    ref, bound = S.sinc_stage(x, filt, S.NORM_W, S.NORM_B, n_pool)
    seen = {name: float(((y - ref).abs() > bound).double().mean()) for name, y in S.sinc_near_misses(x, filt, S.NORM_W, S.NORM_B, n_pool).items()}
    print(f"sinc near misses beyond the bound, {filters} filters: {seen}")
    assert len(seen) == 4
    for name, frac in seen.items():
        assert frac > 0.25, (name, frac)


def test_sinc_dc_finding_in_the_emulation():
    """Splitting the raw samples loses the dropped xl wl term relative to the raw magnitude: under a DC offset the error over the
    output rms grows by orders of magnitude; splitting x - mean keeps it at the zero-mean level (within 4 x)."""
    filt = S.sinc_filter_bank("mel")
    rel = {}
    for inputs in S.SINC_INPUTS[:3]:
        x = S.sinc_wave(inputs, 4081, 1)
        ref, _ = S.sinc_stage(x, filt, S.NORM_W, S.NORM_B, 128)
        rms = float(ref.pow(2).mean().sqrt())
        rel[inputs] = tuple(float((S.sinc_split_emulation(x, filt, S.NORM_W, S.NORM_B, 128, centre=c) - ref).abs().max()) / rms for c in (False, True))
    print(f"sinc split emulation, worst error over output rms (raw split, centred split): {rel}")
    zero = rel["zero-mean"]
    assert rel["dc 0.3 std 0.01"][0] > 10 * zero[0] and rel["dc 0.5 std 1e-3"][0] > 100 * zero[0]
    assert rel["dc 0.3 std 0.01"][1] < 4 * zero[1] and rel["dc 0.5 std 1e-3"][1] < 4 * zero[1]
