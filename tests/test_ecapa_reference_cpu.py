"""CPU: tests/ecapa_reference.py (the fp64 restatement the GPU tests compare against) checked against a SECOND statement assembled
from torch.nn.Conv1d(padding_mode="reflect"), BatchNorm1d.eval() and torch.stft, against hand-derived answers, and for the
conditions of non-degeneracy on exactly the inputs the GPU tests use."""
import math

import pytest
import torch
from torch import nn

from clearconverse_amd.weights import ECAPA_DILATIONS, ecapa_fbank_tables, synthetic_ecapa_state_dict
from tests import ecapa_reference as R

F64 = torch.float64
# bound of tests/test_ecapa_gpu.py on the embedding's rel-L2 (kept equal by test_the_gpu_bound_is_the_one_used_here)
GPU_EMB_REL_L2_BOUND = 2.5 * 4.992e-3


# ------------------------------------------------------------------------------------------------ second statement (torch.nn modules)
class TDNN(nn.Module):
    def __init__(self, sd, p, dilation=1):
        super().__init__()
        w = sd[p + ".conv.conv.weight"]
        k = w.shape[2]
        self.conv = nn.Conv1d(w.shape[1], w.shape[0], k, dilation=dilation, padding=dilation * (k - 1) // 2, padding_mode="reflect")
        self.norm = nn.BatchNorm1d(w.shape[0])
        self.conv.load_state_dict({"weight": w, "bias": sd[p + ".conv.conv.bias"]})
        self.norm.load_state_dict({k2: sd[f"{p}.norm.norm.{k2}"] for k2 in ("weight", "bias", "running_mean", "running_var")}, strict=False)
        self.double().eval()

    def forward(self, x):                       # [1, C, T]
        return self.norm(torch.relu(self.conv(x)))


def second_fbank(wav):
    tb = ecapa_fbank_tables()
    st = torch.stft(wav.to(F64), 400, 160, 400, window=tb["fbank.window"].to(F64), center=True, pad_mode="constant", return_complex=True)
    power = st.real ** 2 + st.imag ** 2                                        # [201, T]
    db = 10.0 * torch.log10(torch.clamp(tb["fbank.filters"].to(F64) @ power, min=1e-10))
    db = torch.maximum(db, db.amax() - 80.0)
    return db - db.mean(dim=1, keepdim=True)                                   # [80, T]


@torch.no_grad()
def second_embed(wav, sd):
    x = TDNN(sd, "blocks.0")(second_fbank(wav)[None])
    outs = []
    for i in (1, 2, 3):
        p, res = f"blocks.{i}", x
        u = TDNN(sd, p + ".tdnn1")(x)
        ys, prev = [], None
        for m, chunk in enumerate(torch.chunk(u, 8, dim=1)):
            if m == 0:
                y = chunk
            else:
                y = TDNN(sd, f"{p}.res2net_block.blocks.{m - 1}", ECAPA_DILATIONS[i])(chunk if m == 1 else chunk + prev)
            ys.append(y)
            prev = y
        t2 = TDNN(sd, p + ".tdnn2")(torch.cat(ys, dim=1))
        s = t2.mean(dim=2, keepdim=True)
        s = torch.relu(nn.functional.conv1d(s, sd[p + ".se_block.conv1.conv.weight"].to(F64), sd[p + ".se_block.conv1.conv.bias"].to(F64)))
        s = torch.sigmoid(nn.functional.conv1d(s, sd[p + ".se_block.conv2.conv.weight"].to(F64), sd[p + ".se_block.conv2.conv.bias"].to(F64)))
        x = s * t2 + res
        outs.append(x)
    m_ = TDNN(sd, "mfa")(torch.cat(outs, dim=1))
    T = m_.shape[2]
    mean = m_.mean(dim=2, keepdim=True)
    std = torch.sqrt(((m_ - mean) ** 2).mean(dim=2, keepdim=True).clamp(min=1e-12))
    attn = torch.cat([m_, mean.expand(-1, -1, T), std.expand(-1, -1, T)], dim=1)
    attn = torch.tanh(TDNN(sd, "asp.tdnn")(attn))
    attn = nn.functional.conv1d(attn, sd["asp.conv.conv.weight"].to(F64), sd["asp.conv.conv.bias"].to(F64))
    attn = torch.softmax(attn, dim=2)
    mu = (attn * m_).sum(dim=2)
    sg = torch.sqrt((attn * (m_ - mu[:, :, None]) ** 2).sum(dim=2).clamp(min=1e-12))
    bn = nn.BatchNorm1d(6144)
    bn.load_state_dict({k: sd[f"asp_bn.norm.{k}"] for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
    pooled = bn.double().eval()(torch.cat([mu, sg], dim=1)[:, :, None])
    return nn.functional.conv1d(pooled, sd["fc.conv.weight"].to(F64), sd["fc.conv.bias"].to(F64))[0, :, 0]


@pytest.mark.parametrize("n", [8000, 8333, 20000])
def test_restatement_equals_the_second_statement(n):
    sd = synthetic_ecapa_state_dict(seed=3)
    wav = R.speechlike(n, 5)
    tb = ecapa_fbank_tables()
    f1, f2 = R.fbank(wav, tb["fbank.window"], tb["fbank.filters"]), second_fbank(wav).T
    assert f1.shape == (1 + n // 160, 80) and float((f1 - f2).abs().max()) < 1e-7
    e1, e2 = R.embed(wav, sd), second_embed(wav, sd)
    assert e1.shape == (192,) and R.rel_l2(e1, e2) < 1e-9


# ------------------------------------------------------------------------------------------------ hand-derived answers
def test_reflection_at_five_frames():
    assert R.reflect_index(torch.arange(-4, 9), 5).tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0]
    # k3, dilation 4, identity-per-tap weights on one channel: out[t] = x[t-4] + 10 x[t] + 100 x[t+4] with reflected indices
    x = torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0]], dtype=F64)
    w = torch.tensor([[[1.0, 10.0, 100.0]]], dtype=F64)
    out = R.conv_reflect(x, w, torch.zeros(1, dtype=F64), 4)[:, 0].tolist()
    assert out == [5 + 10 + 500, 4 + 20 + 400, 3 + 30 + 300, 2 + 40 + 200, 1 + 50 + 100]


def test_top_db_clamp_by_hand():
    # a loud frame and silence: the silent frames sit at max - 80, and the mean is taken AFTER the clamp
    tb = ecapa_fbank_tables()
    wav = torch.zeros(1600)
    wav[:400] = torch.sin(2 * math.pi * 1000 * torch.arange(400) / 16000.0)
    db = R.fbank_db(wav, tb["fbank.window"], tb["fbank.filters"])
    out, clamped = R.fbank(wav, tb["fbank.window"], tb["fbank.filters"], return_clamped=True)
    assert float(db.min()) == -100.0 and float(db.max()) > 0
    floor = float(db.max()) - 80.0
    by_hand = torch.clamp(db, min=floor)
    by_hand = by_hand - by_hand.sum(dim=0, keepdim=True) / db.shape[0]
    assert torch.equal(out, by_hand) and bool(clamped[-1].all()) and not bool(clamped[1].all())


def test_symmetric_triangle_filter_by_hand():
    f = ecapa_fbank_tables()["fbank.filters"].to(F64)
    assert f.shape == (80, 201)
    mel = torch.linspace(0.0, 2595.0 * math.log10(1 + 8000 / 700.0), 82, dtype=F64)
    hz = 700.0 * (10 ** (mel / 2595.0) - 1)
    freqs = torch.arange(201, dtype=F64) * 40.0
    for i in (0, 17, 79):
        left = float(hz[i + 1] - hz[i])                               # BOTH slopes use the left band width
        tri = torch.clamp(1.0 - (freqs - hz[i + 1]).abs() / left, min=0.0)
        assert float((f[i] - tri).abs().max()) < 1e-6, i
    # so the support is symmetric around the centre, narrower on the right than the HTK triangle's
    nz = torch.nonzero(f[79])[:, 0]
    assert float(freqs[nz[-1]]) < float(hz[80]) + float(hz[80] - hz[79])
    assert torch.equal(ecapa_fbank_tables()["fbank.window"], torch.hamming_window(400, periodic=True))


def test_linearity_split_of_the_context_term():
    g = torch.Generator().manual_seed(0)
    T, C_ = 9, 3072
    x = torch.randn(T, C_, generator=g, dtype=F64)
    W = torch.randn(128, 3 * C_, generator=g, dtype=F64)
    b = torch.randn(128, generator=g, dtype=F64)
    mean, std = R.ctx_stats(x)
    full = torch.cat([x, mean[None].expand(T, -1), std[None].expand(T, -1)], dim=1) @ W.T + b
    split = x @ W[:, :C_].T + (W[:, C_:2 * C_] @ mean + W[:, 2 * C_:] @ std + b)[None, :]
    assert float((full - split).abs().max()) < 1e-9
    assert abs(float(std[0]) - math.sqrt(float(((x[:, 0] - x[:, 0].mean()) ** 2).sum()) / T)) < 1e-12      # population std


def test_kernel_contracts_equal_the_network_statement():
    """res2net_ref / se_ref / asp_pool_ref (what the GPU kernel tests compare against) are the pieces `embed` is made of; one block
    against the module statement."""
    sd = synthetic_ecapa_state_dict(seed=4)
    g = torch.Generator().manual_seed(1)
    u = torch.randn(23, 1024, generator=g, dtype=F64)
    w, aff = R.res2net_params(sd, "blocks.2")
    got = R.res2net_ref(u, w, aff, 3)
    ys, prev = [], None
    with torch.no_grad():
        for m, chunk in enumerate(torch.chunk(u.T[None], 8, dim=1)):
            y = chunk if m == 0 else TDNN(sd, f"blocks.2.res2net_block.blocks.{m - 1}", 3)(chunk if m == 1 else chunk + prev)
            ys.append(y)
            prev = y
    assert R.rel_l2(got, torch.cat(ys, dim=1)[0].T) < 1e-12


# ------------------------------------------------------------------------------------------------ conditions of non-degeneracy
@pytest.fixture(scope="module")
def gpu_inputs_reference():
    sd, crops = R.gpu_test_state_dict(), R.gpu_test_crops()
    taps = [dict() for _ in crops]
    embs = [R.embed(c, sd, taps=t) for c, t in zip(crops, taps)]
    return embs, taps


def test_the_gpu_bound_is_the_one_used_here():
    from tests import test_ecapa_gpu
    assert GPU_EMB_REL_L2_BOUND == test_ecapa_gpu.EMB_REL_L2_BOUND


def test_condition_a_embeddings_of_different_crops_differ(gpu_inputs_reference):
    embs, _ = gpu_inputs_reference
    for i in range(len(embs)):
        for j in range(i):
            assert R.rel_l2(embs[i], embs[j]) >= 10 * GPU_EMB_REL_L2_BOUND, (i, j, R.rel_l2(embs[i], embs[j]))


def test_condition_b_attention_is_far_from_uniform(gpu_inputs_reference):
    for t in gpu_inputs_reference[1]:
        a = t["attention"]
        assert float(((a.max(dim=0).values / a.min(dim=0).values) >= 10).double().mean()) >= 0.5


def test_condition_c_top_db_clamp_engages_on_part_of_every_crop(gpu_inputs_reference):
    for t in gpu_inputs_reference[1]:
        frac = float(t["clamped"].double().mean())
        assert 0.05 <= frac <= 0.95, frac


def test_condition_d_se_gates_span_the_sigmoid(gpu_inputs_reference):
    for t in gpu_inputs_reference[1]:
        for e in t["gates"]:
            assert float(e.min()) <= 0.2 and float(e.max()) >= 0.8
