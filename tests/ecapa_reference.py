"""fp64 restatement of the ECAPA-TDNN speaker embedder (speechbrain/spkrec-ecapa-voxceleb) and of the four kernels of csrc/ecapa.hip.

[UPSTREAM-RECALL: speechbrain lobes/models/ECAPA_TDNN.py, lobes/features.py::Fbank, processing/features.py (STFT, Filterbank,
InputNormalization), the model card's hyperparams.yaml.]  speechbrain is not installed here and no checkpoint exists offline, so
parity with the published model is unpinned; tests/test_ecapa_reference_cpu.py checks this statement against a second one assembled
from torch.nn.Conv1d(padding_mode="reflect"), BatchNorm1d.eval() and torch.stft, and against hand-derived answers.

Everything is written with explicit index arithmetic (no torch.nn modules), in float64, channel-last ([T, C]) like the kernels.
It also owns the inputs the GPU tests use (`gpu_test_crops`, `gpu_test_state_dict`), so that the CPU suite can check the conditions of
non-degeneracy on exactly those inputs."""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

from clearconverse_amd.weights import ECAPA_DILATIONS, ecapa_fbank_tables, synthetic_ecapa_state_dict

F64 = torch.float64
N_FFT, HOP, TOP_DB, AMIN = 400, 160, 80.0, 1e-10
GPU_SEED = 23
GPU_CROP_SAMPLES = (8000, 12800, 31234, 144000)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round to bfloat16 and back (the kernels' inputs are rounded first: what is measured is the kernel, not its inputs)."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def reflect_index(q: torch.Tensor, T: int) -> torch.Tensor:
    """torch's `reflect` padding by index: q < 0 -> -q, q > T-1 -> 2 (T-1) - q (one reflection: |pad| <= T-1)."""
    q = torch.where(q < 0, -q, q)
    return torch.where(q > T - 1, 2 * (T - 1) - q, q)


# ---------------------------------------------------------------------------------------------- front end
def fbank_db(wav: torch.Tensor, window: torch.Tensor, filters: torch.Tensor) -> torch.Tensor:
    """[n] samples -> [T, 80] dB values BEFORE the top_db clamp and the mean subtraction; T = 1 + n // 160 (center=True, zero pad)."""
    wav, window, filters = wav.to(F64), window.to(F64), filters.to(F64)
    n = wav.numel()
    T = 1 + n // HOP
    padded = torch.cat([torch.zeros(N_FFT // 2, dtype=F64), wav, torch.zeros(N_FFT // 2, dtype=F64)])
    idx = torch.arange(T)[:, None] * HOP + torch.arange(N_FFT)[None, :]
    frames = padded[idx] * window[None, :]                                       # [T, 400]
    k = torch.arange(N_FFT // 2 + 1, dtype=F64)
    ang = 2.0 * math.pi * torch.outer(torch.arange(N_FFT, dtype=F64), k) / N_FFT  # [400, 201]
    power = (frames @ torch.cos(ang)) ** 2 + (frames @ torch.sin(ang)) ** 2
    return 10.0 * torch.log10(torch.clamp(power @ filters.T, min=AMIN))


def fbank(wav: torch.Tensor, window: torch.Tensor, filters: torch.Tensor, return_clamped: bool = False):
    """Fbank(n_mels=80) + InputNormalization(norm_type="sentence", std_norm=False): clamp from below at (the crop's maximum - 80),
    subtract each bin's mean over the crop's frames."""
    db = fbank_db(wav, window, filters)
    floor = db.max() - TOP_DB
    cl = torch.clamp(db, min=floor)
    out = cl - cl.mean(dim=0, keepdim=True)
    return (out, cl <= floor) if return_clamped else out


# ---------------------------------------------------------------------------------------------- blocks
def bn_fold(sd: Dict[str, torch.Tensor], p: str) -> Tuple[torch.Tensor, torch.Tensor]:
    sc = sd[p + ".weight"].to(F64) / torch.sqrt(sd[p + ".running_var"].to(F64) + 1e-5)
    return sc, sd[p + ".bias"].to(F64) - sd[p + ".running_mean"].to(F64) * sc


def conv_reflect(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, dilation: int) -> torch.Tensor:
    """Conv1d(padding="same", padding_mode="reflect") on channel-last x [T, I]; w [O, I, k] -> [T, O]."""
    T, k = x.shape[0], w.shape[2]
    out = b.to(F64)[None, :].expand(T, -1).clone()
    for tap in range(k):
        q = reflect_index(torch.arange(T) + (tap - (k - 1) // 2) * dilation, T)
        out += x[q] @ w[:, :, tap].to(F64).T
    return out


def tdnn_block(x: torch.Tensor, sd, p: str, dilation: int = 1) -> torch.Tensor:
    """TDNNBlock: Conv1d -> ReLU -> BatchNorm (running statistics)."""
    sc, sh = bn_fold(sd, p + ".norm.norm")
    return torch.relu(conv_reflect(x, sd[p + ".conv.conv.weight"], sd[p + ".conv.conv.bias"], dilation)) * sc + sh


def res2net_ref(x: torch.Tensor, w: torch.Tensor, aff: torch.Tensor, dilation: int) -> torch.Tensor:
    """The kernel's contract: x [T, 1024], w [7, 128, 128, 3], aff [7, 3 (bias | scale | shift), 128] -> y [T, 1024]."""
    x, w, aff = x.to(F64), w.to(F64), aff.to(F64)
    ys = [x[:, :128]]
    prev = None
    for s in range(7):
        z = x[:, 128 * (s + 1):128 * (s + 2)] + (prev if prev is not None else 0.0)
        prev = torch.relu(conv_reflect(z, w[s], aff[s, 0], dilation)) * aff[s, 1] + aff[s, 2]
        ys.append(prev)
    return torch.cat(ys, dim=1)


def res2net_params(sd, p: str) -> Tuple[torch.Tensor, torch.Tensor]:
    w = torch.stack([sd[f"{p}.res2net_block.blocks.{m}.conv.conv.weight"] for m in range(7)]).to(F64)
    aff = torch.stack([torch.stack([sd[f"{p}.res2net_block.blocks.{m}.conv.conv.bias"].to(F64),
                                    *bn_fold(sd, f"{p}.res2net_block.blocks.{m}.norm.norm")]) for m in range(7)])
    return w, aff


def se_ref(x: torch.Tensor, resid: torch.Tensor, w1, b1, w2, b2) -> Tuple[torch.Tensor, torch.Tensor]:
    """x, resid [T, 1024]; w1 [128, 1024], w2 [1024, 128] -> (gates * x + resid, gates [1024])."""
    x = x.to(F64)
    h = torch.relu(w1.to(F64) @ x.mean(dim=0) + b1.to(F64))
    e = torch.sigmoid(w2.to(F64) @ h + b2.to(F64))
    return e[None, :] * x + resid.to(F64), e


def asp_pool_ref(hidden: torch.Tensor, x: torch.Tensor, wa, ba, bn_scale, bn_shift, return_attention: bool = False):
    """hidden [T, 128], x [T, C], wa [C, 128] -> [2 C]: softmax over the frames per channel, weighted mean and std (clamped at
    1e-12 under the root), then asp_bn's affine."""
    hidden, x = hidden.to(F64), x.to(F64)
    a = torch.softmax(hidden @ wa.to(F64).T + ba.to(F64)[None, :], dim=0)
    mean = (a * x).sum(dim=0)
    std = torch.sqrt(torch.clamp((a * (x - mean[None, :]) ** 2).sum(dim=0), min=1e-12))
    out = torch.cat([mean, std]) * bn_scale.to(F64) + bn_shift.to(F64)
    return (out, a) if return_attention else out


def ctx_stats(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    mean = x.mean(dim=0)
    return mean, torch.sqrt(torch.clamp(((x - mean[None, :]) ** 2).mean(dim=0), min=1e-12))


def embed(wav: torch.Tensor, sd: Dict[str, torch.Tensor], tables=None, taps: dict | None = None) -> torch.Tensor:
    """One crop (its own utterance) -> [192] float64.  `taps` (optional dict) receives intermediates: "feats", "clamped", "gates"
    (list of 3), "attention" [T, 3072]."""
    tables = tables or ecapa_fbank_tables()
    feats, clamped = fbank(wav, tables["fbank.window"], tables["fbank.filters"], return_clamped=True)
    x = tdnn_block(feats, sd, "blocks.0", 1)
    outs, gates = [], []
    for i in (1, 2, 3):
        p = f"blocks.{i}"
        u = tdnn_block(x, sd, p + ".tdnn1")
        w, aff = res2net_params(sd, p)
        v = res2net_ref(u, w, aff, ECAPA_DILATIONS[i])
        t2 = tdnn_block(v, sd, p + ".tdnn2")
        x, e = se_ref(t2, x, sd[p + ".se_block.conv1.conv.weight"][:, :, 0], sd[p + ".se_block.conv1.conv.bias"],
                      sd[p + ".se_block.conv2.conv.weight"][:, :, 0], sd[p + ".se_block.conv2.conv.bias"])
        outs.append(x)
        gates.append(e)
    m = tdnn_block(torch.cat(outs, dim=1), sd, "mfa")
    mean, std = ctx_stats(m)
    T = m.shape[0]
    full = torch.cat([m, mean[None, :].expand(T, -1), std[None, :].expand(T, -1)], dim=1)      # [T, 9216]
    hidden = torch.tanh(tdnn_block(full, sd, "asp.tdnn"))
    bsc, bsh = bn_fold(sd, "asp_bn.norm")
    pooled, att = asp_pool_ref(hidden, m, sd["asp.conv.conv.weight"][:, :, 0], sd["asp.conv.conv.bias"], bsc, bsh, return_attention=True)
    if taps is not None:
        taps.update(feats=feats, clamped=clamped, gates=gates, attention=att, mfa=m, hidden=hidden)
    return sd["fc.conv.weight"][:, :, 0].to(F64) @ pooled + sd["fc.conv.bias"].to(F64)


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
def speechlike(n: int, seed: int) -> torch.Tensor:
    """n samples of a voiced-harmonics signal with a slow pitch glide, an on / off envelope (a third of the time is near silence: the
    top_db clamp engages there) and a faint noise floor."""
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.arange(n, dtype=F64) / 16000.0
    f0 = 110.0 + 35.0 * seed + 20.0 * torch.sin(2 * math.pi * (0.7 + 0.1 * seed) * t)
    ph = 2 * math.pi * torch.cumsum(f0, 0) / 16000.0
    amps = torch.rand(12, generator=g, dtype=F64) / torch.arange(1, 13, dtype=F64) ** (0.3 + 0.6 * seed)      # another spectral tilt per crop
    x = sum(amps[h - 1] * torch.sin(h * ph + 0.3 * h) for h in range(1, 13))
    env = (torch.sin(2 * math.pi * (2.1 + 0.3 * seed) * t + seed) > -0.45).to(F64)
    env = torch.clamp(torch.nn.functional.avg_pool1d(env[None, None, :], 161, 1, 80)[0, 0], 0, 1)
    noise = torch.randn(n, generator=g, dtype=F64)
    return (0.3 * env * x / x.abs().max() + (1e-3 * (1 + 4 * seed) * env + 1e-7) * noise).float()


def gpu_test_crops() -> List[torch.Tensor]:
    return [speechlike(n, i) for i, n in enumerate(GPU_CROP_SAMPLES)]


def gpu_test_state_dict() -> Dict[str, torch.Tensor]:
    return synthetic_ecapa_state_dict(seed=GPU_SEED)


def rel_l2(a, b) -> float:
    a, b = torch.as_tensor(a).to(F64), torch.as_tensor(b).to(F64)
    return float((a - b).norm() / b.norm())


def cosine(a, b) -> float:
    a, b = torch.as_tensor(a).to(F64).reshape(-1), torch.as_tensor(b).to(F64).reshape(-1)
    return float(a @ b / (a.norm() * b.norm()))
