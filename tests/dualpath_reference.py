"""fp64 restatement of the dual-path SepFormer (SpeechBrain's `Dual_Path_Model` with `SBTransformerBlock` intra / inter models, its
Encoder / Decoder and `SepformerSeparation.separate_batch`) and of the operators behind ccx_dualpath_op (csrc/dualpath.hip), the case
generators of the GPU tests and the committed bounds.  No GPU, no library: plain torch on the CPU.

[UPSTREAM-RECALL] SpeechBrain is not installed here: this follows lobes/models/dual_path.py (Encoder, Decoder, Dual_Path_Model,
Dual_Computation_Block, _padding / _Segmentation / _over_add, SBTransformerBlock) and lobes/models/transformer/Transformer.py
(TransformerEncoder, PositionalEncoding) from recollection.  PARITY STATUS: **parity unpinned** -- no fixture of a published
checkpoint's output exists offline; the HIP path is checked against this file only.  Rows of a batch are independent utterances.

`mirror=True` rounds to bf16 exactly where the kernels do: GEMM weights; the first GroupNorm's output; every LayerNorm output that
feeds a GEMM; q, k, v after the bias; the un-normalised p = 2^(s - max) as the operand of P V while the normaliser sums the unrounded
p (keys in blocks of KEY_BLOCK with a running maximum); O / l; the FFN hidden activation after ReLU; the PReLU output; the
overlap-add sum; the gate output.  `mut` switches on ONE deliberate mistake (MUTATIONS): tests/test_dualpath_reference_cpu.py shows
that each moves the model output by at least 4 x the bound the GPU model test commits to.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from tests.sep_reference import bf16_round, half_ulp_bf16, layer_norm   # comparators / helpers shared with the RE-SepFormer tests

LOG2E = 1.4426950408889634
EPS_LN, EPS_GN = 1e-6, 1e-8
KEY_BLOCK = 64           # dp_attention_kernel: online softmax over blocks of four 16-key tiles (csrc/dualpath.h CCX_DP_KEY_BLOCK)
U32 = 2.0 ** -24

MUTATIONS = ("mask_source_minor", "oa_average", "gap_simple", "gn_unpadded", "gn_per_chunk", "pe_wrong_axis", "inter_stride1",
             "no_intra_skip", "no_final_ln", "scale_256", "swap_tanh_sigmoid", "prelu_positive")

# ---- committed bounds ("Dual-path SepFormer separator", lists them next to the measured worst) ------------------------
# Each is at most 2.5 x the worst value measured on an MI355X over the GPU tests that use it.
# BOUND_MODEL: relative L2 of an utterance's sources against the mirrored fp64 reference over tests/test_dualpath_gpu.py's ragged
# batches (measured 4.56e-3; the same mirrored computation in fp32 on the CPU sits 1.9e-3 to 4.9e-3 from fp64: bf16 rounding flips,
# not arithmetic).  The weakest mutation (gn_per_chunk) moves the output by 4.9e-2, 4.5 x this bound.
BOUND_MODEL = 1.1e-2
BOUND_MODEL_FULL = 1.4e-2    # the same figure at full depth, 8 layers per transformer (measured 5.69e-3)
BOUND_ATT_EXCESS = 5.8e-5    # attention: |err| beyond half a bf16 ulp, relative to the head's max |v| (measured 2.32e-5)
BOUND_GN = 1.1e-4            # GroupNorm in fp32 (beyond half a bf16 ulp for the bf16 form), max|err| / max|ref| per utterance (4.59e-5)
MUTATION_FACTOR = 4.0


@dataclass
class Dims:
    n_filters: int = 256
    kernel: int = 16
    stride: int = 8
    d_model: int = 256
    n_head: int = 8
    d_ffn: int = 1024
    n_layers: int = 8
    n_blocks: int = 2
    segment: int = 250
    n_spk: int = 2


def _r(t, mirror):
    return bf16_round(t) if mirror else t


def positional_encoding(length: int, d: int) -> torch.Tensor:
    """Transformer.PositionalEncoding: interleaved sin / cos, built in fp32 as the library builds its table"""
    pe = torch.zeros(length, d)
    pos = torch.arange(length, dtype=torch.float32)[:, None]
    den = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(pos * den)
    pe[:, 1::2] = torch.cos(pos * den)
    return pe


# ---------------------------------------------------------------------------------------------------------------------------------
# segmentation / overlap-add  (token layout: [chunk s][position k][channel])
# ---------------------------------------------------------------------------------------------------------------------------------
def geometry(L: int, K: int, mut=None):
    """gap, S of L frames in chunks of K at 50 % overlap"""
    P = K // 2
    gap = K - L % K if mut == "gap_simple" else K - (P + L % K) % K
    return gap, (L + gap + P) // P          # = 2 (L + gap + P) / K chunks at hop P


def segmentation(x, K, mut=None):
    """x [L, C] -> chunks [S, K, C]: chunk j = padded[j P : j P + K] of [P zeros | x | gap zeros | P zeros]"""
    L, C = x.shape
    P = K // 2
    gap, S = geometry(L, K, mut)
    padded = torch.cat([x.new_zeros(P, C), x, x.new_zeros(gap + P, C)])
    return torch.stack([padded[j * P: j * P + K] for j in range(S)])


def valid_mask(L, K, mut=None):
    """[S, K] bool: which chunk entries hold a real frame"""
    return segmentation(torch.ones(L, 1), K, mut)[:, :, 0] > 0


def overlap_add(chunks, L, mut=None):
    """chunks [S, K, C] -> [L, C]: a plain sum of the two entries of every frame"""
    S, K, C = chunks.shape
    P = K // 2
    out = chunks.new_zeros((S + 1) * P, C)
    for j in range(S):
        out[j * P: j * P + K] += chunks[j]
    out = out[P: P + L]
    return out / 2 if mut == "oa_average" else out


def group_norm(x, g, b):
    """GroupNorm(1, C, eps 1e-8) of one utterance: statistics over every value of x [..., C], per-channel affine"""
    mean = x.mean()
    var = ((x - mean) ** 2).mean()
    return g * (x - mean) / torch.sqrt(var + EPS_GN) + b


# ---------------------------------------------------------------------------------------------------------------------------------
# attention of one sequence from q | k | v rows
# ---------------------------------------------------------------------------------------------------------------------------------
def attention_rows(qkv, n_head, mirror, mut=None, round_out=True):
    """qkv [..., len, 3 D] -> [..., len, D] (leading axes: independent sequences); keys consumed in blocks of KEY_BLOCK with a running
    maximum, as the kernel does"""
    lead, (n, D3) = qkv.shape[:-2], qkv.shape[-2:]
    Dm = D3 // 3
    hd = Dm // n_head
    scale = (1.0 / math.sqrt(Dm if mut == "scale_256" else hd)) * LOG2E
    qkv = qkv.reshape(-1, n, D3)
    B = qkv.shape[0]
    q = qkv[..., :Dm].reshape(B, n, n_head, hd).transpose(1, 2)
    k = qkv[..., Dm:2 * Dm].reshape(B, n, n_head, hd).transpose(1, 2)
    v = qkv[..., 2 * Dm:].reshape(B, n, n_head, hd).transpose(1, 2)
    t = (q @ k.transpose(-1, -2)) * scale
    m = torch.full((B, n_head, n), -1e30, dtype=qkv.dtype)
    l = torch.zeros(B, n_head, n, dtype=qkv.dtype)
    o = torch.zeros(B, n_head, n, hd, dtype=qkv.dtype)
    for k0 in range(0, n, KEY_BLOCK):
        tb = t[..., k0:k0 + KEY_BLOCK]
        m_new = torch.maximum(m, tb.max(-1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(tb - m_new[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + _r(p, mirror) @ v[..., k0:k0 + KEY_BLOCK, :]
        m = m_new
    out = _r(o / l[..., None], mirror and round_out)
    return out.transpose(1, 2).reshape(*lead, n, Dm)


def attention_op(qkv, seqs, n_head=8, mirror=True, round_out=True):
    """CCX_DP_ATTENTION: qkv [rows, 768] (bf16 values), seqs [(first, stride, len)] -> the sequences' [len, 256]"""
    outs = []
    for first, stride, n in seqs:
        idx = first + stride * torch.arange(n)
        outs.append(attention_rows(qkv[idx].double(), n_head, mirror, None, round_out))
    return outs


def att_excess(got, ref, vmax, n_head=8):
    """|got - ref| beyond half a bf16 ulp of ref (the unrounded O / l), relative to the head's max |v|"""
    ex = ((got.double() - ref).abs() - half_ulp_bf16(ref)).clamp_min(0.0)
    n = ref.shape[0]
    return float((ex.view(n, n_head, -1) / vmax.view(1, n_head, 1)).max())


def gate_op(g):
    """g [rows, 2 C] -> tanh(g[:, :C]) * sigmoid(g[:, C:])"""
    C = g.shape[1] // 2
    return torch.tanh(g[:, :C]) * torch.sigmoid(g[:, C:])


def prelu_op(x, a, mut=None):
    return torch.where(x >= 0, a * x, x) if mut == "prelu_positive" else torch.where(x >= 0, x, a * x)


def encoder_op(mix, w, stride):
    """mix [T], w [N, kernel] -> [L, N], ReLU"""
    return torch.relu(F.conv1d(mix[None, None], w[:, None, :], None, stride=stride))[0].transpose(0, 1)


def decoder_op(feats, mask, wdec, stride, T, out_len):
    """feats [L, N], mask logits [L, n_spk, N], wdec [N, kernel] -> [out_len, n_spk], zero from T on"""
    L, S, N = mask.shape
    est = []
    for s in range(S):
        sep = (feats * torch.relu(mask[:, s])).transpose(0, 1)[None]
        est.append(F.conv_transpose1d(sep, wdec[:, None, :], None, stride=stride)[0, 0])
    e = torch.stack(est, -1)
    out = e.new_zeros(out_len, S)
    n = min(T, e.shape[0], out_len)
    out[:n] = e[:n]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
class DualPathRef:
    def __init__(self, dims, sd, mirror=False, mut=None, dtype=torch.float64):
        self.d, self.mirror, self.mut, self.dtype = dims, mirror, mut, dtype
        self.sd = {k: v.detach().to(dtype) for k, v in sd.items()}

    def _w(self, name):          # a GEMM weight: bf16 on the device
        w = self.sd[name]
        w = w.reshape(w.shape[0], -1)
        return _r(w, self.mirror)

    def transformer(self, prefix, x, pos):
        """SBTransformerBlock: x [n_seq, len, D], pos [n_seq, len] positions -> same shape"""
        d, sd, mir = self.d, self.sd, self.mirror
        n, L, D = x.shape
        pe = positional_encoding(int(pos.max()) + 1, D).to(self.dtype)
        h = x + pe[pos]
        for l in range(d.n_layers):
            p = f"{prefix}.mdl.layers.{l}"
            y = _r(layer_norm(h, sd[p + ".norm1.norm.weight"], sd[p + ".norm1.norm.bias"], EPS_LN), mir)
            qkv = _r(y @ self._w(p + ".self_att.att.in_proj_weight").T + sd[p + ".self_att.att.in_proj_bias"], mir)
            att = attention_rows(qkv, d.n_head, mir, self.mut)
            h = h + att @ self._w(p + ".self_att.att.out_proj.weight").T + sd[p + ".self_att.att.out_proj.bias"]
            y = _r(layer_norm(h, sd[p + ".norm2.norm.weight"], sd[p + ".norm2.norm.bias"], EPS_LN), mir)
            hid = _r(torch.relu(y @ self._w(p + ".pos_ffn.ffn.0.weight").T + sd[p + ".pos_ffn.ffn.0.bias"]), mir)
            h = h + hid @ self._w(p + ".pos_ffn.ffn.3.weight").T + sd[p + ".pos_ffn.ffn.3.bias"]
        if self.mut != "no_final_ln":
            h = layer_norm(h, sd[prefix + ".mdl.norm.norm.weight"], sd[prefix + ".mdl.norm.norm.bias"], EPS_LN)
        return h

    def _gn(self, y, prefix, valid):
        g, b = self.sd[prefix + ".weight"], self.sd[prefix + ".bias"]
        if self.mut == "gn_per_chunk":
            return torch.stack([group_norm(c, g, b) for c in y])
        if self.mut == "gn_unpadded":
            v = y[valid]
            mean = v.mean()
            var = ((v - mean) ** 2).mean()
            return g * (y - mean) / torch.sqrt(var + EPS_GN) + b
        return group_norm(y, g, b)

    def dual_block(self, b, x, valid):
        """x [S, K, N] -> same"""
        S, K, N = x.shape
        ks = torch.arange(K)[None].expand(S, K)
        intra = self._gn(self.transformer(f"masknet.dual_mdl.{b}.intra_mdl", x, ks), f"masknet.dual_mdl.{b}.intra_norm", valid)
        if self.mut != "no_intra_skip":
            intra = intra + x
        if self.mut == "inter_stride1":          # the flat rows read as K sequences of S CONTIGUOUS rows
            xi = intra.reshape(K, S, N)
        else:
            xi = intra.transpose(0, 1)           # [K, S, N]: rows of one in-chunk position
        pos = torch.arange(K)[:, None].expand(K, S) if self.mut == "pe_wrong_axis" else torch.arange(S)[None].expand(K, S)
        yi = self.transformer(f"masknet.dual_mdl.{b}.inter_mdl", xi, pos)
        yi = yi.reshape(S, K, N) if self.mut == "inter_stride1" else yi.transpose(0, 1)
        return self._gn(yi, f"masknet.dual_mdl.{b}.inter_norm", valid) + intra

    def masks(self, mix_w):
        """mix_w [L, N] -> mask logits [L, n_spk, N] (before the final ReLU)"""
        d, sd, mir, mut = self.d, self.sd, self.mirror, self.mut
        L, N = mix_w.shape
        K = d.segment
        x = _r(group_norm(mix_w, sd["masknet.norm.weight"], sd["masknet.norm.bias"]), mir) @ self._w("masknet.conv1d.weight").T
        x = segmentation(x, K, mut)
        valid = valid_mask(L, K, mut)
        for b in range(d.n_blocks):
            x = self.dual_block(b, x, valid)
        S = x.shape[0]
        x = _r(prelu_op(x, sd["masknet.prelu.weight"], mut), mir)
        fc = x @ self._w("masknet.conv2d.weight").T + sd["masknet.conv2d.bias"]          # [S, K, N n_spk]
        if mut == "mask_source_minor":
            fc = fc.view(S, K, N, d.n_spk).permute(0, 1, 3, 2)                            # channel c n_spk + s
        else:
            fc = fc.view(S, K, d.n_spk, N)                                                # channel s N + c: source-major
        y = _r(overlap_add(fc.reshape(S, K, d.n_spk * N), L, mut), mir).view(L * d.n_spk, N)
        a = y @ self._w("masknet.output.0.weight").T + sd["masknet.output.0.bias"]
        g = y @ self._w("masknet.output_gate.0.weight").T + sd["masknet.output_gate.0.bias"]
        if mut == "swap_tanh_sigmoid":
            a, g = g, a
        z = _r(torch.tanh(a) * torch.sigmoid(g), mir)
        return (z @ self._w("masknet.end_conv1x1.weight").T).view(L, d.n_spk, N)

    def separate1(self, mix, out_len=None, return_masks=False):
        """mix [T] -> [out_len or T, n_spk]"""
        d, sd = self.d, self.sd
        mix = mix.to(self.dtype)
        T = mix.shape[0]
        mix_w = encoder_op(mix, sd["encoder.conv1d.weight"][:, 0], d.stride)
        m = self.masks(mix_w)
        out = decoder_op(mix_w, m, sd["decoder.weight"][:, 0], d.stride, T, out_len or T)
        return (out, torch.relu(m)) if return_masks else out

    def separate(self, mix, n_samples=None):
        """mix [B, T] -> [B, T, n_spk]; n_samples: true lengths of a ragged batch"""
        B, T = mix.shape
        ns = [T] * B if n_samples is None else list(n_samples)
        return torch.stack([self.separate1(mix[b, :ns[b]], T) for b in range(B)])


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def case_state_dict(dims, seed):
    """weights.synthetic_dualpath_state_dict with a WIDE affine on every transformer's final LayerNorm (gamma log-normal with sigma
    1.5, beta unit normal): with gamma near 1 every row leaves that LayerNorm with nearly the same mean and variance, and which rows a GroupNorm takes
    its statistics over (the gn_unpadded / gn_per_chunk mutations) would hardly show in the output."""
    from clearconverse_amd.weights import DualPathDims, synthetic_dualpath_state_dict
    sd = synthetic_dualpath_state_dict(DualPathDims(**dims.__dict__), seed=seed)
    g = torch.Generator().manual_seed(9000 + seed)
    for k in sorted(sd):
        if k.endswith(".mdl.norm.norm.weight"):
            sd[k] = torch.exp(1.5 * torch.randn(dims.d_model, generator=g))
        if k.endswith(".mdl.norm.norm.bias"):
            sd[k] = torch.randn(dims.d_model, generator=g)
    return sd


# frames of the short utterances both the CPU mutation test and the GPU model test run (K = 10: mostly padding; gap 2, 2 and 8)
MUTATION_CASE_FRAMES = (3, 13, 37)


def samples_for_frames(L, kernel=16, stride=8):
    return (L - 1) * stride + kernel


def synthetic_mix(T, seed):
    g = torch.Generator().manual_seed(7000 + seed)
    t = torch.arange(T, dtype=torch.float32) / 8000.0
    f = 100.0 + 300.0 * torch.rand(3, generator=g)
    return (0.3 * torch.sin(2 * math.pi * f[0] * t) + 0.2 * torch.sin(2 * math.pi * f[1] * t + 1.0)
            + 0.1 * torch.sin(2 * math.pi * f[2] * t + 2.0) + 0.05 * torch.randn(T, generator=g))


def samples_with_gap_K(K, kernel=16, stride=8):
    """a sample count whose frames L satisfy L % K == K - K / 2: a whole extra chunk of zeros (gap = K)"""
    L = K + (K - K // 2)
    return (L - 1) * stride + kernel


def attention_case(lens_strides, seed, gap=3):
    """qkv [rows, 768] bf16 values and [(first, stride, len)] laid out with `gap` unused rows around every sequence's span"""
    seqs, r = [], gap
    for n, stride in lens_strides:
        seqs.append((r, stride, n))
        r += (n - 1) * stride + 1 + gap
    g = torch.Generator().manual_seed(3000 + seed)
    return bf16_round(torch.randn(r, 768, generator=g)), seqs, r


def plant_dominant(qkv, seq, pos, margin=24.0, n_head=8):
    """make key `pos` of the sequence the clear winner of every query and head"""
    first, stride, n = seq
    idx = first + stride * torch.arange(n)
    D = qkv.shape[1] // 3
    q = qkv[idx, :D].view(n, n_head, -1)
    kk = q.mean(0)
    kk = kk / kk.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    qkv[idx, :D] = bf16_round((q + 4.0 * kk[None]).reshape(n, D))
    qkv[idx[pos], D:2 * D] = bf16_round((margin * kk).reshape(D))
    return qkv
