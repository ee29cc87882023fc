"""fp64 references of the five SepFormer layer operators behind ccx_sep_op (csrc/sepformer.hip), the case generator of
tests/test_sep_kernels_gpu.py and the comparators both test files share.  No GPU, no library: plain torch on the CPU.

Every reference takes `mirror`.  mirror=False is the plain operation (oracle/sepformer_ref.py in float64, proven in
tests/test_sep_reference_cpu.py).  mirror=True rounds to bf16 exactly where the kernels do: the LayerNorm output; q, k and v after
the bias; the un-normalised p = 2^(s - max) as the operand of P V while the normaliser sums the unrounded p; O / l; the FFN hidden
activation after ReLU.  Weights are bf16 on both sides already.  `mut` switches on ONE deliberate mistake (MUTATIONS): the CPU suite
shows that the comparators reject each of them at the bounds the GPU tests use.  `dtype=torch.float32` repeats the mirrored
computation in single precision: the rounding-flip noise floor the first bounds were taken from.
"""
from __future__ import annotations

import math

import torch

D, NH, HD = 128, 8, 16
LOG2E = 1.4426950408889634
EPS_LN, EPS_GLN = 1e-6, 1e-8
KEY_BLOCK = 160          # sep_attention_kernel: online softmax over blocks of ten 16-key tiles

MUTATIONS = ("mask_minus", "mask_plus", "drop_q_bias", "drop_k_bias", "drop_v_bias", "swap_heads", "scale", "eps", "no_resid",
             "no_b2", "drop_stage_first", "drop_stage_last", "drop_stage_4", "swap_w2_stages", "gln_padded", "swap_taps", "swap_spk")


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _r(t, mirror):
    return bf16_round(t) if mirror else t


def layer_norm(x, g, b, eps=EPS_LN):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


# ---------------------------------------------------------------------------------------------------------------------------------
# attention of one sequence from q | k | v rows: [rows, 384] -> [len, 128]
# ---------------------------------------------------------------------------------------------------------------------------------
def attention_rows(qkv, length, mirror, mut=None, dtype=torch.float64, round_out=True):
    """qkv holds at least length (+ 1 for mask_plus) rows.  Keys are consumed in blocks of KEY_BLOCK with a running maximum, as the
    kernel does: p is rounded to bf16 relative to the maximum known when its block is consumed."""
    n_key = length + (1 if mut == "mask_plus" else -1 if mut == "mask_minus" else 0)
    n_key = max(n_key, 1)
    scale = 0.25 * (1.01 if mut == "scale" else 1.0) * LOG2E
    q = qkv[:length, 0:D].to(dtype).view(length, NH, HD).transpose(0, 1)          # [H, len, 16]
    k = qkv[:n_key, D:2 * D].to(dtype).view(n_key, NH, HD).transpose(0, 1)
    v = qkv[:n_key, 2 * D:].to(dtype).view(n_key, NH, HD).transpose(0, 1)
    t = (q @ k.transpose(1, 2)) * scale                                            # [H, len, n_key], log2 domain
    m = torch.full((NH, length), -1e30, dtype=dtype)
    l = torch.zeros(NH, length, dtype=dtype)
    o = torch.zeros(NH, length, HD, dtype=dtype)
    for k0 in range(0, n_key, KEY_BLOCK):
        tb = t[:, :, k0:k0 + KEY_BLOCK]
        m_new = torch.maximum(m, tb.max(-1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(tb - m_new[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + _r(p, mirror) @ v[:, k0:k0 + KEY_BLOCK]
        m = m_new
    out = _r(o / l[..., None], mirror and round_out)
    if mut == "swap_heads":
        out = out[[1, 0] + list(range(2, NH))]
    return out.transpose(0, 1).reshape(length, D)


def attention_op(qkv, seqs, mirror=True, mut=None, dtype=torch.float64, round_out=True):
    """CCX_SEP_ATTENTION: qkv [rows, 384] (bf16 values) -> the sequences' [len, 128].  round_out=False leaves O / l unrounded: the
    value whose bf16 rounding the kernel stores (bf16_out_excess compares against it)"""
    return [attention_rows(qkv[s0:], n, mirror, mut, dtype, round_out) for s0, n in seqs]


def attn_block_op(h, seqs, P, mirror=True, mut=None, dtype=torch.float64):
    """CCX_SEP_ATTN_BLOCK: h [rows, 128] -> list of the sequences' new rows.  P: ln_g, ln_b, wqkv, bqkv, wo, bo (weights bf16 values)."""
    eps = 1e-5 if mut == "eps" else EPS_LN
    bq = P["bqkv"].to(dtype).clone()
    for name, off in (("drop_q_bias", 0), ("drop_k_bias", D), ("drop_v_bias", 2 * D)):
        if mut == name:
            bq[off + 3 * HD: off + 4 * HD] = 0          # head 3
    outs = []
    for s0, n in seqs:
        extra = 1 if mut == "mask_plus" else 0
        x = h[s0:s0 + n + extra].to(dtype)
        y = _r(layer_norm(x, P["ln_g"].to(dtype), P["ln_b"].to(dtype), eps), mirror)
        qkv = _r(y @ P["wqkv"].to(dtype).T + bq, mirror)
        a = attention_rows(qkv, n, mirror, mut, dtype)
        upd = a @ P["wo"].to(dtype).T + P["bo"].to(dtype)
        outs.append(upd if mut == "no_resid" else x[:n] + upd)
    return outs


def ffn_op(h, n_tok, P, mirror=True, mut=None, dtype=torch.float64):
    """CCX_SEP_FFN: h [rows, 128] -> [n_tok, 128].  P: ln_g, ln_b, w1 [F, 128], b1, w2 [128, F], b2."""
    eps = 1e-5 if mut == "eps" else EPS_LN
    x = h[:n_tok].to(dtype)
    y = _r(layer_norm(x, P["ln_g"].to(dtype), P["ln_b"].to(dtype), eps), mirror)
    hid = _r(torch.relu(y @ P["w1"].to(dtype).T + P["b1"].to(dtype)), mirror)
    w2 = P["w2"].to(dtype).clone()
    n_stage = w2.shape[1] // 64
    drop = {"drop_stage_first": 0, "drop_stage_last": n_stage - 1, "drop_stage_4": 4}.get(mut)
    if drop is not None:
        assert drop < n_stage
        hid = hid.clone()
        hid[:, 64 * drop:64 * drop + 64] = 0
    if mut == "swap_w2_stages":
        assert n_stage >= 2
        a, b = w2[:, 0:64].clone(), w2[:, 64 * (n_stage - 1):].clone()
        w2[:, 0:64], w2[:, 64 * (n_stage - 1):] = b, a
    upd = hid @ w2.T
    if mut != "no_b2":
        upd = upd + P["b2"].to(dtype)
    return upd if mut == "no_resid" else x + upd


def final_norm_op(h, xin, seqs, P, mirror=True, mut=None, dtype=torch.float64, padded_len=None):
    """CCX_SEP_FINAL_NORM (fp32 only, nothing to mirror): y = gLN(LN(h)) + xin per sequence.  mut gln_padded: the statistics taken
    over the sequence padded with zero rows (LayerNorm gives beta there) to the next whole chunk of 150."""
    outs = []
    for s0, n in seqs:
        v = layer_norm(h[s0:s0 + n].to(dtype), P["ln_g"].to(dtype), P["ln_b"].to(dtype), EPS_LN)
        st = v
        if mut == "gln_padded":
            st = torch.cat([v, P["ln_b"].to(dtype).expand(n + (150 - n % 150) - n, D)])
        mean = st.mean()
        var = ((st - mean) ** 2).mean()
        outs.append(P["gln_g"].to(dtype) * (v - mean) / torch.sqrt(var + EPS_GLN) + P["gln_b"].to(dtype) + xin[s0:s0 + n].to(dtype))
    return outs


def decoder_op(feats, fc, utts, wdec, out_stride, mirror=True, mut=None, dtype=torch.float64):
    """CCX_SEP_DECODER: feats [rows, 128], fc [rows, 256] (channel-major, speaker minor), utts [(tok0, L, T)], wdec [128, 16]
    -> [n_utt, out_stride, 2]: est[t][s] = sum_l sum_c feats[l][c] relu(fc[l][2c + s]) wdec[c][t - 8l], zero from T on."""
    w = wdec.to(dtype)
    if mut == "swap_taps":
        w = torch.cat([w[:, 8:], w[:, :8]], dim=1)
    out = torch.zeros(len(utts), out_stride, 2, dtype=dtype)
    for u, (tok0, L, T) in enumerate(utts):
        f = feats[tok0:tok0 + L].to(dtype)
        m = torch.relu(fc[tok0:tok0 + L].to(dtype)).view(L, D, 2)
        if mut == "swap_spk":
            m = m.flip(-1)
        g = f[:, :, None] * m                                   # [L, 128, 2]
        frames = torch.einsum("lcs,ck->lks", g, w)              # [L, 16, 2]
        est = torch.zeros(8 * (L - 1) + 16, 2, dtype=dtype)
        for l in range(L):
            est[8 * l:8 * l + 16] += frames[l]
        n = min(T, est.shape[0], out_stride)
        out[u, :n] = est[:n]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# comparators and bounds
# ---------------------------------------------------------------------------------------------------------------------------------
# 2 x the worst value measured on an MI355X over tests/test_sep_kernels_gpu.py (profiles/sep_kernels_measured_deviations.json; rounded
# up to three digits).  The unit, special and dominant regimes are one row of the bound table (unit-variance statistics; a saturated
# softmax alone measures 3e-7, a figure one rounding flip would leave behind) and share twice the worst of the three.  They replaced
# the a-priori 4 x CPU noise floor (the mirrored reference in fp32 against itself in fp64, printed by
# tests/test_sep_reference_cpu.py::test_noise_floor): 1.4e-3 unit / special / dominant, 4.8e-3 offset, 1.06e-2 lowvar, 1.8e-2 per
# row, 1e-4 split.  DESIGN.md section 3 lists them next to the measured worst.
BOUNDS_A_PRIORI = False   # True: tests/test_sep_reference_cpu.py holds the bounds to 4 x the CPU floor from both sides
BOUND_SEQ = {"unit": 0.00111, "special": 0.00111, "dominant": 0.00111, "offset": 0.00142, "lowvar": 0.00454}   # per sequence / 32-token group
BOUND_ROW = 0.0065      # per row, all regimes
BOUND_SPLIT = 3.65e-05   # split attention, excess / max|v|


def update_rel_l2(got, ref, h_in):
    """the fused ops change h by an update: || got - ref || / || ref - h_in || over the given rows"""
    got, ref, h_in = got.double(), ref.double(), h_in.double()
    return float((got - ref).norm() / (ref - h_in).norm())


def update_rel_rows(got, ref, h_in):
    got, ref, h_in = got.double(), ref.double(), h_in.double()
    return float(((got - ref).norm(dim=-1) / (ref - h_in).norm(dim=-1)).max())


def half_ulp_bf16(ref):
    a = ref.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 8.0)


def bf16_out_excess(got, ref, vmax):
    """split attention writes bf16 from bf16 inputs: |got - ref| beyond half a bf16 ulp of ref, relative to the head's max |v|.
    got / ref [len, 128], vmax [8]"""
    ex = ((got.double() - ref).abs() - half_ulp_bf16(ref)).clamp_min(0.0)
    return float((ex.view(-1, NH, HD) / vmax.view(1, NH, 1)).max())


U32 = 2.0 ** -24


def final_norm_allowance(h, xin, seq, P):
    """Per-element allowance of the fp32 final norm for one sequence, derived in DESIGN.md section 3.  u = 2^-24; an n-term fp32 sum
    is off by at most (n + 3) u sum |terms|, every other operation by u |result|; an error of x - mean reaches the output scaled by
    rstd (447 in the low-variance regime: there the mean's own rounding, 131 u |x|, is the whole allowance).
      e_dx   = 131 u mean|x| + 2 u |x|                                        the row mean, then the subtraction
      e_rstd = 66 u + mean(|dx| e_dx) / (var + eps) + 2 u                      relative: half the variance's error, rsqrt
      e_v    = (e_dx rstd + |xhat| e_rstd + 3 u |xhat|) |g| + u |v|            v = xhat g + b
      gLN statistics over len x 128 values (128 len / 256 per lane, then 64 lanes, then 4 waves: chains of len / 2 + 70 terms):
      e_mean = chain u mean|v| + mean e_v,   e_sd (relative) = chain u + 2 (mean e_v + e_mean) / sd
      e_y    = |gg| (e_v + e_mean) / sd + |core| e_sd + 3 u (|core| + |bb| + |xin|),   core = gg (v - mean) / sd"""
    s0, n = seq
    x = h[s0:s0 + n].double()
    g, b = P["ln_g"].double(), P["ln_b"].double()
    mean = x.mean(-1, keepdim=True)
    dx = x - mean
    var = (dx ** 2).mean(-1, keepdim=True) + EPS_LN
    rstd = 1.0 / torch.sqrt(var)
    xhat = dx * rstd
    v = xhat * g + b
    e_dx = 131 * U32 * x.abs().mean(-1, keepdim=True) + 2 * U32 * x.abs()
    e_rstd = 66 * U32 + (dx.abs() * e_dx).mean(-1, keepdim=True) / var + 2 * U32
    e_v = (e_dx * rstd + xhat.abs() * e_rstd + 3 * U32 * xhat.abs()) * g.abs() + U32 * v.abs()
    gm = v.mean()
    sd = torch.sqrt(((v - gm) ** 2).mean() + EPS_GLN)
    chain = (n / 2 + 70) * U32
    e_mean = chain * v.abs().mean() + e_v.mean()
    e_sd = chain + 2 * (e_v.mean() + e_mean) / sd
    gg, bb = P["gln_g"].double(), P["gln_b"].double()
    core = gg * (v - gm) / sd
    return gg.abs() / sd * (e_v + e_mean) + core.abs() * e_sd + 3 * U32 * (core.abs() + bb.abs() + xin[s0:s0 + n].double().abs())


def decoder_allowance(feats, fc, utts, wdec, out_stride):
    """|est - ref| <= (n + 3) u sum |terms| with n = 256 products per sample and two factors rounded per product (+ 2)"""
    return (256 + 3 + 2) * U32 * decoder_op(feats.abs(), fc.abs(), utts, wdec.abs(), out_stride, mirror=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# case generator
# ---------------------------------------------------------------------------------------------------------------------------------
def make_params(seed, d_ffn=256):
    """bf16-rounded weights, random per-channel biases / LayerNorm parameters, the bias mean distinct per head"""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    head_mean = torch.linspace(-0.4, 0.4, NH).repeat_interleave(HD)
    P = {
        "ln_g": 1.0 + 0.2 * rn(D), "ln_b": 0.2 * rn(D), "gln_g": 1.0 + 0.2 * rn(D), "gln_b": 0.2 * rn(D),
        "wqkv": bf16_round(rn(3 * D, D) / math.sqrt(D)), "bqkv": 0.2 * rn(3 * D) + torch.cat([head_mean, -head_mean, head_mean.flip(0)]),
        "wo": bf16_round(rn(D, D) / math.sqrt(D)), "bo": 0.2 * rn(D),
        "w1": bf16_round(rn(d_ffn, D) / math.sqrt(D)), "b1": 0.2 * rn(d_ffn),
        "w2": bf16_round(rn(D, d_ffn) / math.sqrt(d_ffn)), "b2": 0.2 * rn(D),
        "wdec": 0.25 * rn(D, 16),
    }
    return P


def make_rows(regime, rows, seed):
    """h [rows, 128] f32 of an input regime.  Rows 0 and 1 of `lowvar` are not special; `special_rows` plants them."""
    g = torch.Generator().manual_seed(2000 + seed)
    z = torch.randn(rows, D, generator=g)
    if regime == "offset":
        return 30.0 + z
    if regime == "lowvar":
        return 5.0 + 2e-3 * z
    return z


def special_rows(h, zero_row, const_row):
    """one all-zero and one constant row: LayerNorm must give beta there"""
    h[zero_row] = 0.0
    h[const_row] = 3.0
    return h


def dominant_params(P, gain=3.0):
    """q and k of the `dominant` regime gain 3: the softmax of a planted key saturates"""
    Q = dict(P)
    w = P["wqkv"].clone()
    w[:2 * D] = bf16_round(w[:2 * D] * gain)
    Q["wqkv"] = w
    return Q


def plant_dominant_qkv(qkv, s0, length, pos, margin=24.0):
    """split attention: make key `pos` of the sequence the clear winner of every query and head (q, k stay bf16 values): the key
    becomes `margin` x the mean query direction of its head"""
    q = qkv[s0:s0 + length, :D].view(length, NH, HD)
    kk = q.mean(0)
    kk = kk / kk.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    q += 6.0 * kk[None]                                   # every query leans towards it
    qkv[s0 + pos, D:2 * D] = (margin * kk).reshape(D)
    qkv[s0:s0 + length] = bf16_round(qkv[s0:s0 + length])
    return qkv


def dominance_margin(qkv, s0, length, pos):
    """smallest gap, in the log2 domain of the kernel, between the planted key's score and the best other key's, over queries and heads"""
    q = qkv[s0:s0 + length, :D].double().view(length, NH, HD).transpose(0, 1)
    k = qkv[s0:s0 + length, D:2 * D].double().view(length, NH, HD).transpose(0, 1)
    t = (q @ k.transpose(1, 2)) * 0.25 * LOG2E
    if length == 1:
        return math.inf
    win = t[:, :, pos].clone()
    t[:, :, pos] = -math.inf
    gap = win - t.max(-1).values
    others = [i for i in range(length) if i != pos]      # the planted row's own query is no part of the construction
    return float(gap[:, others].min())


def mean_over_std(h):
    return float((h.double().mean(-1).abs() / h.double().std(-1, unbiased=False).clamp_min(1e-30)).min())


# ---------------------------------------------------------------------------------------------------------------------------------
# committed cases (the GPU tests and the CPU proofs use the same ones)
# ---------------------------------------------------------------------------------------------------------------------------------
FUSED_LENS = (1, 2, 15, 16, 17, 31, 33, 97, 150, 150, 159, 160)
SPLIT_LENS = (1, 16, 17, 150, 160, 161, 174, 320, 321, 335)
FFN_TOKENS = (1, 31, 257, 600)
FFN_WIDTHS = (64, 128, 192, 256, 320, 1024)
NORM_LENS = (1, 7, 150, 321)
ALL_REGIMES = ("unit", "offset", "lowvar", "special", "dominant")


def layout(lens, gap=3):
    """sequences laid out with `gap` unused rows in front of, between and behind them: [(start, len)], rows"""
    seqs, r = [], gap
    for n in lens:
        seqs.append((r, n))
        r += n + gap
    return seqs, r


def in_sequence_mask(seqs, rows):
    m = torch.zeros(rows, dtype=torch.bool)
    for s0, n in seqs:
        m[s0:s0 + n] = True
    return m


def dominant_pos(length, kind):
    """kind 0: position 0; 1: len - 1; 2: first key of the last tile; 3: last valid key of a partial tile (len - 1 again, asked for
    only at lengths that are no multiple of 16: FUSED_DOMINANT_KIND)"""
    assert kind != 3 or length % 16
    return (0, length - 1, (length - 1) // 16 * 16, length - 1)[kind]


# which key is planted in each sequence of FUSED_LENS: kind 3 sits on the partial tiles of 15, 31 and 150 tokens
FUSED_DOMINANT_KIND = (0, 1, 3, 2, 0, 3, 2, 1, 0, 3, 2, 1)


def plant_dominant_h(h, P, s0, length, pos):
    """fused attention, `dominant` regime: the rows of the sequence become one base row + 5 % noise, so every query is close to q0;
    row `pos` becomes the LayerNorm pre-image of the direction whose key best matches q0 in all heads at once."""
    g, b = P["ln_g"].double(), P["ln_b"].double()
    base = h[s0].double().clone()
    h[s0:s0 + length] = (base[None] + 0.05 * h[s0:s0 + length].double()).float()
    y0 = layer_norm(base, g, b)
    q0 = P["wqkv"][:D].double() @ y0 + P["bqkv"][:D].double()
    # per-head directions v_h = Wk_h^T q0_h, mixed with weights that even out the heads' margins over the base key
    wk = P["wqkv"][D:2 * D].double()
    vh = (wk * q0[:, None]).view(NH, HD, D).sum(1)                       # [8, 128]
    base_score = vh @ y0
    c = torch.ones(NH, dtype=torch.float64)
    for _ in range(300):
        y = c @ vh
        y = (y - y.mean()) / y.std(unbiased=False)
        gap = vh @ y - base_score
        c = c * torch.exp(-0.001 * (gap - gap.mean()))
        c = c / c.mean()
    h[s0 + pos] = ((y - b) / g).float()
    return h


def fused_margin(h, P, s0, length, pos):
    """dominance margin of a planted fused-attention case from the mirrored q and k (log2 domain, min over queries and heads)"""
    y = bf16_round(layer_norm(h[s0:s0 + length].double(), P["ln_g"].double(), P["ln_b"].double()))
    qkv = bf16_round(y @ P["wqkv"].double().T + P["bqkv"].double())
    return dominance_margin(qkv, 0, length, pos)


def fused_case(regime, seed):
    """h [rows, 128], seqs, parameters of the fused attention launch over FUSED_LENS"""
    seqs, rows = layout(FUSED_LENS)
    P = make_params(seed)
    h = make_rows("unit" if regime in ("special", "dominant") else regime, rows, seed)
    planted = []
    if regime == "special":
        for i, (s0, n) in enumerate(seqs):
            if n >= 15:
                special_rows(h, s0 + (i % n), s0 + n - 1 - (i % 7))
    if regime == "dominant":
        P = dominant_params(P)
        for i, (s0, n) in enumerate(seqs):
            pos = dominant_pos(n, FUSED_DOMINANT_KIND[i])
            plant_dominant_h(h, P, s0, n, pos)
            planted.append(pos)
    return h, seqs, rows, P, planted


def split_case(seed, dominant=None):
    """qkv [rows, 384] bf16 values over SPLIT_LENS; dominant: None, "first" (a key of the first key block) or "last" (of the last)"""
    seqs, rows = layout(SPLIT_LENS)
    g = torch.Generator().manual_seed(3000 + seed)
    qkv = bf16_round(torch.randn(rows, 3 * D, generator=g))
    planted = []
    if dominant:
        for i, (s0, n) in enumerate(seqs):
            last0 = (n - 1) // KEY_BLOCK * KEY_BLOCK
            pos = min(n - 1, 5 + i) if dominant == "first" else max(last0, n - 1 - (i if i % 2 else 0))
            plant_dominant_qkv(qkv, s0, n, pos)
            planted.append(pos)
    return qkv, seqs, rows, planted


def head_vmax(qkv, s0, n):
    return qkv[s0:s0 + n, 2 * D:].double().abs().view(n, NH, HD).amax(dim=(0, 2))


def ffn_case(regime, n_tok, d_ffn, seed):
    rows = n_tok + 5
    P = make_params(seed, d_ffn)
    h = make_rows("unit" if regime == "special" else regime, rows, seed)
    if regime == "special":
        special_rows(h, 0, n_tok - 1)
        if n_tok > 40:
            special_rows(h, 33, 17)
    return h, rows, P


def ffn_groups(n_tok):
    return [(a, min(a + 32, n_tok)) for a in range(0, n_tok, 32)]


def norm_case(regime, seed):
    seqs, rows = layout(NORM_LENS)
    P = make_params(seed)
    h = make_rows(regime, rows, seed)
    xin = make_rows("unit", rows, seed + 50)
    return h, xin, seqs, rows, P


def decoder_case(seed, segment=150, out_stride=1003):
    """three utterances: L = 1 (T = 16); T = 8 L + 13 (samples past 8 (L + 1) are zero); L = 150 exactly (a whole chunk of padding),
    trimmed to T = out_stride, no multiple of 8"""
    L = (1, 37, 150)
    T = (16, 8 * 37 + 13, out_stride)
    utts, r = [], 0
    for l, t in zip(L, T):
        utts.append((r, l, t))
        r += l + (segment - l % segment)
    rows = r + 2
    g = torch.Generator().manual_seed(4000 + seed)
    feats = torch.relu(torch.randn(rows, D, generator=g))
    fc = torch.randn(rows, 2 * D, generator=g)
    wdec = make_params(seed)["wdec"]
    return feats, fc, utts, rows, wdec, out_stride
