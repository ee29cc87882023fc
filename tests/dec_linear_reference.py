"""Plain fp64 reference of the decode step's skinny linear (csrc/decoder.hip dec_linear_kernel) with its three prologues and four
epilogues, the inputs and cases of tests/test_dec_linear_gpu.py, the comparators that file uses, one-unit mutations of the reference and
the fp32 yardstick of its bounds.  CPU only: tests/test_dec_linear_reference_cpu.py checks this file against torch, shows that the
comparators reject every mutation at the GPU test's own inputs and bounds, and recomputes the yardstick (stored by
`python -m tests.dec_linear_reference`).

  resolved rows   x + slab 0 + slab 1 .. in fp32, one after the other (the kernel: fmaf(1, q, a)) -- exact, compared bit for bit
  LayerNorm       of those rows in fp64: two-pass variance, eps inside the root, gamma / beta; mirror=True rounds the result to
                  bf16, as the kernel rounds it into LDS
  centre_shift    the row's mean where |mean| * rstd > 1, else 0 (DEPI_RESOLVE's centring shift, written to ln_mean_out)
  combine         tests/dec_reference.py merge_partials in fp64, mirrored to bf16
  linear          act @ bf16(W)^T + bias in fp64
  split-K slabs   ksplit = ceil(K / 1024), or ceil(K / 1280) where that exceeds 4 (ccx_dec_linear_ksplit restated); slab z is the
                  product over the k-steps [z per_z, min((z + 1) per_z, K / 32)), per_z = ceil(K / 32 / ksplit); the bias in slab 0
  GELU            erf-GELU in fp64
  cache scatter   k / v rows into [n_seq][H][cache_T][64] at (row_seq[m] or m, h, pos[m])

Figures.  f32 outputs: per row ||got - ref|| / ||ref||.  bf16 outputs (GELU rows, cache k / v): the excess of |got - ref| over half a
bf16 ulp of ref, relative to the row's max |ref|.  Yardstick: the same figure for an fp32 evaluation of the same mirrored computation on
the CPU (slabs added in fp32, two-pass LayerNorm in fp32, bf16 rounding, fp32 matmul of bf16-rounded weights), worst over the GPU test's
inputs of a group; the bound is 4 x it and never above 2^-8 + K 2^-24 (bound()).
"""
import json
import math
from pathlib import Path

import torch

from tests import dec_reference as DR

PARTIAL, F32, SELF_QKV, GELU = range(4)                    # CCX_DEC_EPI_*
ACT_LN, ACT_BF16, ACT_COMBINE = range(3)                   # CCX_DEC_ACT_*
EPS = 1e-5
PROFILE = Path(__file__).resolve().parent.parent / "profiles" / "dec_linear_measured_deviations.json"

# ---- the GPU test's cases -----------------------------------------------------------------------------------------------------
LN_WIDTHS = (128, 384, 768, 896, 1024, 1152, 1280)         # 128, 384: a float4 slot partly live; 896 / 1024: depth 8; 1152 / 1280: 5 slots
LN_ROWS = (1, 4, 5, 9, 13, 16)
LN_PEND = (0, 1, 3, 4)
SIDE_PEND = (0, 3)                                         # pending slabs under the GELU and SELF_QKV epilogues (x_out, ln_mean_out there)
N_SMALL = 96                                               # 6 column blocks
GELU_CASES = ((128, 512, 520), (768, 96, 96), (1280, 96, 96))          # K, N, ldo
GELU_BF16_CASES = ((128, 512, 520), (768, 96, 96))                     # the same from bf16 rows, M = 5 and 16
QKV_WIDTHS = (128, 768, 1280)
QKV_CACHE_T = (8, 448)
COMBINE_HEADS = (2, 12, 20)
COMBINE_ROWS = (1, 7, 16)
COMBINE_NSPLIT = (1, 2, 5, 8)
SLICE_WIDTHS = (1536, 2048, 2560, 3072, 4096, 5120)        # 2 x 24, 2 x 32, 27 + 27 + 26, 3 x 32, 4 x 32, 4 x 40 k-steps
SLICE_ROWS = (3, 16)
TAIL_N = (4, 20, 104)
TAIL_WIDTHS = (128, 768)

# names of the figures (tests.conftest.within, profiles/dec_linear_measured_deviations.json)
N_LN = "dec linear: LayerNorm -> linear, f32 rows, rel-L2 per row"
N_COMBINE = "dec linear: combine -> linear, f32 slab rows, rel-L2 per row"
N_GELU = "dec linear: GELU rows, excess over half a bf16 ulp / row max"
N_CACHE_LN = "dec linear: cache k / v rows from LayerNorm rows, excess over half a bf16 ulp / row max"
N_CACHE_BF16 = "dec linear: cache k / v rows from bf16 rows, excess over half a bf16 ulp / row max"
N_GELU_BF16 = "dec linear: GELU rows from bf16 rows, excess over half a bf16 ulp / row max"


def n_bf16(K):
    return f"dec linear: bf16 -> linear, K = {K}, f32 rows, rel-L2 per row"


def ceiling(K):
    """the project's a-priori bound of a bf16 x bf16 -> fp32 linear: 2^-8 + K 2^-24"""
    return 2.0 ** -8 + K * 2.0 ** -24


def bound(name, K):
    """4 x the stored yardstick of the figure, never above the a-priori ceiling"""
    y = json.loads(PROFILE.read_text())["yardstick"][name]
    return min(4.0 * y, ceiling(K))


def bound_gelu_bf16(K):
    """A priori, not 4 x a yardstick.  Without a LayerNorm in front no activation can land on the other side of a rounding boundary; the
    excess over half an ulp that is left is the fp32 error of the value before it is rounded, and it shows only where that error
    carries the value across a boundary of the OUTPUT -- a handful of the elements at most, often none, so the fp32 evaluation's worst
    is a zero-count statistic (test_yardstick prints it).  The fp32 sum: the K 2^-24 of the project's ceiling; erf-GELU in fp32: 4 ulp
    of a value no larger than the row's maximum, 2^-22.  Tanh-GELU stands 2e-4 away from erf-GELU in this figure."""
    return K * 2.0 ** -24 + 2.0 ** -22


# ---- restated launcher rules ---------------------------------------------------------------------------------------------------
def ksplit(K, epi):
    ks = -(-K // 1024)
    if epi != PARTIAL:
        return 1 if K <= 1280 else ks
    if ks > 4:
        ks = -(-K // 1280)
    return max(ks, 1)


def slab_columns(K, ks, move=0):
    """[(first column, end column)] of every slab; move: the boundaries shifted by that many k-steps (a mutation)"""
    ksteps = K // 32
    per_z = -(-ksteps // ks)
    cuts = [0] + [min(z * per_z + move, ksteps) for z in range(1, ks)] + [ksteps]
    return [(32 * cuts[z], 32 * cuts[z + 1]) for z in range(ks)]


def starved(K, ks):
    """whether a slice leaves one of the four waves without a k-step (the launcher refuses it)"""
    return any((b - a) // 32 <= 3 * -(-((b - a) // 32) // 4) for a, b in slab_columns(K, ks))


# ---- the reference ----------------------------------------------------------------------------------------------------------
def resolve(x, pend, pend_n, order=None):
    """x + the first pend_n slabs in fp32, one after the other (order: a permutation of the slabs, a mutation)"""
    xr = x.clone()
    for s in (order if order is not None else range(pend_n)):
        xr = xr + pend[s]
    return xr


def row_stats(xr):
    xd = xr.double()
    mean = xd.mean(dim=-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=-1, keepdim=True)
    return mean, var


def layer_norm(xr, g, b, eps=EPS, mirror=True):
    mean, var = row_stats(xr)
    xn = (xr.double() - mean) / torch.sqrt(var + eps) * g.double() + b.double()
    return DR.bf16_round(xn.float()).double() if mirror else xn


def centre_shift(xr, eps=EPS, threshold=1.0):
    mean, var = row_stats(xr)
    ratio = mean.abs() / torch.sqrt(var + eps)
    return torch.where(ratio > threshold, mean, torch.zeros_like(mean))[:, 0], ratio[:, 0]


def combine(part_o, part_ml, mirror=True):
    """[M, H, ns, 64], [M, H, ns, 2] -> activation rows [M, 64 H]"""
    a = DR.merge_partials(part_o, part_ml).reshape(part_o.shape[0], -1)
    return DR.bf16_round(a.float()).double() if mirror else a


def linear(act, w, bias=None):
    y = act.double() @ DR.bf16_round(w).double().T
    return y if bias is None else y + bias.double()


def partial_slabs(act, w, bias, ks=None, bias_every=False, move=0):
    """the split-K slabs [ks, M, N] of a PARTIAL epilogue"""
    K = w.shape[1]
    ks = ksplit(K, PARTIAL) if ks is None else ks
    out = []
    for z, (a, b) in enumerate(slab_columns(K, ks, move)):
        out.append(linear(act[:, a:b], w[:, a:b], bias if (z == 0 or bias_every) else None))
    return torch.stack(out)


def gelu(y, tanh=False):
    y = y.double()
    if tanh:
        return 0.5 * y * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def cache_scatter(rows, pos, row_seq, n_seq, cache_T):
    """k or v rows [M, 64 H] -> (expected cache [n_seq, H, cache_T, 64] fp64, NaN where nothing is written; written [n_seq, cache_T])"""
    M, K = rows.shape
    H = K // 64
    exp = torch.full((n_seq, H, cache_T, 64), math.nan, dtype=torch.float64)
    written = torch.zeros(n_seq, cache_T, dtype=torch.bool)
    for m in range(M):
        s = m if row_seq is None else int(row_seq[m])
        exp[s, :, int(pos[m])] = rows[m].double().reshape(H, 64)
        written[s, int(pos[m])] = True
    return exp, written


# ---- the fp32 yardstick's side ---------------------------------------------------------------------------------------------
def layer_norm_f32(xr, g, b, eps=EPS):
    mean = xr.mean(dim=-1, keepdim=True)
    d = xr - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return DR.bf16_round(d * torch.rsqrt(var + eps) * g + b)


def combine_f32(part_o, part_ml):
    m, l = part_ml[..., 0], part_ml[..., 1]
    w = torch.exp2(m - m.amax(dim=-1, keepdim=True))
    a = (w[..., None] * part_o).sum(dim=-2) / (w * l).sum(dim=-1)[..., None]
    return DR.bf16_round(a.reshape(part_o.shape[0], -1))


def linear_f32(act, w, bias=None):
    y = act.float() @ DR.bf16_round(w).T
    return y if bias is None else y + bias


def partial_slabs_f32(act, w, bias):
    K = w.shape[1]
    return torch.stack([linear_f32(act[:, a:b], w[:, a:b], bias if z == 0 else None)
                        for z, (a, b) in enumerate(slab_columns(K, ksplit(K, PARTIAL)))])


# ---- comparators -----------------------------------------------------------------------------------------------------------
def row_rel_l2(got, ref):
    """worst ||got_r - ref_r|| / ||ref_r|| over the rows (last dimension) of a tensor"""
    g, r = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    return float(((g - r).norm(dim=1) / r.norm(dim=1)).max())


def bf16_excess(got, ref):
    """worst excess of |got - ref| over half a bf16 ulp of ref, relative to the row's max |ref| (rows: the last dimension)"""
    g, r = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    ex = ((g - r).abs() - DR.half_ulp_bf16(r)).clamp_min(0.0)
    return float((ex / r.abs().amax(dim=1, keepdim=True)).max())


def cache_figures(got, exp, written, sentinel_ok):
    """got [n_seq, H, T, 64] (the cache widened), sentinel_ok [n_seq, H, T, 64] bool (the element still holds the sentinel bits) ->
    (bf16 excess over the slots named, whether every other element is untouched)"""
    w = written[:, None, :, None].expand_as(sentinel_ok)
    g = got.double().permute(0, 2, 1, 3)[written]          # [slots, H, 64]
    e = exp.permute(0, 2, 1, 3)[written]
    if not bool(torch.isfinite(g).all()):
        return math.inf, bool(sentinel_ok[~w].all())
    return bf16_excess(g.reshape(g.shape[0], -1), e.reshape(e.shape[0], -1)), bool(sentinel_ok[~w].all())


# ---- inputs ------------------------------------------------------------------------------------------------------------------
_cache = {}
ROW_HI, ROW_LO, ROW_FLAT = 0, 1, 2       # |mean| / std >= 40; <= 0.1; all-equal (variance 0: eps decides)


def weights(K, N):
    key = ("w", K, N)
    if key not in _cache:
        g = torch.Generator().manual_seed(4000 + K + 13 * N)
        _cache[key] = {"w": (torch.randn(N, K, generator=g) / math.sqrt(K)).contiguous(), "bias": 0.1 * torch.randn(N, generator=g),
                       "ln_g": 1.0 + 0.1 * torch.randn(K, generator=g), "ln_b": 0.1 * torch.randn(K, generator=g)}
    return _cache[key]


def ln_inputs(K):
    """16 residual rows (randn + 0.5, column 3 x 20, then moved as a whole) and 4 pending slabs (0.5 randn) of width K.  Row ROW_HI
    sits 60 std from zero, ROW_LO has mean 0 under every slab count, ROW_FLAT is all-equal (1.5, its slab rows 0.25: every sum exact);
    of the other rows the odd ones keep |mean| / std in (0.5, 0.8] and the even ones >= 1.25 under every slab count of LN_PEND, so
    that the centring-shift threshold (1) is pinned from both sides while no row is near it."""
    key = ("ln", K)
    if key not in _cache:
        g = torch.Generator().manual_seed(500 + K)
        x = torch.randn(16, K, generator=g) + 0.5
        x[:, 3] *= 20.0
        pend = 0.5 * torch.randn(4, 16, K, generator=g)
        pend[:, ROW_LO] -= pend[:, ROW_LO].mean(dim=-1, keepdim=True)
        pend[:, ROW_FLAT] = 0.25
        xd = x.double()
        mean, std0 = xd.mean(dim=1), xd.std(dim=1, unbiased=False)
        std4 = torch.sqrt(std0 ** 2 + 1.0)                   # under four slabs of variance 0.25
        target = torch.where(torch.arange(16) % 2 == 1, 0.7 * std0, 1.6 * std4)
        target[ROW_HI], target[ROW_LO] = 60.0 * std4[ROW_HI], 0.0
        x = (xd + (target - mean)[:, None]).float()
        x[ROW_LO] -= x[ROW_LO].double().mean().float()
        x[ROW_FLAT] = 1.5
        _cache[key] = (x.contiguous(), pend.contiguous())
    return _cache[key]


def bf16_rows(M, K):
    """M activation rows of width K as the chain hands them on: bf16 values of LayerNorm-like size"""
    key = ("a", M, K)
    if key not in _cache:
        g = torch.Generator().manual_seed(900 + M + 3 * K)
        _cache[key] = DR.bf16_round(torch.randn(M, K, generator=g))
    return _cache[key]


def qkv_addressing(case, cache_T):
    """(M, n_seq, pos, row_seq) of the three addressing cases"""
    if case == "a":        # one row per sequence: pos 0, cache_T - 1 and values between
        pos = [0, cache_T - 1] + [(5 * m + 3) % cache_T for m in range(2, 16)]
        return 16, 16, pos, None
    if case == "b":        # 2 sequences x 5 prompt rows; sequence 2 is never named
        return 10, 3, [0, 1, 2, 3, 4] + list(range(cache_T - 5, cache_T)), [0] * 5 + [1] * 5
    # c: the prefill's shape, 4 sequences x 10 rows (three row tiles); cache_T = 8 holds 8 of them, so 5 sequences x 8 rows there
    per = 10 if cache_T >= 10 else 8
    n = 40 // per
    return 40, n, [cache_T - per + i for _ in range(n) for i in range(per)], [s for s in range(n) for _ in range(per)]


def combine_inputs(H, M, nsplit, T=None, spike=False):
    """split-KV partials of M rows x H heads from DR.attention_ref in f32, as the attention kernels leave them: an empty split is
    (m, l, o) = (-1e30, 0, 0).  T: keys (default 37); spike: one split's m stands 40 above the others."""
    key = ("c", H, M, nsplit, T, spike)
    if key not in _cache:
        T = 37 if T is None else T
        g = torch.Generator().manual_seed(7000 + 64 * H + 8 * M + T)    # (not the split count: the same keys under every split)
        q = torch.randn(M, H, 64, generator=g)
        k = DR.bf16_round(torch.randn(M, H, T, 64, generator=g))
        v = DR.bf16_round(torch.randn(M, H, T, 64, generator=g))
        if spike:
            per = -(-T // nsplit)
            k[:, :, per] = DR.bf16_round(q * (40.0 / DR.LOG2E * 8.0 / 64.0) + k[:, :, per])    # the first key of split 1
        _, _, (pm, pl, po) = DR.attention_ref(q, k, v, [T] * M, nsplit=nsplit)
        pm = torch.where(torch.isinf(pm), torch.full_like(pm, -1e30), pm)
        _cache[key] = (po.float().contiguous(), torch.stack([pm, pl], dim=-1).float().contiguous())
    return _cache[key]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def yardstick():
    """the figures of the fp32 evaluation against the mirrored fp64 reference, worst over the GPU test's inputs per group"""
    y = {}

    def keep(name, v):
        y[name] = max(y.get(name, 0.0), v)

    for K in LN_WIDTHS:                                                            # LayerNorm -> F32
        x, pend = ln_inputs(K)
        w = weights(K, N_SMALL)
        for n in LN_PEND:
            xr = resolve(x, pend, n)
            ref = linear(layer_norm(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"])
            keep(N_LN, row_rel_l2(linear_f32(layer_norm_f32(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"]), ref))
    for K, N, _ in GELU_CASES:                                                     # LayerNorm -> GELU
        x, pend = ln_inputs(K)
        w = weights(K, N)
        for n in SIDE_PEND:
            xr = resolve(x, pend, n)
            ref = gelu(linear(layer_norm(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"]))
            got = DR.bf16_round(torch.nn.functional.gelu(linear_f32(layer_norm_f32(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"])))
            keep(N_GELU, bf16_excess(got, ref))
    for K, N, _ in GELU_BF16_CASES:                                                # bf16 rows -> GELU (listed, not a bound: bound_gelu_bf16)
        a, w = bf16_rows(16, K), weights(K, N)
        got = DR.bf16_round(torch.nn.functional.gelu(linear_f32(a, w["w"], w["bias"])))
        keep(N_GELU_BF16, bf16_excess(got, gelu(linear(a, w["w"], w["bias"]))))
    for K in QKV_WIDTHS:                                                           # q | k | v from both activations
        w = weights(K, 3 * K)
        x, pend = ln_inputs(K)
        acts = [(N_LN, layer_norm(resolve(x, pend, n), w["ln_g"], w["ln_b"]), layer_norm_f32(resolve(x, pend, n), w["ln_g"], w["ln_b"])) for n in SIDE_PEND]
        for name, a64, a32 in acts + [(n_bf16(K), bf16_rows(40, K).double(), bf16_rows(40, K))]:
            ref, got = linear(a64, w["w"], w["bias"]), linear_f32(a32, w["w"], w["bias"])
            keep(name, row_rel_l2(got[:, :K], ref[:, :K]))
            for cols in (slice(K, 2 * K), slice(2 * K, 3 * K)):    # a row of the figure is one slot of one cache, as in cache_figures
                keep(N_CACHE_LN if name == N_LN else N_CACHE_BF16, bf16_excess(DR.bf16_round(got[:, cols]), ref[:, cols]))
    for H in COMBINE_HEADS:                                                        # combine -> PARTIAL
        for M, ns, T, spike, N in combine_cases(H):
            po, pml = combine_inputs(H, M, ns, T, spike)
            w = weights(64 * H, N)
            keep(N_COMBINE, row_rel_l2(partial_slabs_f32(combine_f32(po, pml), w["w"], w["bias"]), partial_slabs(combine(po, pml), w["w"], w["bias"])))
    for K in SLICE_WIDTHS:                                                         # bf16 -> PARTIAL, K slices
        a, w = bf16_rows(16, K), weights(K, N_SMALL)
        ref, got = partial_slabs(a, w["w"], w["bias"]), partial_slabs_f32(a, w["w"], w["bias"])
        keep(n_bf16(K), max(row_rel_l2(got, ref), row_rel_l2(got.double().sum(0), ref.sum(0))))
    for K in TAIL_WIDTHS:                                                          # bf16 -> F32, N tails
        for N in TAIL_N:
            a, w = bf16_rows(5, K), weights(K, N)
            keep(n_bf16(K), row_rel_l2(linear_f32(a, w["w"], w["bias"]), linear(a, w["w"], w["bias"])))
    return y


def write_yardstick():
    """`python -m tests.dec_linear_reference`: computes the yardstick and stores it in PROFILE under "yardstick" (the "measured" column
    is copied there by hand from a GPU run of tests/test_dec_linear_gpu.py)"""
    doc = json.loads(PROFILE.read_text()) if PROFILE.exists() else {}
    doc["yardstick"] = {k: float(f"{v:.4e}") for k, v in sorted(yardstick().items())}
    PROFILE.write_text(json.dumps(doc, indent=1) + "\n")


def combine_cases(H):
    """(M, nsplit, T, spike, N) of one head count: every row count and split count, T smaller than the split count (empty splits), a
    split 40 above the others, and N = K"""
    cases = [(M, ns, None, False, N_SMALL) for M in COMBINE_ROWS for ns in COMBINE_NSPLIT]
    cases += [(7, 8, 5, False, N_SMALL), (7, 5, None, True, N_SMALL), (16, 2, None, False, 64 * H)]
    return cases


if __name__ == "__main__":
    write_yardstick()
