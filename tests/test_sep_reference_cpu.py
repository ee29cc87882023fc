"""CPU: the references of tests/sep_reference.py are what tests/test_sep_kernels_gpu.py believes.
 (a) unmirrored and chained they are oracle/sepformer_ref.py (`_block` and the decoder) in float64;
 (b) the mirrored references stay within a bf16-sized distance of the plain ones (twice what the committed inputs give);
 (c) the comparators, at the bounds the GPU tests use, reject every deliberate mistake of sep_reference.MUTATIONS in every input
     regime where it has an effect;
 (d) the case generator delivers the regimes it names (|mean| / std, eps against the variance, dominance margins).
"""

import pytest
import torch
import torch.nn.functional as F

from oracle import sepformer_ref as S
from tests import sep_reference as SR

D = SR.D


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) plain == oracle in float64
# ---------------------------------------------------------------------------------------------------------------------------------
class _Ref64(S.SepformerRef):
    """the oracle restated in float64: same code, double tensors (its positional encoding is added in double too)"""

    def __init__(self, dims, sd):
        self.d = dims
        self.sd = {k: v.detach().double() for k, v in sd.items()}


def _oracle_block(prefix, params, x):
    dims = S.SepDims(n_layers=len(params), d_ffn=params[0]["w1"].shape[0])
    sd = {}
    for l, P in enumerate(params):
        p = f"{prefix}.mdl.layers.{l}"
        sd.update({p + ".norm1.norm.weight": P["ln_g"], p + ".norm1.norm.bias": P["ln_b"],
                   p + ".self_att.att.in_proj_weight": P["wqkv"], p + ".self_att.att.in_proj_bias": P["bqkv"],
                   p + ".self_att.att.out_proj.weight": P["wo"], p + ".self_att.att.out_proj.bias": P["bo"],
                   p + ".norm2.norm.weight": P["ln2_g"], p + ".norm2.norm.bias": P["ln2_b"],
                   p + ".pos_ffn.ffn.0.weight": P["w1"], p + ".pos_ffn.ffn.0.bias": P["b1"],
                   p + ".pos_ffn.ffn.3.weight": P["w2"], p + ".pos_ffn.ffn.3.bias": P["b2"]})
    F_ = params[-1]
    sd.update({prefix + ".mdl.norm.norm.weight": F_["lnf_g"], prefix + ".mdl.norm.norm.bias": F_["lnf_b"],
               prefix + ".norm.weight": F_["gln_g"], prefix + ".norm.bias": F_["gln_b"]})
    return _Ref64(dims, sd)._block(prefix, x.double())


@pytest.mark.parametrize("length", [1, 17, 150])
def test_plain_chain_is_the_oracle_block(length):
    params = []
    for l in range(2):
        P = SR.make_params(10 + l, d_ffn=192)
        Q = SR.make_params(20 + l)
        P.update(ln2_g=Q["ln_g"], ln2_b=Q["ln_b"], lnf_g=Q["gln_g"], lnf_b=Q["gln_b"])
        params.append(P)
    g = torch.Generator().manual_seed(length)
    x = torch.randn(2, length, D, generator=g)                       # two sequences
    want = _oracle_block("b", params, x)
    # the same through the five-op vocabulary: block input (x + pe) by hand, then the ops over a flat token buffer
    h = (x.double() + S.positional_encoding(length, D).double()).reshape(2 * length, D)
    seqs = [(0, length), (length, length)]
    for P in params:
        h = torch.cat(SR.attn_block_op(h, seqs, P, mirror=False))
        P2 = dict(P, ln_g=P["ln2_g"], ln_b=P["ln2_b"])
        h = SR.ffn_op(h, 2 * length, P2, mirror=False)
    PF = dict(params[-1], ln_g=params[-1]["lnf_g"], ln_b=params[-1]["lnf_b"])
    got = torch.cat(SR.final_norm_op(h, x.reshape(2 * length, D), seqs, PF, mirror=False)).view(2, length, D)
    assert float((got - want).abs().max()) < 1e-10
    # the split form (LayerNorm, QKV by hand, attention_op, out-proj by hand) is the same attention
    P = params[0]
    h0 = (x.double() + S.positional_encoding(length, D).double()).reshape(2 * length, D)
    qkv = SR.layer_norm(h0, P["ln_g"].double(), P["ln_b"].double()) @ P["wqkv"].double().T + P["bqkv"].double()
    att = torch.cat(SR.attention_op(qkv, seqs, mirror=False))
    split = h0 + att @ P["wo"].double().T + P["bo"].double()
    assert float((split - torch.cat(SR.attn_block_op(h0, seqs, P, mirror=False))).abs().max()) < 1e-10


def test_plain_decoder_is_the_oracle_decoder():
    feats, fc, utts, rows, wdec, out_stride = SR.decoder_case(0)
    utts = utts + [(utts[1][0], 37, 8 * 36 + 16 + 5)]                # T - 16 not a multiple of 8
    got = SR.decoder_op(feats, fc, utts, wdec, out_stride, mirror=False)
    for u, (tok0, L, T) in enumerate(utts):
        f = feats[tok0:tok0 + L].double()
        masks = F.relu(fc[tok0:tok0 + L].double().view(L, D, 2))
        est = []
        for s in range(2):
            sep = (f * masks[:, :, s]).transpose(0, 1)[None]
            est.append(F.conv_transpose1d(sep, wdec.double()[:, None, :], None, stride=8)[0, 0])
        e = torch.stack(est, dim=-1)
        e = F.pad(e, (0, 0, 0, T - e.shape[0])) if T > e.shape[0] else e[:T]
        assert float((got[u, :T] - e).abs().max()) < 1e-10
        assert bool((got[u, T:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# noise floor and (b): mirrored against plain
# ---------------------------------------------------------------------------------------------------------------------------------
def _fused_metrics(a, b, h, seqs):
    return (max(SR.update_rel_l2(x, y, h[s0:s0 + n]) for x, y, (s0, n) in zip(a, b, seqs)),
            max(SR.update_rel_rows(x, y, h[s0:s0 + n]) for x, y, (s0, n) in zip(a, b, seqs)))


def _ffn_metrics(a, b, h, n_tok):
    return (max(SR.update_rel_l2(a[i:j], b[i:j], h[i:j]) for i, j in SR.ffn_groups(n_tok)), SR.update_rel_rows(a, b, h[:n_tok]))


FFN_PROOF_SHAPES = ((31, 64), (257, 320), (600, 1024))


def _a_priori(floor, bound, what):
    """an a-priori bound is 4 x the floor the committed inputs give: no tighter, and (rounding of the written figure aside) no looser"""
    assert 4 * floor <= bound * 1.05 and bound <= 4.5 * floor, (what, floor, bound)


def test_noise_floor():
    """fp32 against fp64, both mirrored: what rounding flips alone do to the comparators (printed with -s).  Every a-priori bound of
    sep_reference is 4 x its figure, checked from both sides."""
    row_floor = 0.0
    for regime in SR.ALL_REGIMES:
        worst_seq = worst_row = 0.0
        for seed in (0, 1):
            h, seqs, rows, P, _ = SR.fused_case(regime, seed)
            s, r = _fused_metrics(SR.attn_block_op(h, seqs, P, dtype=torch.float32), SR.attn_block_op(h, seqs, P), h, seqs)
            worst_seq, worst_row = max(worst_seq, s), max(worst_row, r)
            if regime != "dominant":
                for n_tok, d_ffn in FFN_PROOF_SHAPES:
                    h, rows, P = SR.ffn_case(regime, n_tok, d_ffn, seed)
                    s, r = _ffn_metrics(SR.ffn_op(h, n_tok, P, dtype=torch.float32), SR.ffn_op(h, n_tok, P), h, n_tok)
                    worst_seq, worst_row = max(worst_seq, s), max(worst_row, r)
        print(f"noise floor {regime}: per sequence {worst_seq:.2e}, per row {worst_row:.2e}")
        if SR.BOUNDS_A_PRIORI:
            _a_priori(worst_seq, SR.BOUND_SEQ[regime], regime)
        row_floor = max(row_floor, worst_row)
    worst = 0.0
    for seed in (0, 1):
        for dom in (None, "first", "last"):
            qkv, seqs, rows, _ = SR.split_case(seed, dom)
            ref = SR.attention_op(qkv, seqs, round_out=False)
            got = SR.attention_op(qkv, seqs, dtype=torch.float32)
            worst = max(worst, max(SR.bf16_out_excess(g, r, SR.head_vmax(qkv, s0, n)) for g, r, (s0, n) in zip(got, ref, seqs)))
    print(f"noise floor split attention: {worst:.2e}")
    if SR.BOUNDS_A_PRIORI:
        _a_priori(row_floor, SR.BOUND_ROW, "per row")
        _a_priori(worst, SR.BOUND_SPLIT, "split")


# twice what the committed inputs give (printed by the test): a bf16 rounding is 2^-9 relative per element, and the update is a sum of
# ~100 such terms of either sign
MIRROR_DISTANCE = {"unit": 6.6e-3, "offset": 6.6e-3, "lowvar": 6.1e-3, "special": 6.6e-3, "dominant": 1.5e-2}
MIRROR_DISTANCE_SPLIT = 3.3e-3   # |mirrored - plain| / the head's max |v|, split attention


def test_mirrored_stays_within_bf16_distance_of_plain():
    for regime in SR.ALL_REGIMES:
        worst = 0.0
        for seed in (0, 1):
            h, seqs, rows, P, _ = SR.fused_case(regime, seed)
            worst = max(worst, _fused_metrics(SR.attn_block_op(h, seqs, P), SR.attn_block_op(h, seqs, P, mirror=False), h, seqs)[0])
            if regime != "dominant":
                for n_tok, d_ffn in FFN_PROOF_SHAPES:
                    h, rows, P = SR.ffn_case(regime, n_tok, d_ffn, seed)
                    worst = max(worst, _ffn_metrics(SR.ffn_op(h, n_tok, P), SR.ffn_op(h, n_tok, P, mirror=False), h, n_tok)[0])
        print(f"mirrored - plain, {regime}: {worst:.2e}")
        assert worst < MIRROR_DISTANCE[regime], (regime, worst)
        assert worst > 2.0 ** -12, (regime, worst)                   # and the mirror does round
    worst = 0.0
    for seed in (0, 1):
        qkv, seqs, rows, _ = SR.split_case(seed)
        m, p = SR.attention_op(qkv, seqs), SR.attention_op(qkv, seqs, mirror=False)
        for a, b, (s0, n) in zip(m, p, seqs):
            worst = max(worst, float(((a - b).abs().view(n, SR.NH, SR.HD) / SR.head_vmax(qkv, s0, n).view(1, SR.NH, 1)).max()))
    print(f"mirrored - plain, split attention: {worst:.2e}")
    assert 2.0 ** -12 < worst < MIRROR_DISTANCE_SPLIT, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) every mutation is rejected at the bounds of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
# where a mutation has an effect: eps only against a variance of its own size (lowvar).  A 1 % scale error moves an update by ~6e-3
# (2.4e-3 where the softmax is saturated): above every regime's measured bound
FUSED_MUTATIONS = {
    "mask_minus": SR.ALL_REGIMES, "mask_plus": SR.ALL_REGIMES, "drop_q_bias": SR.ALL_REGIMES, "drop_v_bias": SR.ALL_REGIMES,
    "swap_heads": SR.ALL_REGIMES, "no_resid": SR.ALL_REGIMES, "scale": SR.ALL_REGIMES, "eps": ("lowvar",)}
FFN_MUTATIONS = {
    "no_resid": None, "no_b2": None, "drop_stage_first": None, "drop_stage_last": None, "drop_stage_4": None, "swap_w2_stages": None,
    "eps": ("lowvar",)}


def test_every_listed_mutation_is_tried():
    tried = set(FUSED_MUTATIONS) | set(FFN_MUTATIONS) | {"drop_k_bias", "gln_padded", "swap_taps", "swap_spk"}
    assert tried == set(SR.MUTATIONS)


@pytest.mark.parametrize("regime", SR.ALL_REGIMES)
def test_fused_attention_comparator_rejects_mutations(regime):
    h, seqs, rows, P, _ = SR.fused_case(regime, 0)
    ref = SR.attn_block_op(h, seqs, P)
    for mut, where in FUSED_MUTATIONS.items():
        if regime not in where:
            continue
        s, r = _fused_metrics(SR.attn_block_op(h, seqs, P, mut=mut), ref, h, seqs)
        print(f"{regime} {mut}: per sequence {s:.2e} (bound {SR.BOUND_SEQ[regime]:.1e})")
        assert s > SR.BOUND_SEQ[regime], (regime, mut, s)


def test_k_bias_cannot_matter():
    """q . (k + b) = q . k + q . b: the same for every key of a query, so softmax never sees a key bias.  Dropping head 3's changes
    nothing in exact arithmetic (and only rounding flips in the mirrored one): no comparator can or needs to reject it."""
    h, seqs, rows, P, _ = SR.fused_case("unit", 0)
    a, b = SR.attn_block_op(h, seqs, P, mirror=False, mut="drop_k_bias"), SR.attn_block_op(h, seqs, P, mirror=False)
    assert max(float((x - y).abs().max()) for x, y in zip(a, b)) < 1e-12


@pytest.mark.parametrize("regime", ["unit", "offset", "lowvar", "special"])
def test_ffn_comparator_rejects_mutations(regime):
    for n_tok, d_ffn in FFN_PROOF_SHAPES:
        h, rows, P = SR.ffn_case(regime, n_tok, d_ffn, 0)
        ref = SR.ffn_op(h, n_tok, P)
        for mut, where in FFN_MUTATIONS.items():
            if (where and regime not in where) or (mut == "drop_stage_4" and d_ffn < 320) or (mut == "swap_w2_stages" and d_ffn < 128):
                continue
            s, r = _ffn_metrics(SR.ffn_op(h, n_tok, P, mut=mut), ref, h, n_tok)
            assert s > SR.BOUND_SEQ[regime], (regime, n_tok, d_ffn, mut, s)


@pytest.mark.parametrize("dominant", [None, "first", "last"])
def test_split_attention_comparator_rejects_mutations(dominant):
    qkv, seqs, rows, _ = SR.split_case(0, dominant)
    ref = SR.attention_op(qkv, seqs, round_out=False)
    # a saturated softmax feels neither its scale nor one more ordinary key; a key less only where that key is the planted one
    muts = {None: ("mask_minus", "mask_plus", "swap_heads", "scale"), "first": ("swap_heads",), "last": ("mask_minus", "swap_heads")}[dominant]
    for mut in muts:
        got = SR.attention_op(qkv, seqs, mut=mut)
        worst = max(SR.bf16_out_excess(g, r, SR.head_vmax(qkv, s0, n)) for g, r, (s0, n) in zip(got, ref, seqs))
        print(f"split {dominant} {mut}: {worst:.2e} (bound {SR.BOUND_SPLIT:.1e})")
        assert worst > SR.BOUND_SPLIT, (dominant, mut, worst)


@pytest.mark.parametrize("regime", ["offset", "lowvar"])
def test_final_norm_allowance_holds_in_fp32_and_rejects_padded_statistics(regime):
    h, xin, seqs, rows, P = SR.norm_case(regime, 0)
    ref = SR.final_norm_op(h, xin, seqs, P)
    f32 = SR.final_norm_op(h, xin, seqs, P, dtype=torch.float32)
    for i, seq in enumerate(seqs):
        allow = SR.final_norm_allowance(h, xin, seq, P)
        assert bool(((f32[i].double() - ref[i]).abs() <= allow).all()), (regime, seq)
        s0, n = seq
        pad = SR.final_norm_op(h, xin, [seq], P, mut="gln_padded")[0]
        assert bool(((pad - ref[i]).abs() > allow).any()), (regime, seq)


def test_decoder_allowance_holds_in_fp32_and_rejects_mutations():
    feats, fc, utts, rows, wdec, out_stride = SR.decoder_case(0)
    ref = SR.decoder_op(feats, fc, utts, wdec, out_stride)
    allow = SR.decoder_allowance(feats, fc, utts, wdec, out_stride)
    f32 = SR.decoder_op(feats, fc, utts, wdec, out_stride, dtype=torch.float32)
    assert bool(((f32.double() - ref).abs() <= allow).all())
    for mut in ("swap_taps", "swap_spk"):
        bad = SR.decoder_op(feats, fc, utts, wdec, out_stride, mut=mut)
        for u in range(len(utts)):
            assert bool(((bad[u] - ref[u]).abs() > allow[u]).any()), (mut, u)


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the case generator's own numbers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_regimes_are_what_they_claim():
    assert SR.mean_over_std(SR.make_rows("offset", 200, 0)) > 20.0
    low = SR.make_rows("lowvar", 200, 0).double()
    var = low.var(-1, unbiased=False)
    assert SR.mean_over_std(low) > 2000.0
    assert 0.15 < float((SR.EPS_LN / var).min()) and float((SR.EPS_LN / var).max()) < 0.4      # eps is ~ a quarter of the variance
    h, seqs, rows, P, _ = SR.fused_case("special", 0)
    n_zero = int((h.abs().amax(-1) == 0).sum())
    n_const = int(((h.amax(-1) == h.amin(-1)) & (h.amax(-1) != 0)).sum())
    assert n_zero >= 5 and n_const >= 5
    y = SR.layer_norm(h[h.abs().amax(-1) == 0].double(), P["ln_g"].double(), P["ln_b"].double())
    assert torch.equal(y, P["ln_b"].double().expand_as(y))


def test_dominant_cases_dominate():
    h, seqs, rows, P, planted = SR.fused_case("dominant", 0)
    kinds = set()
    for i, ((s0, n), pos) in enumerate(zip(seqs, planted)):
        kind = SR.FUSED_DOMINANT_KIND[i]
        kinds.add(kind)
        assert pos == SR.dominant_pos(n, kind) and 0 <= pos < n
        assert kind != 3 or (n % 16 and pos == n - 1)                          # the last valid key of a PARTIAL tile
        if n > 1:
            assert SR.fused_margin(h, P, s0, n, pos) > 15.0, (n, pos)          # 2^-15 of the winner at most for any other key
    assert kinds == {0, 1, 2, 3}
    for dom in ("first", "last"):
        qkv, seqs, rows, planted = SR.split_case(0, dom)
        for (s0, n), pos in zip(seqs, planted):
            if n > 1:
                assert SR.dominance_margin(qkv, s0, n, pos) > 15.0, (dom, n, pos)
            assert (pos < SR.KEY_BLOCK) if dom == "first" else (pos >= (n - 1) // SR.KEY_BLOCK * SR.KEY_BLOCK)
