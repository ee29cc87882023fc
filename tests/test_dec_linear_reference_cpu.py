"""CPU: tests/dec_linear_reference.py against torch, the proof that the comparators of tests/test_dec_linear_gpu.py reject one-unit
mutations of the computation at that file's own inputs and bounds, and the fp32 yardstick those bounds are 4 x of
(profiles/dec_linear_measured_deviations.json, "yardstick")."""
import json

import torch
import torch.nn.functional as Fn

from tests import dec_linear_reference as LR
from tests import dec_reference as DR


def test_unmirrored_reference_is_torch_in_fp64():
    for K, N in ((128, 96), (768, 96), (1280, 96)):
        x, pend = LR.ln_inputs(K)
        w = LR.weights(K, N)
        xr = LR.resolve(x, pend, 3)
        assert torch.equal(xr, ((x + pend[0]) + pend[1]) + pend[2])
        wb = DR.bf16_round(w["w"]).double()
        ln = Fn.layer_norm(xr.double(), (K,), w["ln_g"].double(), w["ln_b"].double(), LR.EPS)
        mine = LR.layer_norm(xr, w["ln_g"], w["ln_b"], mirror=False)
        assert float((mine - ln).abs().max()) < 1e-12
        y = LR.linear(mine, w["w"], w["bias"])
        assert float((y - Fn.linear(ln, wb, w["bias"].double())).abs().max()) < 1e-12
        assert float((LR.gelu(y) - Fn.gelu(Fn.linear(ln, wb, w["bias"].double()))).abs().max()) < 1e-12
    for K in LR.SLICE_WIDTHS:
        a, w = LR.bf16_rows(16, K), LR.weights(K, LR.N_SMALL)
        slabs = LR.partial_slabs(a, w["w"], w["bias"])
        assert slabs.shape[0] == LR.ksplit(K, LR.PARTIAL)
        full = LR.linear(a, w["w"], w["bias"])
        assert float((slabs.sum(0) - full).abs().max()) < 1e-12 * float(full.abs().max()) * K
    for H in LR.COMBINE_HEADS:
        po, pml = LR.combine_inputs(H, 7, 5)
        po1, pml1 = LR.combine_inputs(H, 7, 1)                                  # the same keys in one split: the attention output itself
        assert float((LR.combine(po, pml, mirror=False) - LR.combine(po1, pml1, mirror=False)).abs().max()) < 1e-5


def test_restated_launcher_rules():
    assert [LR.ksplit(K, LR.PARTIAL) for K in (768, 1024, 1280, 1536, 2560, 3072, 4096, 5120)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [LR.ksplit(K, LR.F32) for K in (768, 1280)] == [1, 1]
    assert [b - a for a, b in LR.slab_columns(2560, 3)] == [27 * 32, 27 * 32, 26 * 32]
    assert [b - a for a, b in LR.slab_columns(5120, 4)] == [1280] * 4
    bad = [K for K in range(32, 1281, 32) if LR.starved(K, 1)]
    assert bad == [32, 64, 96, 160, 192, 288]
    for K in LR.LN_WIDTHS + LR.SLICE_WIDTHS + LR.QKV_WIDTHS + LR.TAIL_WIDTHS + tuple(64 * H for H in LR.COMBINE_HEADS):
        assert not LR.starved(K, LR.ksplit(K, LR.PARTIAL)), K


def test_rows_pin_the_shift_threshold_from_both_sides():
    """every row of every width and slab count has |mean| / std <= 0.8 or >= 1.25; the special rows are what they are said to be"""
    for K in LR.LN_WIDTHS:
        x, pend = LR.ln_inputs(K)
        for n in LR.LN_PEND:
            _, ratio = LR.centre_shift(LR.resolve(x, pend, n))
            assert bool(((ratio <= 0.8) | (ratio >= 1.25)).all()), (K, n, ratio)
            assert float(ratio[LR.ROW_HI]) >= 40.0 and float(ratio[LR.ROW_LO]) <= 0.1, (K, n, ratio)
            assert int(((ratio > 0.5) & (ratio <= 0.8)).sum()) >= 3 and int(((ratio >= 1.25) & (ratio < 2.5)).sum()) >= 3, (K, n, ratio)
            xr = LR.resolve(x, pend, n)
            assert float(xr[LR.ROW_FLAT].max()) == float(xr[LR.ROW_FLAT].min())


def _ln_case(K=768, n=3):
    x, pend = LR.ln_inputs(K)
    w = LR.weights(K, LR.N_SMALL)
    xr = LR.resolve(x, pend, n)
    ref = LR.linear(LR.layer_norm(xr, w["ln_g"], w["ln_b"]), w["w"], w["bias"])
    return x, pend, w, xr, ref


def test_mutations_of_the_layernorm_prologue_are_rejected():
    K = 768
    x, pend, w, xr, ref = _ln_case(K, 3)
    tol = LR.bound(LR.N_LN, K)

    def out(xr_, g=w["ln_g"], b=w["ln_b"]):
        return LR.linear(LR.layer_norm(xr_, g, b), w["w"], w["bias"])

    assert LR.row_rel_l2(out(xr), ref) == 0.0
    # one pending slab dropped
    dropped = LR.resolve(x, pend, 2)
    assert not torch.equal(dropped, xr) and LR.row_rel_l2(out(dropped), ref) >= tol
    # the slabs added in another order: only the bit check sees it
    assert not torch.equal(LR.resolve(x, pend, 3, order=(2, 1, 0)), xr)
    # rows r and r + 4 swapped
    swapped = out(xr).clone()
    swapped[[1, 5]] = swapped[[5, 1]]
    assert LR.row_rel_l2(swapped, ref) >= tol
    # gamma / beta off by one float4 slot of the 64 lanes
    assert LR.row_rel_l2(out(xr, g=torch.roll(w["ln_g"], 256)), ref) >= tol
    assert LR.row_rel_l2(out(xr, b=torch.roll(w["ln_b"], 256)), ref) >= tol
    # the centring shift with its threshold at 0.5: the rows between 0.5 and 0.8 must read exactly 0
    shift, ratio = LR.centre_shift(xr)
    wrong, _ = LR.centre_shift(xr, threshold=0.5)
    low = ratio <= 0.8
    assert bool((shift[low] == 0.0).all()) and not bool((wrong[low] == 0.0).all())
    # tanh-GELU for erf-GELU.  Behind a LayerNorm the bound is 4 x a yardstick made of rounding-boundary flips of the activations
    # (2.4e-4), and tanh-GELU (1.8e-4 .. 2.2e-4 at these inputs) hides below it; the cases from bf16 rows are what rejects it
    for Kg, N, _ in LR.GELU_BF16_CASES:
        for M in (5, 16):
            y = LR.linear(LR.bf16_rows(16, Kg)[:M], LR.weights(Kg, N)["w"], LR.weights(Kg, N)["bias"])
            assert LR.bf16_excess(DR.bf16_round(LR.gelu(y).float()), LR.gelu(y)) == 0.0
            assert LR.bf16_excess(DR.bf16_round(LR.gelu(y, tanh=True).float()), LR.gelu(y)) >= LR.bound_gelu_bf16(Kg), (Kg, N, M)


def test_mutations_of_the_split_k_epilogue_are_rejected():
    for K in (1536, 2560, 5120):
        a, w = LR.bf16_rows(16, K), LR.weights(K, LR.N_SMALL)
        ref = LR.partial_slabs(a, w["w"], w["bias"])
        tol = LR.bound(LR.n_bf16(K), K)
        assert LR.row_rel_l2(LR.partial_slabs(a, w["w"], w["bias"], bias_every=True), ref) >= tol
        for move in (1, -1):
            moved = LR.partial_slabs(a, w["w"], w["bias"], move=move)
            assert LR.row_rel_l2(moved, ref) >= tol
            assert LR.row_rel_l2(moved.sum(0), ref.sum(0)) < 1e-12      # which the sum of the slabs alone would not see


def test_mutations_of_the_cache_addressing_are_rejected():
    K, T = 128, 8
    w = LR.weights(K, 3 * K)
    tol = LR.bound(LR.N_CACHE_BF16, K)
    for case in ("a", "b", "c"):
        M, n_seq, pos, row_seq = LR.qkv_addressing(case, T)
        assert len(pos) == M and len({(m if row_seq is None else row_seq[m], pos[m]) for m in range(M)}) == M
        assert 0 in pos and T - 1 in pos
        rows = LR.linear(LR.bf16_rows(40, K)[:M], w["w"], w["bias"])[:, K:2 * K]
        exp, written = LR.cache_scatter(rows, pos, row_seq, n_seq, T)

        def kernel(pos_, row_seq_, n_alloc):
            """a cache as an epilogue with that addressing would leave it, over NaN sentinels, cut to the real sequences"""
            got, _ = LR.cache_scatter(DR.bf16_round(rows.float()), pos_, row_seq_, n_alloc, T + 1)
            return got[:n_seq, :, :T], ~torch.isnan(got[:n_seq, :, :T])

        got, touched = kernel(pos, row_seq, n_seq)
        ex, clean = LR.cache_figures(got, exp, written, ~touched)
        assert ex < tol and clean
        got, touched = kernel([p + 1 for p in pos], row_seq, n_seq)                          # pos off by one
        ex, clean = LR.cache_figures(got, exp, written, ~touched)
        assert not (ex < tol) or not clean
        if row_seq is not None:                                                             # row_seq ignored: row m is sequence m
            got, touched = kernel(pos, None, max(M, n_seq))
            ex, clean = LR.cache_figures(got, exp, written, ~touched)
            assert not (ex < tol) or not clean
    M, n_seq, pos, row_seq = LR.qkv_addressing("b", 448)
    assert 2 not in row_seq and n_seq == 3


def test_mutations_of_the_combine_prologue_are_rejected():
    for H in LR.COMBINE_HEADS:
        K = 64 * H
        po, pml = LR.combine_inputs(H, 7, 5)
        w = LR.weights(K, LR.N_SMALL)
        act = LR.combine(po, pml)
        ref = LR.partial_slabs(act, w["w"], w["bias"])
        sw = act.clone().reshape(7, H, 64)
        sw[:, [0, 1]] = sw[:, [1, 0]]                                                       # heads h and h + 1 swapped
        assert LR.row_rel_l2(LR.partial_slabs(sw.reshape(7, K), w["w"], w["bias"]), ref) >= LR.bound(LR.N_COMBINE, K)
    # the special partials are what they are said to be
    po, pml = LR.combine_inputs(2, 7, 8, 5, False)
    assert bool((pml[:, :, 5:, 0] == -1e30).all()) and bool((pml[:, :, 5:, 1] == 0).all()) and bool((po[:, :, 5:] == 0).all())
    po, pml = LR.combine_inputs(2, 7, 5, None, True)
    m = pml[..., 0]
    assert float((m[:, :, 1] - m[:, :, [0, 2, 3, 4]].amax(dim=-1)).min()) > 25.0
    assert bool(torch.isfinite(LR.combine(po, pml)).all())


def test_yardstick():
    """The fp32 evaluation's figures.  They involve no code under test.  The stored values are what the GPU test's bounds are 4 x of, so
    they must be what this file computes, as closely as the kind of figure allows (two x86 hosts, 1 .. 16 threads, were compared):
      * set by which activations land on the other side of a bf16 rounding boundary (behind a LayerNorm or the combine): a flip more
        or fewer moves them by tens of per cent, the hosts agree to 1e-4 -- within 10 %;
      * the fp32 sum's own error against fp64 (bf16 -> linear, 1e-7): the summation order is the host BLAS's, the hosts differ by up
        to 1.4 x -- within 2 x either way;
      * bf16 outputs from bf16 rows (GELU, cache): the excess exists only where the fp32 error carries ONE value across an output
        rounding boundary, a statistic of a count near 1 (7.8e-8 on one host, 4.7e-8 on the other) -- within 4 x either way."""
    y = LR.yardstick()
    for k, v in sorted(y.items()):
        print(f"  {k:90s} {v:.4e}")
    assert LR.PROFILE.exists(), f"{LR.PROFILE} is missing: regenerate it with `python -m tests.dec_linear_reference`"
    stored = json.loads(LR.PROFILE.read_text()).get("yardstick")
    assert stored is not None and set(stored) == set(y), "the stored yardstick is stale: regenerate it with `python -m tests.dec_linear_reference`"
    flips = {LR.N_LN: 1.1, LR.N_GELU: 1.1, LR.N_CACHE_LN: 1.1, LR.N_COMBINE: 1.1, LR.N_GELU_BF16: 4.0, LR.N_CACHE_BF16: 4.0}
    for k, v in y.items():
        f = flips.get(k, 2.0)
        assert stored[k] / f <= v <= stored[k] * f, (k, v, stored[k], "regenerate with `python -m tests.dec_linear_reference`")
        if k == LR.N_GELU_BF16:                            # listed only: its bound is a priori (LR.bound_gelu_bf16)
            assert v < LR.bound_gelu_bf16(128), (k, v)
        else:
            assert 0.0 < v < LR.ceiling(128) / 4.0, (k, v)
