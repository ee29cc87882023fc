"""CPU: tests/dualpath_reference.py proven against independent statements -- the segmentation rule as known answers, a transformer
block against torch.nn.TransformerEncoderLayer(norm_first=True), GroupNorm against torch.nn.GroupNorm, one tiny model in closed form --
and shown to be sensitive: every mutation of MUTATIONS moves the model output by at least MUTATION_FACTOR x the bound the GPU model
test commits to.  Also the ctypes mirrors of the two new structs against include/ccx.h."""
import ctypes as C
import functools
import math
import re
from pathlib import Path

import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.weights import DualPathDims, synthetic_dualpath_state_dict
from tests import dualpath_reference as R

ROOT = Path(__file__).resolve().parent.parent


# ---- segmentation known answers ---------------------------------------------------------------------------------------------
def _lengths(K):
    return (1, 4, 5, 6, K - K // 2, K - K // 2 - 1, K, K + 1, 2 * K + 3, 999)


@pytest.mark.parametrize("K", [10, 250])
def test_chunk_j_is_a_slice_of_the_padded_signal(K):
    P = K // 2
    for L in _lengths(K):
        gap, S = R.geometry(L, K)
        assert 1 <= gap <= K and (gap == K) == (L % K == K - P)
        assert S == 2 * (L + gap + P) // K and S % 2 == 0 and S >= 2 and (2 * (L + gap + P)) % K == 0
        x = torch.arange(1.0, 3 * L + 1).view(L, 3)
        padded = torch.cat([torch.zeros(P, 3), x, torch.zeros(gap + P, 3)])
        chunks = R.segmentation(x, K)
        assert chunks.shape == (S, K, 3)
        for j in range(S):
            assert torch.equal(chunks[j], padded[j * P: j * P + K])
        assert int(R.valid_mask(L, K).sum()) == 2 * L


@pytest.mark.parametrize("K", [10, 250])
def test_overlap_add_of_the_segmentation_is_twice_the_signal(K):
    for L in _lengths(K):
        x = torch.randn(L, 3, dtype=torch.float64)
        assert torch.equal(R.overlap_add(R.segmentation(x, K), L), 2 * x)


# ---- the transformer block and GroupNorm against torch's own modules -----------------------------------------------------------
def test_transformer_block_against_torch_encoder_layers():
    dims = R.Dims(n_filters=32, d_model=32, n_head=4, d_ffn=64, n_layers=2, n_blocks=1, segment=6, n_spk=2)
    sd = synthetic_dualpath_state_dict(DualPathDims(**dims.__dict__), seed=3)
    ref = R.DualPathRef(dims, sd)
    prefix = "masknet.dual_mdl.0.intra_mdl"
    layers = []
    for l in range(dims.n_layers):
        m = torch.nn.TransformerEncoderLayer(32, 4, 64, dropout=0.0, activation="relu", layer_norm_eps=1e-6, batch_first=True, norm_first=True).double()
        p = f"{prefix}.mdl.layers.{l}"
        m.load_state_dict({
            "self_attn.in_proj_weight": sd[p + ".self_att.att.in_proj_weight"], "self_attn.in_proj_bias": sd[p + ".self_att.att.in_proj_bias"],
            "self_attn.out_proj.weight": sd[p + ".self_att.att.out_proj.weight"], "self_attn.out_proj.bias": sd[p + ".self_att.att.out_proj.bias"],
            "linear1.weight": sd[p + ".pos_ffn.ffn.0.weight"], "linear1.bias": sd[p + ".pos_ffn.ffn.0.bias"],
            "linear2.weight": sd[p + ".pos_ffn.ffn.3.weight"], "linear2.bias": sd[p + ".pos_ffn.ffn.3.bias"],
            "norm1.weight": sd[p + ".norm1.norm.weight"], "norm1.bias": sd[p + ".norm1.norm.bias"],
            "norm2.weight": sd[p + ".norm2.norm.weight"], "norm2.bias": sd[p + ".norm2.norm.bias"]})
        layers.append(m.eval())
    ln = torch.nn.LayerNorm(32, eps=1e-6).double()
    ln.load_state_dict({"weight": sd[prefix + ".mdl.norm.norm.weight"], "bias": sd[prefix + ".mdl.norm.norm.bias"]})
    x = torch.randn(3, 70, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(0))     # 70 keys: two key blocks
    pos = torch.arange(70)[None].expand(3, 70)
    with torch.no_grad():
        h = x + R.positional_encoding(70, 32).double()
        for m in layers:
            h = m(h)
        want = ln(h)
    got = ref.transformer(prefix, x, pos)
    assert float((got - want).abs().max()) < 1e-11


def test_group_norm_against_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 5, 16, dtype=torch.float64, generator=g) * 3 + 2          # [S, K, N]
    w, b = torch.randn(16, dtype=torch.float64, generator=g), torch.randn(16, dtype=torch.float64, generator=g)
    m = torch.nn.GroupNorm(1, 16, eps=1e-8).double()
    m.load_state_dict({"weight": w, "bias": b})
    with torch.no_grad():
        want = m(x.permute(2, 1, 0)[None])[0].permute(2, 1, 0)                   # [1, N, K, S]
    assert float((R.group_norm(x, w, b) - want).abs().max()) < 1e-12


# ---- one tiny model in closed form ----------------------------------------------------------------------------------------------
def test_tiny_model_by_hand():
    """N = 2, kernel 2 (stride 1), K = 2, two sources.  Every transformer's final LayerNorm and every block norm has gamma = beta = 0,
    so a dual block is the identity; what is left is written out below sample by sample."""
    dims = R.Dims(n_filters=2, kernel=2, stride=1, d_model=2, n_head=1, d_ffn=4, n_layers=1, n_blocks=2, segment=2, n_spk=2)
    sd = synthetic_dualpath_state_dict(DualPathDims(**dims.__dict__), seed=5)
    for k in sd:
        if ".mdl.norm.norm." in k or "_norm." in k:
            sd[k] = torch.zeros_like(sd[k])
    mix = torch.tensor([0.5, -1.0, 2.0, 0.25], dtype=torch.float64)
    got = R.DualPathRef(dims, sd).separate1(mix)

    D = lambda k: sd[k].double()
    we, wd = D("encoder.conv1d.weight")[:, 0], D("decoder.weight")[:, 0]
    feats = [[max(0.0, float(we[c, 0] * mix[l] + we[c, 1] * mix[l + 1])) for c in range(2)] for l in range(3)]      # L = 3
    vals = [v for row in feats for v in row]
    mean = sum(vals) / 6
    var = sum((v - mean) ** 2 for v in vals) / 6
    est = [[0.0, 0.0] for _ in range(4)]
    for l in range(3):
        xn = [float(D("masknet.norm.weight")[c]) * (feats[l][c] - mean) / math.sqrt(var + 1e-8) + float(D("masknet.norm.bias")[c]) for c in range(2)]
        x = [sum(float(D("masknet.conv1d.weight")[o, c, 0]) * xn[c] for c in range(2)) for o in range(2)]
        a = float(D("masknet.prelu.weight")[0])
        x = [v if v >= 0 else a * v for v in x]
        for s in range(2):
            # every frame sits in exactly two chunks: the overlap-add doubles the 1 x 1 convolution (bias included); rows s N + c
            y = [2 * (sum(float(D("masknet.conv2d.weight")[s * 2 + o, c, 0, 0]) * x[c] for c in range(2)) + float(D("masknet.conv2d.bias")[s * 2 + o]))
                 for o in range(2)]
            t = [sum(float(D("masknet.output.0.weight")[o, c, 0]) * y[c] for c in range(2)) + float(D("masknet.output.0.bias")[o]) for o in range(2)]
            g = [sum(float(D("masknet.output_gate.0.weight")[o, c, 0]) * y[c] for c in range(2)) + float(D("masknet.output_gate.0.bias")[o]) for o in range(2)]
            z = [math.tanh(t[o]) / (1 + math.exp(-g[o])) for o in range(2)]
            m = [max(0.0, sum(float(D("masknet.end_conv1x1.weight")[o, c, 0]) * z[c] for c in range(2))) for o in range(2)]
            for k in range(2):
                est[l + k][s] += sum(feats[l][c] * m[c] * float(wd[c, k]) for c in range(2))
    assert float((got - torch.tensor(est, dtype=torch.float64)).abs().max()) < 1e-12


# ---- the committed model case: non-degenerate, and every mutation shows ---------------------------------------------------------------
CASE_DIMS = R.Dims(n_layers=1, n_blocks=2, d_ffn=64, segment=10, n_spk=3)
CASE_T = R.samples_for_frames(37)         # L = 37 frames: gap = 8, S = 10 chunks of K = 10


@functools.lru_cache(maxsize=None)
def _case(L=37):
    sd = R.case_state_dict(CASE_DIMS, 11)
    mix = R.synthetic_mix(R.samples_for_frames(L), L)
    out, masks = R.DualPathRef(CASE_DIMS, sd).separate1(mix, return_masks=True)
    return sd, mix, out, masks


def test_case_is_not_degenerate():
    _, _, out, masks = _case()
    assert torch.isfinite(out).all()
    for a in range(3):
        for b in range(a + 1, 3):
            assert R.rel_l2(out[:, a], out[:, b]) > 0.1, "two sources coincide"
    frac_zero = float((masks == 0).double().mean())
    assert 0.05 < frac_zero < 0.95, frac_zero              # ReLU masks: neither all zero nor all open
    assert float(masks.max()) > 0.05


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_moves_the_output(mut):
    """on at least one of the utterances the GPU model test runs (MUTATION_CASE_FRAMES, the same weights and mixtures) the mistake moves
    the sources by MUTATION_FACTOR x the bound that test holds every utterance to"""
    moved = []
    for L in R.MUTATION_CASE_FRAMES:
        sd, mix, out, _ = _case(L)
        moved.append(R.rel_l2(R.DualPathRef(CASE_DIMS, sd, mut=mut).separate1(mix), out))
    print(mut, ["%.3e" % m for m in moved])
    assert max(moved) >= R.MUTATION_FACTOR * R.BOUND_MODEL, (mut, moved)


def test_mirroring_stays_far_below_the_mutations():
    sd, mix, out, _ = _case()
    assert R.rel_l2(R.DualPathRef(CASE_DIMS, sd, mirror=True).separate1(mix), out) < 0.1


# ---- ctypes mirrors against the header ----------------------------------------------------------------------------------------------
def _c_struct_fields(name):
    text = (ROOT / "include" / "ccx.h").read_text()
    end = text.index("} " + name + ";")
    start = text.rindex("typedef struct", 0, end)
    body = re.sub(r"/\*.*?\*/", "", text[text.index("{", start) + 1:end], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"((?:const )?\w+ ?\*?) ?(\w+(?:, ?\w+)*)", decl)
        assert m, decl
        ctype = m.group(1).replace(" *", "*").strip()
        fields += [(nm.strip(), ctype) for nm in m.group(2).split(",")]
    return fields


@pytest.mark.parametrize("cname,mirror", [("ccx_dualpath_dims", _lib.DualPathDims), ("ccx_dualpath_desc", _lib.DualPathDesc)])
def test_ctypes_mirrors_match_the_header(cname, mirror):
    want = _c_struct_fields(cname)
    got = list(mirror._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "const void*": C.c_void_p, "void*": C.c_void_p, "const int*": C.POINTER(C.c_int)}
    for (n, t), (_, ct) in zip(got, want):
        assert t is kinds[ct] or t == kinds[ct], (n, ct, t)


def test_prototypes_name_the_new_entry_points():
    for fn in ("create", "destroy", "set_tensor", "finalize", "separate", "op"):
        assert f"ccx_dualpath_{fn}" in _lib.PROTOTYPES
    text = (ROOT / "include" / "ccx.h").read_text()
    for i, nm in enumerate(("ATTENTION", "GROUP_NORM", "SEGMENT", "OVERLAP_ADD", "PE_ADD", "GATE", "ENCODER", "DECODER", "PRELU")):
        assert re.search(rf"#define CCX_DP_{nm} {i}\b", text) and getattr(_lib, "DP_" + nm) == i
