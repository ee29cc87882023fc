"""-m gpu: the Whisper decoder and encoder under stressed residual-stream statistics (tests/stressed_whisper.py), against the float64
oracle (oracle/whisper_ref.py, dtype=torch.float64).

Offset stress adds a constant to every residual row without changing the model (every LayerNorm removes it), so the stressed model
has the SAME oracle as the plain one and every path must meet the bounds it meets on the plain weights.  Offset levels: 0 (the
control), |mean| / std >= 10 and >= 40 at every cross_attn_ln input.  The rows of the X-stream path's LayerNorm-free cross-attention
query (DEPI_RESOLVE in csrc/decoder.hip, dec_xq_lnfree_kernel in csrc/cross_x.hip) are rounded to bf16 before the query applies its
LayerNorm algebraically: rounded uncentred, their error grows with |mean| / std, so the default chain is also held to 1.25 x the error
of round 3's chain (CCX_DEC_LNFREE=0: resolve + two-pass LayerNorm, then the query) on the same weights and positions.

Paths: the split-KV kernels of <= 16 sequences ("kv16", B = 2, the fused query), the K / V stream of 17 - 80 ("kv_stream", B = 24) and
the cross attention against the encoder output ("xa_stream", B = 24 with CCX_CROSS_X_MIN_ROWS=1; every group of bench.py).  Bounds are
those of the plain-weight tests: logits rel-L2 1e-2 per position, walks eps 0.02 (mini) / 0.0275 (full), encoder rel-L2 8e-3 (mini)
/ 9.5e-3 (full), |sum_logprob LayerNorm-free - round 3| 6e-4.
"""
import math

import numpy as np
import pytest
import torch

from tests.conftest import within
from tests.stressed_whisper import MU, OUTLIER_CHANNELS, OUTLIER_SCALE, offset_state_dict, outlier_state_dict
from tests.test_whisper_long_gpu import walk_cached

from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

PATHS = {"kv16": dict(B=2, env=None), "kv_stream": dict(B=24, env=None), "xa_stream": dict(B=24, env="1")}
CHAINS = {"round3": "0", "default": None}
LOGITS_TOL, WALK_EPS_MINI, WALK_EPS_FULL = 1e-2, 0.02, 0.0275


def _rel(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rules():
    r = DecodeRules()
    return r, R.Rules(suppress=tuple(r.suppress))


def _clips(lengths_s, seed0=0):
    clips = [synthetic_clip(seed0 + i, 30.0)[: int(s * 16000)] for i, s in enumerate(lengths_s)]
    n = [len(c) for c in clips]
    host = np.zeros((len(clips), max(n)), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return n, torch.from_numpy(host).cuda()


def _prompts(rules):
    """1 token (stepwise), 4 and 11 tokens (one prefill pass), 22 tokens (two passes: pf_xb / pf_st2 rows of both)"""
    g = np.random.default_rng(21)
    return [[rules.sot], [rules.sot_prev, 1000, 2000, rules.sot],
            [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, 9)] + [rules.sot],
            [rules.sot_prev] + [int(x) for x in g.integers(1000, 40000, 20)] + [rules.sot]]


def _weights(dims, level, seed):
    """the stressed weights as the model loads them (float32) -- the float64 oracle runs on these same values"""
    sd = synthetic_whisper_state_dict(dims, seed=seed)
    return sd, {k: v.float() for k, v in offset_state_dict(sd, dims, MU[level], MU[level]).items()}


def _orc(dims, sd, dtype=torch.float64):
    return R.WhisperRef(R.Dims(**dims.__dict__), sd, dtype=dtype)


def _encode(m, n, dev, B):
    reps = B // dev.shape[0] if B >= dev.shape[0] else 1
    rows = dev.repeat(reps, 1).contiguous()[:B]
    mel = m.log_mel(rows, (n * reps)[:B], return_mel=True)
    return mel, m.encode(B, return_xa=True).cpu()


def _set_env(monkeypatch, path, chain):
    for k, v in (("CCX_CROSS_X_MIN_ROWS", PATHS[path]["env"]), ("CCX_DEC_LNFREE", CHAINS[chain])):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def mini_dims():
    return WhisperDims.mini(n_layer=2, n_state=128)


@pytest.mark.parametrize("level", sorted(MU))
def test_teacher_forced_logits_and_encoder_under_offset(ccx_ctx, monkeypatch, mini_dims, level):
    """6a / 6e: every path x chain, per position against the float64 oracle on the GPU's own xa; the default chain's rel-L2 within
    1.25 x round 3's; the encoder output against the oracle of the PLAIN weights."""
    from clearconverse_amd.whisper import WhisperModel
    dims = mini_dims
    plain, sd = _weights(dims, level, 3)
    m = WhisperModel(dims, sd, max_batch=24, ctx=ccx_ctx)
    try:
        n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        g = torch.Generator().manual_seed(level)
        toks4 = torch.randint(0, 50000, (4, 9), generator=g)
        toks4[:, 0] = 50257
        orc = _orc(dims, sd)
        for path, cfg in PATHS.items():
            B = cfg["B"]
            mel, xa = _encode(m, n, dev, B)
            if path == "kv16":
                ref_xa = _orc(dims, plain, torch.float32).encode(mel[:2].cpu())
                within(f"whisper mini offset {level}: encoder output rel-L2 against the plain weights' oracle", _rel(xa, ref_xa), 8e-3)
            k = min(B, 4)
            ref = orc.decoder_logits(toks4[:k], xa[:k])
            toks = toks4.repeat(B // k, 1)[:B]
            err = {}
            for chain in CHAINS:
                _set_env(monkeypatch, path, chain)
                got = m.decoder_logits(toks.numpy()).cpu()[:k]
                assert torch.isfinite(got).all()
                for b in range(k):
                    for t in range(toks.shape[1]):
                        within(f"whisper mini offset {level}: teacher-forced logits rel-L2 per position [{chain} chain]",
                               _rel(got[b, t], ref[b, t]), LOGITS_TOL, (path, b, t))
                err[chain] = _rel(got, ref)
            within(f"whisper mini offset {level}: logits rel-L2 default chain / round-3 chain [{path}]", err["default"] / err["round3"], 1.25)
    finally:
        m.close()


def test_decoder_logits_follow_the_chain_switches(ccx_ctx, monkeypatch, mini_dims):
    """ccx_whisper_decoder_logits reads CCX_DEC_LNFREE / CCX_FUSE_CROSS_Q itself: on a fresh X-stream instance its logits before
    and after a default decode are bit-identical, and CCX_DEC_LNFREE=0 gives round 3's chain (other bits, the same bound)."""
    from clearconverse_amd.whisper import WhisperModel
    dims = mini_dims
    _, sd = _weights(dims, 40, 3)
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
        _, xa = _encode(m, n, dev, 4)
        toks = torch.randint(0, 50000, (4, 9), generator=torch.Generator().manual_seed(7))
        toks[:, 0] = rules.sot
        first = m.decoder_logits(toks.numpy()).cpu()
        m.decode_greedy(_prompts(rules), sample_len=8)
        assert m.last_cross_path == "xa_stream"
        assert torch.equal(m.decoder_logits(toks.numpy()).cpu(), first)
        monkeypatch.setenv("CCX_DEC_LNFREE", "0")
        r3 = m.decoder_logits(toks.numpy()).cpu()
        m.decode_greedy(_prompts(rules), sample_len=8)
        monkeypatch.delenv("CCX_DEC_LNFREE")
        assert not torch.equal(r3, first)
        assert torch.equal(m.decoder_logits(toks.numpy()).cpu(), first)       # a round-3 decode in between changes nothing
        ref = _orc(dims, sd).decoder_logits(toks, xa)
        for got in (first, r3):
            for b in range(4):
                for t in range(9):
                    within("whisper mini offset 40: decoder_logits rel-L2 per position, fresh X-stream instance", _rel(got[b, t], ref[b, t]), LOGITS_TOL)
    finally:
        m.close()


@pytest.mark.parametrize("level", sorted(MU))
def test_greedy_walks_under_offset(ccx_ctx, monkeypatch, mini_dims, level):
    """6b: greedy decodes of 40 tokens from prompts of 1, 4, 11 and 22 tokens on every path x chain, each walked through the
    float64 cached decoder; LayerNorm-free vs round 3 where the tokens agree; 4 sequences alone = the same 4 among 40 in two lanes."""
    from clearconverse_amd.whisper import WhisperModel
    dims = mini_dims
    _, sd = _weights(dims, level, 3)
    m = WhisperModel(dims, sd, max_batch=40, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        prompts = _prompts(rules)
        n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        orc = _orc(dims, sd)
        S = 40
        for path, cfg in PATHS.items():
            B = cfg["B"]
            _, xa = _encode(m, n, dev, B)
            k = min(B, 4)
            res = {}
            for chain in CHAINS:
                _set_env(monkeypatch, path, chain)
                r = m.decode_greedy((prompts * (B // k + 1))[:B] if k == 4 else prompts[:B], sample_len=S)
                assert m.last_cross_path == path, (path, m.last_cross_path)
                for i in range(k, B):
                    assert r[i]["tokens"] == r[i % k]["tokens"] and r[i]["sum_logprob"] == r[i % k]["sum_logprob"], (path, chain, i)
                res[chain] = r
                same = chain == "default" and all(r[i] == res["round3"][i] for i in range(k))
                if same:
                    continue                                    # the chains coincide off the X-stream path: walked once
                for i in range(k):
                    walk_cached(orc, xa[i:i + 1], prompts[i], r[i], S, WALK_EPS_MINI, f"whisper mini offset {level} walk [{chain} chain]")
            if path == "xa_stream":
                for i in range(k):
                    a, b = res["default"][i], res["round3"][i]
                    if a["tokens"] == b["tokens"]:
                        within(f"whisper mini offset {level}: |sum_logprob LayerNorm-free chain - round-3 chain| / max(1, |.|)",
                               abs(a["sum_logprob"] - b["sum_logprob"]) / max(1.0, abs(b["sum_logprob"])), 6e-4, i)
        # 4 alone = the same 4 among 40 in two lanes (default chain, X-stream path)
        _set_env(monkeypatch, "xa_stream", "default")
        _encode(m, n, dev, 4)
        alone = m.decode_greedy(prompts, sample_len=S)
        _encode(m, n, dev, 40)
        monkeypatch.setenv("CCX_DEC_LANES", "2")
        many = m.decode_greedy(prompts * 10, sample_len=S)
        for i in range(40):
            assert many[i]["tokens"] == alone[i % 4]["tokens"] and many[i]["sum_logprob"] == alone[i % 4]["sum_logprob"], i
    finally:
        m.close()


def test_full_size_under_the_strongest_offset(ccx_ctx, monkeypatch):
    """6c / 6e at full small.en size (the <768> kernels bench.py runs), |mean| / std >= 40: the encoder against the plain weights'
    oracle, 24 sequences on the X-stream path (default chain) and 2 on kv16 (the fused query), 8 of them walked in float64."""
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.small_en()
    plain, sd = _weights(dims, 40, 0)
    m = WhisperModel(dims, sd, max_batch=24, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        n, dev = _clips([30.0, 9.0, 4.0, 17.5, 2.0, 24.0])
        mel, xa = _encode(m, n, dev, 24)
        ref_xa = _orc(dims, plain, torch.float32).encode(mel[:1].cpu())
        within("whisper small.en FULL size offset 40: encoder output rel-L2 against the plain weights' oracle", _rel(xa[:1], ref_xa), 9.5e-3)
        shapes = _prompts(rules)
        prompts = [shapes[i // 6] for i in range(24)]
        S = 40
        orc = _orc(dims, sd)
        _set_env(monkeypatch, "xa_stream", "default")
        xs = m.decode_greedy(prompts, sample_len=S)
        assert m.last_cross_path == "xa_stream"
        for i in range(0, 24, 4):
            walk_cached(orc, xa[i:i + 1], prompts[i], xs[i], S, WALK_EPS_FULL, "whisper small.en FULL size offset 40 walk [xa_stream, default chain]")
        _set_env(monkeypatch, "kv16", "default")
        kv = m.decode_greedy([shapes[0], shapes[3]], sample_len=S)
        assert m.last_cross_path == "kv16"
        for i, p in enumerate([shapes[0], shapes[3]]):
            walk_cached(orc, xa[i:i + 1], p, kv[i], S, WALK_EPS_FULL, "whisper small.en FULL size offset 40 walk [kv16]")
    finally:
        m.close()


def test_outlier_channels(ccx_ctx, monkeypatch, mini_dims):
    """6d: three residual channels at 50 - 150 x the rms of the others (a different model): encoder output, teacher-forced logits and
    greedy walks against the float64 oracle of the same weights, kv16 and xa_stream (default chain)."""
    from clearconverse_amd.whisper import WhisperModel
    dims = mini_dims
    sd = {k: v.float() for k, v in outlier_state_dict(synthetic_whisper_state_dict(dims, seed=3), dims, OUTLIER_CHANNELS,
                                                      OUTLIER_SCALE["mini"]).items()}
    m = WhisperModel(dims, sd, max_batch=24, ctx=ccx_ctx)
    try:
        rules, _ = _rules()
        prompts = _prompts(rules)
        n, dev = _clips([6.0, 11.0, 3.0, 8.0])
        orc = _orc(dims, sd)
        toks = torch.randint(0, 50000, (4, 9), generator=torch.Generator().manual_seed(5))
        toks[:, 0] = rules.sot
        for path in ("kv16", "xa_stream"):
            B = PATHS[path]["B"]
            mel, xa = _encode(m, n, dev, B)
            k = min(B, 4)
            if path == "kv16":
                within("whisper mini outlier channels: encoder output rel-L2", _rel(xa, orc.encode(mel.cpu())), 8e-3)
            _set_env(monkeypatch, path, "default")
            got = m.decoder_logits(toks.repeat(B // k, 1)[:B].numpy()).cpu()
            ref = orc.decoder_logits(toks[:k], xa[:k])
            for b in range(k):
                for t in range(9):
                    within("whisper mini outlier channels: teacher-forced logits rel-L2 per position", _rel(got[b, t], ref[b, t]), LOGITS_TOL, (path, b, t))
            res = m.decode_greedy((prompts * 6)[:B] if k == 4 else prompts[:B], sample_len=40)
            assert m.last_cross_path == path
            for i in range(k):
                walk_cached(orc, xa[i:i + 1], prompts[i], res[i], 40, WALK_EPS_MINI, "whisper mini outlier channels walk")
    finally:
        m.close()


def _ulp(x):
    x = abs(float(x))
    return 2.0 ** (math.frexp(x)[1] - 24) if x > 0 else 2.0 ** -149


@pytest.mark.parametrize("D", [128, 768, 1024])
def test_layernorm_kernel_under_offset_outliers_and_eps(ccx_ctx, D):
    """ccx_layernorm (layernorm_kernel: the encoder's and SepFormer's LayerNorm) against float64 F.layer_norm of the SAME float32
    inputs.  Two-pass mean / variance in float32: the mean carries a rounding error of a few ulp(|mean|), which every output of the row
    inherits times gamma / sqrt(var + eps); the output itself rounds to ulp(|y|).  Bound per row: 4 units of
    ulp(|mean|) max|gamma| / sqrt(var + eps) + ulp(max|y|) (1.77 measured).  Rows: mean / std 10, 100, 1000; three channels at 300 x rms; near-constant
    rows (var << eps: eps dominates); plain rows; a ragged M."""
    g = torch.Generator().manual_seed(D)
    rows = []
    for ratio in (10.0, 100.0, 1000.0):
        rows.append(torch.randn(7, D, generator=g) * 0.5 + ratio * 0.5 * torch.sign(torch.randn(7, 1, generator=g)))
    o = torch.randn(7, D, generator=g)
    for r in range(7):
        ch = torch.randperm(D, generator=g)[:3]
        o[r, ch] = 300.0 * torch.tensor([1.0, -1.0, 1.0])
    rows.append(o)
    rows.append(1.5 + 1e-4 * torch.randn(7, D, generator=g))            # var ~1e-8 << eps = 1e-5
    rows.append(-3.0 + 1e-6 * torch.randn(5, D, generator=g))
    rows.append(torch.randn(6, D, generator=g) * 3 + 0.5)
    x = torch.cat(rows).contiguous()
    M = x.shape[0]
    assert M % 4 != 0                                                   # a ragged last block of rows
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    of = torch.empty(M, D, dtype=torch.float32, device="cuda")
    ob = torch.empty(M, D, dtype=torch.bfloat16, device="cuda")
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    ccx_ctx.check(ccx_ctx.lib.ccx_layernorm(ccx_ctx.handle, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), ob.data_ptr(), of.data_ptr(),
                                            M, D, 1e-5, int(torch.cuda.current_stream().cuda_stream)), "layernorm")
    torch.cuda.synchronize()
    got = of.cpu().double()
    gmax = float(gamma.abs().max())
    xd64 = x.double()
    for r in range(M):
        mean, var = float(xd64[r].mean()), float(xd64[r].var(unbiased=False))
        unit = _ulp(mean) * gmax / math.sqrt(var + 1e-5) + _ulp(float(ref[r].abs().max()))
        err = float((got[r] - ref[r]).abs().max())
        within("layernorm_kernel: max abs error / (ulp(|mean|) max|gamma| / sqrt(var + eps) + ulp(max|y|)), stressed rows", err / unit, 4.0, (D, r))
    assert float((ob.cpu().double() - ref).abs().max() / ref.abs().max()) < 2 ** -8       # the bf16 copy: one rounding
