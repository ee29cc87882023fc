"""GPU: the opt-in FP8 encoder-output stream in the model (WhisperModel(cross_fp8=True); include/ccx.h ccx_whisper_set_cross_fp8), at
the mini dims of the other decode tests.

An FP8 instance keeps xhat, the dequantised encoder output, as its bf16 encoder output and the FP8 image beside it; the image decodes
to xhat exactly.  So the instance can be compared WITH ITSELF bit for bit: CCX_XS_FP8=0 makes the X-stream read the bf16 xhat instead
of the image, and every decode must return the same tokens, sum_logprob and no_speech_prob either way -- greedy, sampled, over a row
map, as a beam search, with step graphs and without, in lanes.  Closeness to the oracle and agreement across the cross-attention
paths are asserted with the helpers and bounds of tests/test_whisper_gpu.py, the oracle fed with the xhat the instance returned."""
import ctypes as C
import os
import subprocess
import sys
from dataclasses import asdict
from pathlib import Path

import numpy as np
import pytest
import torch

from clearconverse_amd import _lib
from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.tokenizer import DecodeRules
from clearconverse_amd.weights import SepDims, WhisperDims, synthetic_whisper_state_dict
from tests import xa_fp8_reference as R
from tests.test_whisper_gpu import _batch_mates, _check_greedy, _clips

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LANE_ROWS = 320          # the smallest decode an X-stream instance cuts into more than one lane (csrc/whisper.hip lane_policy)
RULES = DecodeRules()
PROMPTS = [[RULES.sot], [RULES.sot_prev, 1000, 2000, RULES.sot], [RULES.sot], [RULES.sot_prev, 77, RULES.sot]]
LENGTHS = [6.0, 11.0, 3.0, 8.0]


def _dims_sd():
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    return dims, synthetic_whisper_state_dict(dims, seed=3)


@pytest.fixture(scope="module")
def fp8(ccx_ctx):
    """one FP8 instance for the file, with the four test windows encoded"""
    from clearconverse_amd.whisper import WhisperModel
    dims, sd = _dims_sd()
    m = WhisperModel(dims, sd, max_batch=LANE_ROWS, ctx=ccx_ctx, cross_fp8=True)
    assert m.cross_fp8 is True
    yield m
    m.close()


def _encode4(m, reps=1):
    _, n, dev = _clips(LENGTHS)
    big = dev.repeat(reps, 1).contiguous()
    m.log_mel(big, n * reps)
    return m.encode(4 * reps, return_xa=True).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _key(results):
    """what must be bit-identical: tokens, sum_logprob, no_speech_prob (hypothesis lists of a beam decode flattened)"""
    flat = [h for r in results for h in (r if isinstance(r, list) else [r])]
    return [(tuple(h["tokens"]), np.float32(h["sum_logprob"]).tobytes(), np.float32(h["no_speech_prob"]).tobytes()) for h in flat]


def _ab(m, monkeypatch, call):
    """call() with the FP8 stream and with CCX_XS_FP8=0 (the instance's bf16 xhat through the bf16 stream) -> the FP8 results"""
    monkeypatch.delenv("CCX_XS_FP8", raising=False)
    a = call()
    assert m.last_cross_path == "xa_stream"
    monkeypatch.setenv("CCX_XS_FP8", "0")
    b = call()
    assert m.last_cross_path == "xa_stream"
    monkeypatch.delenv("CCX_XS_FP8")
    assert _key(a) == _key(b)
    assert any(len(k[0]) > 0 for k in _key(a))
    return a


def test_encode_returns_the_reference_quantiser_of_the_default_output(ccx_ctx, fp8):
    from clearconverse_amd.whisper import WhisperModel
    dims, sd = _dims_sd()
    d = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx)
    try:
        assert d.cross_fp8 is False
        xa = _encode4(d)
        again = _encode4(d)
        assert torch.equal(_bits(xa), _bits(again))
        xa_bf16 = xa.to(torch.bfloat16).to(torch.float32)               # what a default instance keeps and streams
        want = R.xhat_of(xa_bf16)
        assert not torch.equal(want, xa_bf16), "the default instance's output is already quantised?"
        got = _encode4(fp8)
        assert torch.equal(_bits(got), _bits(want))
        # ... and the quantisation is the small perturbation the format promises: 3 mantissa bits, relative step 2^-3 at worst
        rel = float((got - xa_bf16).norm() / xa_bf16.norm())
        assert rel < 2.0 ** -4, rel
    finally:
        d.close()


@pytest.mark.parametrize("graphs", [True, False])
def test_fp8_stream_equals_the_instances_own_bf16_stream(fp8, monkeypatch, graphs):
    m = fp8
    _encode4(m)
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
    if not graphs:
        monkeypatch.setenv("CCX_NO_GRAPH", "1")
    before = m.graph_count()
    _ab(m, monkeypatch, lambda: m.decode_greedy(PROMPTS, sample_len=12))
    if graphs:
        assert m.graph_count() >= before + 2          # the two plans side by side: the switch is in the step graphs' key
        mid = m.graph_count()
        _ab(m, monkeypatch, lambda: m.decode_greedy(PROMPTS, sample_len=12))
        assert m.graph_count() == mid                 # ... and both are found again
    else:
        assert m.graph_count() == before
    _ab(m, monkeypatch, lambda: m.decode(PROMPTS, sample_len=12, temperature=0.7, seed=5))
    windows = [2, 0, 3, 0, 2, 1, 3, 0, 2]                                  # repeating, not monotone
    prompts = [PROMPTS[w] for w in windows]
    _ab(m, monkeypatch, lambda: m.decode_rows(prompts, windows, sample_len=10, temperature=0.5, seed=9, n_windows=4))
    _ab(m, monkeypatch, lambda: m.decode_beam([PROMPTS[1], PROMPTS[0], PROMPTS[3]], 3, sample_len=8, windows=[3, 1, 3], n_windows=4))


def test_the_fp8_kernels_are_what_runs(ccx_ctx, fp8, monkeypatch):
    """the launch records: an encode of the FP8 instance ends in the quantise kernel, its X-stream launches are the FP8 instantiation,
    and under CCX_XS_FP8=0 the bf16 one.  (Eager steps: the records are not taken inside a graph capture.)"""
    m = fp8
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
    monkeypatch.setenv("CCX_NO_GRAPH", "1")
    ccx_ctx.prof_enable(True)
    try:
        def names(call):
            n0 = ccx_ctx.lib.ccx_prof_count(ccx_ctx.handle)
            call()
            return [r[0] for r in ccx_ctx.prof_records()[n0:]]
        enc = names(lambda: _encode4(m))
        assert enc.count("xa_fp8_quantise_kernel") == 1, enc[-3:]
        on = [n for n in names(lambda: m.decode_greedy(PROMPTS, sample_len=4)) if n.startswith("dec_xs_stream_kernel")]
        monkeypatch.setenv("CCX_XS_FP8", "0")
        off = [n for n in names(lambda: m.decode_greedy(PROMPTS, sample_len=4)) if n.startswith("dec_xs_stream_kernel")]
        assert on and all("fp8" in n for n in on), set(on)
        assert len(off) == len(on) and not any("fp8" in n for n in off), set(off)
    finally:
        ccx_ctx.prof_enable(False)


def test_fp8_stream_in_lanes(fp8, monkeypatch):
    m = fp8
    reps = LANE_ROWS // 4
    xa = _encode4(m, reps)
    assert torch.equal(_bits(xa[:4]), _bits(xa[4:8]))
    m.prepare_lanes()
    res = _ab(m, monkeypatch, lambda: m.decode_greedy(PROMPTS * reps, sample_len=8))
    for i in range(4, LANE_ROWS):
        assert _key([res[i]]) == _key([res[i % 4]]), i           # a sequence's numbers do not depend on its lane or batch mates


def test_oracle_walk_on_the_returned_xhat(fp8, monkeypatch):
    """the teacher-forced walk of tests/test_whisper_gpu.py::test_greedy_mini (its helper, its tolerances), the oracle fed with xhat"""
    m = fp8
    dims, sd = _dims_sd()
    xa = _encode4(m)
    monkeypatch.setenv("CCX_CROSS_X_MIN_ROWS", "1")
    res, n_req = _check_greedy(dims, sd, m, xa, PROMPTS[:3], sample_len=20, tol=0.05)
    assert m.last_cross_path == "xa_stream" and n_req > 0


def test_paths_agree_on_an_fp8_instance(fp8, monkeypatch):
    """kv16 (4 sequences, default minimum rows), kv_stream (20) and the X-stream (4 and 20): the helper and bounds of
    tests/test_whisper_gpu.py::test_large_batch_decode_path_matches_small_batch -- the K / V paths project xhat"""
    m = fp8
    dims, sd = _dims_sd()
    _, n, dev = _clips(LENGTHS)
    _batch_mates(m, dims, sd, dev, n, PROMPTS, 5, 16, monkeypatch)


def test_refusals(ccx_ctx, fp8):
    from clearconverse_amd.whisper import WhisperModel
    wide = WhisperDims.mini(n_layer=1, n_state=1280)                      # WhisperDims.large's width: no X-stream path
    with pytest.raises(_lib.CcxError) as e:
        WhisperModel(wide, {}, max_batch=1, ctx=ccx_ctx, cross_fp8=True)
    assert "1280" in str(e.value)
    # the library's own refusal (the constructor's check comes first): the setter on a 1280-wide handle, and after finalize
    lib, h = ccx_ctx.lib, C.c_void_p()
    cd = _lib.WhisperDims(**asdict(wide))
    ccx_ctx.check(lib.ccx_whisper_create(ccx_ctx.handle, C.byref(cd), 1, C.byref(h)), "ccx_whisper_create")
    try:
        assert lib.ccx_whisper_cross_fp8(h) == 0
        with pytest.raises(_lib.CcxError) as e:
            ccx_ctx.check(lib.ccx_whisper_set_cross_fp8(h, 1), "ccx_whisper_set_cross_fp8")
        assert "1280" in str(e.value)
        assert lib.ccx_whisper_cross_fp8(h) == 0
        ccx_ctx.check(lib.ccx_whisper_set_cross_fp8(h, 0), "ccx_whisper_set_cross_fp8")       # off is always allowed
    finally:
        lib.ccx_whisper_destroy(h)
    with pytest.raises(_lib.CcxError) as e:
        ccx_ctx.check(lib.ccx_whisper_set_cross_fp8(fp8.handle, 0), "ccx_whisper_set_cross_fp8")
    assert "after finalize" in str(e.value)
    assert fp8.cross_fp8 is True and lib.ccx_whisper_cross_fp8(fp8.handle) == 1


def _child():
    """CCX_CROSS_X=0 is read when an instance is built: a fresh process (as tests/test_xs_full_lines_gpu.py starts one)"""
    from clearconverse_amd.whisper import WhisperModel
    dims, sd = _dims_sd()
    assert os.environ.get("CCX_CROSS_X") == "0"
    try:
        WhisperModel(dims, sd, max_batch=2, cross_fp8=True)
        print("constructor: accepted")
    except _lib.CcxError as e:
        print("constructor: refused:", e)
    ctx = _lib.Context(0)
    h = C.c_void_p()
    cd = _lib.WhisperDims(**asdict(dims))
    ctx.check(ctx.lib.ccx_whisper_create(ctx.handle, C.byref(cd), 2, C.byref(h)), "ccx_whisper_create")
    try:
        ctx.check(ctx.lib.ccx_whisper_set_cross_fp8(h, 1), "ccx_whisper_set_cross_fp8")
        print("library: accepted")
    except _lib.CcxError as e:
        print("library: refused:", e)
    ctx.lib.ccx_whisper_destroy(h)
    # CCX_CROSS_FP8=1 with the path off: ignored, a default instance
    os.environ["CCX_CROSS_FP8"] = "1"
    m = WhisperModel(dims, sd, max_batch=2)
    print("env on a K/V instance: cross_fp8 =", m.cross_fp8)
    m.close()


def test_refused_under_cross_x_0(ccx_ctx):
    env = dict(os.environ, CCX_CROSS_X="0", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("CCX_CROSS_FP8", None)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "child"], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = {ln.split(":")[0]: ln for ln in r.stdout.splitlines() if ":" in ln}
    assert "refused" in lines["constructor"] and "CCX_CROSS_X=0" in lines["constructor"], r.stdout
    assert "refused" in lines["library"] and "CCX_CROSS_X=0" in lines["library"], r.stdout
    assert lines["env on a K/V instance"].endswith("False"), r.stdout


def test_environment_switch_at_finalize(ccx_ctx, monkeypatch):
    """CCX_CROSS_FP8=1 (the benchmark's A/B) turns the stream on where the setter was not called"""
    from clearconverse_amd.whisper import WhisperModel
    dims, sd = _dims_sd()
    monkeypatch.setenv("CCX_CROSS_FP8", "1")
    m = WhisperModel(dims, sd, max_batch=4, ctx=ccx_ctx)
    monkeypatch.delenv("CCX_CROSS_FP8")
    try:
        assert m.cross_fp8 is True
        xa = _encode4(m)
        assert torch.equal(_bits(xa), _bits(R.xhat_of(xa)))           # what it returns is quantised: a fixed point of the quantiser
    finally:
        m.close()


def test_public_surface(ccx_ctx):
    from clearconverse_amd.models import build_state_dicts, load_models
    sds = build_state_dicts(None, whisper_dims=WhisperDims.mini(2, 128), sep_dims=SepDims(n_layers=2), seed=0)
    models = load_models(None, 0, whisper_batch=2, ctx=ccx_ctx, state_dicts=sds, sep_tokens=60_000, max_crops=16, gate_max_clips=2,
                         whisper_cross_fp8=True)
    try:
        w = models["whisper_model"]
        assert w.cross_fp8 is True and all(x.cross_fp8 is True for x in models["whisper_models"])
        out = w.transcribe_batch([synthetic_clip(1, 30.0)[:16000 * 4], synthetic_clip(2, 30.0)[:16000 * 2]])
        assert len(out) == 2
        for o in out:
            assert isinstance(o["text"], str) and isinstance(o["segments"], list) and "tokens" in o
    finally:
        for k in ("whisper_model", "separator", "embedding_model", "diarization_embedder", "segmentation_vad", "segmentation_diar", "denoiser"):
            models[k].close()


if __name__ == "__main__":
    _child()
