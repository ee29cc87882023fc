"""GPU: a whole decode under CCX_DEC_PACKED_MID against the form it replaces (csrc/decoder.h): the switch changes how rows travel between
the chain's kernels, never a bit of a result.  A mini-dims greedy decode of 24 tokens on the X-stream path (one lane), each
configuration in a fresh child process (the library reads the switch per decode; a child makes sure nothing of the other form is left
in a graph cache): 96 rows (16 columns per block in the out projections) and 144 rows (32 columns per block, the big lanes'
instantiations).  Tokens, sum_logprob and no_speech_prob must be byte-equal,
and inside every child the graph replay must equal the eager first step, as tests/test_whisper_gpu.py::test_greedy_graph_equals_eager
checks for a small decode."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ROWS = (96, 144)
NEW = dict(CCX_DEC_PACKED_MID="1")
OLD = dict(CCX_DEC_PACKED_MID="0")


def _child(out_path):
    from clearconverse_amd.audio import synthetic_clip
    from clearconverse_amd.tokenizer import DecodeRules
    from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
    from clearconverse_amd.whisper import WhisperModel
    dims = WhisperDims.mini(n_layer=2, n_state=128)
    m = WhisperModel(dims, synthetic_whisper_state_dict(dims, seed=3), max_batch=max(ROWS))
    rules = DecodeRules()
    clips = np.stack([synthetic_clip(i, 30.0)[: 16000 * 6] for i in range(8)])
    res = {}
    for rows in ROWS:
        dev = torch.from_numpy(clips).cuda().repeat(rows // 8, 1).contiguous()
        m.log_mel(dev, [clips.shape[1]] * rows)
        m.encode(rows)
        prompts = [[rules.sot] if b % 2 == 0 else [rules.sot_prev, 5000 + b, rules.sot] for b in range(rows)]
        for mode in ("graph", "eager"):
            if mode == "eager":
                os.environ["CCX_NO_GRAPH"] = "1"
            try:
                r = m.decode_greedy(prompts, sample_len=24)
            finally:
                os.environ.pop("CCX_NO_GRAPH", None)
            assert m.last_cross_path == "xa_stream", m.last_cross_path
            n = max(len(x["tokens"]) for x in r)
            res[f"{rows}_{mode}_tokens"] = np.array([x["tokens"] + [-1] * (n - len(x["tokens"])) for x in r], dtype=np.int32)
            res[f"{rows}_{mode}_sum_logprob"] = np.array([x["sum_logprob"] for x in r], dtype=np.float32)
            res[f"{rows}_{mode}_no_speech_prob"] = np.array([x["no_speech_prob"] for x in r], dtype=np.float32)
    m.close()
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def forms(ccx_ctx, tmp_path_factory):
    """{"new" / "old": the child's arrays} (ccx_ctx: skipped without a GPU, like the other GPU tests)"""
    d = tmp_path_factory.mktemp("decode_mid_images")
    got = {}
    for name, sw in (("new", NEW), ("old", OLD)):
        env = dict(os.environ, CCX_CROSS_X_MIN_ROWS="1", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), **sw)
        path = d / f"{name}.npz"
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{sw}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        got[name] = dict(np.load(path))
    return got


@pytest.mark.parametrize("rows", ROWS)
def test_switch_changes_no_bit(forms, rows):
    for what in ("tokens", "sum_logprob", "no_speech_prob"):
        new, old = forms["new"][f"{rows}_graph_{what}"], forms["old"][f"{rows}_graph_{what}"]
        assert new.shape == old.shape and new.tobytes() == old.tobytes(), (rows, what)
    assert (forms["new"][f"{rows}_graph_tokens"] >= 0).sum() > rows          # the decode sampled something


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("form", ["new", "old"])
def test_graph_replay_equals_eager(forms, form, rows):
    for what in ("tokens", "sum_logprob"):
        a, b = forms[form][f"{rows}_graph_{what}"], forms[form][f"{rows}_eager_{what}"]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (form, rows, what)


if __name__ == "__main__":
    _child(sys.argv[1])
