"""The two load forms of dec_xs_stream_kernel (csrc/cross_x.hip) compute the same numbers BIT FOR BIT: half-line loads
(CCX_XS_FULL_LINES=0: 16 keys x 64 B per instruction, the score operand's own image) and full-line loads (=1, the default: 8 keys x
128 B per instruction, the score operand read back from the wave's staging strip).  Every case runs through the stand-alone operator
ccx_cross_attention_xa in one fresh child process per switch value (this file run as a script), and the outputs are compared with
torch.equal.  The cases are the smallest shapes that reach every edge of the tile loop: ragged last tiles, halves of one and two tiles,
an empty second half, prefetch longer than the range, the three widths that have the full-line form (D = 256, 512, 768) and the two
that keep the half-line kernel (128, 384), a repeated / non-monotone row map, the prefill form (four rows per block, ragged group)
and the repeat pass.  The full-line outputs are also held against the fp32 restatement of tests/test_cross_x_gpu.py at that file's
tolerances (1e-2 rel-L2 per row; 6e-3 for the mapped and the peaked cases), should both forms be wrong the same way."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.conftest import within

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _reference(q, wk, wv, bv, xa, row_seq, H):
    """fp32 result of an fp64 evaluation with explicit K/V (the reference's formulation); weights and xa as the kernel sees them"""
    D = 64 * H
    out = torch.empty(q.shape[0], D)
    for r in range(q.shape[0]):
        x = xa[row_seq[r]].double()
        k = x @ wk.double().T
        v = x @ wv.double().T + bv.double()
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            s = (k[:, sl] @ q[r, sl].double()) * 0.125
            p = torch.softmax(s, dim=0)
            out[r, sl] = (p @ v[:, sl]).float()
    return out


def _case(seed, H, S, rows, n_seq, q_gain=1.0, row_seq=None):
    g = torch.Generator().manual_seed(seed)
    D = 64 * H
    q = torch.randn(rows, D, generator=g) * q_gain
    wk = _bf16_round(torch.randn(D, D, generator=g) / D ** 0.5)
    wv = _bf16_round(torch.randn(D, D, generator=g) / D ** 0.5)
    bv = torch.randn(D, generator=g) * 0.1
    xa = _bf16_round(torch.randn(n_seq, S, D, generator=g))
    rs = list(range(rows)) if row_seq is None else row_seq
    return q, wk, wv, bv, xa, rs


def _peaked(boost):
    """the construction of test_cross_x_gpu.test_peaked_scores_and_the_repeat_pass"""
    q, wk, wv, bv, xa, rs = _case(7, 12, 1500, 3, 3)
    for seq, key, h in ((1, 1001, 5), (2, 777, 0)):
        qe = (q[seq, 64 * h:64 * h + 64] @ wk[64 * h:64 * h + 64, :])
        xa[seq, key] = _bf16_round(qe / qe.norm() * boost * 4.0)
    return q, wk, wv, bv, xa, rs


# name -> (builder of (q, wk, wv, bv, xa, row_seq), heads, pass the row map, rows_per_seq, tolerance against the reference)
CASES = {
    "H12_S1500_r3": (lambda: _case(1612, 12, 1500, 3, 3, q_gain=2.0), 12, False, 0, 1e-2),     # 94 tiles, last tile 12 live keys, halves of 47
    "H12_S1499_r1": (lambda: _case(1611, 12, 1499, 1, 1, q_gain=2.0), 12, False, 0, 1e-2),
    "H12_S40_r2": (lambda: _case(152, 12, 40, 2, 2, q_gain=2.0), 12, False, 0, 1e-2),          # 3 tiles: halves of 1 and 2, PF longer than the range
    "H12_S16_r2": (lambda: _case(128, 12, 16, 2, 2, q_gain=2.0), 12, False, 0, 1e-2),          # one tile: the second half is empty
    "H8_S100_r2": (lambda: _case(208, 8, 100, 2, 2, q_gain=2.0), 8, False, 0, 1e-2),           # D = 512
    "H4_S37_r3": (lambda: _case(141, 4, 37, 3, 3, q_gain=2.0), 4, False, 0, 1e-2),             # D = 256
    "row_map": (lambda: _case(11, 12, 1500, 7, 3, row_seq=[2, 0, 0, 1, 2, 2, 0]), 12, True, 0, 6e-3),
    "prefill_P5": (lambda: _case(305, 12, 200, 10, 2, q_gain=1.5, row_seq=[0] * 5 + [1] * 5), 12, True, 5, 1e-2),   # a group of 4 and one of 1
    "prefill_P1": (lambda: _case(301, 12, 200, 2, 2, q_gain=1.5, row_seq=[0, 1]), 12, True, 1, 1e-2),
    "prefill_P5_D512": (lambda: _case(306, 8, 100, 10, 2, q_gain=1.5, row_seq=[1] * 5 + [0] * 5), 8, True, 5, 1e-2),
    "peaked_2pow60": (lambda: _peaked(6.0), 12, False, 0, 6e-3),
    "peaked_repeat_pass": (lambda: _peaked(40.0), 12, False, 0, 6e-3),
    # widths without the full-line form: today's kernel under either switch value
    "fallback_H2_S1500_r3": (lambda: _case(1502, 2, 1500, 3, 3, q_gain=2.0), 2, False, 0, 1e-2),
    "fallback_H6_S100_r2": (lambda: _case(106, 6, 100, 2, 2, q_gain=2.0), 6, False, 0, 1e-2),
}


def _child(out_path):
    """every case through the operator under this process's CCX_XS_FULL_LINES; outputs saved by case name"""
    from clearconverse_amd import _lib
    lib = _lib.load()
    ctx = _lib.Context(0)
    res = {}
    for name, (build, H, mapped, rps, _) in CASES.items():
        q, wk, wv, bv, xa, rs = build()
        rows, D = q.shape
        n_seq, S, _ = xa.shape
        qd = q.contiguous().cuda()
        xd = xa.to(torch.bfloat16).contiguous().cuda()
        out = torch.empty(rows, D, device="cuda")
        wk_h, wv_h, bv_h = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (wk, wv, bv))
        rsp = (C.c_int * rows)(*[int(v) for v in rs]) if mapped else None
        ctx.check(lib.ccx_cross_attention_xa(ctx.handle, qd.data_ptr(), wk_h.ctypes.data, wv_h.ctypes.data, bv_h.ctypes.data, xd.data_ptr(),
                                             rsp, rps, rows, n_seq, H, S, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "ccx_cross_attention_xa")
        res[name] = out.cpu()
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def forms(ccx_ctx, tmp_path_factory):
    """{switch value: {case: output}}, one fresh child process per value (ccx_ctx: skipped without a GPU, like the other GPU tests)"""
    d = tmp_path_factory.mktemp("xs_full_lines")
    got = {}
    for sw in ("0", "1"):
        env = dict(os.environ, CCX_XS_FULL_LINES=sw, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
        path = d / f"out_{sw}.pt"
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"CCX_XS_FULL_LINES={sw}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        got[sw] = torch.load(path)
    return got


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(name):
        if name not in cache:
            build, H, _, _, _ = CASES[name]
            q, wk, wv, bv, xa, rs = build()
            cache[name] = _reference(q, wk, wv, bv, xa, rs, H)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_forms_are_bit_identical(forms, name):
    old, new = forms["0"][name], forms["1"][name]
    assert torch.isfinite(new).all()
    assert old.shape == new.shape and torch.equal(old, new), f"{name}: {int((old != new).sum())} of {old.numel()} values differ, max |d| {float((old - new).abs().max()):.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_full_line_form_against_explicit_kv(forms, references, name):
    got, want = forms["1"][name], references(name)
    tol = CASES[name][4]
    for r in range(got.shape[0]):
        rel = float((got[r] - want[r]).norm() / want[r].norm())
        print(f"{name} row {r}: rel-L2 {rel:.3e} (tolerance {tol:g})")
        within(f"cross attention against xa, full-line loads (bound {tol:g}): output rel-L2", rel, tol, (name, r))


if __name__ == "__main__":
    _child(sys.argv[1])
