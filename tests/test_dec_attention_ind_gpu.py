"""GPU: the self attention of a decode step through a cache indirection (dec_attention_kernel<true, true>, csrc/decoder.hip; form 8 of
ccx_dec_attention_desc) -- what lets a beam-search hypothesis that moved to another row keep reading the K/V its ancestors wrote.
Key t of row r comes from cache slot ind[r][t].  Against the fp64 reference of tests/dec_reference.py on the K/V gathered by the table,
under the self form's own bound; bit for bit against form 0 (dec_attention_kernel<true>) on K/V gathered PHYSICALLY by the table; and,
with an identity table, bit for bit against form 0 on the same buffers.  6 rows in two groups of 3 (a row's keys come from its group's
slots, as a beam window's do), H = 2, key counts at the edges of the wave chunk (64) and the block stride (256)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import dec_reference as DR
from tests.test_dec_attention_gpu import N_BF16, TOL_BF16_OUT, _operands, _run
from tests.conftest import within

pytestmark = pytest.mark.gpu

SELF, SELF_IND = 0, 8
LABEL = "dec_attention_kernel<true,true> (self, indirect)"
KEYS = (1, 63, 64, 65, 255, 256, 257, 448)
ROWS, GROUP, H, KV_T = 6, 3, 2, 448


def _table(ind):
    flat = np.ascontiguousarray(ind, dtype=np.uint16)
    return flat, flat.ctypes.data_as(C.POINTER(C.c_uint16))


def _case(n_a, n_b, pattern, seed):
    """group A (rows 0..2) attends to n_a keys, group B to n_b; keys behind a group's count are NaN in all of its slots"""
    q, k, v = _operands(seed, ROWS, ROWS, H, KV_T, gain=2.0)
    n_keys = [n_a] * GROUP + [n_b] * GROUP
    for s in range(ROWS):
        k[s, :, n_keys[s]:], v[s, :, n_keys[s]:] = math.nan, math.nan
    g = np.random.default_rng(seed)
    ind = np.full((ROWS, KV_T), 60000, dtype=np.uint16)                # never read behind a row's keys (out of range on purpose)
    for r in range(ROWS):
        base = r // GROUP * GROUP
        ind[r, :n_keys[r]] = r if pattern == "identity" else base + g.integers(0, GROUP, n_keys[r])
    kg, vg = torch.full_like(k, math.nan), torch.full_like(v, math.nan)
    t = torch.arange(KV_T)
    for r in range(ROWS):
        n = n_keys[r]
        src = torch.from_numpy(ind[r, :n].astype(np.int64))
        kg[r, :, :n] = k[src, :, t[:n]].transpose(0, 1)
        vg[r, :, :n] = v[src, :, t[:n]].transpose(0, 1)
    return q, k, v, kg, vg, ind, n_keys


@pytest.mark.parametrize("pattern", ["permuted", "identity"])
@pytest.mark.parametrize("i", range(len(KEYS)))
def test_indirect_equals_gathered(ccx_ctx, i, pattern):
    n_a, n_b = KEYS[i], KEYS[(i + 3) % len(KEYS)]
    q, k, v, kg, vg, ind, n_keys = _case(n_a, n_b, pattern, 40 + i)
    pos = [n - 1 for n in n_keys]
    flat, ptr = _table(ind)
    res = _run(ccx_ctx, SELF_IND, k, v, q=q, pos=pos, override=dict(ind=ptr, ind_ld=KV_T), labels=True)
    assert res["labels"] == [LABEL]
    assert torch.isfinite(res["out"]).all()
    ref, vmax = DR.attention_ref(q, kg, vg, n_keys)
    within(N_BF16, DR.bf16_out_excess(res["out"], ref, vmax), TOL_BF16_OUT, (pattern, n_a, n_b))
    gathered = _run(ccx_ctx, SELF, kg, vg, q=q, pos=pos)
    assert torch.equal(res["out"], gathered["out"]), (pattern, n_a, n_b)            # bit for bit: same loads' values, same arithmetic
    if pattern == "identity":
        same = _run(ccx_ctx, SELF, k, v, q=q, pos=pos)
        assert torch.equal(res["out"], same["out"]), (n_a, n_b)
    else:
        moved = sum(int((ind[r, :n_keys[r]] != r).sum()) for r in range(ROWS))
        assert moved > 0                                                                # the table really moves keys


@pytest.mark.parametrize("what,change", [
    ("ind[1][2] = 6 out of range", "entry"),
    ("ind is NULL", "null"),
    ("needs ind_ld > it", "ld"),
    ("row_seq is not taken by form 8", "row_seq"),
])
def test_rejections(ccx_ctx, what, change):
    from clearconverse_amd import _lib
    q, k, v, kg, vg, ind, n_keys = _case(8, 8, "permuted", 3)
    pos = [7] * ROWS
    ind[:, 8:] = 0
    kw = dict(ind_ld=KV_T)
    row_seq = None
    if change == "entry":
        ind[1, 2] = 6
    if change == "ld":
        kw["ind_ld"] = 7
    if change == "row_seq":
        row_seq = list(range(ROWS))
    flat, ptr = _table(ind)
    if change != "null":
        kw["ind"] = ptr
    with pytest.raises(_lib.CcxError) as e:
        _run(ccx_ctx, SELF_IND, k, v, q=q, pos=pos, row_seq=row_seq, override=kw)
    assert "ccx_dec_attention_desc" in str(e.value) and what in str(e.value), str(e.value)
