"""GPU: the sequence-bias kernel (dec_bias_kernel, csrc/dec_bias.hip) on logits, histories and a table the test chooses, through
ccx_dec_bias_step, against the plain statement of the rule in tests/bias_reference.py (which tests/test_bias_reference_cpu.py checks
by hand and against the installed transformers' processors).

EXACT: the whole [rows, ld] buffer is compared with apply_bias_np's rows as int32 -- the kernel adds float32 numbers in the order the
rule states and uses no atomics, so there is nothing to tolerate.  That covers every element the rule does not edit, the columns
[n_vocab, ld) (a NaN with a payload) and the rows outside the sampling phase.

V = 515, ld = 520, text_end = 500; 1, 3 and 70 rows; sample_len 8 and 64; the table of bias_reference.kernel_table: entries of 1, 2, 3,
4, 5 and 32 ids, L - 1 == m and L - 1 == m + 1, [a, b, v] and [b, v] and a 4-gram on one target whose sum is 0 in table order and 1
in any other, a length-1 and a longer term on one id, -inf entries, a -inf logit under a finite bias, -0.0, targets 0 and
text_end - 1, a context id >= text_end, the first, the last and three absent keys, m = 0, finished and prompt-phase rows, and one key
with 480 groups so that the block's 256 threads loop.  A vocabulary of 515 ids cannot hold a key with 600 groups (a group is one
(key, target) pair and a target is < text_end), so the 600-group key runs in a launch of its own at V = 771, ld = 776, text_end = 760.
Then the composition with ccx_dec_history_step in the rule's order, and every rejection of the host check.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import bias_reference as BR
from tests import history_rules_reference as HR

pytestmark = pytest.mark.gpu

V, LD, E = 515, 520, 500
MANY = 480


def _states(rows):
    from clearconverse_amd import _lib
    return (_lib.DecSeqState * len(rows))(*[_lib.DecSeqState(r.pos, r.prompt_len, len(r.history), r.done, -1, -1, -1, 0, 0.0, 0.0) for r in rows])


def _launch(ctx, rows, table, sample_len, V=V, ld=LD, text_end=E, override=None, state_override=None, hist_override=None,
            table_override=None, logits_d=None):
    """one launch over `rows`; returns (input [R, ld] f32 with NaN patterns behind n_vocab, output [R, ld], the device buffer)"""
    from clearconverse_amd import _lib
    lib = _lib.load()
    R = len(rows)
    inp = np.empty((R, ld), dtype=np.float32)
    inp.view(np.int32)[:] = 0x7FC0BEEF                                  # a NaN with a payload: a store behind n_vocab shows
    for r, row in enumerate(rows):
        inp[r, :V] = row.logits
    if logits_d is None:
        logits_d = torch.from_numpy(inp.copy()).cuda()
    st_c = _states(rows)
    for r, (name, val) in (state_override or {}).items():
        setattr(st_c[r], name, val)
    hist = np.full((R, sample_len), -12345, dtype=np.int32)             # behind n_gen: never read (an id the host check would refuse)
    for r, row in enumerate(rows):
        hist[r, :len(row.history)] = row.history
    for (r, t), val in (hist_override or {}).items():
        hist[r, t] = val
    offsets, ids, bias = BR.to_arrays(table)
    for name, (i, val) in (table_override or {}).items():
        {"offsets": offsets, "ids": ids, "bias": bias}[name][i] = val
    d = _lib.DecBiasDesc()
    d.logits, d.logits_elems, d.ld, d.n_vocab, d.rows = logits_d.data_ptr(), logits_d.numel(), ld, V, R
    d.state, d.hist, d.sample_len, d.text_end = st_c, hist.ctypes.data_as(C.POINTER(C.c_int)), sample_len, text_end
    d.table.n_entries = len(bias)
    d.table.offsets, d.table.ids = offsets.ctypes.data_as(C.POINTER(C.c_int)), ids.ctypes.data_as(C.POINTER(C.c_int))
    d.table.bias = bias.ctypes.data_as(C.POINTER(C.c_float))
    for name, val in (override or {}).items():
        tgt = d.table if name.startswith("table.") else d
        name = name.split(".")[-1]
        setattr(tgt, name, val(getattr(tgt, name)) if callable(val) else val)
    rc = lib.ccx_dec_bias_step(ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check(rc, "ccx_dec_bias_step")
    return inp, logits_d.cpu().numpy(), logits_d


def _want(rows, inp, table, text_end, V=V):
    want = inp.copy()
    for r, row in enumerate(rows):
        if row.live:
            want[r, :V] = BR.apply_bias_np(row.logits, row.history, table, text_end)
    return want


@pytest.mark.parametrize("n_rows", [1, 3, 70])
@pytest.mark.parametrize("sample_len", [8, 64])
def test_kernel_is_the_rule_bit_for_bit(ccx_ctx, sample_len, n_rows):
    table = BR.kernel_table(V, E, MANY)
    rows = BR.bias_rows(V, E, sample_len, n_rows)
    inp, out, _ = _launch(ccx_ctx, rows, table, sample_len)
    want = _want(rows, inp, table, E)
    bad = np.argwhere(want.view(np.int32) != out.view(np.int32))
    assert bad.size == 0, [(rows[r].name, int(c), float(out[r, c]), float(want[r, c])) for r, c in bad[:6]]
    if n_rows >= 3:
        assert np.array_equal(inp[-2:].view(np.int32), out[-2:].view(np.int32))      # the finished and the prompt-phase row
        assert not np.array_equal(inp.view(np.int32), out.view(np.int32))            # ... and the launch did edit the others


def test_chosen_values(ccx_ctx):
    """the cases of the module docstring, one by one, on rows of ones (and planted values)"""
    table = BR.kernel_table(V, E, MANY)
    x = np.ones(V, dtype=np.float32)
    x[33], x[52] = -np.inf, -0.0
    hs = [[], [20], [40, 41], [39, 40, 41], [37, 39, 40, 41], list(BR.LONG), [99] + list(BR.LONG[1:]), [70], [5, 70], [3, E + 3], [1], [V - 1], [45]]
    rows = [BR.BiasRow(str(h[-3:]), h, x) for h in hs]
    inp, out, _ = _launch(ccx_ctx, rows, table, 64)
    assert np.array_equal(_want(rows, inp, table, E).view(np.int32), out.view(np.int32))
    o = {tuple(h): out[i] for i, h in enumerate(hs)}
    for h, row in zip(hs, out):                                                         # the length-1 terms land on every row, m = 0 included
        assert row[9] == -np.inf and row[E - 1] in (2.5, 2.0) and (row[0] == -1.0 or h[-1] == 70)
    assert o[()][7] == 1.75 and _only(o[()], x, {7, 9, E - 1, 0})                        # m = 0: nothing but the length-1 entries
    assert o[(20,)][7] == 3.75 and o[(20,)][30] == 2.0 and o[(20,)][31] == -np.inf and o[(20,)][33] == -np.inf and o[(20,)][E - 1] == 2.0
    assert o[(40, 41)][50] == np.float32(1.0) + np.float32(BR.BIG)                       # two of the three entries of one group
    assert o[(39, 40, 41)][50] == 1.0 and o[(39, 40, 41)][51] == 1.0                     # (BIG + 1) - BIG = 0; L - 1 == m + 1 did not fire
    assert o[(37, 39, 40, 41)][51] == 65.0
    assert np.signbit(o[(40, 41)][52]) and o[(40, 41)][52] == 0                          # -0.0 + -0.0
    assert o[tuple(BR.LONG)][60] == 5.0 and o[tuple([99] + list(BR.LONG[1:]))][60] == 1.0
    assert o[(70,)][3] == -np.inf and o[(70,)][4] == np.float32(1.0 + 0.125 * 5) and o[(5, 70)][4] == np.float32(1.0 + 0.125 * 5 + 0.5)
    assert o[(70,)][MANY - 1] == np.float32(1.0 + 0.125 * (1 + (MANY - 1) % 5)) and o[(70,)][MANY] == 1.0
    assert o[(3, E + 3)][25] == 2.0 and o[(1,)][26] == 4.0 and o[(V - 1,)][27] == 4.0
    assert _only(o[(45,)], x, {7, 9, E - 1, 0})                                          # an absent key


def _only(row, x, ids):
    changed = set(np.flatnonzero(row[:V].view(np.int32) != x.view(np.int32)).tolist())
    return changed == set(ids)


def test_a_key_with_600_groups(ccx_ctx):
    V2, LD2, E2 = 771, 776, 760
    table = BR.kernel_table(V2, E2, 600)
    g = np.random.default_rng(5)
    rows = [BR.BiasRow(f"{h}", h, (3.0 * g.standard_normal(V2)).astype(np.float32)) for h in ([70], [5, 70], [20], [])]
    inp, out, _ = _launch(ccx_ctx, rows, table, 8, V=V2, ld=LD2, text_end=E2)
    want = _want(rows, inp, table, E2, V=V2)
    assert np.array_equal(want.view(np.int32), out.view(np.int32))
    assert (inp[0, :600] != out[0, :600]).sum() >= 598 and np.array_equal(inp[0, 600:E2 - 1].view(np.int32), out[0, 600:E2 - 1].view(np.int32))


def test_only_multi_token_entries_and_m_0_change_nothing(ccx_ctx):
    table = [e for e in BR.kernel_table(V, E, MANY) if len(e[0]) > 1]
    rows = [BR.BiasRow("m = 0", [], np.ones(V, dtype=np.float32)) for _ in range(3)]
    inp, out, _ = _launch(ccx_ctx, rows, table, 8)
    assert np.array_equal(inp.view(np.int32), out.view(np.int32))
    inp, out, _ = _launch(ccx_ctx, BR.bias_rows(V, E, 8, 70), [], 8)                     # an empty table: a launch that edits nothing
    assert np.array_equal(inp.view(np.int32), out.view(np.int32))


def test_rows_outside_the_sampling_phase_are_not_validated_or_touched(ccx_ctx):
    """a finished row's and a prompt-phase row's history is never read: ids the check would refuse for a live row pass"""
    table = BR.kernel_table(V, E, MANY)
    rows = [BR.BiasRow("done", [20, 20], np.ones(V, dtype=np.float32), done=1),
            BR.BiasRow("prompt phase", [20, 20], np.ones(V, dtype=np.float32), prompt_len=4, pos=0),
            BR.BiasRow("live", [20, 20], np.ones(V, dtype=np.float32))]
    inp, out, _ = _launch(ccx_ctx, rows, table, 8, hist_override={(0, 0): 60000, (1, 1): -5})
    assert np.array_equal(inp[:2].view(np.int32), out[:2].view(np.int32))
    assert out[2, 30] == 2.0 and out[2, 31] == -np.inf


def test_bias_then_history_in_the_rules_order(ccx_ctx):
    """ccx_dec_bias_step then ccx_dec_history_step on the same device buffer: (x + b) / p, and a ban on top; the bias lands exactly,
    the penalty within the 2 ulp tests/test_dec_history_gpu.py allows the fp32 divide"""
    from clearconverse_amd import _lib
    lib = _lib.load()
    table = BR.kernel_table(V, E, MANY)
    g = np.random.default_rng(12)
    hs = [[20, 30, 20], [7, 20], [40, 41, 50, 40, 41], [70, 4, 70], []]
    rows = [BR.BiasRow(str(h), h, np.abs(3.0 * g.standard_normal(V)).astype(np.float32) + 0.5) for h in hs]
    SL, p, n = 8, 1.5, 2
    inp, biased, logits_d = _launch(ccx_ctx, rows, table, SL)
    hist = np.full((len(rows), SL), -12345, dtype=np.int32)
    for r, row in enumerate(rows):
        hist[r, :len(row.history)] = row.history
    d = _lib.DecHistoryDesc()
    d.logits, d.logits_elems, d.ld, d.n_vocab, d.rows = logits_d.data_ptr(), logits_d.numel(), LD, V, len(rows)
    d.state, d.hist, d.sample_len, d.text_end = _states(rows), hist.ctypes.data_as(C.POINTER(C.c_int)), SL, E
    d.repetition_penalty, d.no_repeat_ngram_size = p, n
    rc = lib.ccx_dec_history_step(ccx_ctx.handle, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ccx_ctx.check(rc, "ccx_dec_history_step")
    out = logits_d.cpu().numpy()
    for r, row in enumerate(rows):
        b = BR.apply_bias_np(row.logits, row.history, table, E)
        assert np.array_equal(b.view(np.int32), biased[r, :V].view(np.int32)), row.name
        want = HR.apply_history_rules_np(b, row.history, E, p, n)
        assert HR.ulp_distance(out[r, :V], want).max() <= 2, row.name
        other = BR.apply_bias_np(HR.apply_history_rules_np(row.logits, row.history, E, p, 0), row.history, table, E)
        if r == 0:                                       # 30 is biased behind 20 and completes the bigram [20, 30]: the ban on top
            assert biased[r, 30] == np.float32(row.logits[30] + np.float32(1.0)) and out[r, 30] == -np.inf
            assert out[r, 7] == biased[r, 7] == np.float32(np.float32(row.logits[7] + np.float32(0.75)) + np.float32(2.0))   # 7 not sampled: bias only
        if r == 1:                                       # 7 was sampled: ((x + 0.75) + 2) / 1.5
            x7 = np.float32(np.float32(row.logits[7] + np.float32(0.75)) + np.float32(2.0))
            assert HR.ulp_distance(out[r, 7:8], np.array([x7 / np.float32(p)], dtype=np.float32)).max() <= 2
            assert abs(float(out[r, 7]) - float(other[7])) > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections: one per host check
# ---------------------------------------------------------------------------------------------------------------------------------
def _bump2(p):
    return p + 2


REJECTIONS = [
    ("no rows", {"rows": 0}, None, None, None, "rows = 0"),
    ("n_vocab zero", {"n_vocab": 0}, None, None, None, "n_vocab = 0"),
    ("n_vocab beyond 13 groups", {"n_vocab": 53249, "ld": 53376}, None, None, None, "n_vocab = 53249"),
    ("ld below n_vocab", {"ld": 512}, None, None, None, "ld = 512"),
    ("logits null", {"logits": None}, None, None, None, "logits null or not 4-byte"),
    ("logits misaligned", {"logits": _bump2}, None, None, None, "logits null or not 4-byte"),
    ("logits_elems short", {"logits_elems": LD + V - 1}, None, None, None, "logits are written"),
    ("state null", {"state": None}, None, None, None, "state or hist is NULL"),
    ("hist null", {"hist": None}, None, None, None, "state or hist is NULL"),
    ("sample_len zero", {"sample_len": 0}, None, None, None, "sample_len = 0"),
    ("sample_len beyond the cap", {"sample_len": 2049}, None, None, None, "sample_len = 2049"),
    ("text_end behind the vocabulary", {"text_end": V + 1}, None, None, None, f"text_end = {V + 1}"),
    ("negative text_end", {"text_end": -1}, None, None, None, "text_end = -1"),
    ("n_gen beyond sample_len", {}, (0, ("n_gen", 9)), None, None, "n_gen = 9"),
    ("negative n_gen", {}, (0, ("n_gen", -1)), None, None, "n_gen = -1"),
    ("done neither 0 nor 1", {}, (1, ("done", 2)), None, None, "done = 2"),
    ("a history id behind the vocabulary", {}, None, ((0, 1), V), None, f"hist[0][1] = {V}"),
    ("a negative history id", {}, None, ((1, 0), -1), None, "hist[1][0] = -1"),
    ("negative n_entries", {"table.n_entries": -1}, None, None, None, "opts.n_entries = -1"),
    ("too many entries", {"table.n_entries": 8193}, None, None, None, "opts.n_entries = 8193"),
    ("offsets null", {"table.offsets": None}, None, None, None, "opts.offsets, opts.ids or opts.bias is NULL"),
    ("ids null", {"table.ids": None}, None, None, None, "opts.offsets, opts.ids or opts.bias is NULL"),
    ("bias null", {"table.bias": None}, None, None, None, "opts.offsets, opts.ids or opts.bias is NULL"),
    ("offsets do not start at 0", {}, None, None, {"offsets": (0, 1)}, "opts.offsets[0] = 1"),
    ("offsets descend", {}, None, None, {"offsets": (2, 0)}, "opts.offsets[2] = 0 does not ascend"),
    ("an empty entry", {}, None, None, {"offsets": (2, 1)}, "entry 1 has 0 ids"),
    ("an id behind the vocabulary", {}, None, None, {"ids": (1, V)}, f"opts.ids[1] = {V}"),
    ("a negative id", {}, None, None, {"ids": (1, -3)}, "opts.ids[1] = -3"),
    ("a target at text_end", {}, None, None, {"ids": (2, E)}, f"opts.ids[2] = {E}: the target of entry 1"),
    ("a bias of +inf", {}, None, None, {"bias": (1, math.inf)}, "opts.bias[1] = inf"),
    ("a bias of NaN", {}, None, None, {"bias": (0, math.nan)}, "opts.bias[0]"),
]
REJ_TABLE = [((7,), 1.0), ((20, 30), 1.0), ((20, 31), -math.inf)]              # offsets 0 1 3 5, ids 7 20 30 20 31


@pytest.mark.parametrize("name,override,state_change,hist_change,table_change,fragment", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(ccx_ctx, name, override, state_change, hist_change, table_change, fragment):
    from clearconverse_amd import _lib
    rows = [BR.BiasRow("a", [400, 401, 400], np.zeros(V, dtype=np.float32)), BR.BiasRow("b", [402, 403], np.zeros(V, dtype=np.float32))]
    so = None if state_change is None else {state_change[0]: state_change[1]}
    ho = None if hist_change is None else {hist_change[0]: hist_change[1]}
    with pytest.raises(_lib.CcxError) as e:
        _launch(ccx_ctx, rows, REJ_TABLE, 8, override=override, state_override=so, hist_override=ho, table_override=table_change)
    assert fragment in str(e.value) and "ccx_dec_bias_step" in str(e.value) and "(1)" in str(e.value), str(e.value)


def test_rejections_of_the_limits(ccx_ctx):
    from clearconverse_amd import _lib
    rows = [BR.BiasRow("a", [400], np.zeros(V, dtype=np.float32))]
    for table, fragment in (([(tuple(range(33)), 1.0)], "entry 0 has 33 ids"),
                            ([(tuple(range(32)), 1.0)] * 2048 + [((1,), 1.0)], "more than 65536 ids"),
                            ([((1,), 3e38), ((2, 3), 1.0), ((1,), 3e38)], "length-1 entries of target 1 sum to")):
        with pytest.raises(_lib.CcxError) as e:
            _launch(ccx_ctx, rows, table, 8)
        assert fragment in str(e.value) and "ccx_dec_bias_step" in str(e.value) and "(1)" in str(e.value), str(e.value)
    # at the limits: 8192 entries, 65536 ids
    inp, out, _ = _launch(ccx_ctx, rows, [((400, 5), 0.5)] * 8192, 8)
    assert out[0, 5] == np.float32(4096.0)
    inp, out, _ = _launch(ccx_ctx, rows, [(tuple(range(32)), 1.0)] * 2048, 8)
    assert np.array_equal(inp.view(np.int32), out.view(np.int32))
