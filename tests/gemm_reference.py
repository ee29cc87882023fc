"""Plain-torch fp64 reference of the GEMM family's descriptor semantics (csrc/gemm_bf16.h GemmParams) and the comparator the
kernel tests use.  CPU only; tests/test_gemm_reference_cpu.py checks this file against torch's own convolutions and against
one-unit mutations of a descriptor, tests/test_gemm_family_gpu.py checks the kernels against it.

A descriptor is a dict with the GemmParams field names (missing fields are 0 / None) plus "epi".  `tensors` holds the FLAT
buffers as the kernel sees them from each pointer: "A", "W" (bf16), "bias", "scale", "shift" (fp32 or None), "out" (the
destination as it is BEFORE the launch: sentinel-filled, or holding the residual for an in-place launch), "resid" (fp32; pass the
same tensor as "out" for in-place), "resid_bf16", and "hq" / "hk" / "hv" for EPI_HEADS.

What the descriptor means (from the comments of gemm_bf16.h):
  C[m][n] = sum over taps t of  A[m * lda + t * a_tap_stride + k] * W[n * ldw + t * K + k],  k < K        (ntaps <= 1: one tap)
  rows arrive in groups of rpb_in: row i of group g goes to g * rpb_out + i + roff, rows i >= rpb_valid are dropped; with
  img_rows_in > 0 the groups themselves come in images of img_rows_in, group r of image j goes to group j * img_rows_out + r and
  groups r >= img_rows_valid are dropped.  The residual row is the DESTINATION row (modulo resid_mod if that is > 0).
"""
import math

import torch

EPI_BF16, EPI_BF16_GELU, EPI_F32_RESID, EPI_F32, EPI_HEADS, EPI_BF16_RELU, EPI_F32_GELU_POS, EPI_BF16_LRELU_AFFINE, \
    EPI_BF16_ADD_RELU = range(9)
F32_OUT = (EPI_F32_RESID, EPI_F32, EPI_F32_GELU_POS)
U24 = 2.0 ** -24          # unit roundoff of fp32
GELU_LIPSCHITZ = 1.13     # max |d/dx gelu(x)| = 1.1289 (at x = +-1.4142 ... the derivative Phi(x) + x phi(x) peaks at x = sqrt(2))

FIELDS = ("lda", "ldw", "M", "N", "K", "ntaps", "a_tap_stride", "ldo", "ldr", "resid_mod", "slope", "rpb_in", "rpb_out", "roff",
          "rpb_valid", "img_rows_in", "img_rows_valid", "img_rows_out", "ldrb", "d_model", "n_head", "S", "Spad", "v_transposed",
          "first_block")


def ceil16(n):
    return (n + 15) // 16 * 16


def dest_rows(d):
    """(destination row, kept?) of every GEMM row 0 .. M-1 -- the two-level row remap, restated from the header comment."""
    m = torch.arange(d["M"], dtype=torch.int64)
    keep = torch.ones(d["M"], dtype=torch.bool)
    rpb_in = d.get("rpb_in", 0)
    if rpb_in <= 0:
        return m, keep
    group, i = m // rpb_in, m % rpb_in
    keep = i < d["rpb_valid"]
    img_in = d.get("img_rows_in", 0)
    if img_in > 0:
        image, r = group // img_in, group % img_in
        keep = keep & (r < d["img_rows_valid"])
        group = image * d["img_rows_out"] + r
    return group * d["rpb_out"] + i + d.get("roff", 0), keep


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _rows2d(flat, rows, ld, n):
    """flat[rows[i] * ld + c] for c < n, as an [len(rows), n] gather."""
    idx = rows[:, None] * ld + torch.arange(n, dtype=torch.int64)[None, :]
    return flat[idx.reshape(-1)].reshape(len(rows), n), idx


def gemm_reference(d, t):
    """-> {destination name: {"init", "ref" (fp64, flat, = init where nothing is written), "writable" (bool: may be written at
    all), "checked" (bool: value asserted -- columns < N of kept rows), "budget" (fp64: L * E of the module docstring of the
    tests, 0 where not checked), "bf16" (output type)}}"""
    epi = d["epi"]
    M, N, K = d["M"], d["N"], d["K"]
    taps = max(d.get("ntaps", 0), 1)
    Kt = K * taps
    A, W = t["A"], t["W"]
    assert A.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and A.dim() == 1 and W.dim() == 1
    acc = torch.zeros(M, N, dtype=torch.float64)
    mag = torch.zeros(M, N, dtype=torch.float64)
    for tap in range(taps):
        a = torch.as_strided(A, (M, K), (d["lda"], 1), tap * d.get("a_tap_stride", 0)).double()
        w = torch.as_strided(W, (N, K), (d["ldw"], 1), tap * K).double()
        acc += a @ w.T
        mag += (a.abs().float() @ w.abs().float().T).double()      # a bound's magnitude: fp32 is plenty (and 3x cheaper)
    if t.get("bias") is not None:
        b = t["bias"].double()[:N]
        acc += b
        mag += b.abs()

    if epi == EPI_HEADS:
        return _heads(d, t, acc, mag, Kt)

    orow, keep = dest_rows(d)
    kept = torch.nonzero(keep).flatten()
    orow_k = orow[kept]
    acc, mag = acc[kept], mag[kept]
    out0 = t["out"]
    bf16 = epi not in F32_OUT
    assert out0.dtype == (torch.bfloat16 if bf16 else torch.float32) and out0.dim() == 1
    ldo = d["ldo"]

    resid = None
    if epi in (EPI_F32_RESID, EPI_F32_GELU_POS, EPI_BF16_LRELU_AFFINE) and t.get("resid") is not None:
        rrow = orow_k % d["resid_mod"] if d.get("resid_mod", 0) > 0 else orow_k
        resid = _rows2d(t["resid"].double(), rrow, d["ldr"], N)[0]
    if epi == EPI_BF16_ADD_RELU and t.get("resid_bf16") is not None:
        resid = _rows2d(t["resid_bf16"].double(), orow_k, d["ldrb"], N)[0]

    lip = torch.ones(N, dtype=torch.float64)
    extra = 0.0
    if epi in (EPI_BF16, EPI_F32):
        val = acc
    elif epi == EPI_BF16_GELU:
        val, lip = gelu64(acc), lip * GELU_LIPSCHITZ
    elif epi == EPI_BF16_RELU:
        val = acc.clamp(min=0)
    elif epi == EPI_F32_RESID:
        val, mag = acc + resid, mag + resid.abs()
    elif epi == EPI_F32_GELU_POS:
        val, mag, lip = gelu64(acc) + resid, mag + resid.abs(), lip * GELU_LIPSCHITZ
    elif epi == EPI_BF16_LRELU_AFFINE:
        if resid is not None:
            acc, mag = acc + resid, mag + resid.abs()
        slope = float(torch.tensor(d.get("slope", 0.0), dtype=torch.float32))     # the kernel holds it in fp32
        val = torch.where(acc >= 0, acc, slope * acc)
        lip = lip * max(1.0, abs(slope))
        if t.get("scale") is not None:
            sc = t["scale"].double()[:N]
            val, lip = val * sc, lip * sc.abs()
        # three more fp32 roundings after the sum (slope *, scale *, + shift), each of a value no larger than L * mag (+ |shift|)
        extra = 3 * U24 * (mag * lip)
        if t.get("shift") is not None:
            sh = t["shift"].double()[:N]
            val = val + sh
            extra = extra + 3 * U24 * sh.abs()
    elif epi == EPI_BF16_ADD_RELU:
        if resid is not None:
            acc, mag = acc + resid, mag + resid.abs()
        val = acc.clamp(min=0)
    else:
        raise ValueError(epi)
    budget = (Kt + 3) * U24 * mag * lip + extra

    Nw = ceil16(N)
    ref = out0.double().clone()
    writable = torch.zeros(out0.numel(), dtype=torch.bool)
    checked = torch.zeros(out0.numel(), dtype=torch.bool)
    bud = torch.zeros(out0.numel(), dtype=torch.float64)
    idx_w = (orow_k[:, None] * ldo + torch.arange(Nw, dtype=torch.int64)[None, :]).reshape(-1)
    idx_c = (orow_k[:, None] * ldo + torch.arange(N, dtype=torch.int64)[None, :]).reshape(-1)
    assert len(torch.unique(orow_k)) == len(orow_k), "two GEMM rows map to one destination row"
    writable[idx_w] = True
    checked[idx_c] = True
    ref[idx_c] = val.reshape(-1)
    bud[idx_c] = budget.reshape(-1)
    return {"out": {"init": out0, "ref": ref, "writable": writable, "checked": checked, "budget": bud, "bf16": bf16}}


def _heads(d, t, acc, mag, Kt):
    """EPI_HEADS: column block j (d_model wide) goes to destination first_block + j of (hq, hk, hv), head-major [B, n_head, Spad, 64];
    the third destination is [B, n_head, 64, Spad] (V^T) when v_transposed."""
    M, N, dm, H, S, Spad = d["M"], d["N"], d["d_model"], d["n_head"], d["S"], d["Spad"]
    B = M // S
    assert B * S == M and dm == 64 * H and N % dm == 0
    budget = (Kt + 3) * U24 * mag
    res = {}
    for j in range(N // dm):
        blk = d.get("first_block", 0) + j
        name = ("hq", "hk", "hv")[blk]
        init = t[name]
        assert init.dtype == torch.bfloat16 and init.dim() == 1
        v = acc[:, j * dm:(j + 1) * dm].reshape(B, S, H, 64)
        e = budget[:, j * dm:(j + 1) * dm].reshape(B, S, H, 64)
        if blk == 2 and d.get("v_transposed", 0):
            shape, v, e = (B, H, 64, Spad), v.permute(0, 2, 3, 1), e.permute(0, 2, 3, 1)
            sel = (slice(None), slice(None), slice(None), slice(0, S))
        else:
            shape, v, e = (B, H, Spad, 64), v.permute(0, 2, 1, 3), e.permute(0, 2, 1, 3)
            sel = (slice(None), slice(None), slice(0, S), slice(None))
        n = B * H * Spad * 64
        ref = init.double().clone()
        mask = torch.zeros(init.numel(), dtype=torch.bool)
        bud = torch.zeros(init.numel(), dtype=torch.float64)
        ref[:n].view(shape)[sel] = v
        mask[:n].view(shape)[sel] = True
        bud[:n].view(shape)[sel] = e
        res[name] = {"init": init, "ref": ref, "writable": mask, "checked": mask.clone(), "budget": bud, "bf16": True}
    return res


class Verdict:
    def __init__(self):
        self.ok, self.reason, self.rel_l2, self.worst_ratio, self.excess = True, "", 0.0, 0.0, 0.0

    def fail(self, why):
        if self.ok:
            self.ok, self.reason = False, why


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def compare(exp, got, gelu_excess=0.0):
    """One destination buffer against its expectation (an entry of gemm_reference's result).  `got` is the flat buffer after the
    launch, in the output type.
      (a) every element outside `writable` is bit-identical to `init`; writable but unchecked elements (columns N .. ceil16(N)) are
          finite;
      (b) every checked element: |got - ref| <= ulp + budget + gelu_excess, with ulp = 2^-8 (|ref| + budget) for bf16 outputs
          (round-to-nearest of a value within `budget` of ref moves it by at most half a bf16 ulp <= 2^-8 of its size), 0 for fp32;
      (c) the aggregate rel-L2 over the checked elements is RETURNED (the caller bounds it).
    Also returned: the worst ratio error / allowance of (b) and `excess` = max(|got - ref| - budget, 0) (the measured term of the
    GELU epilogues)."""
    v = Verdict()
    init = exp["init"]
    assert got.dtype == init.dtype and got.shape == init.shape, (got.dtype, init.dtype, got.shape, init.shape)
    un = ~exp["writable"]
    if not torch.equal(_bits(got)[un], _bits(init)[un]):
        bad = torch.nonzero(un & (_bits(got) != _bits(init))).flatten()
        v.fail(f"{len(bad)} elements that may not be written changed, first at flat index {int(bad[0])}")
    g = got.double()
    if not bool(torch.isfinite(g[exp["writable"]]).all()):
        v.fail("non-finite value in a written element")
    ck = exp["checked"]
    ref, bud = exp["ref"][ck], exp["budget"][ck]
    err = (g[ck] - ref).abs()
    allow = bud + gelu_excess + ((2.0 ** -8) * (ref.abs() + bud + gelu_excess) if exp["bf16"] else 0.0)
    if err.numel():
        ratio = err / allow.clamp(min=1e-300)
        v.worst_ratio = float(ratio.max())
        v.excess = float((err - bud).clamp(min=0).max())
        v.rel_l2 = float(err.norm() / (ref.norm() + 1e-30))
        if not bool((err <= allow).all()):
            k = int(ratio.argmax())
            flat = int(torch.nonzero(ck).flatten()[k])
            v.fail(f"element at flat index {flat}: got {float(g[ck][k])!r} ref {float(ref[k])!r} error {float(err[k]):.3e} "
                   f"allowed {float(allow[k]):.3e}; {int((err > allow).sum())} elements over")
    return v


def round_like(exp):
    """The reference rounded to the output type: what a perfect kernel would leave in the buffer."""
    return exp["ref"].to(exp["init"].dtype)
