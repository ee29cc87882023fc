"""Stand-alone timing of the X-stream cross attention (csrc/cross_x.hip) through ccx_cross_attention_xa: per-launch HIP-event times
of its three kernels for a range of row counts (one row per sequence), full small.en width; the streaming kernel once per load form
(CCX_XS_FULL_LINES = 0 half lines, 1 full lines; the operator reads the switch per call; 8 = the FP8 stream, through
ccx_cross_attention_xa_fp8), `reps` timed launches each: mean and (min .. max); TB/s of the bytes the form actually moves.
usage: python tools/xs_bench.py [rows ...]      XS_BENCH_FORMS=0,1,8 XS_BENCH_REPS=5 override the forms and the repetitions"""
import os
import sys
import numpy as np
import torch
from clearconverse_amd import _lib

def main():
    rows_list = [int(a) for a in sys.argv[1:]] or [128, 256, 368, 384, 512, 768]
    ctx = _lib.Context(0)
    lib = _lib.load()
    H, S = 12, 1500
    D = 64 * H
    g = torch.Generator().manual_seed(0)
    wk = (torch.randn(D, D, generator=g) / D ** 0.5).numpy().astype(np.float32)
    wv = (torch.randn(D, D, generator=g) / D ** 0.5).numpy().astype(np.float32)
    bv = np.zeros(D, np.float32)
    nmax = max(rows_list)
    xa = torch.randn(nmax, S, D, generator=g).to(torch.bfloat16).cuda()
    q = torch.randn(nmax, D, generator=g).cuda()
    out = torch.empty(nmax, D, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    forms = os.environ.get("XS_BENCH_FORMS", "0,1,8").split(",")
    xhat = torch.empty(nmax, S, D, dtype=torch.bfloat16, device="cuda") if "8" in forms else None
    reps = int(os.environ.get("XS_BENCH_REPS", "5"))
    names = {"0": "half lines", "1": "full lines", "8": "fp8"}
    for rows in rows_list:
        line = f"rows {rows:4d}:"
        for form in forms:
            if form != "8":
                os.environ["CCX_XS_FULL_LINES"] = form
            for it in range(2 + reps):
                if it == 2:
                    ctx.prof_enable(True)
                if form == "8":
                    ctx.check(lib.ccx_cross_attention_xa_fp8(ctx.handle, q.data_ptr(), wk.ctypes.data, wv.ctypes.data, bv.ctypes.data, xa.data_ptr(),
                                                             None, 0, rows, rows, H, S, out.data_ptr(), xhat.data_ptr(), st))
                else:
                    ctx.check(lib.ccx_cross_attention_xa(ctx.handle, q.data_ptr(), wk.ctypes.data, wv.ctypes.data, bv.ctypes.data, xa.data_ptr(), None,
                                                         0, rows, rows, H, S, out.data_ptr(), st))
            torch.cuda.synchronize()
            recs = ctx.prof_records()
            ctx.prof_enable(False)
            if form == forms[0]:
                for name, fl, by, ms in [r for r in recs if r[0].startswith("dec_x")][-3:]:
                    if "stream" not in name:
                        line += f"  {name.split('<')[0][4:]} {ms * 1e3:6.1f} us"
            v = [(ms * 1e3, by) for name, fl, by, ms in recs if "stream" in name]
            mean = sum(t for t, _ in v) / len(v)
            line += f"  | {names.get(form, form)}: {mean:6.1f} us ({min(t for t, _ in v):.1f} .. {max(t for t, _ in v):.1f}; {v[0][1] / (mean * 1e-6) / 1e12:.2f} TB/s)"
        os.environ.pop("CCX_XS_FULL_LINES", None)
        print(line, flush=True)

if __name__ == "__main__":
    main()
