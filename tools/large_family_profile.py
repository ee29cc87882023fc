"""One-run measurements of the full large_v3_turbo() / large_v3() presets with seeded weights (and a 1024-wide sibling at reduced
depth for the per-launch comparison): one 30 s window x 8, ccx_prof kernel sums.

    python tools/large_family_profile.py {turbo|v3|w1024} OUT.json        (from the repository root, on the GPU)
"""
import json, os, sys, time
os.environ["CCX_PROF_SHAPES"] = "1"
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from clearconverse_amd import _lib
from clearconverse_amd.audio import synthetic_clip
from clearconverse_amd.weights import WhisperDims, synthetic_whisper_state_dict
from clearconverse_amd.whisper import WhisperModel

which = sys.argv[1]
out_path = sys.argv[2]
B, STEPS = 8, 8
dims = {"turbo": WhisperDims.large_v3_turbo, "v3": WhisperDims.large_v3,
        "w1024": lambda: WhisperDims.mini(n_layer=4, n_state=1024, n_vocab=51865)}[which]()
res = {"which": which, "dims": dims.__dict__, "B": B}
t0 = time.time(); sd = synthetic_whisper_state_dict(dims, seed=1); res["weights_s"] = round(time.time() - t0, 1)
print(which, "weights", res["weights_s"], "s", flush=True)
ctx = _lib.Context(0)
t0 = time.time(); m = WhisperModel(dims, sd, max_batch=B, ctx=ctx); res["load_s"] = round(time.time() - t0, 1)
del sd
print("load", res["load_s"], "s", flush=True)
clip = synthetic_clip(5, 30.0)
dev = torch.from_numpy(np.tile(clip[None], (B, 1))).cuda()
ns = [len(clip)] * B
prompts = [m.rules.sot_sequence("en")] * B

def front():
    m.log_mel(dev, ns); m.encode(B)

def timed(fn, n=3):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return ts

res["front_ms_wall"] = [round(t, 2) for t in timed(front)]
r = m.decode(prompts, sample_len=4)
res["cross_path"] = m.last_cross_path
# graph-resident decode, wall: 64 sampled positions (suppressing nothing extra: synthetic weights rarely emit eot early)
for sl in (32, 64):
    ts = timed(lambda: m.decode(prompts, sample_len=sl), 2)
    res[f"decode_ms_wall_sample_len_{sl}"] = [round(t, 2) for t in ts]
res["decode_ms_per_step_wall"] = round((min(res["decode_ms_wall_sample_len_64"]) - min(res["decode_ms_wall_sample_len_32"])) / 32, 4)
n32 = [len(x["tokens"]) for x in m.decode(prompts, sample_len=64)]
res["tokens_sampled_of_64"] = n32

def agg(recs):
    d = {}
    for name, fl, by, ms in recs:
        a = d.setdefault(name, [0, 0.0, 0.0, 0.0]); a[0] += 1; a[1] += fl; a[2] += by; a[3] += ms
    return {k: dict(launches=v[0], ms=round(v[3], 4), us_per_launch=round(v[3] * 1e3 / v[0], 2),
                    gbs=round(v[2] / (v[3] * 1e-3) / 1e9, 1) if v[3] > 0 and v[2] > 0 else None,
                    tflops=round(v[1] / (v[3] * 1e-3) / 1e12, 2) if v[3] > 0 and v[1] > 0 else None,
                    bytes_per_launch=v[2] / v[0]) for k, v in sorted(d.items(), key=lambda kv: -kv[1][3])}

ctx.prof_enable(True); front(); torch.cuda.synchronize(); recs = ctx.prof_records(); ctx.prof_enable(False)
res["front_kernel_ms_sum"] = round(sum(r[3] for r in recs), 3)
res["front_kernels"] = agg(recs)
os.environ["CCX_NO_GRAPH"] = "1"
m.decode(prompts, sample_len=STEPS); torch.cuda.synchronize()
ctx.prof_enable(True); m.decode(prompts, sample_len=STEPS); torch.cuda.synchronize(); recs = ctx.prof_records(); ctx.prof_enable(False)
del os.environ["CCX_NO_GRAPH"]
steps = sum(1 for r in recs if r[0].startswith("dec_select"))
res["decode_probe"] = dict(sample_len=STEPS, select_launches=steps, kernel_ms_sum=round(sum(r[3] for r in recs), 3))
res["decode_kernels"] = agg(recs)
res["hbm_used_gb"] = round((torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 1e9, 1)
m.close()
json.dump(res, open(out_path, "w"), indent=1)
print(json.dumps({k: v for k, v in res.items() if not k.endswith("kernels")}))
for sec in ("front_kernels", "decode_kernels"):
    for k, v in list(res[sec].items())[:14]:
        print(sec, k, v)
