"""HipAdam (vg_adam_step), HipAdam with the non-finite guard (vg_adam_step_checked) and torch's fused Adam on the
reference's parameter set (109.5 M fp32 parameters): one step() over all parameters between device events, the three
interleaved round by round; medians and min ... max.  `time_adam.py [out.json]`."""
import json, sys, os, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from disentangle_mlp_amd.optim import HipAdam
from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
tr = BetaVAEGANTrainer(beta=25.0)
params = [p for p in list(tr.netEG.parameters()) + list(tr.netD.parameters())]
n = sum(p.numel() for p in params)
for p in params:
    p.grad = torch.randn_like(p)
def timeit(opt, reps=20):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): opt.step()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps
opts = {"HipAdam": HipAdam(params, lr=1e-6), "HipAdam guarded": HipAdam(params, lr=1e-6, nonfinite_guard=True),
        "torch fused Adam": torch.optim.Adam(params, lr=1e-6, fused=True)}
for opt in opts.values():
    for _ in range(5): opt.step()
runs = {name: [] for name in opts}
for _ in range(7):
    for name, opt in opts.items():
        runs[name].append(timeit(opt))
assert opts["HipAdam guarded"].nonfinite() == {}
out = {"parameters": n, "unit": "ms per step() over all parameters (5 launches)", "steps_per_run": 20}
for name, v in runs.items():
    ms = statistics.median(v)
    out[name] = {"median": round(ms, 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(f"{name:18s}: {ms*1e3:7.1f} us ({min(v)*1e3:.1f} ... {max(v)*1e3:.1f}) for {n/1e6:.1f} M parameters = {n*28/ms/1e9:6.2f} TB/s of ~8 (28 B per parameter)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
