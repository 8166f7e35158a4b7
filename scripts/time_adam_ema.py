"""Cost of the weight EMA inside the fused Adam step (optim.HipAdam(ema_decay=...)): the EG optimizer's step over netEG's
73.4 M parameters, eager, between device events, interleaved round by round -- the plain step (vg_adam_step_dev), the
fused step (vg_adam_step_dev_ema), and the plain step followed by ``torch._foreach_lerp_`` on the same tensors (the
unfused route).  Medians with min ... max; `time_adam_ema.py [out.json]`."""
import json, sys, os, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from disentangle_mlp_amd.optim import HipAdam
from disentangle_mlp_amd.trainer import BetaVAEGANTrainer

ROUNDS, STEP_REPS, DECAY = 7, 20, 0.999


def events(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "runs": [round(x, 4) for x in v]}


out = {"rounds": ROUNDS, "decay": DECAY}

# ---- the step ------------------------------------------------------------------------------------------------------
tr = BetaVAEGANTrainer(beta=25.0, graph=False)
params = list(tr.netEG.parameters())
n = sum(p.numel() for p in params)
for p in params:
    p.grad = torch.randn_like(p)
plain = HipAdam(params, lr=1e-6, capturable=True, nonfinite_guard=True)
fused = HipAdam(params, lr=1e-6, capturable=True, nonfinite_guard=True, ema_decay=DECAY)
shadow = [p.detach().clone() for p in params]
live = [p.detach() for p in params]


def unfused():
    plain.step()
    torch._foreach_lerp_(shadow, live, 1.0 - DECAY)


legs = {"plain step": plain.step, "fused step + EMA": fused.step, "plain step, then _foreach_lerp_": unfused}
for fn in legs.values():
    for _ in range(5):
        fn()
runs = {k: [] for k in legs}
for _ in range(ROUNDS):
    for k, fn in legs.items():
        runs[k].append(events(fn, STEP_REPS))
assert plain.nonfinite() == {} and fused.nonfinite() == {}
bytes_per_param = {"plain step": 28, "fused step + EMA": 36, "plain step, then _foreach_lerp_": 40}
out["step"] = {"parameters": n, "tensors": len(params), "unit": "ms per step() of the EG optimizer (eager, device events)",
               "steps_per_run": STEP_REPS}
for k, v in runs.items():
    s = summary(v)
    s["bytes_per_parameter"] = bytes_per_param[k]
    s["GB_per_s_at_median"] = round(n * bytes_per_param[k] / s["median"] / 1e6, 1)
    out["step"][k] = s
    print(f"{k:34s}: {s['median'] * 1e3:7.1f} us ({s['min'] * 1e3:.1f} ... {s['max'] * 1e3:.1f})  "
          f"{s['GB_per_s_at_median']:.0f} GB/s at {bytes_per_param[k]} B/parameter", flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
