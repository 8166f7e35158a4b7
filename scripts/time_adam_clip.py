"""Cost of clipping by global norm in front of / inside the fused Adam step (optim.HipAdam(max_grad_norm=...)).

Step: the EG optimizer's step over netEG's 73.4 M parameters, eager, between device events, interleaved round by round --
the plain step (vg_adam_step_dev_checked), the norm pass + finalize + clip step (vg_grad_sumsq_multi,
vg_grad_clip_finalize, vg_adam_step_dev_clip), and ``torch.nn.utils.clip_grad_norm_(foreach=True)`` followed by the plain
step (the unfused recipe).  Iteration: the graphed B = 128 beta-VAE-GAN iteration with ``max_grad_norm`` set against
unset, alternating.  Medians with min ... max; `time_adam_clip.py [out.json]`."""
import json, sys, os, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from disentangle_mlp_amd.optim import HipAdam
from disentangle_mlp_amd.trainer import BetaVAEGANTrainer

ROUNDS, STEP_REPS, ITER_REPS, MAX_NORM, B = 7, 20, 20, 1.0, 128


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


out = {"rounds": ROUNDS, "max_grad_norm": MAX_NORM}

# ---- the step ------------------------------------------------------------------------------------------------------
tr = BetaVAEGANTrainer(beta=25.0, graph=False)
params = list(tr.netEG.parameters())
n = sum(p.numel() for p in params)
for p in params:
    p.grad = torch.randn_like(p)
plain = HipAdam(params, lr=1e-6, capturable=True, nonfinite_guard=True)
fused = HipAdam(params, lr=1e-6, capturable=True, nonfinite_guard=True, max_grad_norm=MAX_NORM, skip_nonfinite=True)


def unfused():
    torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)      # (writes every gradient back)
    plain.step()


legs = {"plain step": plain.step, "norm pass + clip step": fused.step, "clip_grad_norm_, then plain step": unfused}
for fn in legs.values():
    for _ in range(5):
        fn()
runs = {k: [] for k in legs}
for _ in range(ROUNDS):
    for k, fn in legs.items():
        runs[k].append(events(fn, STEP_REPS))
assert plain.nonfinite() == {} and fused.nonfinite() == {} and fused.skipped_steps() == 0
bytes_per_param = {"plain step": 28, "norm pass + clip step": 32, "clip_grad_norm_, then plain step": 40}
out["step"] = {"parameters": n, "tensors": len(params), "unit": "ms per step() of the EG optimizer (eager, device events)",
               "steps_per_run": STEP_REPS}
for k, v in runs.items():
    s = summary(v)
    s["bytes_per_parameter"] = bytes_per_param[k]
    s["GB_per_s_at_median"] = round(n * bytes_per_param[k] / s["median"] / 1e6, 1)
    out["step"][k] = s
    print(f"{k:34s}: {s['median'] * 1e3:7.1f} us ({s['min'] * 1e3:.1f} ... {s['max'] * 1e3:.1f})  "
          f"{s['GB_per_s_at_median']:.0f} GB/s at {bytes_per_param[k]} B/parameter", flush=True)
del tr, plain, fused, params

# ---- the graphed iteration -----------------------------------------------------------------------------------------
gen = torch.Generator().manual_seed(0)
x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
trainers = {"max_grad_norm unset": BetaVAEGANTrainer(beta=25.0, graph=True),
            "max_grad_norm set": BetaVAEGANTrainer(beta=25.0, graph=True, max_grad_norm=MAX_NORM)}
for t in trainers.values():
    for _ in range(5):                                           # two eager iterations, the capture, two replays
        t.step(x, *lat)
    assert len(t._graphs) == 1 and t.graph
runs = {k: [] for k in trainers}
for _ in range(ROUNDS):
    for k, t in trainers.items():
        runs[k].append(events(lambda: t.step(x, *lat), ITER_REPS))
for t in trainers.values():
    t.check_finite()
out["iteration"] = {"batch": B, "unit": "ms per graphed iteration (device events)", "iterations_per_run": ITER_REPS}
for k, v in runs.items():
    out["iteration"][k] = s = summary(v)
    print(f"{k:34s}: {s['median']:7.3f} ms ({s['min']:.3f} ... {s['max']:.3f})", flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
