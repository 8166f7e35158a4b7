"""BatchNorm backward: the team form of the one pass (bn_bwd_team_kernel) against the two passes (bn_partial_kernel<1> +
bn_apply_kernel<true>), eager, between device events, the two forms interleaved in ONE process (boxes and clock states
differ by more than the forms do), on the benchmark's two large layer shapes at B = 128 and on one shape of every team
size T from 2 to 16.

Both forms run on the same tensors through the tuning knob: vg_debug_set_bn_team(8, 0) forces the team form with the
product's NV = 8; with max_wgs capped at 1 no team fits and the dispatch falls back to the two passes (their 16-byte loops).

    python scripts/time_bn_bwd.py [--json out.json] [--reps 30]

Prints one line per shape: T, rounds, median and min..max of each form in microseconds, the ratio, and the achieved
bytes per second of each (12 B and 20 B per element).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from disentangle_mlp_amd import ops, _lib

lib = _lib.use_tuning().__enter__()      # the vg_debug_* knobs live in the tuning build only

BENCH = [(128, 128, 32, 32), (128, 32, 64, 64)]                                  # the 16 two-pass launches of an iteration
BY_T = [(8 * t, 128 if t <= 4 else 64 if t <= 8 else 32, 64, 64) for t in range(2, 17)]   # B * 4096 = T * 32768


def plan(shape, t):
    out = (ctypes.c_int * 5)()
    assert lib.vg_debug_bn_bwd_plan(shape[0], shape[1], shape[2] * shape[3], t.data_ptr(), t.data_ptr(), t.data_ptr(), out) == 0
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(12)
    results = []
    for shape in BENCH + [s for s in BY_T if s not in BENCH]:
        B, C = shape[0], shape[1]
        x = torch.randn(*shape, device="cuda", generator=g) * 2 + 0.5
        gy = torch.randn(*shape, device="cuda", generator=g)
        gamma, beta = torch.rand(C, device="cuda", generator=g) + 0.5, torch.randn(C, device="cuda", generator=g)
        _, mean, invstd = ops.bn_act_fwd(x, gamma, beta, None, None, 1e-5, 0.1, 1)
        forms = {"team": (8, 0), "two": (8, 1)}        # knob (nv, max_wgs): max_wgs = 1 < T leaves the two passes
        plans = {}
        for name, knob in forms.items():
            lib.vg_debug_set_bn_team(*knob)
            plans[name] = plan(shape, x)
        assert plans["team"][0] == 4 and plans["two"][0] == 3, (shape, plans)

        def run(name):
            lib.vg_debug_set_bn_team(*forms[name])
            return ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, 1)

        same = all(torch.allclose(p, q, rtol=1e-4, atol=1e-5) for p, q in zip(run("team"), run("two")))
        for _ in range(30):                            # the clock takes tens of launches to settle after idle
            run("team"), run("two")
        torch.cuda.synchronize()
        ts = {"team": [], "two": []}
        for _ in range(a.reps):
            for name in ("team", "two"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(name)
                e1.record()
                torch.cuda.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
        n = x.numel()
        r = dict(shape=list(shape), T=plans["team"][2], teams=plans["team"][3], rounds=plans["team"][4], agree=bool(same))
        for name, bpe in (("team", 12), ("two", 20)):
            med = statistics.median(ts[name])
            r[name] = dict(median_us=round(med, 1), min_us=round(min(ts[name]), 1), max_us=round(max(ts[name]), 1),
                           TBps=round(n * bpe / med / 1e6, 2))
        r["team_over_two"] = round(r["team"]["median_us"] / r["two"]["median_us"], 3)
        results.append(r)
        print(f"{str(shape):20s} T={r['T']:2d} rounds={r['rounds']} team {r['team']['median_us']:7.1f} us "
              f"({r['team']['min_us']:.1f}..{r['team']['max_us']:.1f}, {r['team']['TBps']} TB/s)   two {r['two']['median_us']:7.1f} us "
              f"({r['two']['min_us']:.1f}..{r['two']['max_us']:.1f}, {r['two']['TBps']} TB/s)   ratio {r['team_over_two']:.3f}"
              f"{'' if same else '   RESULTS DIFFER'}", flush=True)
        del x, gy
    lib.vg_debug_set_bn_team(0, 0)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, timing="eager, device events, forms interleaved",
                           shapes=results), f, indent=1)


if __name__ == "__main__":
    main()
