"""What a per-iteration schedule costs: the B = 128 beta-VAE-GAN iteration on one GPU under a ``LambdaLR`` on both
optimizers plus a linear beta warm-up, in images/s.

  (a) the parent commit, the schedule applied by hand each iteration (``param_groups[0]["lr"] = ...``, ``trainer.beta =
      ...``): what a user could do before -- lr and beta are part of its capture key, so every iteration is a new key; how
      many of its iterations replayed is recorded;
  (p) the parent commit, unscheduled (its captured iteration);
  (b) this tree, scheduled (``lr_scheduler=``, ``beta_schedule=``: lr and beta in device words, one capture);
  (c) this tree, unscheduled (the switches off: the parent's launches).

Every leg is a process of its own (the parent is another checkout of the package), the legs are interleaved round by
round, and each reports WARM + TIMED iterations timed by a host clock around work that ends in a device synchronise.
Medians with min ... max.

    schedule_throughput.py --parent-tree DIR [--out profiles/r10_schedules.json] [--rounds 5]
    schedule_throughput.py --leg a|p|b|c --tree DIR          (one leg, one JSON line: what the driver starts)

Without ``--parent-tree`` the legs (a) and (p) run on this tree with none of the new arguments -- the same launches, but
not the parent's build -- and the result says so."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED, LR0 = 128, 10, 50, 1e-3
LR_GAMMA, BETA_FROM, BETA_TO, BETA_OVER = 0.999, 1.0, 25.0, 1000


def lr_factor(i):
    return LR_GAMMA ** i


def beta_at(it):
    return BETA_FROM + (BETA_TO - BETA_FROM) * min(it, BETA_OVER) / BETA_OVER


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    if not torch.cuda.is_available():
        raise SystemExit("schedule_throughput.py measures on the GPU; none found")
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    if leg == "b":
        tr = T.BetaVAEGANTrainer(beta=BETA_FROM, lr=LR0, graph=True, beta_schedule=beta_at,
                                 lr_scheduler=lambda opt: torch.optim.lr_scheduler.LambdaLR(opt, lr_factor))
    else:
        tr = T.BetaVAEGANTrainer(beta=BETA_TO if leg in "pc" else BETA_FROM, lr=LR0, graph=True)

    def one(it):
        if leg == "a":                                            # by hand, as the parent allows
            for opt in (tr.optimizerEG, tr.optimizerD):
                opt.param_groups[0]["lr"] = LR0 * lr_factor(it)
            tr.beta = beta_at(it)
        tr.step(x, *lat)

    for it in range(WARM):
        one(it)
    torch.cuda.synchronize()
    r0 = replays["n"]
    t0 = time.perf_counter()
    for it in range(WARM, WARM + TIMED):
        one(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.check_finite()
    print(json.dumps({"leg": leg, "images_per_s": B * TIMED / dt, "ms_per_iteration": 1e3 * dt / TIMED,
                      "timed_iterations": TIMED, "replayed": replays["n"] - r0, "captures": len(tr._graphs),
                      "lr_end": tr.optimizerEG.param_groups[0]["lr"], "beta_end": tr.beta}), flush=True)


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def drive(parent, out_path, rounds):
    trees = {"a": parent or HERE, "p": parent or HERE, "b": HERE, "c": HERE}
    names = {"a": "parent, schedule applied by hand", "p": "parent, unscheduled", "b": "this tree, scheduled",
             "c": "this tree, unscheduled"}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:                                  # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"leg {leg} failed with status {p.returncode}")
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:34s}: {res['images_per_s']:9.1f} images/s  "
                  f"{res['replayed']}/{res['timed_iterations']} replayed, {res['captures']} capture(s)", flush=True)
    out = {"what": "throughput of the B = 128 beta-VAE-GAN iteration under a per-iteration schedule (LambdaLR "
                   f"{LR_GAMMA}**i on both optimizers, beta {BETA_FROM} -> {BETA_TO} linearly over {BETA_OVER} iterations)",
           "device": "one MI355X (gfx950), default arithmetic, per-GPU batch 128",
           "method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then {TIMED} "
                     "timed by a host clock ending in a device synchronise",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new arguments (no parent checkout was given)",
           "legs": {}}
    for leg, rs in runs.items():
        out["legs"][leg] = {"name": names[leg], "images_per_s": summary([r["images_per_s"] for r in rs]),
                            "ms_per_iteration": summary([r["ms_per_iteration"] for r in rs], 3),
                            "replayed_of_timed": [r["replayed"] for r in rs], "timed_iterations": TIMED,
                            "captures_alive": [r["captures"] for r in rs]}
    med = {k: out["legs"][k]["images_per_s"]["median"] for k in runs}
    spread = {k: round(out["legs"][k]["images_per_s"]["max"] - out["legs"][k]["images_per_s"]["min"], 2) for k in runs}
    out["comparison"] = {
        "rule": "two legs are 'the same' if their medians differ by no more than the larger same-leg spread (max - min)",
        "scheduled_vs_unscheduled": {"b_minus_c": round(med["b"] - med["c"], 2), "spread_b": spread["b"],
                                     "spread_c": spread["c"],
                                     "same": abs(med["b"] - med["c"]) <= max(spread["b"], spread["c"])},
        "unscheduled_vs_parent": {"c_minus_p": round(med["c"] - med["p"], 2), "spread_c": spread["c"],
                                  "spread_p": spread["p"], "same": abs(med["c"] - med["p"]) <= max(spread["c"], spread["p"])},
        "scheduled_over_by_hand": round(med["b"] / med["a"], 2)}
    print(json.dumps(out["comparison"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=list("apbc"))
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, os.path.abspath(a.tree))
    else:
        drive(os.path.abspath(a.parent_tree) if a.parent_tree else None, a.out, a.rounds)
