"""What the trainer-driven weight EMA costs: the B = 128 beta-VAE-GAN iteration on one GPU, in images/s.

  (p) the parent commit (it has no ``ema_decay=``): its captured iteration;
  (c) this tree, ``ema_decay=None`` (the switch off: the parent's launches);
  (e) this tree, ``ema_decay=ema_warmup(0.999)``: the phase-3 EG step averages into the shadow network, the decay -- another
      value every iteration -- read from a device word; how many of its iterations replayed is recorded.

Every leg is a process of its own (the parent is another checkout of the package), the legs are interleaved round by
round, and each reports WARM + TIMED iterations timed by a host clock around work that ends in a device synchronise.
Medians with min ... max.  ``--bench-rounds N`` appends N alternating rounds of ``bench.py --gpus 1 --steps 40 --warmup 5``
in the parent checkout and in this tree (the default path).

    trainer_ema_throughput.py --parent-tree DIR [--out profiles/r11_trainer_ema.json] [--rounds 5] [--bench-rounds 3]
    trainer_ema_throughput.py --leg p|c|e --tree DIR          (one leg, one JSON line: what the driver starts)

Without ``--parent-tree`` the leg (p) runs on this tree without the new argument -- the same launches, but not the
parent's build -- and the result says so."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED, DECAY = 128, 10, 50, 0.999
R08_EXTRA_MS = (535 - 421) / 1000        # profiles/r08_adam_ema.json: an averaged EG step against a plain one


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    if not torch.cuda.is_available():
        raise SystemExit("trainer_ema_throughput.py measures on the GPU; none found")
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    tr = T.BetaVAEGANTrainer(graph=True, **(dict(ema_decay=T.ema_warmup(DECAY)) if leg == "e" else {}))
    for _ in range(WARM):
        tr.step(x, *lat)
    torch.cuda.synchronize()
    r0 = replays["n"]
    t0 = time.perf_counter()
    for _ in range(TIMED):
        out = tr.step(x, *lat)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.check_finite()
    res = {"leg": leg, "images_per_s": B * TIMED / dt, "ms_per_iteration": 1e3 * dt / TIMED, "timed_iterations": TIMED,
           "replayed": replays["n"] - r0, "captures": len(tr._graphs), "mse_enc_end": float(out["mse_enc"])}
    if leg == "e":
        res["decay_end"] = tr.optimizerEG.ema_decay
        res["shadow_differs"] = not all(torch.equal(e, p) for e, p in zip(tr.ema_model.parameters(), tr.netEG.parameters()))
    print(json.dumps(res), flush=True)


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def child(cmd, cwd=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{' '.join(cmd)} failed with status {p.returncode}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def drive(parent, out_path, rounds, bench_rounds):
    trees = {"p": parent or HERE, "c": HERE, "e": HERE}
    names = {"p": "parent, no EMA", "c": "this tree, ema_decay=None", "e": f"this tree, ema_decay=ema_warmup({DECAY})"}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            res = child([sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:40s}: {res['images_per_s']:9.1f} images/s  "
                  f"{res['replayed']}/{res['timed_iterations']} replayed, {res['captures']} capture(s)", flush=True)
    out = {"what": "throughput of the B = 128 beta-VAE-GAN iteration with the trainer-driven weight EMA "
                   f"(BetaVAEGANTrainer(ema_decay=ema_warmup({DECAY})): the phase-3 EG step averages into the shadow network, "
                   "the decay read from a device word) against the parent commit without EMA",
           "device": "one MI355X (gfx950), default arithmetic, per-GPU batch 128",
           "method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then {TIMED} "
                     "timed by a host clock ending in a device synchronise",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new argument (no parent checkout was given)",
           "legs": {}}
    for leg, rs in runs.items():
        out["legs"][leg] = {"name": names[leg], "images_per_s": summary([r["images_per_s"] for r in rs]),
                            "ms_per_iteration": summary([r["ms_per_iteration"] for r in rs], 3),
                            "replayed_of_timed": [r["replayed"] for r in rs], "timed_iterations": TIMED,
                            "captures_alive": [r["captures"] for r in rs],
                            "mse_enc_of_the_last_timed_step": sorted({r["mse_enc_end"] for r in rs})}
    out["legs"]["e"]["decay_of_the_last_timed_step"] = sorted({r["decay_end"] for r in runs["e"]})
    out["legs"]["e"]["shadow_differs_from_live"] = all(r["shadow_differs"] for r in runs["e"])
    ms = {k: [r["ms_per_iteration"] for r in rs] for k, rs in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    slow = med["e"] - med["p"]
    allowed = R08_EXTRA_MS + max(spread["p"], spread["e"])
    out["comparison"] = {
        "ema_minus_parent_ms_of_medians": round(slow, 3),
        "ema_minus_parent_ms_per_round": [round(e - p, 3) for e, p in zip(ms["e"], ms["p"])],
        "slowdown_percent_of_medians": round(100 * slow / med["p"], 2),
        "same_leg_spread_ms": spread,
        "expected_from_r08_adam_ema_ms": round(R08_EXTRA_MS, 3),
        "condition": "slowdown <= the r08 difference + the run's own spread (the larger same-leg max - min of p and e)",
        "allowed_ms": round(allowed, 3), "holds": bool(slow <= allowed),
        "no_ema_minus_parent_ms_of_medians": round(med["c"] - med["p"], 3),
        "live_run_unchanged": len({r["mse_enc_end"] for rs in runs.values() for r in rs}) == 1}
    print(json.dumps(out["comparison"]), flush=True)
    if bench_rounds:
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "40", "--warmup", "5"]
        bench = {"parent": [], "this_commit_defaults": []}
        for r in range(bench_rounds):
            for key, tree in (("parent", parent or HERE), ("this_commit_defaults", HERE)):
                bench[key].append(child(cmd, cwd=tree))
                print(f"bench round {r} {key}: {bench[key][-1]['value']} images/s", flush=True)
        out["default_path"] = {"command": "python bench.py --gpus 1 --steps 40 --warmup 5",
                               "method": f"{bench_rounds} rounds in the same session, each round: the parent commit, then "
                                         "this commit (ema_decay at its default), one process each"}
        for key, rs in bench.items():
            out["default_path"][key] = {"images_per_s": summary([b["value"] for b in rs]),
                                        "ms_per_step": summary([b["ms_per_step"] for b in rs], 3)}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=list("pce"))
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-rounds", type=int, default=0)
    a = ap.parse_args()
    if a.leg:
        run_leg(a.leg, os.path.abspath(a.tree))
    else:
        drive(os.path.abspath(a.parent_tree) if a.parent_tree else None, a.out, a.rounds, a.bench_rounds)
