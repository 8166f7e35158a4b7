"""What adaptive discriminator augmentation (``ada=``, vg_ada_update and the _dev twins of csrc/diff_augment.hip; DESIGN.md
section 4.35) costs and does.

  --kernels    (a) the controller alone at B = 128 and 1000, and forward + backward of the augmentation at (128, 3, 64, 64),
               policy 7, p = 0.5, through the value entry points and through the _dev twins: each leg is a HIP graph of
               CHAIN consecutive calls, replayed between two device events; legs interleaved round by round in one process.
               The figure is microseconds per call INSIDE a graph (a kernel and its boundary), not a replay's host floor.
  --leg        (b) the B = 128 beta-VAE-GAN iteration on one GPU, one process per leg, legs interleaved round by round:
                 (p) the parent commit (it has no ``ada=``): its captured iteration, no ``diff_augment``;
                 (n) this tree, no ``diff_augment``  (the parent's launches);
                 (f) this tree, ``diff_augment=(policy, 0.5)``: a fixed p;
                 (a) this tree, the same and ``ada=True``: p in the device word, the controller behind the iteration.
               (p) and (n) also print SHA-256 digests of the last step's outputs and of the final weights: the bit-neutrality
               record of the default path.  The parent cannot share an interpreter with this tree (one package name), so the
               legs are processes of one job, not loops of one process.
  --regime     (c) on the benchmark's fixed batch (seed 999, generator 1234, labels 0.9 / 0.1) with ``ada=dict(kimg=KIMG)``
               small enough to move: r_t, p and D(x) after 25 and after 100 iterations.  A record; no threshold, no claim.

    ada_timing.py --parent-tree DIR [--out profiles/r25_ada.json] [--rounds 3]
    ada_timing.py --kernels | --leg p|n|f|a --tree DIR | --regime none|logistic            (one JSON line each)

Without ``--parent-tree`` the leg (p) runs on this tree and the result says so."""
import argparse, hashlib, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED = 128, 10, 50
POLICY, P_FIXED = "color,translation,cutout", 0.5
K_ROUNDS, K_REPLAYS, CHAIN = 7, 50, 20
REGIME_KIMG, REGIME_MARKS = 10.0, (25, 100)


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes()).hexdigest()


def need_gpu(torch):
    if not torch.cuda.is_available():
        raise SystemExit("ada_timing.py measures on the GPU; none found")


def run_kernels():
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd import ops
    need_gpu(torch)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1).cuda()
    gy = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1).cuda()
    u = torch.rand(B, 8, generator=g).cuda()
    state = ops.ada_state("cuda", P_FIXED)
    word = state[0:1].view(torch.float32)
    d = {n: torch.randn(n, generator=g).cuda() for n in (128, 1000)}

    def twins(p):
        def fn():
            ops.diff_augment_fwd(x, u, 7, p)
            ops.diff_augment_bwd(gy, u, 7, p)
        return fn

    # rate 0: the controller runs its whole body (every 4th call adjusts) and p stays 0.5 for the legs that read it
    legs = {"augment_fwd_bwd_value": twins(P_FIXED), "augment_fwd_bwd_dev": twins(word),
            **{f"ada_update_B{n}": (lambda n=n: ops.ada_update(d[n], state, 0.0, 0.6, 0.0, 4)) for n in d}}
    graphs = {}
    for name, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(CHAIN):
                fn()
    times = {k: [] for k in legs}
    for _ in range(K_ROUNDS):
        for name, graph in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(K_REPLAYS):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * a.elapsed_time(b) / (K_REPLAYS * CHAIN))
    res = {name: {"us_per_call_inside_a_graph": summary(v, 3),
                  "spread_of_median": round((max(v) - min(v)) / statistics.median(v), 4)} for name, v in times.items()}
    res["dev_over_value_of_medians"] = round(statistics.median(times["augment_fwd_bwd_dev"])
                                             / statistics.median(times["augment_fwd_bwd_value"]), 4)
    res["p_after"] = ops.ada_read(state)["p"]
    print(json.dumps({"kernels": res}), flush=True)


def leg_keywords(leg):
    return {"p": {}, "n": {}, "f": dict(diff_augment=(POLICY, P_FIXED)),
            "a": dict(diff_augment=(POLICY, P_FIXED), ada=True)}[leg]


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    need_gpu(torch)
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    tr = T.BetaVAEGANTrainer(graph=True, **leg_keywords(leg))
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
    digests = {k: sha(v) for k, v in out.items()}
    digests["weights"] = sha(torch.cat([p.detach().reshape(-1) for net in (tr.netEG, tr.netD) for p in net.parameters()]))
    res = {"leg": leg, "images_per_s": B * TIMED / dt, "ms_per_iteration": 1e3 * dt / TIMED, "timed_iterations": TIMED,
           "replayed": replays["n"] - r0, "captures": len(tr._graphs), "mse_enc_end": float(out["mse_enc"]),
           "D_x_mean_end": float(out["D_x_sum"]) / B, "digests": digests}
    if leg == "a":
        res["ada_report_end"] = tr.ada_report()
    print(json.dumps(res), flush=True)


def run_regime(loss):
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
    need_gpu(torch)
    tr = BetaVAEGANTrainer(seed=999, beta=25.0, diff_augment=POLICY, ada=dict(kimg=REGIME_KIMG),
                           **({} if loss == "none" else dict(gan_loss=loss)))
    g = torch.Generator().manual_seed(1234)                      # bench.py's batch
    data = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1).cuda()
    noise = [torch.randn(B, 128, generator=g).cuda() for _ in range(3)]
    res = {"loss": loss, "ada": tr.ada, "p0": 0.0, "p_step_per_adjustment": B * tr.ada["interval"] * tr.ada["rate"], "after": {}}
    for it in range(1, max(REGIME_MARKS) + 1):
        out = tr.step(data, *noise, real_label=0.9, fake_label=0.1)
        if it in REGIME_MARKS:
            rep = tr.ada_report()
            res["after"][str(it)] = {"r_t": rep["rt"], "p": rep["p"], "adjustments": rep["adjustments"],
                                     "D_x_mean": float(out["D_x_sum"]) / B}
    print(json.dumps({"regime": res}), flush=True)


def child(cmd, cwd=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{' '.join(cmd)} failed with status {p.returncode}")
    return p.stdout


def child_json(cmd, cwd=None):
    return json.loads([ln for ln in child(cmd, cwd).splitlines() if ln.startswith("{")][-1])


def drive(parent, out_path, rounds):
    me = os.path.abspath(__file__)
    out = {"what": "adaptive discriminator augmentation: the controller and the device-word twins of the augmentation kernels "
                   "alone, the B = 128 beta-VAE-GAN iteration with ada=True / the same policy at a fixed p / without "
                   "diff_augment / on the parent commit, and r_t and p on the benchmark's batch",
           "device": "one MI355X (gfx950), default arithmetic",
           "kernels_method": f"one process; {K_ROUNDS} rounds, the legs interleaved; a leg is a HIP graph of {CHAIN} consecutive "
                             f"calls, {K_REPLAYS} replays between two device events; microseconds per call inside the graph",
           "iteration_method": f"{rounds} interleaved rounds, one process per leg and round (the parent cannot share an "
                               f"interpreter with this tree); {WARM} warm-up iterations, then {TIMED} timed by a host clock "
                               "ending in a device synchronise; a fixed batch, the uniforms drawn anew every iteration",
           "not_measured": "whether ADA holds D(x) off 1 on CelebA, or helps FID: no run on real data; data parallel; "
                           "rocprofv3 kernel times",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new keyword (no parent checkout was given)"}
    out.update(child_json([sys.executable, me, "--kernels"]))
    print("kernels", json.dumps({k: (v["us_per_call_inside_a_graph"]["median"] if isinstance(v, dict) else v)
                                 for k, v in out["kernels"].items()}), flush=True)
    trees = {"p": parent or HERE, "n": HERE, "f": HERE, "a": HERE}
    names = {"p": "parent", "n": "this tree, no diff_augment", "f": f"this tree, diff_augment=(policy, {P_FIXED})",
             "a": f"this tree, diff_augment=(policy, {P_FIXED}), ada=True"}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            res = child_json([sys.executable, me, "--leg", leg, "--tree", tree])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:52s}: {res['ms_per_iteration']:8.3f} ms  "
                  f"{res['replayed']}/{res['timed_iterations']} replayed, {res['captures']} capture(s)", flush=True)
    out["legs"] = {}
    for leg, rs in runs.items():
        out["legs"][leg] = {"name": names[leg], "images_per_s": summary([r["images_per_s"] for r in rs]),
                            "ms_per_iteration": summary([r["ms_per_iteration"] for r in rs], 3),
                            "replayed_of_timed": [r["replayed"] for r in rs], "captures_alive": [r["captures"] for r in rs],
                            "D_x_mean_of_the_last_timed_step": sorted({r["D_x_mean_end"] for r in rs})}
    out["legs"]["a"]["ada_report_of_the_last_timed_step"] = runs["a"][0]["ada_report_end"]
    ms = {k: [r["ms_per_iteration"] for r in rs] for k, rs in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    dp, dn = runs["p"][0]["digests"], runs["n"][0]["digests"]
    out["comparison"] = {
        "no_keyword_minus_parent_ms_of_medians": round(med["n"] - med["p"], 3),
        "same_leg_spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
        "no_keyword_median_inside_the_parents_range": bool(min(ms["p"]) <= med["n"] <= max(ms["p"])),
        "no_keyword_median_outside_the_parents_range_by_ms": round(max(min(ms["p"]) - med["n"], med["n"] - max(ms["p"]), 0.0), 3),
        "fixed_p_minus_no_keyword_ms_of_medians": round(med["f"] - med["n"], 3),
        "ada_minus_fixed_p_ms_of_medians": round(med["a"] - med["f"], 3),
        "ada_minus_fixed_p_ms_per_round": [round(a - f, 3) for a, f in zip(ms["a"], ms["f"])],
        "ada_over_fixed_p_of_medians": round(med["a"] / med["f"], 4),
        "iteration_digests_no_keyword_vs_parent": {"compared": len(dp), "equal": sum(dn.get(k) == v for k, v in dp.items()),
                                                   "every_run_of_p_and_n_agrees_with_its_first":
                                                       all(r["digests"] == runs[k][0]["digests"] for k in "pn" for r in runs[k])}}
    print(json.dumps(out["comparison"]), flush=True)
    out["regime"] = {}
    for loss in ("none", "logistic"):
        out["regime"][loss] = child_json([sys.executable, me, "--regime", loss])["regime"]
        print("regime", json.dumps(out["regime"][loss]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--leg", choices=list("pnfa"))
    ap.add_argument("--regime", choices=["none", "logistic"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.kernels:
        run_kernels()
    elif a.leg:
        run_leg(a.leg, os.path.abspath(a.tree))
    elif a.regime:
        run_regime(a.regime)
    else:
        drive(os.path.abspath(a.parent_tree) if a.parent_tree else None, a.out, a.rounds)
