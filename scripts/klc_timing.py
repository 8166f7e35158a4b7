"""What the KL capacity over free bits (``kl_control=``, csrc/reparam_klc.hip) costs.

  --kernel     forward + backward of the fused kernels (`functional.reparam_klc`: 2 + 1 launches) at (B, D) = (128, 128) and
               (256, 128) against the same objective composed from ATen ops on the device through autograd (the fp32
               restatement of tests/_klc_refs.py); legs interleaved round by round inside one process, device events
               around ITER calls per round; launch counts from the profiler's kernel events.
  (driver)     the B = 128 beta-VAE-GAN iteration on one GPU, one process per leg, legs interleaved round by round:
                 (p) the parent commit (it has no ``kl_control=``): its captured iteration;
                 (c) this tree without the argument (the parent's launches);
                 (k) this tree, ``kl_control=(12.5, 0.05)``: a constant capacity, a frozen kernel argument;
                 (h) this tree without the argument, ``device_hyper=True``: what the device words cost by themselves;
                 (t) this tree, ``kl_control=(linear_capacity(25, 100000), 0.05)``: the capacity annealed every iteration,
                     which turns ``device_hyper`` on.
               ``--bench-rounds N`` appends N rounds of ``bench.py --gpus 1 --steps 40 --warmup 5`` in the parent checkout
               and in this tree, the order of the two swapped from round to round.

    klc_timing.py --parent-tree DIR [--out profiles/r21_kl_control.json] [--rounds 5] [--bench-rounds 3]
    klc_timing.py --kernel | --leg p|c|k|h|t --tree DIR        (one JSON line each: what the driver starts)

Without ``--parent-tree`` the leg (p) runs on this tree without the new argument and the result says so."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED = 128, 10, 50
BETA, FREE_BITS = 6.0, 0.05
C_MAX, C_ITERATIONS = 25.0, 100000      # Burgess et al.'s schedule
K_ROUNDS, K_ITER = 7, 200


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def run_kernel():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import _klc_refs as R
    from disentangle_mlp_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("klc_timing.py measures on the GPU; none found")
    out = {}
    for shape in ((128, 128), (256, 128)):
        i = R.make_inputs(*shape)
        capacity = R.capacity_of(i, (0.5, FREE_BITS))               # half the floored total: a live gradient
        i = {k: v.cuda() for k, v in i.items()}
        mu, lv = i["mu"].requires_grad_(True), i["lv"].requires_grad_(True)
        one = torch.ones((), device="cuda")

        def fused():
            mu.grad = lv.grad = None
            z, loss, _ = F.reparam_klc(mu, lv, i["eps"], BETA, capacity, FREE_BITS)
            torch.autograd.backward([loss, z], grad_tensors=[one, i["gz"]])

        def aten():
            mu.grad = lv.grad = None
            z = mu + i["eps"] * torch.exp(0.5 * lv)
            loss = R.objective(mu, lv, BETA, capacity, FREE_BITS)["loss"]
            torch.autograd.backward([loss, z], grad_tensors=[one, i["gz"]])

        legs = {"fused": fused, "aten": aten}
        grads = {}
        for name, fn in legs.items():
            for _ in range(3):
                fn()
            grads[name] = (mu.grad.clone(), lv.grad.clone())
        launches = {}
        for name, fn in legs.items():
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                launches[name] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
            except Exception as e:                                 # the count is a report, not the measurement
                launches[name] = f"not counted ({type(e).__name__})"
        us = {k: [] for k in legs}
        for _ in range(K_ROUNDS):
            for name, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(K_ITER):
                    fn()
                b.record()
                torch.cuda.synchronize()
                us[name].append(1e3 * a.elapsed_time(b) / K_ITER)
        # the kernels alone, captured (no host in the loop): what one graphed iteration pays
        graph = torch.cuda.CUDAGraph()
        fused()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            fused()
        cap = []
        for _ in range(K_ROUNDS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(K_ITER):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            cap.append(1e3 * a.elapsed_time(b) / K_ITER)
        med = {k: statistics.median(v) for k, v in us.items()}
        out[f"{shape[0]}x{shape[1]}"] = {
            "fused_us": summary(us["fused"]), "aten_us": summary(us["aten"]), "fused_captured_us": summary(cap),
            "aten_over_fused_of_medians": round(med["aten"] / med["fused"], 2),
            "fused_is_faster_in_every_round": all(f < a for f, a in zip(us["fused"], us["aten"])),
            "kernel_launches": launches,
            "gradients_agree_rel": [R.rel_err(grads["fused"][n], grads["aten"][n]) for n in (0, 1)]}
    print(json.dumps({"kernel": out}), flush=True)


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    if not torch.cuda.is_available():
        raise SystemExit("klc_timing.py measures on the GPU; none found")
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    kw = {"t": lambda: dict(kl_control=(T.linear_capacity(C_MAX, C_ITERATIONS), FREE_BITS)),
          "k": lambda: dict(kl_control=(0.5 * C_MAX, FREE_BITS)), "h": lambda: dict(device_hyper=True)}.get(leg, dict)()
    tr = T.BetaVAEGANTrainer(graph=True, **kw)
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
    print(json.dumps({"leg": leg, "images_per_s": B * TIMED / dt, "ms_per_iteration": 1e3 * dt / TIMED,
                      "timed_iterations": TIMED, "replayed": replays["n"] - r0, "captures": len(tr._graphs),
                      "device_hyper": bool(tr.device_hyper),
                      "mse_enc_end": float(out["mse_enc"]), "kld_end": float(out["kld"]), "keys": sorted(out)}), flush=True)


def child(cmd, cwd=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{' '.join(cmd)} failed with status {p.returncode}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def drive(parent, out_path, rounds, bench_rounds):
    me = os.path.abspath(__file__)
    option = f"kl_control=(linear_capacity({C_MAX:g}, {C_ITERATIONS}), {FREE_BITS:g})"
    out = {"what": "the KL capacity over free bits as fused kernels (csrc/reparam_klc.hip) against the same objective composed "
                   f"from ATen ops, and the B = 128 beta-VAE-GAN iteration with {option} / without it / on the parent commit",
           "device": "one MI355X (gfx950), default arithmetic",
           "kernel_method": f"one process; {K_ROUNDS} rounds, the legs interleaved, each figure {K_ITER} forward + backward "
                            "calls between two device events (host launches included); fused_captured_us: the same "
                            "fused calls replayed from a HIP graph",
           "iteration_method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then "
                               f"{TIMED} timed by a host clock ending in a device synchronise",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new argument (no parent checkout was given)"}
    out.update(child([sys.executable, me, "--kernel"]))
    print(json.dumps(out["kernel"]), flush=True)
    trees = {"p": parent or HERE, "c": HERE, "k": HERE, "h": HERE, "t": HERE}
    names = {"p": "parent", "c": "this tree, no kl_control", "k": f"this tree, kl_control=({0.5 * C_MAX:g}, {FREE_BITS:g})",
             "h": "this tree, no kl_control, device_hyper=True", "t": f"this tree, {option}"}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            res = child([sys.executable, me, "--leg", leg, "--tree", tree])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:62s}: {res['ms_per_iteration']:8.3f} ms  "
                  f"{res['replayed']}/{res['timed_iterations']} replayed, {res['captures']} capture(s)", flush=True)
    out["legs"] = {}
    for leg, rs in runs.items():
        out["legs"][leg] = {"name": names[leg], "images_per_s": summary([r["images_per_s"] for r in rs]),
                            "ms_per_iteration": summary([r["ms_per_iteration"] for r in rs], 3),
                            "replayed_of_timed": [r["replayed"] for r in rs], "captures_alive": [r["captures"] for r in rs],
                            "loss_keys": rs[0]["keys"], "device_hyper": rs[0]["device_hyper"],
                            "mse_enc_of_the_last_timed_step": sorted({r["mse_enc_end"] for r in rs})}
    ms = {k: [r["ms_per_iteration"] for r in rs] for k, rs in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    out["comparison"] = {
        "no_option_minus_parent_ms_of_medians": round(med["c"] - med["p"], 3),
        "same_leg_spread_ms": spread,
        "no_option_agrees_with_parent_within_spread": bool(abs(med["c"] - med["p"]) <= max(spread["p"], spread["c"])),
        "no_option_computes_what_the_parent_computes": {r["mse_enc_end"] for r in runs["c"]} == {r["mse_enc_end"] for r in runs["p"]},
        "constant_capacity_minus_no_option_ms_of_medians": round(med["k"] - med["c"], 3),
        "constant_capacity_minus_no_option_ms_per_round": [round(k - c, 3) for k, c in zip(ms["k"], ms["c"])],
        "device_hyper_alone_minus_no_option_ms_of_medians": round(med["h"] - med["c"], 3),
        "annealed_capacity_minus_device_hyper_alone_ms_of_medians": round(med["t"] - med["h"], 3),
        "annealed_capacity_minus_device_hyper_alone_ms_per_round": [round(t - h, 3) for t, h in zip(ms["t"], ms["h"])],
        "annealed_capacity_minus_no_option_ms_of_medians": round(med["t"] - med["c"], 3),
        "fused_captured_us_at_128x128": out["kernel"]["128x128"]["fused_captured_us"]["median"]}
    print(json.dumps(out["comparison"]), flush=True)
    if bench_rounds:
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "40", "--warmup", "5"]
        bench = {"parent": [], "this_commit_defaults": []}
        for r in range(bench_rounds):
            for key, tree in (("parent", parent or HERE), ("this_commit_defaults", HERE))[::-1 if r % 2 else 1]:
                bench[key].append(child(cmd, cwd=tree))
                print(f"bench round {r} {key}: {bench[key][-1]['value']} images/s", flush=True)
        out["default_path"] = {"command": "python bench.py --gpus 1 --steps 40 --warmup 5",
                               "method": f"{bench_rounds} rounds in the same session, each round: the parent commit and this "
                                         "commit (kl_control at its default), one process each, the order swapped from "
                                         "round to round"}
        for key, rs in bench.items():
            out["default_path"][key] = {"images_per_s": summary([b["value"] for b in rs]),
                                        "ms_per_step": summary([b["ms_per_step"] for b in rs], 3)}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--leg", choices=list("pckht"))
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-rounds", type=int, default=0)
    a = ap.parse_args()
    if a.kernel:
        run_kernel()
    elif a.leg:
        run_leg(a.leg, os.path.abspath(a.tree))
    else:
        drive(os.path.abspath(a.parent_tree) if a.parent_tree else None, a.out, a.rounds, a.bench_rounds)
