"""What the InfoVAE / WAE-MMD regulariser (``mmd_vae=``, csrc/reparam_mmd.hip) costs.

  --kernel     forward + backward of the fused kernels (`functional.reparam_mmd`: 3 + 1 launches) at (B, D) = (128, 128) and
               (256, 128) against the same objective composed from ATen ops on the device through autograd, twice: the
               fp32 restatement of tests/_mmd_refs.py (differences, a [B, B, D] temporary per pair matrix) and the usual
               short form on `torch.cdist` ([B, B] temporaries only); legs interleaved round by round inside one process,
               device events around ITER calls per round; launch counts from the profiler's kernel events.
  (driver)     the B = 128 beta-VAE-GAN iteration on one GPU, one process per leg, legs interleaved round by round:
                 (p) the parent commit (it has no ``mmd_vae=``): its captured iteration;
                 (c) this tree without the argument (the parent's launches);
                 (t) this tree, ``mmd_vae=("imq", 1000)``.
               ``--bench-rounds N`` appends N alternating rounds of ``bench.py --gpus 1 --steps 40 --warmup 5`` in the
               parent checkout and in this tree.

    mmd_timing.py --parent-tree DIR [--out profiles/r17_mmd_vae.json] [--rounds 5] [--bench-rounds 3]
    mmd_timing.py --kernel | --leg p|c|t --tree DIR        (one JSON line each: what the driver starts)

Without ``--parent-tree`` the leg (p) runs on this tree without the new argument and the result says so."""
import argparse, json, os, statistics, sys, time

from dip_timing import child, summary      # (the sibling script: the same figures, the same child processes)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED = 128, 10, 50
BETA, CASE = 6.0, ("imq", 1000.0)
K_ROUNDS, K_ITER = 7, 200


def run_kernel():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import _mmd_refs as R
    from disentangle_mlp_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("mmd_timing.py measures on the GPU; none found")
    kernel, lam = CASE
    out = {}
    for shape in ((128, 128), (256, 128)):
        i = {k: v.cuda() for k, v in R.make_inputs(*shape).items()}
        mu, lv = i["mu"].requires_grad_(True), i["lv"].requires_grad_(True)
        one = torch.ones((), device="cuda")
        hs = R.default_bandwidths(kernel, shape[1])
        nb = shape[0]
        off = ~torch.eye(nb, dtype=torch.bool, device="cuda")

        def fused():
            mu.grad = lv.grad = None
            z, loss, _ = F.reparam_mmd(mu, lv, i["eps"], i["zp"], BETA, lam, kernel)
            torch.autograd.backward([loss, z], grad_tensors=[one, i["gz"]])

        def aten():
            mu.grad = lv.grad = None
            z = mu + i["eps"] * torch.exp(0.5 * lv)
            loss = R.objective(mu, lv, z, i["zp"], BETA, kernel, lam)["loss"]
            torch.autograd.backward([loss, z], grad_tensors=[one, i["gz"]])

        def aten_cdist():
            mu.grad = lv.grad = None
            z = mu + i["eps"] * torch.exp(0.5 * lv)
            kl = -0.5 * (1.0 + lv - mu ** 2 - torch.exp(lv)).sum()
            kzz = R.kernel_values(torch.cdist(z, z) ** 2, kernel, hs)[off].sum() / (nb * (nb - 1))
            kpp = R.kernel_values(torch.cdist(i["zp"], i["zp"]) ** 2, kernel, hs)[off].sum() / (nb * (nb - 1))
            kzp = R.kernel_values(torch.cdist(z, i["zp"]) ** 2, kernel, hs).sum() / (nb * nb)
            loss = BETA * kl + nb * lam * (kzz + kpp - 2.0 * kzp)
            torch.autograd.backward([loss, z], grad_tensors=[one, i["gz"]])

        legs = {"fused": fused, "aten": aten, "aten_cdist": aten_cdist}
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
            "fused_us": summary(us["fused"]), "aten_us": summary(us["aten"]), "aten_cdist_us": summary(us["aten_cdist"]),
            "fused_captured_us": summary(cap),
            "aten_over_fused_of_medians": round(med["aten"] / med["fused"], 2),
            "aten_cdist_over_fused_of_medians": round(med["aten_cdist"] / med["fused"], 2),
            "fused_is_faster_in_every_round": all(f < min(a, c) for f, a, c in zip(us["fused"], us["aten"], us["aten_cdist"])),
            "kernel_launches": launches,
            "gradients_agree_rel": {name: [R.rel_err(grads["fused"][n], grads[name][n]) for n in (0, 1)]
                                    for name in ("aten", "aten_cdist")}}
    print(json.dumps({"kernel": out}), flush=True)


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    if not torch.cuda.is_available():
        raise SystemExit("mmd_timing.py measures on the GPU; none found")
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    extra = dict(prior=torch.randn(B, 128, generator=gen).cuda()) if leg == "t" else {}
    tr = T.BetaVAEGANTrainer(graph=True, **(dict(mmd_vae=CASE) if leg == "t" else {}))
    for _ in range(WARM):
        tr.step(x, *lat, **extra)
    torch.cuda.synchronize()
    r0 = replays["n"]
    t0 = time.perf_counter()
    for _ in range(TIMED):
        out = tr.step(x, *lat, **extra)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.check_finite()
    print(json.dumps({"leg": leg, "images_per_s": B * TIMED / dt, "ms_per_iteration": 1e3 * dt / TIMED,
                      "timed_iterations": TIMED, "replayed": replays["n"] - r0, "captures": len(tr._graphs),
                      "mse_enc_end": float(out["mse_enc"]), "kld_end": float(out["kld"]), "keys": sorted(out)}), flush=True)


def drive(parent, out_path, rounds, bench_rounds):
    me = os.path.abspath(__file__)
    out = {"what": "the InfoVAE / WAE-MMD objective as fused kernels (csrc/reparam_mmd.hip) against the same objective "
                   f"composed from ATen ops, and the B = 128 beta-VAE-GAN iteration with mmd_vae={CASE!r} / without it / on "
                   "the parent commit",
           "device": "one MI355X (gfx950), default arithmetic",
           "kernel_method": f"one process; {K_ROUNDS} rounds, the legs interleaved, each figure {K_ITER} forward + backward "
                            "calls between two device events (host launches included); aten: the restatement of "
                            "tests/_mmd_refs.py in fp32 ([B, B, D] differences); aten_cdist: the same objective on "
                            "torch.cdist ([B, B] temporaries); fused_captured_us: the same fused calls replayed from a HIP "
                            "graph",
           "iteration_method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then "
                               f"{TIMED} timed by a host clock ending in a device synchronise",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new argument (no parent checkout was given)"}
    out.update(child([sys.executable, me, "--kernel"]))
    print(json.dumps(out["kernel"]), flush=True)
    trees = {"p": parent or HERE, "c": HERE, "t": HERE}
    names = {"p": "parent", "c": "this tree, no mmd_vae", "t": f"this tree, mmd_vae={CASE!r}"}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            res = child([sys.executable, me, "--leg", leg, "--tree", tree])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:40s}: {res['ms_per_iteration']:8.3f} ms  "
                  f"{res['replayed']}/{res['timed_iterations']} replayed, {res['captures']} capture(s)", flush=True)
    out["legs"] = {}
    for leg, rs in runs.items():
        out["legs"][leg] = {"name": names[leg], "images_per_s": summary([r["images_per_s"] for r in rs]),
                            "ms_per_iteration": summary([r["ms_per_iteration"] for r in rs], 3),
                            "replayed_of_timed": [r["replayed"] for r in rs], "captures_alive": [r["captures"] for r in rs],
                            "loss_keys": rs[0]["keys"],
                            "mse_enc_of_the_last_timed_step": sorted({r["mse_enc_end"] for r in rs})}
    ms = {k: [r["ms_per_iteration"] for r in rs] for k, rs in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    out["comparison"] = {
        "no_option_minus_parent_ms_of_medians": round(med["c"] - med["p"], 3),
        "same_leg_spread_ms": spread,
        "no_option_agrees_with_parent_within_spread": bool(abs(med["c"] - med["p"]) <= max(spread["p"], spread["c"])),
        "no_option_computes_what_the_parent_computes": {r["mse_enc_end"] for r in runs["c"]} == {r["mse_enc_end"] for r in runs["p"]},
        "option_minus_no_option_ms_of_medians": round(med["t"] - med["c"], 3),
        "option_minus_no_option_ms_per_round": [round(t - c, 3) for t, c in zip(ms["t"], ms["c"])],
        "fused_captured_us_at_128x128": out["kernel"]["128x128"]["fused_captured_us"]["median"]}
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
                                         "this commit (mmd_vae at its default), one process each"}
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
    ap.add_argument("--leg", choices=list("pct"))
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
