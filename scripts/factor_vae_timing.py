"""What FactorVAE (``factor_vae=``, csrc/factor_vae.hip) costs.

  --kernel     `ops.permute_dims` at (128, 128) and (1024, 128) against the ATen composition it replaces -- the uniforms
               given, ``argsort(stable)`` + ``gather`` --, and the two loss kernels (`functional.factor_tc`,
               `functional.factor_critic_loss`, forward + backward) against their ATen compositions through autograd; legs
               interleaved round by round inside one process, device events around ITER calls per round; every leg also
               replayed from a HIP graph; launch counts from the profiler's kernel events.
  (driver)     the B = 128 beta-VAE-GAN iteration on one GPU, one process per leg, legs interleaved round by round:
                 (p) the parent commit (it has no ``factor_vae=``): its captured iteration;
                 (c) this tree without the argument (the parent's launches);
                 (f) this tree, ``factor_vae=6.4`` (Kim & Mnih's critic: width 1000, depth 6), the uniforms of
                     ``permute_dims`` drawn anew every iteration; after the timed iterations ONE eager iteration under the
                     profiler gives the device time of the critic phase's kernels and of the whole iteration's.

    factor_vae_timing.py --parent-tree DIR [--out profiles/r23_factor_vae.json] [--rounds 5]
    factor_vae_timing.py --kernel | --leg p|c|f --tree DIR        (one JSON line each: what the driver starts)

Without ``--parent-tree`` the leg (p) runs on this tree without the new argument and the result says so."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED = 128, 10, 50
GAMMA = 6.4
K_ROUNDS, K_ITER = 7, 100


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def _launches(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                         # the count is a report, not the measurement
        return f"not counted ({type(e).__name__})"


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(K_ITER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / K_ITER


def compare(legs):
    """``legs``: name -> callable.  Eager and graph-replayed microseconds per call, the legs interleaved, and launch counts."""
    import torch
    for fn in legs.values():
        for _ in range(3):
            fn()
    launches = {name: _launches(fn) for name, fn in legs.items()}
    graphs = {}
    for name, fn in legs.items():
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fn()
    eager, replayed = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(K_ROUNDS):
        for name, fn in legs.items():
            eager[name].append(_timed(fn))
        for name in legs:
            replayed[name].append(_timed(graphs[name].replay))
    names = list(legs)
    med = {k: statistics.median(v) for k, v in replayed.items()}
    return {"eager_us": {k: summary(v) for k, v in eager.items()}, "replayed_us": {k: summary(v) for k, v in replayed.items()},
            "kernel_launches": launches,
            f"{names[1]}_over_{names[0]}_replayed_of_medians": round(med[names[1]] / med[names[0]], 2),
            f"{names[0]}_is_faster_replayed_in_every_round": all(a < b for a, b in zip(replayed[names[0]], replayed[names[1]]))}


def run_kernel():
    sys.path.insert(0, HERE)
    import torch
    import torch.nn.functional as tF
    from disentangle_mlp_amd import functional as F, ops
    if not torch.cuda.is_available():
        raise SystemExit("factor_vae_timing.py measures on the GPU; none found")
    out = {}
    g = torch.Generator().manual_seed(0)
    for shape in ((128, 128), (1024, 128)):
        z, u = torch.randn(*shape, generator=g).cuda(), torch.rand(*shape, generator=g).cuda()
        res = compare({"fused": lambda: ops.permute_dims(z, u),
                       "aten": lambda: z.gather(0, torch.argsort(u, dim=0, stable=True))})
        res["results_are_equal"] = bool(torch.equal(ops.permute_dims(z, u), z.gather(0, torch.argsort(u, dim=0, stable=True))))
        res["the_uniforms"] = "given to both legs; drawing them (one launch) is the same in both and not timed"
        out["permute_dims_" + "x".join(map(str, shape))] = res
    for rows in (128, 1024):
        logits = (3 * torch.randn(rows, 2, generator=g)).cuda().requires_grad_(True)
        kl = torch.full((), 37.25, device="cuda", requires_grad=True)

        def tc_fused():
            logits.grad = kl.grad = None
            F.factor_tc(logits, kl, 4.0, GAMMA)[0].backward()

        def tc_aten():
            logits.grad = kl.grad = None
            (4.0 * kl + GAMMA * (logits[:, 0] - logits[:, 1]).sum()).backward()

        out[f"factor_tc_B{rows}"] = compare({"fused": tc_fused, "aten": tc_aten})
        both = (3 * torch.randn(2 * rows, 2, generator=g)).cuda().requires_grad_(True)
        labels = (torch.arange(2 * rows, device="cuda") >= rows).long()

        def critic_fused():
            both.grad = None
            F.factor_critic_loss(both, 2.0 * rows)[0].backward()

        def critic_aten():
            both.grad = None
            loss = tF.cross_entropy(both, labels, reduction="sum") / (2.0 * rows)
            (both.detach().argmax(1) == labels).float().mean()      # the accuracy the fused launch also returns
            loss.backward()

        out[f"factor_critic_loss_B{rows}"] = compare({"fused": critic_fused, "aten": critic_aten})
    print(json.dumps({"kernel": out}), flush=True)


def _critic_phase_profile(tr, x, lat):
    """Device time of the kernels of ONE eager iteration, and of those its critic phase launched (profiler kernel events)."""
    import torch
    from torch.profiler import ProfilerActivity, profile, record_function
    inner = tr._owned_phase

    def marked(*a, **k):
        with record_function("critic_phase"):
            return inner(*a, **k)

    tr._owned_phase, graph = marked, tr.graph
    tr.graph = False
    try:
        tr.step(x, *lat)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            with record_function("iteration"):
                tr.step(x, *lat)
            torch.cuda.synchronize()
    finally:
        tr._owned_phase, tr.graph = inner, graph
    dev = lambda e: float(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))      # noqa: E731
    avg = {e.key: e for e in prof.key_averages()}
    kernels = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {"critic_phase_kernel_us": round(dev(avg["critic_phase"]), 1), "iteration_kernel_us": round(dev(avg["iteration"]), 1),
            "iteration_kernel_launches": sum(e.count for e in kernels),
            "method": "one eager iteration under torch.profiler; the sums of the device durations of the kernels launched "
                      "inside the critic phase / the whole iteration (host-paced: gaps between kernels are not in the sums)"}


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    if not torch.cuda.is_available():
        raise SystemExit("factor_vae_timing.py measures on the GPU; none found")
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    tr = T.BetaVAEGANTrainer(graph=True, **(dict(factor_vae=GAMMA) if leg == "f" else {}))
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
           "replayed": replays["n"] - r0, "captures": len(tr._graphs), "mse_enc_end": float(out["mse_enc"]),
           "kld_end": float(out["kld"])}
    if leg == "f":
        res.update(critic_loss_end=float(out["critic_loss"]), critic_acc_end=float(out["critic_acc"]), tc_end=float(out["tc"]))
        try:
            res["profile"] = _critic_phase_profile(tr, x, lat)
        except Exception as e:                                     # a report beside the measurement
            res["profile"] = f"not taken ({type(e).__name__}: {e})"
    print(json.dumps(res), flush=True)


def child(cmd, cwd=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{' '.join(cmd)} failed with status {p.returncode}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def drive(parent, out_path, rounds):
    me = os.path.abspath(__file__)
    out = {"what": "FactorVAE's kernels (csrc/factor_vae.hip) against the ATen compositions they replace, and the B = 128 "
                   f"beta-VAE-GAN iteration with factor_vae={GAMMA} (critic: width 1000, depth 6) / without it / on the parent commit",
           "device": "one MI355X (gfx950), default arithmetic",
           "kernel_method": f"one process; {K_ROUNDS} rounds, the legs interleaved, each figure {K_ITER} calls between two device "
                            "events: eager (host launches included) and replayed from a HIP graph; the loss kernels forward + "
                            "backward through autograd",
           "iteration_method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then "
                               f"{TIMED} timed by a host clock ending in a device synchronise; a fixed batch",
           "not_measured": "whether FactorVAE disentangles CelebA better than beta-TCVAE here (a training result: nobody has "
                           "measured it); data parallel; rocprofv3 kernel times",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new argument (no parent checkout was given)"}
    out.update(child([sys.executable, me, "--kernel"]))
    print(json.dumps(out["kernel"]), flush=True)
    trees = {"p": parent or HERE, "c": HERE, "f": HERE}
    names = {"p": "parent", "c": "this tree, no factor_vae", "f": f"this tree, factor_vae={GAMMA}"}
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
                            "mse_enc_of_the_last_timed_step": sorted({r["mse_enc_end"] for r in rs})}
    out["legs"]["f"].update(critic_phase=[r["profile"] for r in runs["f"]],
                            critic_acc_of_the_last_timed_step=sorted({r["critic_acc_end"] for r in runs["f"]}),
                            critic_loss_of_the_last_timed_step=sorted({r["critic_loss_end"] for r in runs["f"]}))
    ms = {k: [r["ms_per_iteration"] for r in rs] for k, rs in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["comparison"] = {
        "no_option_minus_parent_ms_of_medians": round(med["c"] - med["p"], 3),
        "same_leg_spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
        "no_option_median_inside_the_parents_range": bool(min(ms["p"]) <= med["c"] <= max(ms["p"])),
        "no_option_computes_what_the_parent_computes": {r["mse_enc_end"] for r in runs["c"]} == {r["mse_enc_end"] for r in runs["p"]},
        "option_minus_no_option_ms_of_medians": round(med["f"] - med["c"], 3),
        "option_minus_parent_ms_per_round": [round(a - p, 3) for a, p in zip(ms["f"], ms["p"])],
        "option_over_parent_of_medians": round(med["f"] / med["p"], 4)}
    print(json.dumps(out["comparison"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--leg", choices=list("pcf"))
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.kernel:
        run_kernel()
    elif a.leg:
        run_leg(a.leg, os.path.abspath(a.tree))
    else:
        drive(os.path.abspath(a.parent_tree) if a.parent_tree else None, a.out, a.rounds)
