"""What the differentiable augmentation (``diff_augment=``, csrc/diff_augment.hip) costs.

  --kernel     forward + backward of `functional.diff_augment` (2 + 2 launches with the colour step) at (128, 3, 64, 64) and
               (64, 3, 256, 256) against the same map composed from ATen ops on the device through autograd (the batched
               fp32 form of tests/_augment_refs.py: means, broadcasts, pad, an index gather, a mask product); legs
               interleaved round by round inside one process, device events around ITER calls per round; launch counts
               from the profiler's kernel events; the fused calls also replayed from a HIP graph.
  (driver)     the B = 128 beta-VAE-GAN iteration on one GPU, one process per leg, legs interleaved round by round:
                 (p) the parent commit (it has no ``diff_augment=``): its captured iteration;
                 (c) this tree without the argument (the parent's launches);
                 (a) this tree, ``diff_augment="color,translation,cutout"``, the uniforms drawn anew every iteration.
               ``--bench-rounds N`` appends N rounds of ``bench.py --gpus 1 --steps 40 --warmup 5`` in the parent checkout
               and in this tree, the order of the two swapped from round to round.

    diff_augment_timing.py --parent-tree DIR [--out profiles/r22_diff_augment.json] [--rounds 5] [--bench-rounds 3]
    diff_augment_timing.py --kernel | --leg p|c|a --tree DIR        (one JSON line each: what the driver starts)

Without ``--parent-tree`` the leg (p) runs on this tree without the new argument and the result says so."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED = 128, 10, 50
POLICY = "color,translation,cutout"
K_ROUNDS, K_ITER = 7, 100


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def aten_augment(x, u):
    """The full policy at p = 1 composed from ATen ops, batched, fp32, differentiable in x."""
    import torch
    Bn, C, H, W = x.shape
    b, s, c = (u[:, k].view(Bn, 1, 1, 1) for k in range(3))
    x = x + (b - 0.5)
    xbar = x.mean(dim=1, keepdim=True)
    x = (x - xbar) * (2.0 * s) + xbar
    m = x.mean(dim=(1, 2, 3), keepdim=True)
    x = (x - m) * (c + 0.5) + m
    rh, rw = int(H / 8 + 0.5), int(W / 8 + 0.5)
    tr = torch.clamp(torch.floor(u[:, 3] * (2 * rh + 1)), max=2 * rh).long() - rh
    tc = torch.clamp(torch.floor(u[:, 4] * (2 * rw + 1)), max=2 * rw).long() - rw
    gi = torch.arange(H, device=x.device).view(1, H, 1) + tr.view(Bn, 1, 1) + rh
    gj = torch.arange(W, device=x.device).view(1, 1, W) + tc.view(Bn, 1, 1) + rw
    xp = torch.nn.functional.pad(x, (rw, rw, rh, rh))
    bi = torch.arange(Bn, device=x.device).view(Bn, 1, 1)
    x = xp.permute(0, 2, 3, 1)[bi, gi, gj].permute(0, 3, 1, 2)
    kh, kw = int(H / 2 + 0.5), int(W / 2 + 0.5)
    nh, nw = H + 1 - kh % 2, W + 1 - kw % 2
    orow = torch.clamp(torch.floor(u[:, 5] * nh), max=nh - 1).long().view(Bn, 1, 1)
    ocol = torch.clamp(torch.floor(u[:, 6] * nw), max=nw - 1).long().view(Bn, 1, 1)
    i, j = torch.arange(H, device=x.device).view(1, H, 1), torch.arange(W, device=x.device).view(1, 1, W)
    cut = (i >= orow - kh // 2) & (i <= orow - kh // 2 + kh - 1) & (j >= ocol - kw // 2) & (j <= ocol - kw // 2 + kw - 1)
    return x * (~cut).unsqueeze(1).to(x.dtype)


def run_kernel():
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("diff_augment_timing.py measures on the GPU; none found")
    out = {}
    for shape in ((128, 3, 64, 64), (64, 3, 256, 256)):
        g = torch.Generator().manual_seed(0)
        x = (2 * torch.rand(*shape, generator=g) - 1).cuda().requires_grad_(True)
        gy = (2 * torch.rand(*shape, generator=g) - 1).cuda()
        u = torch.rand(shape[0], 8, generator=g).cuda()

        def fused():
            x.grad = None
            F.diff_augment(x, u, POLICY, 1.0).backward(gy)

        def aten():
            x.grad = None
            aten_augment(x, u).backward(gy)

        legs = {"fused": fused, "aten": aten}
        grads, launches = {}, {}
        for name, fn in legs.items():
            for _ in range(3):
                fn()
            grads[name] = x.grad.clone()
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
        graph = torch.cuda.CUDAGraph()                             # the kernels alone: what one graphed iteration pays per use
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
        nbytes = 4 * x.numel()
        out["x".join(map(str, shape))] = {
            "fused_us": summary(us["fused"]), "aten_us": summary(us["aten"]), "fused_captured_us": summary(cap),
            "aten_over_fused_of_medians": round(med["aten"] / med["fused"], 2),
            "fused_is_faster_in_every_round": all(f < a for f, a in zip(us["fused"], us["aten"])),
            "kernel_launches_forward_plus_backward": launches,
            "bytes_moved_at_least": 6 * nbytes,      # each way: the sum pass reads the tensor, the apply pass reads and writes it
            "captured_GBps_of_that": round(6 * nbytes / (statistics.median(cap) * 1e-6) / 1e9, 1),
            "gradients_agree_max_abs": float((grads["fused"] - grads["aten"]).abs().max())}
    print(json.dumps({"kernel": out}), flush=True)


def run_leg(leg, tree):
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(tree)
    if not torch.cuda.is_available():
        raise SystemExit("diff_augment_timing.py measures on the GPU; none found")
    replays = {"n": 0}
    real = T._CapturedIteration.replay

    def counted(self, *a, **k):
        replays["n"] += 1
        return real(self, *a, **k)

    T._CapturedIteration.replay = counted
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).cuda()
    lat = [torch.randn(B, 128, generator=gen).cuda() for _ in range(3)]
    tr = T.BetaVAEGANTrainer(graph=True, **(dict(diff_augment=POLICY) if leg == "a" else {}))
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
                      "mse_enc_end": float(out["mse_enc"]), "D_x_mean_end": float(out["D_x_sum"]) / B}), flush=True)


def child(cmd, cwd=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{' '.join(cmd)} failed with status {p.returncode}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def drive(parent, out_path, rounds, bench_rounds):
    me = os.path.abspath(__file__)
    out = {"what": "the differentiable augmentation as fused kernels (csrc/diff_augment.hip) against the same map composed from "
                   f"ATen ops, and the B = 128 beta-VAE-GAN iteration with diff_augment=\"{POLICY}\" / without it / on the "
                   "parent commit",
           "device": "one MI355X (gfx950), default arithmetic",
           "kernel_method": f"one process; {K_ROUNDS} rounds, the legs interleaved, each figure {K_ITER} forward + backward "
                            "calls between two device events (host launches included); fused_captured_us: the same "
                            "fused calls replayed from a HIP graph",
           "iteration_method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then "
                               f"{TIMED} timed by a host clock ending in a device synchronise; a fixed batch",
           "not_measured": "whether the option keeps D(x) away from 1.0 on real data (a training result); data parallel; "
                           "rocprofv3 kernel times",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new argument (no parent checkout was given)"}
    out.update(child([sys.executable, me, "--kernel"]))
    print(json.dumps(out["kernel"]), flush=True)
    trees = {"p": parent or HERE, "c": HERE, "a": HERE}
    names = {"p": "parent", "c": "this tree, no diff_augment", "a": f"this tree, diff_augment=\"{POLICY}\""}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            res = child([sys.executable, me, "--leg", leg, "--tree", tree])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:56s}: {res['ms_per_iteration']:8.3f} ms  "
                  f"{res['replayed']}/{res['timed_iterations']} replayed, {res['captures']} capture(s)", flush=True)
    out["legs"] = {}
    for leg, rs in runs.items():
        out["legs"][leg] = {"name": names[leg], "images_per_s": summary([r["images_per_s"] for r in rs]),
                            "ms_per_iteration": summary([r["ms_per_iteration"] for r in rs], 3),
                            "replayed_of_timed": [r["replayed"] for r in rs], "captures_alive": [r["captures"] for r in rs],
                            "mse_enc_of_the_last_timed_step": sorted({r["mse_enc_end"] for r in rs}),
                            "D_x_mean_of_the_last_timed_step": sorted({r["D_x_mean_end"] for r in rs})}
    ms = {k: [r["ms_per_iteration"] for r in rs] for k, rs in runs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    out["comparison"] = {
        "no_option_minus_parent_ms_of_medians": round(med["c"] - med["p"], 3),
        "same_leg_spread_ms": spread,
        "no_option_median_inside_the_parents_range": bool(min(ms["p"]) <= med["c"] <= max(ms["p"])),
        "no_option_agrees_with_parent_within_spread": bool(abs(med["c"] - med["p"]) <= max(spread["p"], spread["c"])),
        "no_option_computes_what_the_parent_computes": {r["mse_enc_end"] for r in runs["c"]} == {r["mse_enc_end"] for r in runs["p"]},
        "option_minus_parent_ms_of_medians": round(med["a"] - med["p"], 3),
        "option_minus_parent_ms_per_round": [round(a - p, 3) for a, p in zip(ms["a"], ms["p"])],
        "option_minus_no_option_ms_of_medians": round(med["a"] - med["c"], 3),
        "option_over_parent_of_medians": round(med["a"] / med["p"], 4)}
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
                                         "commit (diff_augment at its default), one process each, the order swapped from "
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
    ap.add_argument("--leg", choices=list("pca"))
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
