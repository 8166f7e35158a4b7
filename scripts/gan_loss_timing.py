"""What the adversarial losses on the logit (``gan_loss=``, csrc/gan_loss.hip) cost and do.

  --head       (a) forward + backward of the fused head per kind at (B, K) = (128, 2048) and (256, 2048) -- `ops.dot_gan_loss_fwd`
               then `ops.dot_sigmoid_bce_bwd` -- against the existing pair `ops.dot_sigmoid_bce_fwd` / `_bwd`, eager and
               replayed from a HIP graph; legs interleaved round by round inside one process, device events around ITER
               calls per round.  Both read the same 1 MB (2 MB) of features once each way.
  --leg        (b) the B = 128 beta-VAE-GAN iteration on one GPU, one process per leg, legs interleaved round by round:
                 (p) the parent commit (it has no ``gan_loss=``): its captured iteration;
                 (c) this tree without the keyword (the parent's launches);
                 (a) this tree, ``gan_loss="logistic"``.
               Each leg also prints SHA-256 digests of the last step's outputs and of the final weights: (c) against (p) is
               the bit-neutrality record of the default path.
  --regime     (c) on the benchmark's fixed batch (seed 999, generator 1234, labels 0.9 / 0.1), after 5 + 20 iterations from
               the initial weights: one probed (eager) iteration's fraction of exact zeros in ``grad_wrt_fake`` and
               ``D_x_sum / B``, for the default and for each loss.  A training observation; no threshold.
  (driver)     all of the above, and `scripts/objective_bits.py` on this tree and on the parent: the count of equal digests.

    gan_loss_timing.py --parent-tree DIR [--out profiles/r24_gan_loss.json] [--rounds 3]
    gan_loss_timing.py --head | --leg p|c|a --tree DIR | --regime none|logistic|hinge|lsgan      (one JSON line each)

Without ``--parent-tree`` the leg (p) runs on this tree without the keyword and the result says so."""
import argparse, hashlib, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, WARM, TIMED = 128, 10, 50
H_ROUNDS, H_ITER = 7, 200
KINDS = {"logistic": 0, "lsgan": 1, "hinge_real": 2, "hinge_fake": 3, "hinge_gen": 4}
REGIME_WARMUP, REGIME_STEPS = 5, 20


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "runs": [round(x, nd) for x in v]}


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes()).hexdigest()


def need_gpu(torch):
    if not torch.cuda.is_available():
        raise SystemExit("gan_loss_timing.py measures on the GPU; none found")


def run_head():
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd import ops
    need_gpu(torch)
    out = {}
    for Bn, K in ((128, 2048), (256, 2048)):
        g = torch.Generator().manual_seed(0)
        feat = torch.nn.functional.leaky_relu(torch.randn(Bn, K, generator=g), 0.2).cuda()
        w = (torch.randn(1, K, generator=g) * (1.5 / K ** 0.5)).cuda()
        bias = torch.tensor([0.25]).cuda()
        lab = torch.tensor([0.9], device="cuda")
        one = torch.ones((), device="cuda")

        def bce():
            _, _, d = ops.dot_sigmoid_bce_fwd(feat, w, bias, lab)
            ops.dot_sigmoid_bce_bwd(d, one, feat, w)

        def new(kind):
            def fn():
                _, _, _, d = ops.dot_gan_loss_fwd(feat, w, bias, kind, lab)
                ops.dot_sigmoid_bce_bwd(d, one, feat, w)
            return fn

        legs = {"dot_sigmoid_bce": bce, **{name: new(kind) for name, kind in KINDS.items()}}
        graphs = {}
        for name, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                fn()
        eager, cap = {k: [] for k in legs}, {k: [] for k in legs}

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(H_ITER):
                call()
            b.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b) / H_ITER

        for _ in range(H_ROUNDS):
            for name, fn in legs.items():
                eager[name].append(timed(fn))
            for name in legs:
                cap[name].append(timed(graphs[name].replay))
        base_e, base_c = statistics.median(eager["dot_sigmoid_bce"]), statistics.median(cap["dot_sigmoid_bce"])
        spread = lambda v: round((max(v) - min(v)) / statistics.median(v), 4)      # noqa: E731
        res = {"bytes_read_each_way": 4 * Bn * K}
        for name in legs:
            res[name] = {"eager_us": summary(eager[name]), "captured_us": summary(cap[name]),
                         "eager_over_bce_of_medians": round(statistics.median(eager[name]) / base_e, 4),
                         "captured_over_bce_of_medians": round(statistics.median(cap[name]) / base_c, 4),
                         "captured_spread_of_median": spread(cap[name])}
        out[f"{Bn}x{K}"] = res
    print(json.dumps({"head": out}), flush=True)


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
    tr = T.BetaVAEGANTrainer(graph=True, **(dict(gan_loss="logistic") if leg == "a" else {}))
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
    print(json.dumps({"leg": leg, "images_per_s": B * TIMED / dt, "ms_per_iteration": 1e3 * dt / TIMED,
                      "timed_iterations": TIMED, "replayed": replays["n"] - r0, "captures": len(tr._graphs),
                      "mse_enc_end": float(out["mse_enc"]), "D_x_mean_end": float(out["D_x_sum"]) / B,
                      "digests": digests}), flush=True)


def run_regime(loss):
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
    need_gpu(torch)
    tr = BetaVAEGANTrainer(seed=999, beta=25.0, **({} if loss == "none" else dict(gan_loss=loss)))
    g = torch.Generator().manual_seed(1234)                      # bench.py's batch
    data = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1).cuda()
    noise = [torch.randn(B, 128, generator=g).cuda() for _ in range(3)]
    for _ in range(REGIME_WARMUP + REGIME_STEPS):
        out = tr.step(data, *noise, real_label=0.9, fake_label=0.1)
    res = {"loss": loss, "iterations_since_initial_weights": REGIME_WARMUP + REGIME_STEPS,
           "D_x_mean_last_step": float(out["D_x_sum"]) / B}
    if "D_logit_real_sum" in out:
        res["D_logit_real_mean_last_step"] = float(out["D_logit_real_sum"]) / B
        res["D_logit_fake_mean_last_step"] = float(out["D_logit_fake_sum"]) / B

    def probe(name, gten):
        if name == "grad_wrt_fake":
            res["grad_wrt_fake_zero_fraction"] = float((gten == 0).float().mean())
            res["grad_wrt_fake_absmax"] = float(gten.abs().max())

    tr.probe = probe
    out = tr.step(data, *noise, real_label=0.9, fake_label=0.1)
    tr.probe = None
    res["D_x_mean_probed_step"] = float(out["D_x_sum"]) / B
    res["errG_fake_probed_step"] = float(out["errG_fake"])
    print(json.dumps({"regime": res}), flush=True)


def child(cmd, cwd=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{' '.join(cmd)} failed with status {p.returncode}")
    return p.stdout


def child_json(cmd, cwd=None):
    return json.loads([ln for ln in child(cmd, cwd).splitlines() if ln.startswith("{")][-1])


def flat(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from flat(v, f"{prefix}{k}/")
        else:
            yield prefix + k, v


def drive(parent, out_path, rounds):
    me = os.path.abspath(__file__)
    out = {"what": "the adversarial losses on the logit (csrc/gan_loss.hip): the fused head per kind against the existing "
                   "dot_sigmoid_bce pair, the B = 128 beta-VAE-GAN iteration with gan_loss=\"logistic\" / without the keyword / "
                   "on the parent commit, the regime on the benchmark's batch, and the default path's digests against the parent",
           "device": "one MI355X (gfx950), default arithmetic",
           "head_method": f"one process; {H_ROUNDS} rounds, the legs interleaved, each figure {H_ITER} forward + backward calls "
                          "between two device events: eager (host launches included) and replayed from a HIP graph",
           "iteration_method": f"{rounds} interleaved rounds, one process per leg and round; {WARM} warm-up iterations, then "
                               f"{TIMED} timed by a host clock ending in a device synchronise; a fixed batch",
           "not_measured": "whether any of the losses trains CelebA better (FID, a real data set): the regime record is "
                           f"{REGIME_WARMUP + REGIME_STEPS} iterations on one synthetic batch; data parallel; rocprofv3 kernel times",
           "parent_is": "another checkout of the parent commit" if parent else
                        "THIS tree without the new keyword (no parent checkout was given)"}
    out.update(child_json([sys.executable, me, "--head"]))
    for shape, res in out["head"].items():
        print(shape, {k: (v["captured_us"]["median"], v["captured_over_bce_of_medians"]) for k, v in res.items() if isinstance(v, dict)},
              flush=True)
    trees = {"p": parent or HERE, "c": HERE, "a": HERE}
    names = {"p": "parent", "c": "this tree, no gan_loss", "a": "this tree, gan_loss=\"logistic\""}
    runs = {k: [] for k in trees}
    for r in range(rounds):
        for leg, tree in trees.items():
            res = child_json([sys.executable, me, "--leg", leg, "--tree", tree])
            runs[leg].append(res)
            print(f"round {r} ({leg}) {names[leg]:36s}: {res['ms_per_iteration']:8.3f} ms  "
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
    dp, dc = runs["p"][0]["digests"], runs["c"][0]["digests"]
    out["comparison"] = {
        "no_keyword_minus_parent_ms_of_medians": round(med["c"] - med["p"], 3),
        "same_leg_spread_ms": spread,
        "no_keyword_median_inside_the_parents_range": bool(min(ms["p"]) <= med["c"] <= max(ms["p"])),
        "no_keyword_median_outside_the_parents_range_by_ms":
            round(max(min(ms["p"]) - med["c"], med["c"] - max(ms["p"]), 0.0), 3),
        "keyword_minus_no_keyword_ms_of_medians": round(med["a"] - med["c"], 3),
        "keyword_minus_parent_ms_per_round": [round(a - p, 3) for a, p in zip(ms["a"], ms["p"])],
        "keyword_over_no_keyword_of_medians": round(med["a"] / med["c"], 4),
        "iteration_digests_no_keyword_vs_parent": {"compared": len(dp), "equal": sum(dc.get(k) == v for k, v in dp.items()),
                                                   "every_run_of_a_leg_agrees_with_its_first":
                                                       all(r["digests"] == rs[0]["digests"] for rs in runs.values() for r in rs)}}
    print(json.dumps(out["comparison"]), flush=True)
    out["regime"] = {}
    for loss in ("none", "logistic", "hinge", "lsgan"):
        out["regime"][loss] = child_json([sys.executable, me, "--regime", loss])["regime"]
        print("regime", json.dumps(out["regime"][loss]), flush=True)
    bits = os.path.join(HERE, "scripts", "objective_bits.py")
    here = json.loads(child([sys.executable, bits, "--tree", HERE]))
    there = json.loads(child([sys.executable, bits, "--tree", parent or HERE]))
    a, b = dict(flat(here)), dict(flat(there))
    out["objective_bits_no_keyword_vs_parent"] = {"script": "scripts/objective_bits.py", "digests_compared": len(b),
                                                  "digests_equal": sum(a.get(k) == v for k, v in b.items()),
                                                  "sha256_of_all": [here["sha256_of_all"], there["sha256_of_all"]]}
    print(json.dumps(out["objective_bits_no_keyword_vs_parent"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", action="store_true")
    ap.add_argument("--leg", choices=list("pca"))
    ap.add_argument("--regime", choices=["none", "logistic", "hinge", "lsgan"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.head:
        run_head()
    elif a.leg:
        run_leg(a.leg, os.path.abspath(a.tree))
    elif a.regime:
        run_regime(a.regime)
    else:
        drive(os.path.abspath(a.parent_tree) if a.parent_tree else None, a.out, a.rounds)
