"""What the sample-quality metrics (`ops.pair_knn` / `ops.pair_hits`, csrc/pair_dist.hip; `sample_quality.report`) cost.

  vs ATen      (M, N, D) = (10000, 10000, 2048) and (50000, 50000, 2048): `pair_knn` (K = 5, self-excluded), `pair_hits`
               and the whole `report` (KID off: it is the same fp64 matmuls on either side) against the same outputs
               composed from ATen ops on the device -- `torch.cdist` of a chunk of rows against all columns ([cm, N]
               fp32, sized to CHUNK_ELEMS, or to DIFF_CHUNK_ELEMS where `torch.cdist`'s own launch allows no more), squared, the diagonal of a self chunk set to +inf, `topk` / a comparison
               and a sum.  Two ATen legs, because `torch.cdist` has two arithmetics: "diff" (compute_mode
               donot_use_mm_for_euclid_dist: from the differences, what the fused kernels compute) and "mm" (its default
               at these sizes: |a|^2 + |b|^2 - 2 a.b on the matrix cores -- the Gram form the metrics must not use,
               identical rows do not come out as 0; timed for orientation).  Legs interleaved round by round inside
               one process, device events around each call; launch counts from the profiler's kernel events; peak
               memory from the caching allocator, above what was allocated before the call.
  vs the VALU  the achieved pair terms per second as a fraction of the fp32 vector rate at two lane-operations (a
               subtraction, an FMA) per term: 256 CUs x 4 SIMDs x 64 lanes x 2 (packed) / 4 cycles of issue x 2.4 GHz =
               7.86e13 lane-operations per second -- the 157.3 TFLOP/s "vector peak" of MI355X_MICROARCH.md (Matrix cores
               table) with an FMA counted as two -- taken from there, not measured by a loop of this script.

    sample_quality_timing.py [--out profiles/r19_sample_quality.json] [--rounds 5]
"""
import argparse, json, os, statistics, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((10000, 10000, 2048), (50000, 50000, 2048))
CHUNK_ELEMS = 1 << 28                       # 1 GiB of fp32 distances per chunk ...
DIFF_CHUNK_ELEMS = 1 << 23                  # ... but cdist's "diff" kernel launches one 256-thread workgroup per distance, and a
                                            # HIP grid holds fewer than 2^32 threads: larger chunks come back partly unwritten
K = 5
LANE_OPS_PER_S = 256 * 4 * 64 * 2 / 4 * 2.4e9      # v_pk_add_f32 / v_pk_fma_f32: two lanes' worth per lane every 4 cycles


def summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd), "runs": [round(x, nd) for x in v]}


def _chunks(a, b, mode, exclude_self):
    import torch
    cm = max(1, (DIFF_CHUNK_ELEMS if mode.startswith("donot") else CHUNK_ELEMS) // b.shape[0])
    for s in range(0, a.shape[0], cm):
        d = torch.cdist(a[s:s + cm], b, compute_mode=mode).square_()
        if exclude_self:
            n = d.shape[0]
            d[torch.arange(n, device=d.device), torch.arange(s, s + n, device=d.device)] = float("inf")
        yield d


def aten_knn(a, b, k, mode, exclude_self=False):
    import torch
    return torch.cat([d.topk(k, dim=1, largest=False).values for d in _chunks(a, b, mode, exclude_self)])


def aten_hits(a, b, thr, mode):
    import torch
    return torch.cat([(d <= thr[None, :]).sum(1, dtype=torch.int32) for d in _chunks(a, b, mode, False)])


def aten_report(real, fake, mode, k_pr=3, k_dc=5):
    knn_real = aten_knn(real, real, max(k_pr, k_dc), mode, True)
    r_pr, r_dc, r_fake = knn_real[:, k_pr - 1], knn_real[:, k_dc - 1], aten_knn(fake, fake, k_pr, mode, True)[:, k_pr - 1]
    density = aten_hits(fake, real, r_dc, mode).double().sum() / (k_dc * fake.shape[0])
    return {"precision": float((aten_hits(fake, real, r_pr, mode) > 0).double().mean()),
            "recall": float((aten_hits(real, fake, r_fake, mode) > 0).double().mean()), "density": float(density),
            "coverage": float((aten_knn(real, fake, 1, mode)[:, 0] <= r_dc).double().mean())}


def launches_of(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                                  # the count is a report, not the measurement
        return f"not counted ({type(e).__name__})"


def timed_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def peak_mib(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def mixture(n, d, centres, basis, gen):
    """16 clusters with per-row scales in [0.2, 1.5] on a 16-dimensional subspace of the d features: at full rank the
    distances of a 2048-dimensional Gaussian concentrate and every metric is 0."""
    import torch
    which = torch.randint(0, centres.shape[0], (n,), device="cuda", generator=gen)
    scale = 0.2 + 1.3 * torch.rand(n, device="cuda", generator=gen)
    low = centres[which] + scale[:, None] * torch.randn(n, basis.shape[0], device="cuda", generator=gen)
    return (low @ basis).contiguous()


def main(out_path, rounds, sizes=None):
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd import ops, sample_quality
    if not torch.cuda.is_available():
        raise SystemExit("sample_quality_timing.py measures on the GPU; none found")
    out = {"what": "k-NN radii (K = 5, self-excluded), ball-membership counts and the whole precision / recall / density / "
                   "coverage report over all pairs of two feature sets: the fused kernels of csrc/pair_dist.hip against "
                   "the same outputs composed from torch.cdist in row chunks + topk / comparisons",
           "device": "one MI355X (gfx950)",
           "method": f"one process; {rounds} rounds, the legs interleaved, one call between two device events per figure "
                     "(host launches included); ms",
           "lane_ops_per_s": LANE_OPS_PER_S,
           "lane_ops_source": "MI355X_MICROARCH.md: 256 CUs x 4 SIMDs x 64 lanes, packed fp32 (2 per lane) every 4 cycles, "
                              "2.4 GHz (= the 157.3 TFLOP/s vector peak counted in FMAs); not measured here",
           "shapes": {}}
    for M, N, D in (s for s in SHAPES if not sizes or s[0] in sizes):
        g = torch.Generator("cuda").manual_seed(M + N)
        centres, basis = 2.0 * torch.randn(16, 16, device="cuda", generator=g), torch.randn(16, D, device="cuda", generator=g)
        real, fake = mixture(N, D, centres, basis, g), mixture(M, D, centres + 0.3, basis, g)
        thr = ops.pair_knn(real, k=3)[:, 2].contiguous()
        legs = {
            "knn": {"fused": lambda: ops.pair_knn(real, k=K),
                    "aten_diff": lambda: aten_knn(real, real, K, "donot_use_mm_for_euclid_dist", True),
                    "aten_mm": lambda: aten_knn(real, real, K, "use_mm_for_euclid_dist", True)},
            "hits": {"fused": lambda: ops.pair_hits(fake, real, thr),
                     "aten_diff": lambda: aten_hits(fake, real, thr, "donot_use_mm_for_euclid_dist"),
                     "aten_mm": lambda: aten_hits(fake, real, thr, "use_mm_for_euclid_dist")},
            "report": {"fused": lambda: sample_quality.report(real, fake, kid=False),
                       "aten_diff": lambda: aten_report(real, fake, "donot_use_mm_for_euclid_dist"),
                       "aten_mm": lambda: aten_report(real, fake, "use_mm_for_euclid_dist")}}
        pair_terms = {"knn": float(N) * N * D, "hits": float(M) * N * D,
                      "report": (float(N) * N + float(M) * M + 4.0 * M * N) * D}      # 2 k-NN passes, 3 hits, 1 nearest
        res = {"splits_chosen": ops.pair_splits(M, N, D)}
        for what, by_leg in legs.items():
            first = {k: fn() for k, fn in by_leg.items()}                   # (warm-up: allocator, workspace)
            torch.cuda.synchronize()
            if what == "report":
                agree = dict(first)
            else:
                ref = first["aten_diff"].double()      # knn: largest relative difference; hits: rows whose counts differ
                agree = {k: float(((first[k].double() - ref).abs() / ref).max()) if what == "knn"
                         else int((first[k].long() != first["aten_diff"].long()).sum()) for k in ("fused", "aten_mm")}
            del first
            counts = {k: launches_of(fn) for k, fn in by_leg.items()}
            peaks = {k: peak_mib(fn) for k, fn in by_leg.items()}
            ms = {k: [] for k in by_leg}
            for _ in range(rounds):
                for k, fn in by_leg.items():
                    ms[k].append(timed_ms(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rate = pair_terms[what] / (1e-3 * med["fused"])
            res[what] = {
                "ms": {k: summary(v) for k, v in ms.items()}, "kernel_launches": counts, "peak_mib_above_inputs": peaks,
                "aten_diff_over_fused_of_medians": round(med["aten_diff"] / med["fused"], 2),
                "aten_mm_over_fused_of_medians": round(med["aten_mm"] / med["fused"], 2),
                "fused_not_slower_than": {k: bool(med["fused"] <= med[k]) for k in med if k != "fused"},
                "agreement_with_aten_diff": agree, "pair_terms": pair_terms[what], "fused_pair_terms_per_s": rate,
                "fraction_of_valu_rate": round(2.0 * rate / LANE_OPS_PER_S, 4)}
            print(json.dumps({f"{M}x{N}x{D}": {what: res[what]}}), flush=True)
        out["shapes"][f"{M}x{N}x{D}"] = res
        del real, fake, thr
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", help="only these M of SHAPES (default: all)")
    a = ap.parse_args()
    main(a.out, a.rounds, a.sizes)
