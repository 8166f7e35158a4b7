"""What the aggregate-posterior log-sum-exps (`ops.agg_posterior_lse`, csrc/agg_posterior.hip) cost.

  vs ATen      (M, N, D) = (16384, 16384, 128) and (4096, 65536, 128): the six launches of the fused sequence against the
               same two outputs composed from ATen ops on the device -- the per-row constants formed once, the pair terms
               of a chunk of points against a chunk of rows built in place ([cm, cn, D] fp32, sized to CHUNK_ELEMS),
               `logsumexp` over the rows of each chunk, the chunks of rows merged with `logaddexp`.  Legs interleaved
               round by round inside one process, device events around each call; launch counts from the profiler's
               kernel events.
  vs reparam_tc  (1024, 1024, 128) beside `ops.reparam_tc_fwd` at B = 1024, D = 128 (the same pair terms plus the
               reparameterisation and the per-sample parts): time per pair term, for orientation.
  vs v_exp_f32   the achieved pair terms per second as a fraction of the rate one exponential per term allows: CUs x 4
               SIMDs x 64 lanes / 8 cycles of issue x 2.4 GHz, figures of MI355X_MICROARCH.md (256 CUs;
               the constants table's row 'vector-instruction ISSUE cost': v_exp_f32 8 cycles; 2.4 GHz) -- taken from
               there, not measured by a loop of this script.

    latent_metrics_timing.py [--out profiles/r16_latent_metrics.json] [--rounds 5]
"""
import argparse, json, math, os, statistics, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((16384, 16384, 128), (4096, 65536, 128))
CHUNK_ELEMS = 1 << 28                       # 1 GiB of fp32 pair terms per chunk
LOG_2PI = math.log(2.0 * math.pi)
EXP_PER_S = 256 * 4 * 64 / 8 * 2.4e9        # one v_exp_f32 per pair term, every SIMD issuing nothing else


def summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd), "runs": [round(x, nd) for x in v]}


def aten_lse(z, mu, lv):
    """The two log-sum-exps from ATen ops: (lse_joint fp64 [M], lse_dim fp32 [M, D])."""
    import torch
    (M, D), N = z.shape, mu.shape[0]
    a, c = -0.5 * torch.exp(-lv), -0.5 * (LOG_2PI + lv)                    # once per row
    cn = min(N, max(1, CHUNK_ELEMS // (64 * D)))
    cm = max(1, CHUNK_ELEMS // (cn * D))
    joint, dim = torch.empty(M, dtype=torch.float64, device=z.device), torch.empty(M, D, device=z.device)
    for i0 in range(0, M, cm):
        zi, lj, ld = z[i0:i0 + cm, None, :], None, None
        for j0 in range(0, N, cn):
            lq = (zi - mu[None, j0:j0 + cn]).square_().mul_(a[None, j0:j0 + cn]).add_(c[None, j0:j0 + cn])
            pj, pd = torch.logsumexp(lq.sum(2, dtype=torch.float64), dim=1), torch.logsumexp(lq, dim=1)
            lj, ld = (pj, pd) if lj is None else (torch.logaddexp(lj, pj), torch.logaddexp(ld, pd))
        joint[i0:i0 + cm], dim[i0:i0 + cm] = lj, ld
    return joint, dim


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


def main(out_path, rounds):
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("latent_metrics_timing.py measures on the GPU; none found")
    out = {"what": "log-density of M points under the aggregate posterior of N diagonal Gaussians, jointly and per "
                   "dimension: the fused sequence of csrc/agg_posterior.hip against the same outputs composed from ATen ops",
           "device": "one MI355X (gfx950)",
           "method": f"one process; {rounds} rounds, the legs interleaved, one call between two device events per figure "
                     "(host launches included); ms",
           "exp_rate_per_s": EXP_PER_S,
           "exp_rate_source": "MI355X_MICROARCH.md: 256 CUs, constants table row 'vector-instruction ISSUE cost' "
                              "(v_exp_f32 8 cycles per wavefront instruction), 2.4 GHz; not measured here",
           "shapes": {}}

    def rnd(n, d, gen):
        return torch.randn(n, d, device="cuda", generator=gen)

    for M, N, D in SHAPES:
        g = torch.Generator("cuda").manual_seed(M + N)
        mu, lv = rnd(N, D, g), (rnd(N, D, g) * 1.5 - 1.0).clamp_(-6.0, 2.0)
        rows = torch.arange(M, device="cuda") % N
        z = (mu[rows] + rnd(M, D, g) * torch.exp(0.5 * lv[rows])).contiguous()
        legs = {"fused": lambda: ops.agg_posterior_lse(z, mu, lv), "aten": lambda: aten_lse(z, mu, lv)}
        res = {k: fn() for k, fn in legs.items()}                           # (warm-up: allocator, workspace)
        torch.cuda.synchronize()
        agree = [float((res["fused"][n].double() - res["aten"][n].double()).abs().max()
                       / res["aten"][n].double().abs().max()) for n in (0, 1)]
        del res
        counts = {k: launches_of(fn) for k, fn in legs.items()}
        ms = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                ms[k].append(timed_ms(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spreads = sum(max(v) - min(v) for v in ms.values())
        terms = float(M) * N * D
        out["shapes"][f"{M}x{N}x{D}"] = {
            "splits_chosen": ops.agg_posterior_splits(M, N, D), "fused_ms": summary(ms["fused"]), "aten_ms": summary(ms["aten"]),
            "kernel_launches": counts, "aten_over_fused_of_medians": round(med["aten"] / med["fused"], 2),
            "fused_faster_by_more_than_both_spreads": bool(med["aten"] - med["fused"] > spreads),
            "outputs_agree_rel": agree, "pair_terms": terms,
            "fused_pair_terms_per_s": terms / (1e-3 * med["fused"]),
            "fraction_of_exp_rate": round(terms / (1e-3 * med["fused"]) / EXP_PER_S, 4)}
        print(json.dumps({f"{M}x{N}x{D}": out["shapes"][f"{M}x{N}x{D}"]}), flush=True)
        del mu, lv, z
        torch.cuda.empty_cache()

    B, D = 1024, 128
    g = torch.Generator("cuda").manual_seed(1)
    mu, lv, eps = rnd(B, D, g), (rnd(B, D, g) * 1.5 - 1.0).clamp_(-6.0, 2.0), rnd(B, D, g)
    z = (mu + eps * torch.exp(0.5 * lv)).contiguous()
    legs = {"agg_posterior_lse": lambda: ops.agg_posterior_lse(z, mu, lv),
            "reparam_tc_fwd": lambda: ops.reparam_tc_fwd(mu, lv, eps, 6.0, 1.0, 1.0, math.log(B * 162770))}
    for fn in legs.values():
        fn()
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            us[k].append(1e3 * timed_ms(lambda: [fn() for _ in range(20)]) / 20)
    out["beside_reparam_tc_fwd_at_1024x1024x128"] = {
        "us_per_call": {k: summary(v, 1) for k, v in us.items()},
        "ps_per_pair_term": {k: round(1e6 * statistics.median(v) / (B * B * D), 3) for k, v in us.items()},
        "note": "reparam_tc_fwd also reparameterises and forms the per-sample parts; 20 calls between two events per figure"}
    print(json.dumps(out["beside_reparam_tc_fwd_at_1024x1024x128"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    main(a.out, a.rounds)
