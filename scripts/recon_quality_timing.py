"""What the reconstruction-quality kernel (`ops.recon_quality`, csrc/recon_quality.hip) costs, and what the ATen forms get
wrong.

  vs ATen   (B, C, H, W) = (128, 3, 64, 64), (256, 3, 128, 128) and (64, 3, 256, 256): the fused call against the same
            three per-image outputs (sse, mean SSIM, mean cs) composed from ATen ops on the device -- the five planes
            x, y, x^2, y^2, xy stacked to [B, 5C, H, W], a grouped `conv2d` with the 1 x 11 taps and one with the 11 x 1
            taps, the SSIM algebra, three reductions -- once in fp64 ("aten_fp64": the arithmetic the kernel matches) and
            once in fp32 ("aten_fp32": the textbook form, timed for orientation; its values are not usable, see below).
            Legs interleaved round by round inside one process; a figure is CALLS calls between two device events (host
            launches included), divided by CALLS; launch counts from the profiler's kernel events; peak memory from the
            caching allocator, above what was allocated before the call.
  accuracy  on the near-flat input 0.9 + 1e-3 randn (what a saturated tanh decoder produces): the worst per-PIXEL error of
            the fp32 composition's SSIM and cs maps against the fp64 composition's, and the worst per-image difference of
            the fused kernel from the fp64 composition.

    recon_quality_timing.py [--out profiles/r20_recon_quality.json] [--rounds 7]
"""
import argparse, json, os, statistics, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((128, 3, 64, 64), (256, 3, 128, 128), (64, 3, 256, 256))
CALLS = 10
WINDOW, SIGMA, L, K1, K2 = 11, 1.5, 2.0, 0.01, 0.03


def summary(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd), "runs": [round(x, nd) for x in v]}


def taps(dtype):
    import torch
    i = torch.arange(WINDOW, dtype=torch.float64, device="cuda") - (WINDOW - 1) // 2
    w = torch.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return (w / w.sum()).to(dtype)


def aten_maps(x, y, dtype):
    """(ssim map, cs map, x - y) in ``dtype``: grouped separable conv2d over the five stacked planes."""
    import torch
    import torch.nn.functional as F
    x, y = x.to(dtype), y.to(dtype)
    C = x.shape[1]
    planes = torch.cat([x, y, x * x, y * y, x * y], 1)
    w = taps(dtype)
    m = F.conv2d(planes, w.view(1, 1, 1, -1).expand(5 * C, 1, 1, -1).contiguous(), groups=5 * C)
    m = F.conv2d(m, w.view(1, 1, -1, 1).expand(5 * C, 1, -1, 1).contiguous(), groups=5 * C)
    mx, my, mxx, myy, mxy = m.split(C, 1)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    sxx, syy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    return (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs, cs, x - y


def aten_quality(x, y, dtype):
    import torch
    ss, cs, d = aten_maps(x, y, dtype)
    return torch.stack([(d * d).sum((1, 2, 3)), ss.mean((1, 2, 3)), cs.mean((1, 2, 3))], 1)


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
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def peak_mib(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def main(out_path, rounds):
    sys.path.insert(0, HERE)
    import torch
    from disentangle_mlp_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("recon_quality_timing.py measures on the GPU; none found")
    out = {"what": "per-image sum of squared errors, mean SSIM and mean contrast-structure term (11 x 11 Gaussian window, "
                   "valid positions) of an image batch against another: the fused kernel of csrc/recon_quality.hip against "
                   "the same outputs composed from ATen ops (grouped separable conv2d over five stacked planes) in fp64 "
                   "and in fp32",
           "device": "one MI355X (gfx950)",
           "method": f"one process; {rounds} rounds, the legs interleaved; a figure is {CALLS} calls between two device "
                     "events (host launches included) divided by the calls; ms per call",
           "shapes": {}}
    g = torch.Generator("cuda").manual_seed(20)
    for shape in SHAPES:
        x = torch.rand(shape, device="cuda", generator=g) * 2 - 1
        y = (x + 0.1 * torch.randn(shape, device="cuda", generator=g)).clamp(-1, 1)
        legs = {"fused": lambda: ops.recon_quality(x, y),
                "aten_fp64": lambda: aten_quality(x, y, torch.float64),
                "aten_fp32": lambda: aten_quality(x, y, torch.float32)}
        first = {k: fn().double() for k, fn in legs.items()}                 # (warm-up: allocator, workspace, conv plans)
        torch.cuda.synchronize()
        agree = {k: {"ssim": float((first[k][:, 1] - first["aten_fp64"][:, 1]).abs().max()),
                     "cs": float((first[k][:, 2] - first["aten_fp64"][:, 2]).abs().max()),
                     "sse_relative": float(((first[k][:, 0] - first["aten_fp64"][:, 0]).abs() / first["aten_fp64"][:, 0]).max())}
                 for k in ("fused", "aten_fp32")}
        counts = {k: launches_of(fn) for k, fn in legs.items()}
        peaks = {k: peak_mib(fn) for k, fn in legs.items()}
        ms = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                ms[k].append(timed_ms(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"ms_per_call": {k: summary(v) for k, v in ms.items()}, "kernel_launches": counts,
               "peak_mib_above_inputs": peaks,
               "aten_fp64_over_fused_of_medians": round(med["aten_fp64"] / med["fused"], 2),
               "aten_fp32_over_fused_of_medians": round(med["aten_fp32"] / med["fused"], 2),
               "fused_not_slower_than": {k: bool(med["fused"] <= med[k]) for k in med if k != "fused"},
               "per_image_difference_from_aten_fp64": agree,
               "input_mib": round(2 * x.numel() * 4 / 2 ** 20, 1),
               "fused_input_gb_per_s": round(2 * x.numel() * 4 / (1e-3 * med["fused"]) / 1e9, 1)}
        print(json.dumps({"x".join(map(str, shape)): res}), flush=True)
        out["shapes"]["x".join(map(str, shape))] = res
        del x, y, first
        torch.cuda.empty_cache()
    # the near-flat input: per-pixel maps
    shape = (16, 3, 64, 64)
    x = 0.9 + 1e-3 * torch.randn(shape, device="cuda", generator=g)
    y = 0.9 + 1e-3 * torch.randn(shape, device="cuda", generator=g)
    (s64, c64, _), (s32, c32, _) = aten_maps(x, y, torch.float64), aten_maps(x, y, torch.float32)
    fused, whole = ops.recon_quality(x, y), aten_quality(x, y, torch.float64)
    out["near_flat"] = {"input": "0.9 + 1e-3 randn, both images, 16 x 3 x 64 x 64",
                        "aten_fp32_worst_per_pixel_error": {"ssim": float((s32.double() - s64).abs().max()),
                                                            "cs": float((c32.double() - c64).abs().max())},
                        "aten_fp32_worst_per_image_error": {"ssim": float((s32.double().mean((1, 2, 3)) - whole[:, 1]).abs().max()),
                                                            "cs": float((c32.double().mean((1, 2, 3)) - whole[:, 2]).abs().max())},
                        "fused_worst_per_image_difference_from_aten_fp64": {"ssim": float((fused[:, 1] - whole[:, 1]).abs().max()),
                                                                            "cs": float((fused[:, 2] - whole[:, 2]).abs().max())}}
    print(json.dumps({"near_flat": out["near_flat"]}), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    main(a.out, a.rounds)
