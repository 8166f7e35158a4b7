"""fp64 restatement of csrc/recon_quality.hip and recon_quality.py for the tests: the window moments are summed as the
DIRECT 2-D window per pixel (weights ``outer(w, w)``), not as the kernel's separable two-pass filter, so the reference
shares neither the kernel's order of operations nor its tiling.  Everything runs on the CPU in fp64 and returns on the
inputs' device.  `check_self` (run by tests/test_recon_quality_cpu.py) verifies the restatement against closed forms."""
import math

import torch

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def taps(window=11, sigma=1.5):
    i = torch.arange(window, dtype=torch.float64) - (window - 1) // 2
    w = torch.exp(-(i * i) / (2.0 * sigma * sigma))
    return w / w.sum()


def _windows(v, window):
    """[B, C, H, W] -> [B, C, OH, OW, window, window] (a view)."""
    return v.unfold(2, window, 1).unfold(3, window, 1)


def moments_direct(v, w):
    """sum_{i,j} w_i w_j v[r + i, c + j] for every valid (r, c)."""
    return (_windows(v, w.numel()) * torch.outer(w, w)).sum((-1, -2))


def moments_separable(v, w):
    """The kernel's factorisation (horizontal, then vertical), in fp64 tensor operations."""
    h = (v.unfold(3, w.numel(), 1) * w).sum(-1)
    return (h.unfold(2, w.numel(), 1) * w).sum(-1)


def maps(x, y, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03, moments=moments_direct):
    """(ssim map, cs map), each [B, C, OH, OW] fp64."""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    w = taps(window, sigma)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = moments(x, w), moments(y, w)
    sxx, syy, sxy = moments(x * x, w) - mx * mx, moments(y * y, w) - my * my, moments(x * y, w) - mx * my
    cs = (2.0 * sxy + c2) / (sxx + syy + c2)
    return (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * cs, cs


def recon_quality(x, y, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03):
    """ops.recon_quality: [B, 3] fp64 (sse, mean ssim, mean cs)."""
    ss, cs = maps(x, y, data_range, window, sigma, k1, k2)
    d = x.detach().cpu().double() - y.detach().cpu().double()
    return torch.stack([(d * d).sum((1, 2, 3)), ss.mean((1, 2, 3)), cs.mean((1, 2, 3))], 1).to(x.device)


def psnr(x, y, data_range=2.0):
    sse = recon_quality(x, y, data_range, window=3)[:, 0]
    return 10.0 * torch.log10(data_range ** 2 * x[0].numel() / sse)


def default_scales(h, w, window=11):
    return max(s for s in range(1, 6) if min(h, w) // 2 ** (s - 1) >= window)


def ms_ssim(x, y, scales=None, weights=None, **args):
    scales = default_scales(x.shape[2], x.shape[3], args.get("window", 11)) if scales is None else scales
    weights = [w / sum(WEIGHTS[:scales]) for w in WEIGHTS[:scales]] if weights is None else weights
    value = torch.ones(x.shape[0], dtype=torch.float64, device=x.device)
    for j in range(scales):
        if j:
            x, y = (torch.nn.functional.avg_pool2d(t, 2, 2) for t in (x, y))
        out = recon_quality(x, y, **args)
        value = value * out[:, 1 if j == scales - 1 else 2].clamp(min=0.0) ** weights[j]
    return value


def coarse_cs(x, y, scales, **args):
    """[B, scales] fp64: the mean cs of every scale (the tests look for a negative one)."""
    cols = []
    for j in range(scales):
        if j:
            x, y = (torch.nn.functional.avg_pool2d(t, 2, 2) for t in (x, y))
        cols.append(recon_quality(x, y, **args)[:, 2])
    return torch.stack(cols, 1)


def report(x, y, **args):
    out = recon_quality(x, y, **args)
    ps = 10.0 * torch.log10(args.get("data_range", 2.0) ** 2 * x[0].numel() / out[:, 0])
    ms = ms_ssim(x, y, **args)
    return dict(n=x.shape[0], mse=out[:, 0].mean(), psnr=ps.mean(), ssim=out[:, 1].mean(), ms_ssim=ms.mean(),
                ms_ssim_scales=default_scales(x.shape[2], x.shape[3], args.get("window", 11)),
                ssim_std=out[:, 1].std(unbiased=False))


# ---- inputs -----------------------------------------------------------------------------------------------------------
KINDS = ("uniform", "near_flat", "constants", "noisy_copy", "unit_range")


def pair(kind, shape, seed=0):
    """(x, y, data_range) fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1, 2.0
    if kind == "near_flat":                                    # what a saturated tanh decoder gives
        return 0.9 + 1e-3 * torch.randn(shape, generator=g), 0.9 + 1e-3 * torch.randn(shape, generator=g), 2.0
    if kind == "constants":
        return torch.full(shape, -1.0), torch.full(shape, 1.0), 2.0
    if kind == "noisy_copy":
        x = torch.rand(shape, generator=g) * 2 - 1
        return x, (x + 0.1 * torch.randn(shape, generator=g)).clamp(-1, 1), 2.0
    if kind == "unit_range":
        x = torch.rand(shape, generator=g)
        return x, (x + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1), 1.0
    raise ValueError(kind)


def check_self():
    """The restatement against closed forms; returns the largest direct-vs-separable difference seen."""
    worst = 0.0
    for window in (3, 11):
        for a, b in ((-1.0, 1.0), (0.25, 0.25), (0.9, -0.3)):
            x, y = torch.full((1, 2, 13, 14), a), torch.full((1, 2, 13, 14), b)
            a, b = float(x[0, 0, 0, 0]), float(y[0, 0, 0, 0])      # (as fp32 holds them)
            ss, cs = maps(x, y, window=window)
            c1 = (0.01 * 2.0) ** 2
            assert float((cs - 1.0).abs().max()) <= 1e-12
            assert float((ss - (2 * a * b + c1) / (a * a + b * b + c1)).abs().max()) <= 1e-12
        for kind in KINDS:
            x, y, L = pair(kind, (2, 2, 19, 23), seed=3)
            same, _ = maps(x, x, data_range=L, window=window)
            assert float((same - 1.0).abs().max()) <= 1e-12
            for d, s in zip(maps(x, y, data_range=L, window=window),
                            maps(x, y, data_range=L, window=window, moments=moments_separable)):
                worst = max(worst, float((d - s).abs().max()))
    assert worst <= 1e-12, worst
    assert math.isinf(float(psnr(x, x)[0])) and float(recon_quality(x, x)[0, 0]) == 0.0
    return worst
