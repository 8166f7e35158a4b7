"""Reconstruction quality: how well images come back through encoder and decoder -- PSNR, SSIM (Wang et al. 2004) and
MS-SSIM (Wang et al. 2003) per image, from two batches [B, C, H, W] on the device.  DESIGN.md section 4.26.  The counterpart
of sample_quality.py (which scores samples) and metrics.py (which scores the posterior, the RATE side of a beta sweep):
this is the DISTORTION side, the number beta, ``tc_decomposition=``, ``dip_vae=`` and ``mmd_vae=`` all move.

Everything rests on `ops.recon_quality` (csrc/recon_quality.hip): per image the sum of squared errors, the mean SSIM and
the mean contrast-structure term, from fp64 window moments in one fused launch sequence -- the textbook fp32 form
(E[x^2] - mu^2 per window) is off by 1e-4 per pixel on the nearly flat windows a saturated tanh decoder produces.  What
follows the kernel is a handful of fp64 operations on [B] vectors; the scalars of the dicts are 0-dim fp64 device
tensors, so a report costs no host read until the caller asks for one.

The defaults are the published ones (11 x 11 Gaussian window, sigma 1.5, K1 = 0.01, K2 = 0.03, no padding: only window
positions that lie inside the image count) with ``data_range=2.0``, the span of the tanh decoder's [-1, 1]."""
import math

import torch

from . import ops

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003, scales 1 (finest) .. 5


def _pair(x, y):
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor) or x.dim() != 4 or y.shape != x.shape:
        raise ValueError("expected two [B, C, H, W] image batches of one shape")
    return x.float().contiguous(), y.float().contiguous()


def _psnr_of(sse, numel, data_range):
    return 10.0 * torch.log10((float(data_range) ** 2 * numel) / sse)


def psnr(x, y, data_range=2.0):
    """[B] fp64: per image ``10 log10(L^2 C H W / sse)``; an image that comes back identical (sse = 0) gives ``+inf``.
    (The sum of squared errors does not depend on the window: the call runs with the smallest, 3 x 3.)"""
    x, y = _pair(x, y)
    sse = ops.recon_quality(x, y, data_range=data_range, window=3)[:, 0]
    return _psnr_of(sse, x[0].numel(), data_range)


def ssim(x, y, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03):
    """[B] fp64: per image the mean of the SSIM map over all channels and valid window positions."""
    x, y = _pair(x, y)
    return ops.recon_quality(x, y, data_range=data_range, window=window, sigma=sigma, k1=k1, k2=k2)[:, 1]


def ms_ssim_scales(height, width, window=11):
    """The number of scales ``ms_ssim`` uses by default: the largest S <= 5 whose last scale -- the image halved S - 1
    times, rounding down -- still holds one window: 3 at 64 x 64, 4 at 128 x 128, 5 from 176 x 176 on."""
    s = 0
    while s < len(MS_SSIM_WEIGHTS) and (min(int(height), int(width)) >> s) >= int(window):
        s += 1
    if s == 0:
        raise ValueError(f"ms_ssim: a {height} x {width} image does not hold one {window} x {window} window")
    return s


def ms_ssim_weights(scales, weights=None):
    """The exponents of the ``scales`` factors: ``weights`` as given (one per scale), or Wang's five truncated to
    ``scales`` and renormalised to sum 1."""
    scales = int(scales)
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != scales:
            raise ValueError(f"ms_ssim: {len(weights)} weights for {scales} scales")
        return weights
    if not 1 <= scales <= len(MS_SSIM_WEIGHTS):
        raise ValueError(f"ms_ssim: the default weights cover 1..{len(MS_SSIM_WEIGHTS)} scales, got {scales}")
    total = sum(MS_SSIM_WEIGHTS[:scales])
    return [w / total for w in MS_SSIM_WEIGHTS[:scales]]


def _pyramid(x, y, scales, **args):
    """``ops.recon_quality`` of every scale: scale j is scale j - 1 after ``avg_pool2d(2, 2)`` (ATen: plumbing)."""
    outs = []
    for j in range(scales):
        if j:
            x = torch.nn.functional.avg_pool2d(x, 2, 2).contiguous()
            y = torch.nn.functional.avg_pool2d(y, 2, 2).contiguous()
        outs.append(ops.recon_quality(x, y, **args))
    return outs


def _ms_ssim_of(outs, weights):
    value = outs[-1][:, 1].clamp(min=0.0) ** weights[-1]
    for out, w in zip(outs[:-1], weights[:-1]):
        value = value * out[:, 2].clamp(min=0.0) ** w
    return value


def ms_ssim(x, y, scales=None, weights=None, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03):
    """[B] fp64: per image the product over scales of the mean contrast-structure term (scales 1 .. S - 1) and the mean
    SSIM (scale S), each clamped at 0 and raised to its weight.  ``scales=None``: `ms_ssim_scales` of the image size;
    ``weights=None``: `ms_ssim_weights`.  With S < 5 -- every image below 176 x 176 at the default window -- this is NOT
    the published five-scale metric: its values compare only with others of the same S."""
    x, y = _pair(x, y)
    scales = ms_ssim_scales(x.shape[2], x.shape[3], window) if scales is None else int(scales)
    weights = ms_ssim_weights(scales, weights)
    return _ms_ssim_of(_pyramid(x, y, scales, data_range=data_range, window=window, sigma=sigma, k1=k1, k2=k2), weights)


class Accumulator:
    """`report` over a loader: ``update(x, y)`` per batch, ``result()`` at the end.  Keeps three [n] fp64 vectors (sse,
    ssim, ms_ssim), never an image."""

    def __init__(self, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03, scales=None, weights=None, per_image=False):
        self.args = dict(data_range=data_range, window=window, sigma=sigma, k1=k1, k2=k2)
        self.scales, self.weights, self.per_image = scales, weights, per_image
        self.numel = None
        self._sse, self._ssim, self._ms = [], [], []

    def update(self, x, y):
        x, y = _pair(x, y)
        if self.numel is None:
            self.numel = x[0].numel()
            if self.scales is None:
                self.scales = ms_ssim_scales(x.shape[2], x.shape[3], self.args["window"])
            self.weights = ms_ssim_weights(self.scales, self.weights)
        elif x[0].numel() != self.numel:
            raise ValueError("Accumulator: the images of every batch must have one size")
        outs = _pyramid(x, y, int(self.scales), **self.args)
        self._sse.append(outs[0][:, 0])
        self._ssim.append(outs[0][:, 1])
        self._ms.append(_ms_ssim_of(outs, self.weights))
        return self

    def result(self):
        if not self._sse:
            raise ValueError("Accumulator: no batch was scored")
        sse, ss, ms = torch.cat(self._sse), torch.cat(self._ssim), torch.cat(self._ms)
        ps = _psnr_of(sse, self.numel, self.args["data_range"])
        out = dict(n=int(sse.shape[0]), mse=sse.mean(), psnr=ps.mean(), ssim=ss.mean(), ms_ssim=ms.mean(),
                   ms_ssim_scales=int(self.scales), ssim_std=ss.std(unbiased=False))
        if self.per_image:
            out.update(sse_per_image=sse, psnr_per_image=ps, ssim_per_image=ss, ms_ssim_per_image=ms)
        return out


def report(x, y, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03, scales=None, weights=None, per_image=False):
    """All of the above in one dict, the finest scale scored once:

      ``n``        the number of images (int)          ``ms_ssim_scales``  the S of `ms_ssim` (int)
      ``mse``      the mean per-image SUM of squared errors -- the unit of the reference's logged reconstruction loss
      ``psnr``     the mean of the per-image PSNR: ``+inf`` as soon as ONE image comes back identical (its own PSNR is
                   +inf; no NaN can arise, a PSNR is never -inf for finite input) -- read ``mse`` for a finite summary
      ``ssim`` / ``ssim_std``   mean and (population) standard deviation of the per-image SSIM
      ``ms_ssim``  the mean per-image MS-SSIM

    and with ``per_image=True`` the [n] vectors ``sse_per_image``, ``psnr_per_image``, ``ssim_per_image``,
    ``ms_ssim_per_image``."""
    return Accumulator(data_range, window, sigma, k1, k2, scales, weights, per_image).update(x, y).result()
