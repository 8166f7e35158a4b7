"""The InfoVAE / WAE-MMD objective (Zhao et al. 2019; Tolstikhin et al. 2018) restated in torch:
the definitions as they are written down, every pair term materialised as a [B, B, D] tensor of differences, gradients
from autograd.  Evaluated in fp64 it is the reference of tests/test_reparam_mmd_*.py; evaluated in fp32 it is the
yardstick (how far plain fp32 arithmetic is from fp64 on the same inputs).  `closed_form_grads` is the hand-derived
gradient the kernels implement, checked against autograd on the CPU.

`mmd` is a difference of O(1) terms, so the error of `mmd` and of `loss` is taken over the SUM OF THE MAGNITUDES of their
terms (`mmd_terms` / `loss_terms`), not over the value: at (64, 128), imq, mmd is 0.12 against terms of 12.4."""
import torch

from _reparam_refs import bound, expected_grads, gz_grads, rel_err  # noqa: F401  (shared by the four objectives)

LAMBDA = 1000.0
CASES = [("rbf", None, LAMBDA, 6.0), ("imq", None, LAMBDA, 6.0), ("imq", None, LAMBDA, 0.0)]   # (kernel, bandwidths, lambda, beta)
SHAPES = [(2, 1), (2, 3), (5, 7), (17, 65), (33, 32), (64, 128), (128, 128), (130, 200), (256, 128), (3, 600)]
EDGE_SHAPES = [(1024, 32), (32, 1024)]      # every tile slot / every chunk at the contract's edges, run once each
IMQ_SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)
COMPARED = ("z", "loss", "kl", "mmd", "kzz", "gmu_loss", "glv_loss")


def default_bandwidths(kernel, D):
    """WAE's convention with sigma_p^2 = 1."""
    return (2.0 * D,) if kernel == "rbf" else tuple(2.0 * D * s for s in IMQ_SCALES)


def make_inputs(B, D, seed=0):
    """The siblings' recipe -- mu ~ N(0,1); logvar ~ N(-1, 1.5^2) clamped to [-6, 2]; eps ~ N(0,1); gz ~ N(0,1) -- plus
    zp ~ N(0,1) from the same generator, drawn last; fp32."""
    g = torch.Generator().manual_seed(1000 * B + D + seed)
    mu = torch.randn(B, D, generator=g)
    lv = (torch.randn(B, D, generator=g) * 1.5 - 1.0).clamp_(-6.0, 2.0)
    eps = torch.randn(B, D, generator=g)
    gz = torch.randn(B, D, generator=g)
    zp = torch.randn(B, D, generator=g)
    return dict(mu=mu, lv=lv, eps=eps, gz=gz, zp=zp)


def sqdist(a, b):
    """d[i, j] = |a_i - b_j|^2 from the differences, a [B, B, D] tensor in between."""
    return ((a[:, None] - b[None]) ** 2).sum(2)


def kernel_values(d, kernel, hs):
    if kernel == "rbf":
        return sum(torch.exp(-d / h) for h in hs)
    return sum(h / (h + d) for h in hs)


def kernel_slopes(d, kernel, hs):
    """k'(d)"""
    if kernel == "rbf":
        return sum(-torch.exp(-d / h) / h for h in hs)
    return sum(-h / (h + d) ** 2 for h in hs)


def mmd_parts(z, zp, kernel, hs):
    """-> (kzz, kpp, kzp): the three means of the unbiased U-statistic."""
    B = z.shape[0]
    off = ~torch.eye(B, dtype=torch.bool, device=z.device)
    kzz = kernel_values(sqdist(z, z), kernel, hs)[off].sum() / (B * (B - 1))
    kpp = kernel_values(sqdist(zp, zp), kernel, hs)[off].sum() / (B * (B - 1))
    kzp = kernel_values(sqdist(z, zp), kernel, hs).sum() / (B * B)
    return kzz, kpp, kzp


def objective(mu, lv, z, zp, beta, kernel, lambda_mmd, bandwidths=None):
    """-> dict(kl, mmd, kzz, kpp, kzp, loss), every sum over the batch: loss = beta kl + B lambda mmd."""
    hs = default_bandwidths(kernel, mu.shape[1]) if bandwidths is None else tuple(bandwidths)
    kl = -0.5 * (1.0 + lv - mu ** 2 - torch.exp(lv)).sum()
    kzz, kpp, kzp = mmd_parts(z, zp, kernel, hs)
    mmd = kzz + kpp - 2.0 * kzp
    return dict(kl=kl, mmd=mmd, kzz=kzz, kpp=kpp, kzp=kzp, loss=beta * kl + mu.shape[0] * lambda_mmd * mmd)


def reparam_mmd(mu, lv, eps, zp, beta, kernel, lambda_mmd, bandwidths=None, dtype=torch.float64):
    """Forward values and the gradient of the loss term (``gmu_loss, glv_loss`` = d loss / d (mu, logvar), through z and
    directly); the decoder's term comes from `gz_grads`: the kernel's output is linear in the two upstream gradients.
    ``mmd_terms`` / ``loss_terms``: the sums of the magnitudes of the terms of ``mmd`` / ``loss``.  All in ``dtype``."""
    mu = mu.detach().to(dtype).requires_grad_(True)
    lv = lv.detach().to(dtype).requires_grad_(True)
    eps, zp = eps.detach().to(dtype), zp.detach().to(dtype)
    z = mu + eps * torch.exp(0.5 * lv)
    o = objective(mu, lv, z, zp, beta, kernel, lambda_mmd, bandwidths)
    gmu, glv = torch.autograd.grad(o["loss"], (mu, lv), allow_unused=True)
    glv = torch.zeros_like(lv) if glv is None else glv
    o = {k: v.detach() for k, v in o.items()}
    mmd_terms = o["kzz"].abs() + o["kpp"].abs() + 2.0 * o["kzp"].abs()
    loss_terms = (beta * o["kl"]).abs() + mu.shape[0] * lambda_mmd * mmd_terms
    return dict(z=z.detach(), gmu_loss=gmu, glv_loss=glv, mmd_terms=mmd_terms, loss_terms=loss_terms, **o)


def scalar_err(got, ref, scale):
    """|got - ref| over ``scale`` (the sum of the magnitudes of the terms the scalar is made of)."""
    return abs(float(got) - float(ref)) / max(float(scale), 1e-30)


def scalar_bound(r32, r64, name):
    """The project's convention for ``mmd`` and ``loss``, errors over the reference's ``<name>_terms``."""
    return max(1e-6, 5.0 * scalar_err(r32[name], r64[name], r64[name + "_terms"]))


def closed_form_grads(mu, lv, eps, zp, beta, kernel, lambda_mmd, bandwidths=None, dtype=torch.float64):
    """The gradient as the kernels form it (gloss = 1, no gz): the slopes with their prefactors, Gz, then (gmu, glv)."""
    mu, lv, eps, zp = (t.detach().to(dtype) for t in (mu, lv, eps, zp))
    B, D = mu.shape
    hs = default_bandwidths(kernel, D) if bandwidths is None else tuple(bandwidths)
    h = torch.exp(0.5 * lv)
    z = mu + eps * h
    wzz = 4.0 / (B * (B - 1)) * kernel_slopes(sqdist(z, z), kernel, hs)
    wzz = wzz * (1.0 - torch.eye(B, dtype=dtype))
    wzp = -4.0 / (B * B) * kernel_slopes(sqdist(z, zp), kernel, hs)
    Gz = B * lambda_mmd * ((wzz[:, :, None] * (z[:, None] - z[None])).sum(1) + (wzp[:, :, None] * (z[:, None] - zp[None])).sum(1))
    return beta * mu + Gz, beta * 0.5 * (torch.exp(lv) - 1.0) + Gz * eps * 0.5 * h
