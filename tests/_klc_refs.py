"""The controlled KL term -- a capacity (Burgess et al. 2018) over per-dimension free bits (Kingma et al. 2016); DESIGN.md
section 4.30 -- restated in torch: the definitions as they are written down (``clamp(min=)``, ``abs()``), gradients from
autograd.  Evaluated in fp64 it is the reference of tests/test_reparam_klc_*.py; evaluated in fp32 it is the yardstick
(how far plain fp32 arithmetic is from fp64 on the same inputs).  `closed_form_grads` is the hand-derived gradient the
kernels implement -- the gate formula -- checked against autograd on the CPU."""
import torch

from _dip_refs import SHAPES  # noqa: F401  (the same shapes as the DIP-VAE tests)
from _reparam_refs import bound, expected_grads, gz_grads, rel_err  # noqa: F401  (shared by the four objectives)

BETA = 6.0
# (f, lambda): the capacity is C = f * T64 / B with T64 the fp64 floored total of that input -- below, at (f = 0: far
# below) and above the total, so both signs are covered and |T - B C| / T is 1 or 0.5 by construction
CASES = [(0.0, 0.0), (0.5, 0.0), (2.0, 0.0), (0.0, 0.05), (0.5, 0.05), (2.0, 0.05)]
COMPARED = ("z", "loss", "kl", "kl_floored", "kl_dim", "gmu_loss", "glv_loss")
MARGIN = 1e-3      # no K[d] of the fp64 reference lies within this (relative) of its floor B * lambda: every gate is compared


def make_inputs(B, D):
    """Dimensions from collapsed to active: with s = logspace(-2, 0, D) (s = 1 at D = 1), mu = randn * s, logvar =
    ((randn * 1.5 - 1) * s) clamped to [-6, 2]; eps, gz ~ N(0,1) (gz: a decoder's gradient); fp32."""
    g = torch.Generator().manual_seed(1000 * B + D)
    s = torch.logspace(-2.0, 0.0, D) if D > 1 else torch.ones(1)
    mu = torch.randn(B, D, generator=g) * s
    lv = ((torch.randn(B, D, generator=g) * 1.5 - 1.0) * s).clamp_(-6.0, 2.0)
    eps = torch.randn(B, D, generator=g)
    gz = torch.randn(B, D, generator=g)
    return dict(mu=mu, lv=lv, eps=eps, gz=gz)


def kl_per_dim(mu, lv):
    """K[d]: the dimension's KL summed over the batch."""
    return (-0.5 * (1.0 + lv - mu ** 2 - torch.exp(lv))).sum(0)


def objective(mu, lv, beta, capacity, free_bits):
    """-> dict(kl, kl_floored, dims_above, kl_dim, loss), every sum over the batch: loss = beta |kl_floored - B capacity|."""
    B = mu.shape[0]
    K = kl_per_dim(mu, lv)
    T = K.clamp(min=B * free_bits).sum()
    return dict(kl=K.sum(), kl_floored=T, dims_above=(K > B * free_bits).sum(), kl_dim=K / B,
                loss=beta * (T - B * capacity).abs())


def floored_total(mu, lv, free_bits):
    """T64: the fp64 floored total of an input."""
    return float(kl_per_dim(mu.double(), lv.double()).clamp(min=mu.shape[0] * free_bits).sum())


def capacity_of(inputs, case):
    """The C of a case (f, lambda) on these inputs: f * T64 / B, as a Python float."""
    f, lam = case
    return f * floored_total(inputs["mu"], inputs["lv"], lam) / inputs["mu"].shape[0]


def margin(mu, lv, free_bits):
    """min_d |K[d] - B lambda| / (B lambda) in fp64 (inf at lambda = 0 unless a K[d] is exactly 0)."""
    K = kl_per_dim(mu.double(), lv.double())
    fl = mu.shape[0] * free_bits
    if fl == 0.0:
        return float("inf") if bool((K != 0).all()) else 0.0
    return float(((K - fl).abs() / fl).min())


def reparam_klc(mu, lv, eps, beta, capacity, free_bits, dtype=torch.float64):
    """Forward values and the gradient of the loss term (``gmu_loss, glv_loss`` = d loss / d (mu, logvar)); the decoder's
    term comes from `gz_grads`: the kernel's output is linear in the two upstream gradients.  All in ``dtype``."""
    mu = mu.detach().to(dtype).requires_grad_(True)
    lv = lv.detach().to(dtype).requires_grad_(True)
    eps = eps.detach().to(dtype)
    z = mu + eps * torch.exp(0.5 * lv)
    o = objective(mu, lv, beta, capacity, free_bits)
    gmu, glv = torch.autograd.grad(o["loss"], (mu, lv), allow_unused=True)
    gmu = torch.zeros_like(mu) if gmu is None else gmu
    glv = torch.zeros_like(lv) if glv is None else glv
    return dict(z=z.detach(), gmu_loss=gmu, glv_loss=glv, gate=gate(mu.detach(), lv.detach(), capacity, free_bits),
                **{k: v.detach() for k, v in o.items()})


def gate(mu, lv, capacity, free_bits):
    """gate[d] = sgn(T - B C) [K[d] > B lambda] in {-1, 0, +1} (sgn(0) = 0), in the dtype of ``mu``."""
    B = mu.shape[0]
    K = kl_per_dim(mu, lv)
    T = K.clamp(min=B * free_bits).sum()
    return torch.sign(T - B * capacity) * (K > B * free_bits).to(mu.dtype)


def closed_form_grads(mu, lv, beta, capacity, free_bits, dtype=torch.float64):
    """The gradient as the kernels form it (gloss = 1, no gz): gmu = beta gate[d] mu, glv = beta gate[d] (exp(lv) - 1) / 2."""
    mu, lv = (t.detach().to(dtype) for t in (mu, lv))
    g = gate(mu, lv, capacity, free_bits)[None]
    return beta * g * mu, beta * g * 0.5 * (torch.exp(lv) - 1.0)
