"""The DIP-VAE objectives (Kumar et al. 2018, variants I and II) restated in torch: the
definitions as they are written down, gradients from autograd.  Evaluated in fp64 it is the reference of
tests/test_reparam_dip_*.py; evaluated in fp32 it is the yardstick (how far plain fp32 arithmetic is from fp64 on the
same inputs).  `closed_form_grads` is the hand-derived gradient the kernels implement, checked against autograd on the
CPU."""
import torch

from _reparam_refs import bound, expected_grads, gz_grads, make_inputs, rel_err  # noqa: F401  (shared by the four objectives)

BETA = 6.0
CASES = [("i", 10.0, 100.0), ("ii", 10.0, 10.0), ("ii", 0.5, 4.0)]      # (variant, lambda_od, lambda_d)
SHAPES = [(1, 1), (2, 3), (5, 7), (17, 65), (64, 128), (128, 128), (130, 200), (256, 128), (3, 600)]
COMPARED = ("z", "loss", "kl", "od", "dg", "cov", "gmu_loss", "glv_loss")


def covariance(mu, lv, variant):
    """C in its centred form: (1/B) sum_b c_b c_b^T, plus diag(mean_b exp(lv)) in variant II."""
    B = mu.shape[0]
    c = mu - mu.mean(0, keepdim=True)
    C = c.t() @ c / B
    if variant == "ii":
        C = C + torch.diag(torch.exp(lv).mean(0))
    return C


def covariance_uncentred(mu, lv, variant):
    """The same C as E[mu mu^T] - E[mu] E[mu]^T."""
    B = mu.shape[0]
    m = mu.mean(0)
    C = mu.t() @ mu / B - torch.outer(m, m)
    if variant == "ii":
        C = C + torch.diag(torch.exp(lv).mean(0))
    return C


def penalties(C):
    """-> (od, dg) = (sum_{i != j} C_ij^2, sum_i (C_ii - 1)^2)"""
    diag = torch.diagonal(C)
    return ((C - torch.diag(diag)) ** 2).sum(), ((diag - 1.0) ** 2).sum()


def objective(mu, lv, beta, variant, lambda_od, lambda_d):
    """-> dict(kl, od, dg, cov, loss), every sum over the batch: loss = beta kl + B (lambda_od od + lambda_d dg)."""
    kl = -0.5 * (1.0 + lv - mu ** 2 - torch.exp(lv)).sum()
    C = covariance(mu, lv, variant)
    od, dg = penalties(C)
    return dict(kl=kl, od=od, dg=dg, cov=C, loss=beta * kl + mu.shape[0] * (lambda_od * od + lambda_d * dg))


def reparam_dip(mu, lv, eps, beta, variant, lambda_od, lambda_d, dtype=torch.float64):
    """Forward values and the gradient of the loss term (``gmu_loss, glv_loss`` = d loss / d (mu, logvar)); the decoder's
    term comes from `gz_grads`: the kernel's output is linear in the two upstream gradients.  All in ``dtype``."""
    mu = mu.detach().to(dtype).requires_grad_(True)
    lv = lv.detach().to(dtype).requires_grad_(True)
    eps = eps.detach().to(dtype)
    z = mu + eps * torch.exp(0.5 * lv)
    o = objective(mu, lv, beta, variant, lambda_od, lambda_d)
    gmu, glv = torch.autograd.grad(o["loss"], (mu, lv), allow_unused=True)
    glv = torch.zeros_like(lv) if glv is None else glv
    return dict(z=z.detach(), gmu_loss=gmu, glv_loss=glv, **{k: v.detach() for k, v in o.items()})


def closed_form_grads(mu, lv, beta, variant, lambda_od, lambda_d, dtype=torch.float64):
    """The gradient as the kernels form it (gloss = 1, no gz): G from C, Gmu = 2 (c . G), Glv = G_dd exp(lv) (II)."""
    mu, lv = (t.detach().to(dtype) for t in (mu, lv))
    C = covariance(mu, lv, variant)
    G = 2.0 * lambda_od * C
    G[range(len(G)), range(len(G))] = 2.0 * lambda_d * (torch.diagonal(C) - 1.0)
    c = mu - mu.mean(0, keepdim=True)
    gmu = beta * mu + 2.0 * (c @ G)
    glv = beta * 0.5 * (torch.exp(lv) - 1.0)
    if variant == "ii":
        glv = glv + torch.diagonal(G)[None] * torch.exp(lv)
    return gmu, glv
