"""The beta-TCVAE decomposition of the KL term by minibatch-weighted sampling (Chen et al. 2018; DESIGN.md section
4.17), restated in torch: the definitions as they are written down, every pair term materialised as a [B, B, D] tensor,
gradients from autograd.  Evaluated in fp64 it is the reference of tests/test_reparam_tc_*.py; evaluated in fp32 it is
the yardstick (how far plain fp32 arithmetic is from fp64 on the same inputs).  `closed_form_grads` is the hand-derived
gradient the kernels implement, checked against autograd on the CPU."""
import math

import torch

from _reparam_refs import bound, expected_grads, gz_grads, make_inputs, rel_err  # noqa: F401  (shared by the four objectives)

LOG_2PI = math.log(2.0 * math.pi)
DATASET_SIZE = 162770                  # the N of the tests (CelebA's training split)
WEIGHTS = [(1.0, 6.0, 1.0), (0.5, 4.0, 2.0)]      # (alpha, beta, gamma)
SHAPES = [(1, 1), (2, 3), (5, 7), (17, 65), (64, 128), (128, 128), (130, 200), (256, 128)]


def pair_terms(z, mu, lv):
    """lq[i,j,d] = log N(z[i,d]; mu[j,d], exp(lv[j,d]))"""
    return -0.5 * (LOG_2PI + lv[None] + (z[:, None] - mu[None]) ** 2 * torch.exp(-lv)[None])


def decomposition(z, mu, lv, dataset_size):
    """-> dict of the per-sample terms and the three parts (each summed over the batch), z, mu, lv independent."""
    B = z.shape[0]
    log_bn = math.log(B * dataset_size)
    lq = pair_terms(z, mu, lv)
    idx = torch.arange(B)
    lqzx = lq[idx, idx].sum(1)
    lqz = torch.logsumexp(lq.sum(2), dim=1) - log_bn
    lqprod = (torch.logsumexp(lq, dim=1) - log_bn).sum(1)
    lpz = (-0.5 * (LOG_2PI + z ** 2)).sum(1)
    return dict(lqzx=lqzx, lqz=lqz, lqprod=lqprod, lpz=lpz, mi=(lqzx - lqz).sum(), tc=(lqz - lqprod).sum(),
                dwkl=(lqprod - lpz).sum())


def weighted(parts, alpha, beta, gamma):
    return alpha * parts["mi"] + beta * parts["tc"] + gamma * parts["dwkl"]


def reparam_tc(mu, lv, eps, alpha, beta, gamma, dataset_size=DATASET_SIZE, dtype=torch.float64):
    """Forward values and the gradients of the two upstream terms SEPARATELY (the kernel's output is linear in them):
    ``gmu_loss, glv_loss`` = d loss / d (mu, logvar) through z and directly; ``gmu_gz(gz), glv_gz(gz)`` come from
    `gz_grads`.  All in ``dtype``."""
    mu = mu.detach().to(dtype).requires_grad_(True)
    lv = lv.detach().to(dtype).requires_grad_(True)
    eps = eps.detach().to(dtype)
    z = mu + eps * torch.exp(0.5 * lv)
    parts = decomposition(z, mu, lv, dataset_size)
    loss = weighted(parts, alpha, beta, gamma)
    gmu, glv = torch.autograd.grad(loss, (mu, lv))
    return dict(z=z.detach(), loss=loss.detach(), mi=parts["mi"].detach(), tc=parts["tc"].detach(),
                dwkl=parts["dwkl"].detach(), identity=(parts["lqzx"] - parts["lpz"]).sum().detach(), gmu_loss=gmu,
                glv_loss=glv)


def closed_form_grads(mu, lv, eps, alpha, beta, gamma, dtype=torch.float64):
    """The gradient as the kernels form it (gloss = 1, no gz): softmax weights w, v -> Gz, Gmu, Glv -> (gmu, glv)."""
    mu, lv, eps = (t.detach().to(dtype) for t in (mu, lv, eps))
    B = mu.shape[0]
    h = torch.exp(0.5 * lv)
    z = mu + eps * h
    lq = pair_terms(z, mu, lv)
    w = torch.softmax(lq.sum(2), dim=1)                      # [i, j]
    v = torch.softmax(lq, dim=1)                             # [i, j, d]
    c = alpha * torch.eye(B, dtype=dtype)[:, :, None] + (beta - alpha) * w[:, :, None] + (gamma - beta) * v
    diff = z[:, None] - mu[None]
    r = diff * torch.exp(-lv)[None]
    Gz = (c * -r).sum(1) + gamma * z
    Gmu = (c * r).sum(0)
    Glv = (c * (-0.5 + 0.5 * r * diff)).sum(0)
    return Gmu + Gz, Glv + Gz * eps * 0.5 * h
