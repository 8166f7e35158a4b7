"""Whether a run disentangled anything: the ELBO decomposition over a dataset (Chen et al. 2018, section 4 and appendix
C) and MIG, the mutual-information gap, against whatever labels exist.  Both rest on one computation -- the log-density
of M latent points under the aggregate posterior q(z) = 1/N sum_j N(mu_j, sigma_j^2), jointly and per dimension, which is
`ops.agg_posterior_lse` (one fused kernel sequence).  Everything after it is a handful of fp64
reductions on the device; the dicts hold device tensors (0-dim for the scalars), so a report costs no host read until the
caller asks for one.  Unlike the ``mi`` / ``tc`` / ``dwkl`` a ``tc_decomposition=`` trainer returns per step -- minibatch
weighted estimates at the batch size, biased training signals -- these are evaluated against all N posteriors."""
import math

import torch

from . import model as _model
from . import ops

LOG_2PI = math.log(2.0 * math.pi)


def _encode(net, x):
    """(mu, logvar) of a VAE-style network (`encode`) or an Encoder_celeba-style one (`features` and the two heads)."""
    if hasattr(net, "encode"):
        return net.encode(x)
    if all(hasattr(net, a) for a in ("features", "x_to_mu", "x_to_logvar")):
        feat = net.features(x)
        inner = ops.keep_amax(feat, feat.view(x.size(0), -1))
        return net.x_to_mu(inner), net.x_to_logvar(inner)
    raise TypeError(f"{type(net).__name__} has no encoder: expected `encode(x) -> (mu, logvar)` or `features` + "
                    "`x_to_mu` + `x_to_logvar`")


def encode_dataset(net, loader, eval_mode=False, max_samples=None):
    """The posteriors of every image of ``loader`` (``for data, labels in loader``): ``(mu [N, D], logvar [N, D], labels
    [N] or None)`` on the network's device, under ``no_grad``.  BatchNorm runs in training mode by default, as in
    `BetaVAEGANTrainer.evaluate` (batch statistics; the running ones move); ``eval_mode=True`` encodes inside
    ``model.eval_mode(net)``.  ``max_samples``: stop after that many rows."""
    device = next(net.parameters()).device
    mus, lvs, labs, n = [], [], [], 0
    with torch.no_grad(), _model.eval_mode(*((net,) if eval_mode else ())):
        for data, labels in loader:
            mu, logvar = _encode(net, data.to(device))
            mus.append(mu.detach())
            lvs.append(logvar.detach())
            labs.append(None if labels is None else torch.as_tensor(labels).to(device))
            n += mu.shape[0]
            if max_samples is not None and n >= max_samples:
                break
    if not mus:
        raise ValueError("encode_dataset: the loader gave no batch")
    mu, logvar = torch.cat(mus)[:max_samples].contiguous(), torch.cat(lvs)[:max_samples].contiguous()
    labels = None if any(l is None for l in labs) else torch.cat(labs)[:max_samples]
    return mu, logvar, labels


def _posteriors(mu, logvar):
    if mu.dim() != 2 or logvar.shape != mu.shape or mu.shape[0] < 1:
        raise ValueError("mu and logvar must be [N, D] tensors of one shape")
    return mu.float().contiguous(), logvar.float().contiguous()


def _randn(shape, device, generator):
    return torch.randn(shape, device=device if generator is None else generator.device, generator=generator).to(device)


def elbo_decomposition(mu, logvar, n_eval=None, generator=None, threshold=1e-2):
    """The KL term of the ELBO averaged over the dataset, split as Chen et al. 2018 (eq. 2), with q(z) the aggregate
    posterior of ALL N rows: ``n_eval`` row indices are drawn without replacement (default: every row, in order),
    z_m = mu_m + eps sigma_m with ``generator``, one `ops.agg_posterior_lse` call, then fp64 on the device.  Keys:

      ``mi``    mean[log q(z_m|x_m) - log q(z_m)]              index-code mutual information
      ``tc``    mean[log q(z_m) - sum_d log q(z_md)]           total correlation
      ``dwkl``  mean[sum_d log q(z_md) - log p(z_m)]           dimension-wise KL
      ``kl``    the analytic mean KL(q(z|x) || p(z)) over all N rows (mi + tc + dwkl estimates it)
      ``h_joint``  -mean log q(z_m)        ``h_dim`` [D]  -mean log q(z_md)        ``kl_dim`` [D]  the analytic KL per dimension
      ``active_units``  the number of d with Var_x(mu_d) > ``threshold`` (Burda et al. 2016), int64
    """
    mu, logvar = _posteriors(mu, logvar)
    N, D = mu.shape
    if n_eval is None or n_eval >= N:
        mu_e, lv_e = mu, logvar
    else:
        if n_eval < 1:
            raise ValueError("n_eval must be positive")
        gdev = mu.device if generator is None else generator.device
        idx = torch.randperm(N, device=gdev, generator=generator)[:n_eval].to(mu.device)
        mu_e, lv_e = mu[idx], logvar[idx]
    z = (mu_e + _randn(mu_e.shape, mu.device, generator) * torch.exp(0.5 * lv_e)).contiguous()
    lse_joint, lse_dim = ops.agg_posterior_lse(z, mu, logvar)
    log_n = math.log(N)
    zd, md, ld = z.double(), mu_e.double(), lv_e.double()
    lqzx = (-0.5 * (LOG_2PI + ld + (zd - md) ** 2 * torch.exp(-ld))).sum(1)
    lqz = lse_joint - log_n
    lqd = lse_dim.double() - log_n
    lqprod = lqd.sum(1)
    lpz = (-0.5 * (LOG_2PI + zd ** 2)).sum(1)
    mu64, lv64 = mu.double(), logvar.double()
    kl_dim = (0.5 * (mu64 ** 2 + torch.exp(lv64) - lv64 - 1.0)).mean(0)
    return dict(mi=(lqzx - lqz).mean(), tc=(lqz - lqprod).mean(), dwkl=(lqprod - lpz).mean(), kl=kl_dim.sum(),
                h_joint=-lqz.mean(), h_dim=-lqd.mean(0), kl_dim=kl_dim,
                active_units=(mu64.var(0, unbiased=False) > threshold).sum())


def mig(mu, logvar, factors, n_eval_per_value=None, generator=None):
    """The mutual-information gap (Chen et al. 2018, section 4.1) against integer ``factors`` ([N] or [N, K], e.g. the
    image-folder labels).  One z = mu + eps sigma is drawn per row.  Per factor k the rows are sorted by value once; for
    every value v the evaluation points are (the first ``n_eval_per_value`` of) its rows, scored against the value's own
    posteriors -- a contiguous slice: pointer offsets, no mask -- for H(z_d | v), and all of the factor's evaluation
    points against all N posteriors, each weighted by p(v) over its value's count, for H(z_d).  Then

      I(z_d; v_k) = H(z_d) - sum_v p(v) H(z_d | v)      MIG_k = (largest - second largest over d) / H(v_k)

    Keys: ``mig`` (the mean over k), ``mig_per_factor`` [K], ``mi_matrix`` [D, K]; fp64 device tensors.  A factor with a
    single value (H(v) = 0) and D = 1 (no second-largest dimension) raise ``ValueError``."""
    mu, logvar = _posteriors(mu, logvar)
    N, D = mu.shape
    if D < 2:
        raise ValueError("mig needs at least two latent dimensions: there is no second-largest one")
    factors = torch.as_tensor(factors)
    if factors.is_floating_point() or factors.dtype == torch.bool or factors.dim() not in (1, 2) or factors.shape[0] != N:
        raise ValueError("factors must be an integer tensor [N] or [N, K]")
    factors = factors.to(mu.device).reshape(N, -1)
    if n_eval_per_value is not None and n_eval_per_value < 1:
        raise ValueError("n_eval_per_value must be positive")
    z = mu + _randn(mu.shape, mu.device, generator) * torch.exp(0.5 * logvar)
    columns = []
    for k in range(factors.shape[1]):
        values, counts = torch.unique(factors[:, k], return_counts=True)
        counts = counts.tolist()
        if len(counts) < 2:
            raise ValueError(f"factor {k} has a single value: its entropy is zero and MIG is undefined")
        order = torch.sort(factors[:, k], stable=True).indices
        mu_s, lv_s, z_s = mu[order].contiguous(), logvar[order].contiguous(), z[order].contiguous()
        h_cond = torch.zeros(D, dtype=torch.float64, device=mu.device)
        points, weights, h_v, start = [], [], 0.0, 0
        for n_v in counts:
            n_e = n_v if n_eval_per_value is None else min(n_v, int(n_eval_per_value))
            p_v = n_v / N
            z_v = z_s[start:start + n_e]
            _, lse_dim = ops.agg_posterior_lse(z_v, mu_s[start:start + n_v], lv_s[start:start + n_v])
            h_cond -= p_v * (lse_dim.double().mean(0) - math.log(n_v))
            points.append(z_v)
            weights.append(torch.full((n_e,), p_v / n_e, dtype=torch.float64, device=mu.device))
            h_v -= p_v * math.log(p_v)
            start += n_v
        _, lse_dim = ops.agg_posterior_lse(torch.cat(points).contiguous(), mu, logvar)
        h_marg = -(torch.cat(weights)[:, None] * (lse_dim.double() - math.log(N))).sum(0)
        columns.append(((h_marg - h_cond), h_v))
    mi_matrix = torch.stack([c for c, _ in columns], dim=1)
    top = torch.topk(mi_matrix, 2, dim=0).values
    h_factors = torch.tensor([h for _, h in columns], dtype=torch.float64, device=mu.device)
    per_factor = (top[0] - top[1]) / h_factors
    return dict(mig=per_factor.mean(), mig_per_factor=per_factor, mi_matrix=mi_matrix)
