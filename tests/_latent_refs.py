"""The aggregate-posterior metrics of disentangle_mlp_amd/metrics.py restated in torch: the
definitions as they are written down, every pair term lq[m,j,d] = log N(z[m,d]; mu[j,d], exp(lv[j,d])) materialised as an
[M, N, D] tensor (`_tc_refs.pair_terms`).  Evaluated in fp64 it is the reference of tests/test_latent_metrics_*.py;
evaluated in fp32 it is the yardstick (`_tc_refs.bound`).  The evaluation points z are an INPUT (fp32, formed as the
module forms them: mu + eps * exp(lv / 2)), so that a test can hand over exactly the points the module drew.
Keep M * N * D <= 2e7."""
import math

import torch

from _tc_refs import LOG_2PI, bound, pair_terms, rel_err      # noqa: F401  (re-exported for the tests)


def make_inputs(M, N, D, kind="own", seed=0):
    """mu ~ N(0,1), lv ~ N(-1, 1.5^2) clamped to [-6, 2] (as `_tc_refs.make_inputs`), fp32; z: ``own`` -- drawn from the
    set's own posteriors (point m from row m mod N) -- or ``far`` -- independent N(0, 4) points."""
    g = torch.Generator().manual_seed(100003 * M + 1009 * N + D + seed)
    mu = torch.randn(N, D, generator=g)
    lv = (torch.randn(N, D, generator=g) * 1.5 - 1.0).clamp_(-6.0, 2.0)
    eps = torch.randn(M, D, generator=g)
    if kind == "own":
        rows = torch.arange(M) % N
        z = mu[rows] + eps * torch.exp(0.5 * lv[rows])
    else:
        z = 2.0 * eps
    return dict(z=z, mu=mu, lv=lv)


def lse(z, mu, lv, dtype=torch.float64):
    """-> (lse_joint [M], lse_dim [M, D]), unnormalised"""
    lq = pair_terms(z.to(dtype), mu.to(dtype), lv.to(dtype))
    return torch.logsumexp(lq.sum(2), dim=1), torch.logsumexp(lq, dim=1)


def elbo_decomposition(mu, lv, z, rows=None, dtype=torch.float64, threshold=1e-2):
    """z[m] is a point of posterior rows[m] (default: m)."""
    mu, lv, z = mu.to(dtype), lv.to(dtype), z.to(dtype)
    N = mu.shape[0]
    rows = torch.arange(z.shape[0]) if rows is None else rows
    lq = pair_terms(z, mu, lv)
    log_n = math.log(N)
    lqzx = (-0.5 * (LOG_2PI + lv[rows] + (z - mu[rows]) ** 2 * torch.exp(-lv[rows]))).sum(1)
    lqz = torch.logsumexp(lq.sum(2), dim=1) - log_n
    lqd = torch.logsumexp(lq, dim=1) - log_n
    lpz = (-0.5 * (LOG_2PI + z ** 2)).sum(1)
    kl_dim = (0.5 * (mu ** 2 + torch.exp(lv) - lv - 1.0)).mean(0)
    return dict(mi=(lqzx - lqz).mean(), tc=(lqz - lqd.sum(1)).mean(), dwkl=(lqd.sum(1) - lpz).mean(), kl=kl_dim.sum(),
                h_joint=-lqz.mean(), h_dim=-lqd.mean(0), kl_dim=kl_dim,
                active_units=(mu.var(0, unbiased=False) > threshold).sum(),
                identity=(lqzx - lpz).mean())


def mig(mu, lv, z, factors, n_eval_per_value=None, dtype=torch.float64):
    """z [N, D]: one point per row.  Per factor and value v: the evaluation points are the first `n_eval_per_value` rows
    (in dataset order) that carry v; H(z_d|v) scores them against the rows of v, H(z_d) scores all of the factor's
    evaluation points against all rows, each weighted p(v) / (its value's number of points)."""
    mu, lv, z = mu.to(dtype), lv.to(dtype), z.to(dtype)
    N, D = mu.shape
    factors = factors.reshape(N, -1)
    cols, h_factors = [], []
    for k in range(factors.shape[1]):
        f = factors[:, k]
        h_cond, h_marg, h_v = torch.zeros(D, dtype=dtype), torch.zeros(D, dtype=dtype), 0.0
        for v in torch.unique(f).tolist():
            rows = torch.nonzero(f == v).flatten()
            pts = rows if n_eval_per_value is None else rows[:n_eval_per_value]
            p_v = rows.numel() / N
            h_cond -= p_v * (torch.logsumexp(pair_terms(z[pts], mu[rows], lv[rows]), dim=1) - math.log(rows.numel())).mean(0)
            h_marg -= p_v * (torch.logsumexp(pair_terms(z[pts], mu, lv), dim=1) - math.log(N)).mean(0)
            h_v -= p_v * math.log(p_v)
        cols.append(h_marg - h_cond)
        h_factors.append(h_v)
    mi_matrix = torch.stack(cols, dim=1)
    top = torch.topk(mi_matrix, 2, dim=0).values
    per_factor = (top[0] - top[1]) / torch.tensor(h_factors, dtype=dtype)
    return dict(mig=per_factor.mean(), mig_per_factor=per_factor, mi_matrix=mi_matrix)
