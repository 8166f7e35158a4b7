"""The fp64 restatement the sample-quality tests compare against: all pairs formed from the DIFFERENCES of the fp32 inputs
widened to fp64, on whatever device the inputs are on; the metrics of disentangle_mlp_amd/sample_quality.py restated on
it, with a relative `window` on the radii for the bracketing tests; the seeded inputs those tests share."""
import math

import numpy as np
import torch

U = 2.0 ** -24      # fp32 unit roundoff


def tol_of(D):
    """|d2 - d2_64| <= tol d2_64 for d2 = a chain of D fp32 FMAs over fp32 differences: each difference carries one
    rounding (its square two), each of the D accumulations one -- (D + 2) u to first order, D + 3 with the higher orders."""
    return (D + 3) * U


def d2(a, b, rows=64):
    """[M, N] fp64: sum_d (a[i, d] - b[j, d])^2, in row chunks (never more than rows x N x D elements at once)."""
    a64, b64 = a.double(), b.double()
    return torch.cat([((a64[s:s + rows, None, :] - b64[None, :, :]) ** 2).sum(-1) for s in range(0, a64.shape[0], rows)])


def knn_of(dist, k, exclude_self=False):
    """[M, k] fp64 from a distance matrix: the k smallest per row, ascending, +inf where fewer exist."""
    dist = dist.clone()
    if exclude_self:
        dist.fill_diagonal_(math.inf)
    M, N = dist.shape
    out = torch.full((M, k), math.inf, dtype=torch.float64, device=dist.device)
    out[:, :min(k, N)] = dist.sort(dim=1).values[:, :k]
    return out


def knn(a, b=None, k=1):
    return knn_of(d2(a, a if b is None else b), k, exclude_self=b is None)


def hits_of(dist, thr, strict=False):
    """[M] int64: #{j : dist[i, j] <= thr[j]} (``<`` with ``strict``)."""
    t = thr.double()[None, :]
    return ((dist < t) if strict else (dist <= t)).sum(1)


def hits(a, b, thr):
    return hits_of(d2(a, b), thr)


def metrics(real, fake, k_pr=3, k_dc=5, window=0.0, end=0):
    """precision / recall / density / coverage restated.  ``end`` = 0: the definitions (``<=``).  ``end`` = -1 / +1: the
    lower / upper end of the bracket -- a pair counts only if it is inside by more than ``window`` relative (strictly),
    respectively if it is inside or outside by no more than ``window``."""
    rr, ff, fr = d2(real, real), d2(fake, fake), d2(fake, real)
    scale, strict = 1.0 + end * window, end < 0
    r_pr, r_dc = knn_of(rr, k_pr, True)[:, k_pr - 1] * scale, knn_of(rr, k_dc, True)[:, k_dc - 1] * scale
    r_fake = knn_of(ff, k_pr, True)[:, k_pr - 1] * scale
    nearest_fake = fr.min(dim=0).values
    return {"precision": float((hits_of(fr, r_pr, strict) > 0).double().mean()),
            "recall": float((hits_of(fr.t(), r_fake, strict) > 0).double().mean()),
            "density": float(hits_of(fr, r_dc, strict).double().sum() / (k_dc * fake.shape[0])),
            "coverage": float(((nearest_fake < r_dc) if strict else (nearest_fake <= r_dc)).double().mean())}


def undecided(dist, thr, window):
    """The number of pairs within ``window`` relative of their threshold: those the bracket leaves open."""
    t = thr.double()[None, :]
    return int(((dist >= t * (1.0 - window)) & (dist <= t * (1.0 + window))).sum())


def kid_numpy(real, fake, perms, degree=3, gamma=None, coef0=1.0):
    """KID restated in numpy fp64, given the (real, fake) index subsets: mean and population standard deviation of the
    unbiased MMD^2 of each pair of subsets, the sums taken term by term."""
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    gamma = 1.0 / real.shape[1] if gamma is None else gamma
    vals = []
    for pr, pf in perms:
        x, y = real[np.asarray(pr)], fake[np.asarray(pf)]
        m = x.shape[0]
        kxx, kyy, kxy = ((gamma * np.einsum("id,jd->ij", p, q) + coef0) ** degree for p, q in ((x, x), (y, y), (x, y)))
        off = ~np.eye(m, dtype=bool)
        vals.append(kxx[off].sum() / (m * (m - 1)) + kyy[off].sum() / (m * (m - 1)) - 2.0 * kxy.mean())
    return float(np.mean(vals)), float(np.std(vals))


def integers(M, D, seed):
    """Small integers in [-8, 8] as fp32: every d2 is an integer <= 2^19 at D = 2048, exact in fp32 in any order."""
    return torch.randint(-8, 9, (M, D), generator=torch.Generator().manual_seed(seed)).float()


def mixture(M, D, seed, centres_seed=7):
    """A seeded mixture of 4 Gaussian clusters (centres shared by every set of one ``centres_seed``) with per-row scales
    in [0.2, 1.5]: neighbours at every scale, radii that differ by an order of magnitude between rows."""
    centres = torch.randn(4, D, generator=torch.Generator().manual_seed(centres_seed)) * (2.0 / math.sqrt(D))
    g = torch.Generator().manual_seed(seed)
    which = torch.randint(0, 4, (M,), generator=g)
    scale = 0.2 + 1.3 * torch.rand(M, generator=g)
    return (centres[which] + scale[:, None] * torch.randn(M, D, generator=g) / math.sqrt(D)).float().contiguous()


def offset_by_one_float(x):
    """The same values in storage that starts one float past an allocation's (aligned) base."""
    base = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    base[1:] = x.reshape(-1)
    return base[1:].view(x.shape)
