"""Sample quality beyond FID, from two sets of features [n, d] on the device (the pool_3 activations `fid.sample_features`
/ `fid.path_features` keep): improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al.
2020) and KID (Binkowski et al. 2018).  DESIGN.md section 4.25.

FID is one scalar that mixes fidelity and diversity and is biased at the 1000 samples `fit` / `evaluate` score; a beta /
lambda / objective sweep asks which of the two a setting paid with.  Precision and density are fidelity (do the generated
samples lie where real ones do), recall and coverage diversity (are the real samples reached), KID an unbiased distance
at small sample counts.

Precision / recall / density / coverage are k-nearest-neighbour radii and ball-membership counts over all pairs of the
two sets: `ops.pair_knn` / `ops.pair_hits` (csrc/pair_dist.hip: tiled, nothing of size M x N in memory, no atomics, the
same bits every run).  Distances and radii are SQUARED throughout -- the comparisons are the same and no square root
is taken.  Membership is ``d2 <= r2`` (Kynkaanniemi's code; the prdc package uses ``<``: the two differ on exact ties
only).  KID is a handful of fp64 matmuls on whatever device the features are on, like `fid.calculate_frechet_distance`,
and so also runs on CPU tensors.  Results are Python floats."""
import torch

from . import ops


def _features(x, name, k=None):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{name}: expected a [n, d] feature tensor")
    if k is not None and x.shape[0] < k + 1:
        raise ValueError(f"{name}: {x.shape[0]} rows, the {k}-th neighbour needs at least {k + 1}")
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{name}: the features are not finite")
    return x.float().contiguous()


def knn_radii(x, k):
    """[n] fp32: the SQUARED distance of every row of ``x`` to its ``k``-th nearest other row."""
    return ops.pair_knn(x, k=k)[:, k - 1].contiguous()


def _precision_recall(real, fake, r_real, r_fake):
    precision = (ops.pair_hits(fake, real, r_real) > 0).double().mean()
    recall = (ops.pair_hits(real, fake, r_fake) > 0).double().mean()
    return {"precision": float(precision), "recall": float(recall)}


def _density_coverage(real, fake, r_real, k):
    density = ops.pair_hits(fake, real, r_real).double().sum() / (k * fake.shape[0])
    coverage = (ops.pair_knn(real, fake, k=1)[:, 0] <= r_real).double().mean()
    return {"density": float(density), "coverage": float(coverage)}


def precision_recall(real, fake, k=3):
    """``{"precision", "recall"}``: the share of generated samples inside the union of the real samples' k-NN balls, and
    the share of real samples inside the union of the generated samples' balls."""
    real, fake = _features(real, "real", k), _features(fake, "fake", k)
    return _precision_recall(real, fake, knn_radii(real, k), knn_radii(fake, k))


def density_coverage(real, fake, k=5):
    """``{"density", "coverage"}``: the number of real k-NN balls a generated sample lies in, averaged and divided by k
    (unbounded above, 1 in expectation for identical distributions), and the share of real samples whose ball holds at
    least one generated sample."""
    real, fake = _features(real, "real", k), _features(fake, "fake")
    return _density_coverage(real, fake, knn_radii(real, k), k)


def kid(real, fake, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, generator=None, device=None):
    """``{"kid", "kid_std"}``: mean and standard deviation, over ``subsets`` random subsets of ``subset_size`` rows of
    each set (clamped to the smaller set), of the unbiased MMD^2 under k(x, y) = (gamma x.y + coef0)^degree, gamma = 1 / d
    by default: diagonals excluded, divisors m (m - 1) and m^2.  Each subset is ``torch.randperm(n, generator=generator)[:m]``
    on the CPU, the real one drawn first.  fp64 on ``device`` (default: the features')."""
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1]:
        raise ValueError("kid: expected two [n, d] feature tensors of one d")
    device = real.device if device is None else torch.device(device)
    real, fake = real.to(device=device, dtype=torch.float64), fake.to(device=device, dtype=torch.float64)
    d = real.shape[1]
    m = min(int(subset_size), real.shape[0], fake.shape[0])
    if m < 2 or int(subsets) < 1:
        raise ValueError("kid: needs at least one subset of at least 2 rows")
    gamma = 1.0 / d if gamma is None else float(gamma)
    vals = []
    for _ in range(int(subsets)):
        x = real[torch.randperm(real.shape[0], generator=generator)[:m].to(device)]
        y = fake[torch.randperm(fake.shape[0], generator=generator)[:m].to(device)]
        kxx, kyy, kxy = ((gamma * (p @ q.t()) + coef0) ** degree for p, q in ((x, x), (y, y), (x, y)))
        vals.append((kxx.sum() - kxx.diagonal().sum() + kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1))
                    - 2.0 * kxy.sum() / (m * m))
    vals = torch.stack(vals)
    return {"kid": float(vals.mean()), "kid_std": float(vals.std(unbiased=False))}


_kid = kid      # (`report` has a keyword of that name)


def report(real, fake, k_pr=3, k_dc=5, kid=True, **kid_args):
    """All of the above in one dict (``precision``, ``recall``, ``density``, ``coverage`` and, with ``kid``, ``kid`` /
    ``kid_std``); the real radii of both k come from ONE `ops.pair_knn` call.  ``ValueError`` for a non-finite feature
    set or one with fewer than k + 1 rows."""
    k_max = max(int(k_pr), int(k_dc))
    real, fake = _features(real, "real", k_max), _features(fake, "fake", int(k_pr))
    knn_real = ops.pair_knn(real, k=k_max)
    out = _precision_recall(real, fake, knn_real[:, k_pr - 1].contiguous(), knn_radii(fake, k_pr))
    out.update(_density_coverage(real, fake, knn_real[:, k_dc - 1].contiguous(), k_dc))
    if kid:
        out.update(_kid(real, fake, **kid_args))
    return out
