"""CPU: the C ABI of csrc/pair_dist.hip as far as the host alone can tell, the argument checks of ops.pair_*, KID against
a numpy restatement, the glue of sample_quality.report over the fp64 restatement of tests/_pair_refs.py (it is the
reference of the GPU tests), and the feature files of fid.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _pair_refs as R
from conftest import ROOT


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vaegan_hip.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib_path():
    from disentangle_mlp_amd import build
    return build.build(verbose=False)


def test_entries_are_declared_bound_and_exported(lib_path):
    from disentangle_mlp_amd import _lib, ops
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    want = {"vg_pair_splits": (I, [I] * 4),
            "vg_pair_workspace_bytes": (Z, [I] * 5),
            "vg_pair_knn": (I, [P, P, I, P] + [I] * 5 + [P, Z, P]),
            "vg_pair_hits": (I, [P] * 4 + [I] * 4 + [P, Z, P])}
    text = _header()
    lib = ctypes.CDLL(lib_path)
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(sig[1]), name
        assert getattr(lib, name) is not None, name
    for define, value in (("VG_PAIR_TILE", ops.PAIR_TILE), ("VG_PAIR_MAX_K", ops.PAIR_MAX_K)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % define, text).group(1)) == value
    assert re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", text).group(1) == str(_lib.ABI_VERSION) == "7"      # only added


def test_host_side_plan(lib_path):
    """What needs no device: rejected sizes have no workspace and no split count, the workspace grows with the splits
    and with K, a split count above the number of column tiles is clamped, `splits = 0` is a function of the sizes."""
    from disentangle_mlp_amd import _lib, ops
    lib = ctypes.CDLL(lib_path)
    for name in ("vg_pair_splits", "vg_pair_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    splits = lib.vg_pair_splits
    size = lambda M, N, D, s, K=1: lib.vg_pair_workspace_bytes(M, N, D, K, s)
    for bad in ((0, 5, 5, 1), (5, 0, 5, 1), (5, 5, 0, 1), (5, 5, 4097, 1), (5, (1 << 20) + 1, 5, 1), ((1 << 20) + 1, 5, 5, 1),
                (5, 5, 5, -1)):
        assert size(*bad) == 0 and splits(*bad) == 0, bad
    assert size(5, 5, 5, 1, K=0) == 0 and size(5, 5, 5, 1, K=9) == 0
    assert size(5, 5, 4096, 1) > 0 and size(1, 1, 1, 0) > 0 and size(1 << 20, 1 << 20, 4096, 0, K=8) > 0
    T = ops.PAIR_TILE
    assert splits(10, T + 1, 3, 7) == 2 and splits(10, T, 3, 7) == 1
    assert splits(10, 5 * T, 3, 4) == 3                       # ranges of 2 tiles: the fourth would be empty
    assert splits(10, 7 * T, 3, 7) == 7 and splits(10, 7 * T, 3, 7 + 91) == 7
    assert size(10, 7 * T, 3, 7) > size(10, 7 * T, 3, 1)
    assert size(10, 7 * T, 3, 7, K=8) > size(10, 7 * T, 3, 7, K=1)
    assert size(10, T + 1, 3, 7) == size(10, T + 1, 3, 2)
    assert splits(10, 100 * T, 3, 0) == splits(10, 100 * T, 3, 0) >= 1
    assert 1 <= splits(50000, 50000, 2048, 0) <= 50000 // T + 1
    assert ops.pair_splits(10, 5 * T, 3, 4) == 3 and ops.pair_splits(10, 5 * T, 3) >= 1
    with pytest.raises(RuntimeError, match="negative"):
        ops.pair_splits(10, 10, 3, -1)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from disentangle_mlp_amd import ops
    a, b, thr = torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(5)
    for call in (lambda: ops.pair_knn(a), lambda: ops.pair_knn(a, b, k=2), lambda: ops.pair_hits(a, b, thr)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match="k must be in 1..8"):
            ops.pair_knn(a, b, k=k)
    with pytest.raises(RuntimeError, match="negative"):
        ops.pair_knn(a, b, splits=-1)
    with pytest.raises(RuntimeError, match="negative"):
        ops.pair_hits(a, b, thr, splits=-2)


# ---- KID -----------------------------------------------------------------------------------------------------------
def _two_sets(n_real=37, n_fake=29, d=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_real, d, generator=g), torch.randn(n_fake, d, generator=g) * 1.3 + 0.4


def _perms(n_real, n_fake, m, subsets, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randperm(n_real, generator=g)[:m].numpy(), torch.randperm(n_fake, generator=g)[:m].numpy())
            for _ in range(subsets)]


@pytest.mark.parametrize("kw", [{}, {"degree": 2, "gamma": 0.3, "coef0": 0.5}])
def test_kid_matches_the_numpy_restatement(kw):
    from disentangle_mlp_amd import sample_quality as sq
    real, fake = _two_sets()
    got = sq.kid(real, fake, subsets=6, subset_size=20, generator=torch.Generator().manual_seed(5), **kw)
    want = R.kid_numpy(real.numpy(), fake.numpy(), _perms(37, 29, 20, 6, 5), **kw)
    assert set(got) == {"kid", "kid_std"} and all(isinstance(v, float) for v in got.values())
    assert abs(got["kid"] - want[0]) <= 1e-12 * abs(want[0]), (got, want)
    assert abs(got["kid_std"] - want[1]) <= 1e-12 * abs(want[1]), (got, want)
    assert got["kid"] > 0.0                                   # the two sets differ in scale and mean


def test_kid_clamps_the_subset_size():
    from disentangle_mlp_amd import sample_quality as sq
    real, fake = _two_sets()
    got = sq.kid(real, fake, subsets=3, subset_size=1000, generator=torch.Generator().manual_seed(8))
    want = R.kid_numpy(real.numpy(), fake.numpy(), _perms(37, 29, 29, 3, 8))
    assert abs(got["kid"] - want[0]) <= 1e-12 * abs(want[0])
    with pytest.raises(ValueError, match="at least 2 rows"):
        sq.kid(real, fake[:1])


def test_kid_of_a_set_against_itself_is_not_positive():
    """Identical subsets: kxx = kyy = kxy, and the unbiased estimate is -(2 / m) (mean diagonal - mean off-diagonal) of the
    kernel matrix -- exactly that, and negative (Cauchy-Schwarz: the diagonal of a positive semi-definite matrix dominates
    on average).  An estimator that clamped at 0 or dropped the sign would fail here."""
    from disentangle_mlp_amd import sample_quality as sq
    real, _ = _two_sets()
    m, d = 20, real.shape[1]
    vals = []
    for s in range(4):
        idx = torch.randperm(37, generator=torch.Generator().manual_seed(s))[:m]
        x = real[idx]
        got = sq.kid(x, x, subsets=1, subset_size=37)          # clamped to m = 20: every row, both sides the same SET
        k = ((x.double() @ x.double().t()) / d + 1.0) ** 3
        want = -(2.0 / m) * float(k.diagonal().mean() - (k.sum() - k.diagonal().sum()) / (m * (m - 1)))
        assert abs(got["kid"] - want) <= 1e-12 * abs(want) and got["kid"] < 0.0 and got["kid_std"] == 0.0, (got, want)
        vals.append(got["kid"])
    assert max(vals) < 0.0


# ---- report's glue, over the fp64 restatement ----------------------------------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    """ops.pair_knn / ops.pair_hits replaced by the fp64 restatement, the calls recorded."""
    from disentangle_mlp_amd import ops
    calls = []

    def pair_knn(a, b=None, k=1, splits=None):
        calls.append(("knn", a.shape[0], None if b is None else b.shape[0], k))
        return R.knn(a, b, k).float()

    def pair_hits(a, b, thr, splits=None):
        calls.append(("hits", a.shape[0], b.shape[0]))
        return R.hits(a, b, thr).to(torch.int32)
    monkeypatch.setattr(ops, "pair_knn", pair_knn)
    monkeypatch.setattr(ops, "pair_hits", pair_hits)
    return calls


def test_report_of_a_set_against_itself(restated):
    from disentangle_mlp_amd import sample_quality as sq
    real, _ = _two_sets()
    out = sq.report(real, real.clone(), subsets=2, subset_size=10)
    assert set(out) == {"precision", "recall", "density", "coverage", "kid", "kid_std"}
    assert all(isinstance(v, float) for v in out.values())
    assert out["precision"] == out["recall"] == out["coverage"] == 1.0 and out["density"] > 0.0
    # the real radii of both k from ONE self-excluded call at the larger k; the second is the generated set's, at k_pr
    assert [c for c in restated if c[0] == "knn" and c[2] is None and c[1] == 37] == [("knn", 37, None, 5), ("knn", 37, None, 3)]
    assert set(sq.report(real, real, kid=False)) == {"precision", "recall", "density", "coverage"}


def test_report_of_two_far_apart_clusters(restated):
    from disentangle_mlp_amd import sample_quality as sq
    real, fake = _two_sets()
    out = sq.report(real, fake + 1000.0, kid=False)
    assert out == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    assert sq.precision_recall(real, fake + 1000.0) == {"precision": 0.0, "recall": 0.0}
    assert sq.density_coverage(real, fake + 1000.0) == {"density": 0.0, "coverage": 0.0}


def test_a_tie_exactly_on_a_radius_counts(restated):
    """1-D, by hand, k = 1.  real = {0, 2, 5, 9}: squared radii (nearest other real) 4, 4, 9, 16.  fake = {4, 13, 20}:
    squared radii 81, 49, 49.
      fake 4: 16 > 4 | 4 <= 4 TIE | 1 <= 9 | 25 > 16 -> in 2 balls.   fake 13: 169, 121, 64, 16 <= 16 TIE -> 1 ball.
      fake 20: none.   precision = 2/3, density = (2 + 1 + 0) / (1 * 3) = 1.
      coverage: nearest fake of each real, squared: 16 > 4 | 4 <= 4 TIE | 1 <= 9 | 16 <= 16 TIE -> 3/4.
      recall: real r inside a fake ball: 0: 16 <= 81; 2: 4 <= 81; 5: 1 <= 81; 9: 25 <= 81 -> 1.
    With `<` instead of `<=` the three ties fall out: precision 1/3, density 1/3, coverage 1/4."""
    from disentangle_mlp_amd import sample_quality as sq
    real, fake = torch.tensor([[0.0], [2.0], [5.0], [9.0]]), torch.tensor([[4.0], [13.0], [20.0]])
    assert sq.knn_radii(real, 1).tolist() == [4.0, 4.0, 9.0, 16.0]
    out = sq.report(real, fake, k_pr=1, k_dc=1, kid=False)
    assert out == {"precision": 2 / 3, "recall": 1.0, "density": 1.0, "coverage": 0.75}
    assert R.metrics(real, fake, 1, 1) == out                  # the restatement of the GPU tests says the same
    assert R.metrics(real, fake, 1, 1, window=1e-9, end=-1) == {"precision": 1 / 3, "recall": 1.0, "density": 1 / 3,
                                                                "coverage": 0.25}


def test_report_refuses_what_it_cannot_score(restated):
    from disentangle_mlp_amd import sample_quality as sq
    real, fake = _two_sets()
    bad = real.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        sq.report(bad, fake)
    bad[3, 2] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        sq.report(real, bad)
    with pytest.raises(ValueError, match="at least 6"):
        sq.report(real[:5], fake)                              # k_dc = 5 needs 6 real rows
    with pytest.raises(ValueError, match="at least 4"):
        sq.report(real, fake[:3])                              # k_pr = 3 needs 4 generated rows
    assert set(sq.report(real[:6], fake[:4], kid=False)) == {"precision", "recall", "density", "coverage"}
    with pytest.raises(ValueError, match="at least 4"):
        sq.precision_recall(real[:3], fake)


# ---- the feature files -----------------------------------------------------------------------------------------------
def test_feature_file_round_trip_and_fid(tmp_path):
    """One file serves the FID routes and the new metrics: `path_features` returns the rows bit for bit, and `get_fid`
    of the file gives what the statistics route gives today."""
    from disentangle_mlp_amd import fid
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(40, 12, generator=g) * 3.0 + 1.0
    other = torch.randn(50, 12, generator=g) * 2.0
    with_features, statistics_only, reference = (str(tmp_path / n) for n in ("f.npz", "s.npz", "ref.npz"))
    fid.save_features(with_features, feats)
    fid.save_statistics(statistics_only, *fid.calculate_activation_statistics(feats, device="cpu"))
    fid.save_statistics(reference, *fid.calculate_activation_statistics(other, device="cpu"))
    back = fid.path_features(with_features, device="cpu")
    assert back.dtype == torch.float32 and back.is_contiguous() and torch.equal(back, feats)
    with np.load(with_features) as f:
        assert sorted(f.files) == ["features", "mu", "sigma"]
    for a, b in zip(fid.load_statistics(with_features), fid.load_statistics(statistics_only)):
        assert np.array_equal(a, b)
    assert fid.get_fid(with_features, reference, device="cpu") == fid.get_fid(statistics_only, reference, device="cpu")
    with pytest.raises(RuntimeError, match="no `features` array"):
        fid.path_features(statistics_only, device="cpu")
    with pytest.raises(ValueError, match="n >= 2"):
        fid.save_features(str(tmp_path / "one.npz"), feats[:1])


def test_path_features_of_a_folder_follow_the_fid_rule(tmp_path):
    """An image folder: the same files, in the same order, with the same remainder rule as the FID of that folder --
    the statistics of the returned rows ARE `_handle_path`'s."""
    from PIL import Image
    from disentangle_mlp_amd import fid
    g = torch.Generator().manual_seed(4)
    for i in range(53):                                        # one batch of 50; the remainder of 3 is never propagated
        Image.fromarray(torch.randint(0, 256, (8, 8, 3), generator=g, dtype=torch.uint8).numpy()).save(tmp_path / f"{i:02d}.png")
    proj = torch.randn(8 * 8 * 3, 6, generator=g)
    seen = []

    def extractor(images):
        seen.append(images.shape[0])
        return torch.as_tensor(images).reshape(images.shape[0], -1) @ proj
    feats = fid.path_features(str(tmp_path), extractor, device="cpu")
    assert feats.shape == (50, 6) and feats.dtype == torch.float32 and seen == [50]
    mu, sigma = fid._handle_path(str(tmp_path), extractor, "cpu")
    want = fid.ActivationStatistics(6, "cpu").update(feats).finalize()
    assert torch.equal(mu, want[0]) and torch.equal(sigma, want[1])
    with pytest.raises(RuntimeError, match="Inception pool_3"):
        fid.path_features(str(tmp_path), None, device="cpu")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(RuntimeError, match="no \\*.jpg"):
        fid.path_features(str(empty), extractor, device="cpu")
