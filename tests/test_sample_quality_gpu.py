"""MI355X: `ops.pair_knn` / `ops.pair_hits` (csrc/pair_dist.hip) against the fp64 restatement of tests/_pair_refs.py --
exactly on small-integer inputs at every edge of the tiling, bit-identical over `splits`, runs and operand order, within
the DERIVED rounding bound on continuous data -- then `sample_quality.report` end to end inside the bracket that bound
leaves, and the routes that feed it (`fid.sample_features`, `BetaVAEGANTrainer.evaluate(sample_quality=...)`).

The bound: the kernel forms d2 as one chain of D fp32 FMAs over fp32 differences, so |d2 - d2_64| <= tol d2_64 with
tol = (D + 3) 2^-24 (`_pair_refs.tol_of`); the k-th order statistic of perturbed values moves by no more than the largest
perturbation; a count of `d2 <= thr` is bracketed by the pairs that are inside by more than tol and those inside or
outside by no more than tol.  Nothing here is a measured tolerance."""
import math

import pytest
import torch

import _pair_refs as R

pytestmark = pytest.mark.gpu

# (M, N, D): every M, N of {1, 2, 63, 64, 65, 130, 257} and every D of {1, 31, 33, 64, 2048} -- below, at and above one
# tile of 64 rows / columns, several row blocks and column tiles, D below / at / above one chunk of 32 dimensions and odd
EXACT_SHAPES = [(1, 1, 1), (2, 1, 31), (1, 2, 33), (63, 65, 64), (64, 64, 33), (65, 63, 31), (130, 257, 1), (257, 130, 64),
                (257, 257, 33), (64, 130, 2048), (65, 2, 2048), (2, 257, 2048), (130, 63, 31)]
SELF_SHAPES = [(1, 33), (2, 31), (63, 64), (64, 1), (65, 33), (130, 2048), (257, 31)]
CONTINUOUS_SHAPES = [(130, 193, 67), (65, 64, 131), (257, 130, 33), (100, 90, 2048)]
KS = (1, 3, 8)


def _ops():
    from disentangle_mlp_amd import ops
    return ops


def _thresholds_with_ties(dist, seed):
    """One threshold per column, taken from that column's own distances (so `d2 == thr` occurs in every column, for the
    chosen row and for every other row at the same distance) -- every third one a half below, to mix the outcomes."""
    M, N = dist.shape
    pick = torch.randint(0, M, (N,), generator=torch.Generator().manual_seed(seed)).to(dist.device)
    thr = dist[pick, torch.arange(N, device=dist.device)].clone()
    thr[::3] -= 0.5
    return thr.float()


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_on_small_integers(shape):
    """Integers in [-8, 8]: every d2 is an integer <= 2^19, exact in fp32 in any order, so the kernels must EQUAL the fp64
    restatement -- values, +inf tails where N < K, and every exact tie on a threshold.  The operands start one float
    past an aligned base."""
    M, N, D = shape
    ops = _ops()
    a, b = R.offset_by_one_float(R.integers(M, D, 1).cuda()), R.offset_by_one_float(R.integers(N, D, 2).cuda())
    assert a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 4
    dist = R.d2(a, b)
    for k in KS:
        got = ops.pair_knn(a, b, k=k)
        assert got.shape == (M, k) and got.dtype == torch.float32
        assert torch.equal(got.double(), R.knn_of(dist, k)), (shape, k)
        if N < k:
            assert bool(torch.isinf(got[:, N:]).all()) and bool(torch.isfinite(got[:, :N]).all())
    thr = R.offset_by_one_float(_thresholds_with_ties(dist, 3))
    assert int((dist == thr.double()[None, :]).sum()) >= (2 * N) // 3          # the ties are there
    got = ops.pair_hits(a, b, thr)
    assert got.shape == (M,) and got.dtype == torch.int32
    assert torch.equal(got.long(), R.hits_of(dist, thr)), shape
    if N >= 2:
        assert not torch.equal(R.hits_of(dist, thr), R.hits_of(dist, thr, strict=True))   # `<` would have failed here


@pytest.mark.parametrize("shape", SELF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_self_excluded_with_duplicates(shape):
    """`b=None`: row i skips column i BY INDEX.  Duplicates of row 0 are planted in other tiles (rows 70 and 200 where
    they exist, and the last row): their distance 0 must still count, once per duplicate.  N - 1 < K gives a +inf tail."""
    M, D = shape
    ops = _ops()
    a = R.integers(M, D, 5)
    dups = sorted({r for r in (70, 200, M - 1) if 0 < r < M})
    for r in dups:
        a[r] = a[0]
    a = R.offset_by_one_float(a.cuda())
    dist = R.d2(a, a)
    for k in KS:
        got = ops.pair_knn(a, k=k)
        assert torch.equal(got.double(), R.knn_of(dist, k, exclude_self=True)), (shape, k)
        zeros = min(len(dups), k)
        assert bool((got[0, :zeros] == 0).all())
        if M - 1 < k:
            assert bool(torch.isinf(got[:, M - 1:]).all())
    # the same set given twice is NOT self-excluded: every row finds itself at distance exactly 0
    assert bool((ops.pair_knn(a, a.clone(), k=1) == 0).all())


@pytest.fixture(scope="module")
def split_case():
    a, b = R.mixture(130, 33, 11).cuda(), R.mixture(1000, 33, 12).cuda()
    thr = R.knn(b, k=3)[:, 2].float()
    return a, b, thr


def test_splits_runs_and_operand_order_give_the_same_bits(split_case):
    ops = _ops()
    a, b, thr = split_case
    tiles = math.ceil(b.shape[0] / ops.PAIR_TILE)
    knn0, hits0 = ops.pair_knn(a, b, k=8), ops.pair_hits(a, b, thr)
    self0 = ops.pair_knn(b, k=8)
    assert torch.equal(knn0, ops.pair_knn(a, b, k=8)) and torch.equal(hits0, ops.pair_hits(a, b, thr))      # two runs
    ran = set()
    for splits in (1, 2, 7, tiles, tiles + 91):
        ran.add(ops.pair_splits(a.shape[0], b.shape[0], a.shape[1], splits))
        assert torch.equal(knn0, ops.pair_knn(a, b, k=8, splits=splits)), splits
        assert torch.equal(hits0, ops.pair_hits(a, b, thr, splits=splits)), splits
        assert torch.equal(self0, ops.pair_knn(b, k=8, splits=splits)), splits
    assert tiles == 16 and ran == {1, 2, 6, 16}                # (7 -> ranges of 3 tiles -> 6 of them; 16 + 91 is clamped)
    # d2(a_i, b_j) has the same bits whichever operand is which
    assert torch.equal(ops.pair_knn(a, b, k=1).min(), ops.pair_knn(b, a, k=1).min())
    assert torch.equal(ops.pair_knn(a, b, k=1).min(dim=0).values, ops.pair_knn(b, a, k=1).min(dim=0).values)


@pytest.fixture(scope="module", params=CONTINUOUS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def continuous(request):
    """(fake [M, D], real [N, D]) of one seeded mixture, and their fp64 distances -- computed once per shape."""
    M, N, D = request.param
    fake, real = R.mixture(M, D, 200).cuda(), R.mixture(N, D, 100).cuda()
    return fake, real, R.d2(fake, real), R.tol_of(D)


def test_continuous_knn_within_the_derived_bound(continuous):
    ops = _ops()
    fake, real, dist, tol = continuous
    for k in KS:
        got, want = ops.pair_knn(fake, real, k=k).double(), R.knn_of(dist, k)
        err = float(((got - want).abs() / want).max())
        print(f"[pair_knn] {tuple(dist.shape)} D={fake.shape[1]} k={k}: max relative error {err:.3e}, bound {tol:.3e}")
        assert bool(((got - want).abs() <= tol * want).all()), (k, err, tol)
        assert bool((got[:, 1:] >= got[:, :-1]).all())
    got, want = ops.pair_knn(real, k=5).double(), R.knn_of(R.d2(real, real), 5, exclude_self=True)
    assert bool(((got - want).abs() <= tol * want).all())


def test_continuous_hits_are_bracketed(continuous):
    ops = _ops()
    fake, real, dist, tol = continuous
    thr = R.knn_of(R.d2(real, real), 3, exclude_self=True)[:, 2].float()       # the thresholds are given: window tol
    open_pairs = R.undecided(dist, thr, tol)
    assert open_pairs <= 1e-3 * dist.numel(), open_pairs                        # from the reference alone
    lo = R.hits_of(dist, thr.double() * (1.0 - tol), strict=True)
    hi = R.hits_of(dist, thr.double() * (1.0 + tol))
    assert 0 < int(lo.sum()) and int((lo > 0).sum()) < dist.shape[0]            # neither vacuous nor saturated
    got = ops.pair_hits(fake, real, thr).long()
    print(f"[pair_hits] {tuple(dist.shape)}: {open_pairs} undecided pairs, counts sum {int(got.sum())} in "
          f"[{int(lo.sum())}, {int(hi.sum())}]")
    assert bool((lo <= got).all()) and bool((got <= hi).all())


def test_report_lies_inside_the_bracket(continuous):
    """End to end: the radii come from the kernel too, so a pair can be misjudged only within 2 tol of its radius."""
    from disentangle_mlp_amd import sample_quality as sq
    fake, real, dist, tol = continuous
    rr, ff = R.d2(real, real), R.d2(fake, fake)
    open_pairs = (R.undecided(dist, R.knn_of(rr, 3, True)[:, 2], 2 * tol) + R.undecided(dist, R.knn_of(rr, 5, True)[:, 4], 2 * tol)
                  + R.undecided(dist.t(), R.knn_of(ff, 3, True)[:, 2], 2 * tol))
    assert open_pairs <= 1e-3 * dist.numel(), open_pairs
    lo, hi = (R.metrics(real, fake, window=2 * tol, end=e) for e in (-1, +1))
    assert 0.0 < lo["precision"] and hi["precision"] < 1.0 and 0.0 < lo["recall"] and hi["recall"] < 1.0
    got = sq.report(real, fake, subsets=2, subset_size=50)
    print(f"[report] {tuple(dist.shape)}: {open_pairs} undecided pairs; got {got}; bracket {lo} .. {hi}")
    for name in ("precision", "recall", "density", "coverage"):
        assert lo[name] <= got[name] <= hi[name], (name, lo[name], got[name], hi[name])
    assert got["precision"] == sq.precision_recall(real, fake)["precision"]
    assert got["coverage"] == sq.density_coverage(real, fake)["coverage"]
    assert math.isfinite(got["kid"]) and got["kid_std"] >= 0.0


# ---- the routes ------------------------------------------------------------------------------------------------------
N_HIDDEN, N_FEATURES = 16, 24


class _Projection:
    """A seeded random-projection extractor on device uint8 images [n, h, w, 3] -> [n, 24] fp32; counts its calls."""

    def __init__(self):
        self.proj = (torch.randn(64 * 64 * 3, N_FEATURES, generator=torch.Generator().manual_seed(21)) / 64.0).cuda()
        self.calls = 0

    def __call__(self, u8):
        self.calls += 1
        return (u8.reshape(u8.shape[0], -1).float() / 255.0) @ self.proj


@pytest.fixture(scope="module")
def trainer():
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer, ModelOpt
    torch.manual_seed(31)
    return BetaVAEGANTrainer(device="cuda", opt=ModelOpt(n_hidden=N_HIDDEN))


@pytest.fixture(scope="module")
def real_features():
    g = torch.Generator().manual_seed(22)
    return (torch.randn(40, N_FEATURES, generator=g) * 0.3 + 1.5).cuda()


def test_sample_features_are_what_sample_statistics_folds(trainer):
    from disentangle_mlp_amd import fid
    ex = _Projection()
    torch.manual_seed(9)
    feats = fid.sample_features(trainer.netEG.decode, 12, N_HIDDEN, ex)
    assert feats.shape == (12, N_FEATURES) and feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous()
    torch.manual_seed(9)
    mu, sigma = fid.sample_statistics(trainer.netEG.decode, 12, N_HIDDEN, ex)
    got = fid.ActivationStatistics(N_FEATURES, "cuda").update(feats).finalize()
    assert torch.equal(got[0], mu) and torch.equal(got[1], sigma) and ex.calls == 2
    torch.manual_seed(9)
    pieces = fid.sample_features(trainer.netEG.decode, 12, N_HIDDEN, ex, decode_batch=5, eval_mode=True)
    assert pieces.shape == (12, N_FEATURES) and ex.calls == 5 and trainer.netEG.training


def test_evaluate_reports_sample_quality_and_shares_the_features(trainer, real_features, tmp_path, monkeypatch):
    from disentangle_mlp_amd import fid, ops
    reference, real_file = str(tmp_path / "reference.npz"), str(tmp_path / "real.npz")
    fid.save_features(real_file, real_features)
    fid.save_statistics(reference, *fid.load_statistics(real_file))
    ck, kid_args = str(tmp_path / "checkpoint.pt"), {"subsets": 3, "subset_size": 10}
    trainer.save(ck, 1)
    common = dict(n_samples=12, fid_path_pretrained=reference, fid_on_device=True)

    ex = _Projection()
    torch.manual_seed(4)
    plain = trainer.evaluate([ck], calc_fid=True, fid_feature_extractor=ex, **common)
    assert ex.calls == 1 and "sample_quality" not in plain[0] and math.isfinite(plain[0]["FID"])

    ex = _Projection()
    torch.manual_seed(4)
    both = trainer.evaluate([ck], calc_fid=True, fid_feature_extractor=ex, sample_quality=real_file,
                            sample_quality_args=kid_args, **common)
    assert ex.calls == 1                                       # once per batch: the FID came from the same features
    assert both[0]["FID"] == plain[0]["FID"]
    assert {k: v for k, v in both[0].items() if k != "sample_quality"} == plain[0]
    report = both[0]["sample_quality"]
    assert set(report) == {"precision", "recall", "density", "coverage", "kid", "kid_std"}
    assert all(isinstance(v, float) and math.isfinite(v) for v in report.values())

    ex = _Projection()
    torch.manual_seed(4)
    alone = trainer.evaluate([ck], fid_feature_extractor=ex, sample_quality=real_features, sample_quality_args={"kid": False},
                             n_samples=12)
    assert ex.calls == 1 and alone[0]["FID"] == "N/A"
    assert alone[0]["sample_quality"] == {k: report[k] for k in ("precision", "recall", "density", "coverage")}

    def unreachable(*a, **k):
        raise AssertionError("a csrc/pair_dist.hip kernel without the keyword")
    monkeypatch.setattr(ops, "pair_knn", unreachable)
    monkeypatch.setattr(ops, "pair_hits", unreachable)
    torch.manual_seed(4)
    again = trainer.evaluate([ck], calc_fid=True, fid_feature_extractor=_Projection(), **common)
    assert again == plain
