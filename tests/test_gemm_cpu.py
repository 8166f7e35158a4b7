"""CPU: the references of tests/_gemm_refs.py for the Linear fp16x3 GEMM (csrc/gemm_split.hip) -- no GPU, no kernel.

1. The split is what DESIGN.md section 2 and common.hpp say.  With a' = a 2^(14 - Ea) (exact; |a'| < 2^15), ha = rne16(a'),
   ra = a' - ha (exact in fp32), la = rne16(ra), da = a' - ha - la, and u = 2^-11 the unit roundoff of fp16:
     |ra| <= u |a'|;  |da| <= u |ra| <= 2^-22 |a'| where la is a normal fp16 number, |da| <= 2^-25 (half the subnormal
     spacing 2^-24) where it is not: |da| <= 2^-22 |a'| + 2^-25 always.  (|a'| < 2^-14: ha is on the 2^-24 grid
     already, |ra| <= 2^-25 rounds -- ties to even -- to la = 0.)
   The kernel forms ha hb + ha lb + la hb, so
     a'b' - kept = la lb + da b' + (a' - da) db,
     |la lb| <= u^2 (1 + u)^2 |a'b'| (+ cross terms in 2^-36 (|a'| + |b'|)),
   which sums to  |a'b' - kept| <= 3 x 2^-22 (1 + O(u)) |a'b'| + 2^-25 (1 + O(u)) (|a'| + |b'|).  Unscaled by
   2^(Ea - 14) 2^(Eb - 14), with Pa = 2^(Ea + 1) the power of two above A's bound, 2^-25 |b'| becomes 2^-40 Pa |b|:

     |emul64 - ref64| <= C_REL 2^-24 mag + C_ABS 2^-40 (Pa sum_k |B(n, k)| + Pb sum_k |A(m, k)|),
     C_REL = 12 (1 + 2^-9),  C_ABS = 1 + 2^-9          (the 2^-9 covers the O(u) terms)

   checked per element at exact bounds and at bounds loose by 2^1, 2^5, 2^10, with A spread over four and six decades.
   Measured here (pytest -s): the residual over 2^-24 mag is 0.3-1.5 at exact bounds up to four decades, 50 at six, 490
   at four decades with A's bound loose by 2^10 and 3.1e4 at six -- the absolute term is needed, a bound in mag alone is
   wrong for the reference itself (asserted below); the residual stays under a quarter of the model.
2. K_ACC is measured from restate32 against emul64 over every shape of the GPU file (R.ACC_WORST, R.K_ACC).
3. Every mutation of R.MUTATIONS applied to the restatement is rejected by the per-element check of the GPU file
   (R.check at R.k_acc), at the inputs the GPU file uses for that edge, while the unmutated restatement passes with
   every element inside the bound.
"""
import math

import pytest
import torch

import _gemm_refs as R

C_REL = 12.0 * (1 + 2.0 ** -9)
C_ABS = 1 + 2.0 ** -9


def _split_model(A, B, a_bound, b_bound):
    rel = R.U * R.mag(A, B)
    ab = 2.0 ** -40 * (R.pow2_bound(a_bound) * B.double().abs().sum(1)[None, :]
                       + R.pow2_bound(b_bound) * A.double().abs().sum(1)[:, None])
    return rel, ab


@pytest.mark.parametrize("decades", [0, 2, 4, 6])
@pytest.mark.parametrize("shape", [R.SMALL, R.SMALL_SPLIT], ids=str)
def test_split_is_within_the_documented_model(shape, decades):
    A, B, _ = R.matrices(*shape, decades=decades)
    print(f"split model: C_REL = {C_REL:.4f} (x 2^-24 mag), C_ABS = {C_ABS:.4f} (x 2^-40 (Pa |B| + Pb |A|))")
    ref = R.ref64(A, B)
    a0, b0 = R.bound_of(A), R.bound_of(B)
    for la in (0,) + R.LOOSE:
        for lb in (0,) + R.LOOSE:
            if la and lb and la != lb:
                continue                                  # A only, B only, both by the same factor
            ab, bb = a0 * 2.0 ** la, b0 * 2.0 ** lb
            res = (R.emul64(A, B, None, ab, bb) - ref).abs()
            rel, absl = _split_model(A, B, ab, bb)
            over_mag = float((res / rel).max())
            over_model = float((res / (C_REL * rel + C_ABS * absl)).max())
            print(f"{shape} decades {decades} loose 2^{la} / 2^{lb}: residual {over_mag:9.2f} x 2^-24 mag, "
                  f"{over_model:.3f} of the model")
            assert over_model <= 1.0, (shape, decades, la, lb, over_model)
            if decades <= 4 and not la and not lb:
                assert over_mag <= C_REL                  # exact bounds, moderate spread: the relative term alone
            if decades >= 4 and la == 10:
                assert over_mag > C_REL                   # ... which does not hold the reference at a loose bound


def test_planes_are_the_kernels_preparation():
    """Clamps of f16_bound_exp, exact scales, and hi + lo = the scaled value to 22 bits."""
    assert R.bound_exp(0.0) == 15 and R.bound_exp(1e-45) == 15 and R.bound_exp(2.0 ** -112) == 15
    assert R.bound_exp(2.0 ** -111) == 16 and R.bound_exp(1.0) == 127 and R.bound_exp(1.9999) == 127
    assert R.bound_exp(float("inf")) == 254 and R.bound_exp(float("nan")) == 254 and R.bound_exp(3e38) == 254
    for b in (0.0, 2.0 ** -100, 1.0, 3.0, 2.0 ** 100, float("inf")):
        s, u = R.scales(b)
        assert s * u == 1.0 and s == float(torch.tensor(s, dtype=torch.float32)) and u >= 2.0 ** -126
    x = torch.tensor([[3.0, -2.9999998, 1e-3, 3e-8, 0.0]])
    hi, lo = R.planes(x, 3.0)
    assert hi.dtype == lo.dtype == torch.float16 and float(hi.abs().max()) < 2.0 ** 15
    v = x.double() * R.scales(3.0)[0]
    assert bool(((hi.double() + lo.double() - v).abs() <= 2.0 ** -22 * v.abs() + 2.0 ** -25).all())
    assert float(lo[0, 3]) != 0.0 and abs(float(lo[0, 3])) < 2.0 ** -14      # a subnormal lo is kept


def test_k_acc_is_measured_from_the_restatement():
    """Worst |restate32 - emul64| / (2^-24 mag) per shape, bias on, exact bounds (and loose ones at the small shapes)."""
    worst = 0.0
    for (M, N, K) in R.all_shapes():
        A, B, bias = R.matrices(M, N, K)
        ks = R.ksplit_of(M, N, K)
        for loose in ((0,) + R.LOOSE if (M, N, K) in (R.SMALL, R.SMALL_SPLIT) else (0,)):
            ab, bb = R.bound_of(A) * 2.0 ** loose, R.bound_of(B) * 2.0 ** loose
            w = R.ratio(R.restate32(A, B, bias, ab, bb, ks), R.emul64(A, B, bias, ab, bb), R.mag(A, B, bias))
            print(f"M {M:4d} N {N:4d} K {K:5d} splits {ks:3d} loose 2^{loose:<2d}: {w:5.2f} x 2^-24   "
                  f"(cap 3K + splits = {3 * K + ks})")
            assert math.isfinite(w)
            worst = max(worst, w)
    print(f"worst {worst:.3f}; ACC_WORST = {R.ACC_WORST}, K_ACC = ceil(4 x ACC_WORST) = {R.K_ACC}")
    assert 0.8 * R.ACC_WORST <= worst <= R.ACC_WORST
    assert R.K_ACC == math.ceil(4 * R.ACC_WORST)
    assert R.k_acc(32, 1) == min(R.K_ACC, 97)


def test_split_counts_of_the_shapes():
    """The split shapes reach the split counts and per-split stage counts the GPU file claims to cover."""
    got = {(R.ksplit_of(M, N, K), K // R.ksplit_of(M, N, K) // R.GKC) for (M, N) in R.SPLIT_MNS for K in R.SPLIT_KS}
    assert got == R.SPLIT_COVER, got
    assert all(R.ksplit_of(*R.STAGE_MN, K) == 1 for K in R.STAGE_KS)
    assert [R.ksplit_of(M, N, K) for (M, N) in R.RAGGED_MN[:2] for K in R.RAGGED_KS] == [1, 2, 1, 2]
    assert R.ksplit_of(*R.SMALL) == 1 and R.ksplit_of(*R.SMALL_SPLIT) == 4


# ---------------------------------------------------------------------------------------------------- mutations
CASES = {
    "drop_lo_hi": [(*R.STAGE_MN, 32), (*R.STAGE_MN, 224), (130, 136, 2048)],
    "drop_hi_lo": [(*R.STAGE_MN, 32), (*R.STAGE_MN, 224), (130, 136, 2048)],
    "bias_every_split": [(128, 128, 512), (130, 136, 8192), (1, 3, 512)],
    "bias_no_split": [(*R.STAGE_MN, 32), (128, 128, 512), (130, 136, 8192), (128, 3, 96)],
    "skip_last_stage": [(*R.STAGE_MN, K) for K in R.STAGE_KS] + [(128, 128, 768), (130, 136, 1280), (130, 136, 8192)],
    "last_stage_twice": [(*R.STAGE_MN, K) for K in R.STAGE_KS] + [(128, 128, 768), (130, 136, 1280), (130, 136, 8192)],
    "slab_unwritten": [(128, 128, 512), (130, 136, 4096), (130, 136, 8192), (127, 257, 512)],
    "slab_twice": [(128, 128, 512), (130, 136, 4096), (130, 136, 8192), (127, 257, 512)],
    "pad_leak": [(1, 128, 96), (127, 128, 96), (129, 128, 512), (127, 257, 96)],
    "row_off_by_one": [(129, 128, 96), (129, 1, 512), (129, 129, 96), (130, 136, 1024)],
    "col_off_by_one": [(128, 129, 96), (128, 257, 512), (129, 129, 96), (130, 136, 1024)],
}


def test_every_mutation_has_cases():
    assert set(CASES) | {"group_scale0", "group_bound0"} == set(R.MUTATIONS)
    assert all(s in R.all_shapes() for ss in CASES.values() for s in ss)


_clean = {}


def _clean_case(shape):
    if shape not in _clean:
        M, N, K = shape
        A, B, bias = R.matrices(M, N, K)
        ab, bb, ks = R.bound_of(A), R.bound_of(B), R.ksplit_of(M, N, K)
        ref, m = R.emul64(A, B, bias, ab, bb), R.mag(A, B, bias)
        ok, w = R.check(R.restate32(A, B, bias, ab, bb, ks), ref, m, R.k_acc(K, ks))
        assert ok, (shape, w)                             # the unmutated restatement: every element inside the bound
        _clean[shape] = (A, B, bias, ab, bb, ks, ref, m)
    return _clean[shape]


@pytest.mark.parametrize("mut", sorted(CASES))
def test_mutation_is_caught(mut):
    for shape in CASES[mut]:
        A, B, bias, ab, bb, ks, ref, m = _clean_case(shape)
        assert ks > 1 or mut not in R.NEEDS_SPLIT, (mut, shape)
        ok, w = R.check(R.restate32(A, B, bias, ab, bb, ks, mut=mut), ref, m, R.k_acc(shape[2], ks))
        print(f"{mut} at {shape} (splits {ks}): worst {w:.3g} x 2^-24 against K = {R.k_acc(shape[2], ks)}")
        assert not ok, (mut, shape, w)


@pytest.mark.parametrize("shape", [R.SMALL, R.SMALL_SPLIT], ids=str)
def test_group_bound_mutations_are_caught(shape):
    """Group g scaled with group 0's bound -- unscaled with its own, or with group 0's as well: the groups of the GPU
    file's grouped case, whose bounds are decades apart on either side of group 0's.  No bias: next to a group a
    thousand times smaller the bias is most of `mag`, and a loss of the small rows' low bits would hide under it."""
    M, N, K = shape
    ks = R.ksplit_of(M, N, K)
    B, bias = R.matrices(M, N, K)[1], None
    As = [R.matrices(M, N, K, seed=10 + g)[0] * s for g, s in enumerate(R.GROUP_SCALES)]
    bounds, bb = [R.bound_of(a) for a in As], R.bound_of(B)
    for g, A in enumerate(As):
        ref, m = R.emul64(A, B, bias, bounds[g], bb), R.mag(A, B, bias)
        ok, w = R.check(R.restate32(A, B, bias, bounds[g], bb, ks), ref, m, R.k_acc(K, ks))
        assert ok, (g, w)
        if g == 0:
            continue
        for name, unscale in (("group_scale0", bounds[g]), ("group_bound0", bounds[0])):
            ok, w = R.check(R.restate32(A, B, bias, bounds[0], bb, ks, a_unscale_bound=unscale), ref, m, R.k_acc(K, ks))
            print(f"{name} group {g} at {shape}: worst {w:.3g} x 2^-24")
            assert not ok, (name, g, w)
