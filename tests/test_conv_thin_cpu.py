"""CPU: the references of tests/_thin_refs.py for the kernels of the 3-channel edge layers (csrc/conv_thin_fwd.hip,
csrc/conv_thin_mfma.hip, csrc/conv_thin.hip) -- no GPU, no kernel; the library is asked host-only questions (which shapes
it takes, the statistics slots).

1. emul64 stays within the split model of ref64 on every case, for both plane counts: |emul64 - ref64| <= 2^-23 mag
   (three planes), 3 x 2^-16 mag (two); with an affine on load 3 x 2^-24 mag more (the fp64-activated input of ref64
   against the fp32 one of emul64: one rounding of the activated input to fp32, two for the fma's product and sum).
2. ACC_WORST is measured per kernel from restate32 against emul64 over every case of the GPU file, and the unmutated
   restatement passes the GPU file's checks -- the general one on every case, the one-pixel one at every placement.
3. Every mutation of T.MUTATIONS applied to the restatement is rejected by at least one case, under the bound that case
   is judged with on the GPU (general or one-pixel).
4. The tables reach every instantiation written in the three dispatch switches (read from the sources), the band /
   strip / group counts a case claims are the library's, and the refused table agrees with the host-only queries.
"""
import math
import os
import re

import pytest
import torch

import _thin_refs as T

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "disentangle_mlp_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- 1. the split model
@pytest.mark.parametrize("case", [c for c in T.FWD_CASES + T.TRANSPOSED if c.planes == 3], ids=lambda c: c.id)
def test_split_is_within_the_documented_model(case):
    x, w, bias = T.operands(case)
    ref, m = T.ref64(case, x, w, bias), T.mag(case, x, w, bias)
    for NP in (2, 3):
        c = case._replace(planes=NP)
        r = T.ratio(T.emul64(c, x, w, bias), ref, m)
        print(f"{c.id}: residual 2^{math.log2(max(r, 1e-300) * T.U):.1f} mag against 2^{math.log2(T.split_bound(c)):.1f}")
        assert r * T.U <= T.split_bound(c), (c, r)


@pytest.mark.parametrize("act", [T.ACT_NONE, T.ACT_RELU, T.ACT_LRELU])
@pytest.mark.parametrize("case", T.AFFINE_CASES, ids=lambda c: c.id)
def test_split_model_with_an_affine(case, act):
    x, w, bias = T.operands(case)
    affine = T.affine_of(case, act)
    ref, m = T.ref64(case, x, w, bias, affine), T.mag(case, x, w, bias, affine)
    for NP in (2, 3):
        c = case._replace(planes=NP)
        r = T.ratio(T.emul64(c, x, w, bias, affine), ref, m)
        assert r * T.U <= T.split_bound(c) + 3 * T.U, (c, act, r)


def test_valu_reference_is_the_plain_one():
    case = T.VALU_CASES[1]
    x, w, bias = T.operands(case)
    assert torch.equal(T.emul64(case, x, w, bias), T.ref64(case, x, w, bias))


# ---------------------------------------------------------------------------------------------------- 2. K_ACC
_clean = {}


def _clean_case(case, act=None):
    """(x, w, bias, affine, emul64, mag, worst ratio) of a case, after the unmutated restatement passed the check on it."""
    key = (case, act)
    if key not in _clean:
        x, w, bias = T.operands(case)
        affine = None if act is None else T.affine_of(case, act)
        ref, m = T.emul64(case, x, w, bias, affine), T.mag(case, x, w, bias, affine)
        k = T.k_of(case, affine is not None)
        ok, worst = T.check(T.restate32(case, x, w, bias, affine), ref, m, torch.full_like(m, k))
        assert ok, (case, act, worst)                  # the reference alone: every element inside the bound
        _clean[key] = (x, w, bias, affine, ref, m, worst)
    return _clean[key]


def test_k_acc_is_measured_from_the_restatement():
    """Worst |restate32 - emul64| / (2^-24 mag) per kernel over its table, bias on."""
    for kind, table in T.TABLES.items():
        worst = 0.0
        for case in table:
            w_ = _clean_case(case)[-1]
            print(f"{case.id:28s} {w_:5.2f} x 2^-24   (cap {T.cap_of(case)}, k {T.k_of(case)})")
            assert math.isfinite(w_)
            worst = max(worst, w_)
        print(f"{T.KERNEL[kind]}: worst {worst:.3f}; ACC_WORST = {T.ACC_WORST[kind]}, K_ACC = ceil(4 x ACC_WORST) = {T.K_ACC[kind]}")
        assert 0.8 * T.ACC_WORST[kind] <= worst <= T.ACC_WORST[kind], (T.KERNEL[kind], worst)
        assert T.K_ACC[kind] == math.ceil(4 * T.ACC_WORST[kind])


@pytest.mark.parametrize("act", [T.ACT_NONE, T.ACT_RELU, T.ACT_LRELU])
@pytest.mark.parametrize("case", T.AFFINE_CASES, ids=lambda c: c.id)
def test_restatement_passes_with_an_affine(case, act):
    print(f"{case.id} act {act}: {_clean_case(case, act)[-1]:.2f} x 2^-24")


def _pixel_run(case, place, mut=None):
    """(ok under the one-pixel bound, its worst share, ok under the general bound) of the restatement on a one-pixel input."""
    x, (_, w, _) = T.pixel_input(case, place), T.operands(case)
    y = T.restate32(case, x, w, None, mut=mut)
    ok, share = T.pixel_judge(case, y[1], T.ref64(case, x, w, None)[1])
    m = T.mag(case, x, w, None)
    return ok, share, T.check(y, T.emul64(case, x, w, None), m, torch.full_like(m, T.k_of(case)))[0]


@pytest.mark.parametrize("case", T.PIXEL_CASES, ids=lambda c: c.id)
def test_restatement_passes_the_one_pixel_bound(case):
    planes = T.planes3(torch.tensor(T.PIXEL_VALUE), 3)
    assert all(float(p) != 0 for p in planes) and float(sum(p.double() for p in planes)) == T.PIXEL_VALUE
    places = T.pixel_places(case)
    assert len(places) == 4 + (case.strips > 1) + (case.bands > 1) or case.H == 1 or case.W == 1
    for place in places:
        ok, share, general = _pixel_run(case, place)
        print(f"{case.id} pixel {place}: {share:.3f} of the one-pixel bound ({T.pixel_bound(case) / T.U:.2f} x 2^-24 |w v|)")
        assert ok and general, (case, place, share)


# ---------------------------------------------------------------------------------------------------- 3. mutations
# mutation -> [(case, activation of the affine or None, "general" | "pixel")]: the smallest cases that can show each
F1, F2, TT, V = T.FWD1, T.FWD2, T.TRANSPOSED, T.VALU_CASES
MUT_CASES = {
    T.FWD: {
        **{m: [(F1[3], None, "pixel"), (F2[2], None, "pixel")] for m in T.MUTATIONS[T.FWD] if m.startswith("drop_")},
        "zero_tap_let_through": [(F1[4], None, "general"), (F2[2], None, "general")],
        "channel_not_zeroed": [(F1[2], None, "general"), (F1[3], None, "general")],
        "d1_forgotten": [(F1[0], None, "general"), (F2[0], None, "general")],
        "band_last_row_off_by_one": [(F1[3], None, "general"), (F2[2], None, "general")],      # (the row below exists)
        "wid_decode_swapped": [(F1[4], None, "general"), (F1[5], None, "general")],
        "short_band_row_stored": [(F1[1], None, "general"), (F2[2], None, "general")],
    },
    T.TR: {
        **{m: [(TT[3], None, "pixel"), (TT[4], None, "pixel")] for m in T.MUTATIONS[T.TR] if m.startswith("drop_")},
        "bias_per_kw": [(TT[0], None, "general")],
        "antidiagonal_off_by_one": [(TT[1], None, "general")],
        "row_buffer_parity": [(TT[1], None, "general"), (TT[3], None, "general")],
        "halo_not_zero": [(TT[1], None, "general")],
        "pad_before_act": [(TT[3], T.ACT_RELU, "general"), (TT[1], T.ACT_LRELU, "general"), (TT[1], T.ACT_NONE, "general")],
    },
    T.VALU: {
        "tail_reads_previous_chunk": [(V[3], None, "general")],
    },
}


def test_every_mutation_has_cases():
    for kind, muts in T.MUTATIONS.items():
        assert set(MUT_CASES[kind]) == set(muts)
        assert all(c in T.TABLES[kind] for cs in MUT_CASES[kind].values() for c, _, _ in cs)
        assert all(c in T.PIXEL_CASES for cs in MUT_CASES[kind].values() for c, _, how in cs if how == "pixel")
    assert len([m for m in T.MUTATIONS[T.FWD] if m.startswith("drop_")]) == 6 == len([m for m in T.MUTATIONS[T.TR] if m.startswith("drop_")])
    assert all(c.Cin < 3 for c, _, _ in MUT_CASES[T.FWD]["channel_not_zeroed"])
    assert all(c.out_hw[0] % c.rows_per_band for c, _, _ in MUT_CASES[T.FWD]["short_band_row_stored"])
    assert all(c.strips > 1 and c.groups > 1 for c, _, _ in MUT_CASES[T.FWD]["wid_decode_swapped"])
    assert all(c.Cin > 8 and c.Cin % 8 for c, _, _ in MUT_CASES[T.VALU]["tail_reads_previous_chunk"])


@pytest.mark.parametrize("kind,mut", [(k, m) for k in T.MUTATIONS for m in T.MUTATIONS[k]], ids=lambda v: T.KERNEL.get(v, v) if isinstance(v, int) else v)
def test_mutation_is_caught(kind, mut):
    caught = 0
    for case, act, how in MUT_CASES[kind][mut]:
        if how == "pixel":
            oks = []
            for place in T.pixel_places(case):
                ok, share, _ = _pixel_run(case, place, mut)
                oks.append(ok)
                print(f"{mut} at {case.id}, pixel {place}: {share:.3g} of the one-pixel bound")
            ok = all(oks)
        else:
            x, w, bias, affine, ref, m, _ = _clean_case(case, act)
            ok, worst = T.check(T.restate32(case, x, w, bias, affine, mut=mut), ref, m, torch.full_like(m, T.k_of(case, affine is not None)))
            print(f"{mut} at {case.id} act {act}: worst {worst:.3g} x 2^-24 against k = {T.k_of(case, affine is not None)}")
        caught += not ok
    assert caught == len(MUT_CASES[kind][mut]), (mut, caught)      # (more than the one asked for: every listed case rejects it)


def test_dropped_products_of_two_planes_are_caught_by_the_general_bound():
    for case in (T.FWD1[7], T.TRANSPOSED[6]):
        assert case.planes == 2
        x, w, bias, _, ref, m, _ = _clean_case(case)
        for mut in ("drop_w1x0", "drop_w0x1", "drop_w0x0"):
            ok, worst = T.check(T.restate32(case, x, w, bias, mut=mut), ref, m, torch.full_like(m, T.k_of(case)))
            print(f"{mut} at {case.id}: worst {worst:.3g} x 2^-24")
            assert not ok


# ---------------------------------------------------------------------------------------------------- 4. coverage, geometry, refusals
def test_the_tables_reach_every_instantiation():
    fwd = {(int(s), int(n)) for s, n in re.findall(r"conv_thin_fwd_kernel<(\d), (\d)>", _source("conv_thin_fwd.hip"))}
    assert fwd == {(s, n) for s in (1, 2) for n in (2, 3)}
    assert {(c.stride, c.planes) for c in T.FWD_CASES} == fwd
    tr = {(int(c), int(n)) for c, n in re.findall(r"launch_thin_mfma<(\d), (\d)>\(A", _source("conv_thin_mfma.hip"))}
    assert tr == {(c, n) for c in (1, 2, 3) for n in (2, 3)}
    assert {(c.Cout, c.planes) for c in T.TRANSPOSED} == tr
    valu = {int(c) for c in re.findall(r"launch_thin<(\d)>\(x", _source("conv_thin.hip"))}
    assert valu == {1, 2, 3, 4} == {c.Cout for c in T.VALU_CASES}


def test_the_tables_reach_the_launch_edges():
    f = T.FWD_CASES
    assert {c.waves for c in f} >= {1, 2, 3, 4, 6, 8} and {(c.strips, c.groups) for c in f} >= {(8, 1), (2, 4), (3, 2), (1, 3)}
    assert {c.Cin for c in f if c.stride == 1} == {1, 2, 3} == {c.Cin for c in f if c.stride == 2}
    for S in (1, 2):
        rows = {c.out_hw[0] % c.rows_per_band for c in f if c.stride == S}
        assert 0 in rows and 1 in rows                                          # whole bands and a one-row last band
        assert any(c.Cout % 32 == 0 for c in f if c.stride == S) and any(c.Cout % 32 == 1 for c in f if c.stride == S)
    assert any(c.W + 4 > 64 and (c.W + 4) % 64 for c in f)                      # a ragged second staging piece
    t = T.TRANSPOSED
    assert {c.waves for c in t} >= {1, 2, 3, 4, 8} and {c.H % 16 for c in t} >= {0, 1, 5} and max(c.bands for c in t) == 3
    v = T.VALU_CASES
    assert {c.W % 4 == 0 for c in v} == {True, False} and {c.Cin % 8 for c in v} >= {0, 1, 4, 5} and max(c.strips for c in v) == 3
    assert any(c.H == 16 and c.W == 64 for c in v) and any(c.W % 64 == 4 for c in v)
    assert max(c.B * c.Cin * c.H * c.W for c in T.all_cases()) <= 3 * 32 * 33 * 128


@pytest.mark.parametrize("case", T.FWD_CASES, ids=lambda c: c.id)
def test_claimed_forward_geometry_is_the_librarys(lib, case):
    assert lib.vg_conv5x5_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout, case.stride) == 1
    floats = lib.vg_conv5x5_thin_bf16split_stats_floats(*case.shape, case.stride)
    assert floats == case.B * case.bands * case.strips * case.Cout * 2
    assert len(T.slot_regions(case)) == floats // (2 * case.Cout) and 1 <= case.waves <= 8
    assert sorted(s for s, *_ in T.slot_regions(case)) == list(range(case.B * case.bands * case.strips))


def test_claimed_routes_of_the_transposed_tables(lib):
    for case in T.TRANSPOSED:
        assert lib.vg_convT5x5_s1_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout) == 1, case
    for case in T.VALU_CASES:         # every shape the MFMA kernel refuses (Cin != 32, Cout 4, the width)
        assert lib.vg_convT5x5_s1_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout) == 0, case


def test_refused_table_agrees_with_the_queries(lib):
    for what, case, _kw, shape_ok in T.REFUSED_FWD:
        assert lib.vg_conv5x5_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout, case.stride) == int(shape_ok), what
        assert (lib.vg_conv5x5_thin_bf16split_stats_floats(*case.shape, case.stride) > 0) == shape_ok, what
    for what, case, _kw, shape_ok in T.REFUSED_TR:
        assert lib.vg_convT5x5_s1_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout) == int(shape_ok), what
    # one inside each limit is taken
    assert lib.vg_conv5x5_thin_bf16split_ok(3, 8, 96, 64, 1) == 1 and lib.vg_conv5x5_thin_bf16split_ok(3, 8, 256, 32, 1) == 1
    assert lib.vg_conv5x5_thin_bf16split_ok(3, 8, 64, 32, 2) == 1
    assert lib.vg_convT5x5_s1_thin_bf16split_ok(32, 8, 128, 3) == 1 and lib.vg_convT5x5_s1_thin_bf16split_ok(32, 8, 16, 3) == 1
