"""CPU: the references of tests/_general_refs.py for the general fp16x3 forward convolution (csrc/conv_general.hip) -- no
GPU, no kernel; the tuning library is asked one host-only question (which instantiation a launch takes).

1. emul64 stays within the documented split model of ref64 (tests/test_gemm_cpu.py has the
   derivation): per element
     |emul64 - ref64| <= C_REL 2^-24 mag + C_ABS 2^-40 (Px sum |w| + Pw sum |x|),
   Px / Pw the powers of two above the two bounds, the sums over the element's taps inside the image; at exact bounds and
   at bounds loose by 2^1 and 2^5.
2. K_ACC is measured from restate32 against emul64 over every case of the GPU file (G.ACC_WORST, G.K_ACC), and the
   unmutated restatement passes the GPU file's check with every element inside the bound.
3. Every mutation of G.MUTATIONS applied to the restatement is rejected by that check on the named cases of the tables
   (and, where a mutation needs an edge, is NOT rejected by a case without it: the edge is what the table is for).
4. The routes the tables claim are the library's (vg_debug_conv_general_tile: the launch's own cg_tile), the restated
   heuristic agrees with it on both sides of every switch, and the tables reach every instantiation of the source.
"""
import ctypes
import math
import os
import re

import pytest
import torch

import _gemm_refs as M
import _general_refs as G

C_REL = 12.0 * (1 + 2.0 ** -9)
C_ABS = 1 + 2.0 ** -9
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "disentangle_mlp_amd", "csrc")


def _bounds(x, w, loose=0):
    return G.bound_of(x) * 2.0 ** loose, G.bound_of(w) * 2.0 ** loose


# ---------------------------------------------------------------------------------------------------- 1. the split model
@pytest.mark.parametrize("case", [G.TILE_CASES[1], G.FILTER_CASES[2], G.FILTER_CASES[14], G.FILTER_CASES[-1], G.K_CASES[3]],
                         ids=lambda c: c.id)
def test_split_is_within_the_documented_model(case):
    x, w, bias = G.operands(case)
    ref, m = G.ref64(case, x, w, bias), G.mag(case, x, w, bias)
    sum_w = G._conv64(case, torch.ones_like(x).double(), w.double().abs())
    sum_x = G._conv64(case, x.double().abs(), torch.ones_like(w).double())
    for loose in (0, 1, 5):
        xb, wb = _bounds(x, w, loose)
        res = (G.emul64(case, x, w, bias, xb, wb) - ref).abs()
        model = C_REL * G.U * m + C_ABS * 2.0 ** -40 * (M.pow2_bound(xb) * sum_w + M.pow2_bound(wb) * sum_x)
        over = float((res / model).max())
        print(f"{case.id} loose 2^{loose}: residual {float((res / (G.U * m)).max()):7.2f} x 2^-24 mag, {over:.3f} of the model")
        assert over <= 1.0, (case, loose, over)


# ---------------------------------------------------------------------------------------------------- 2. K_ACC
_clean = {}


def _clean_case(case, relu=False, nonneg=False):
    """(operands, bounds, emul64, mag, worst ratio) of a case, after the unmutated restatement passed the check on it."""
    key = (case.geometry, relu, nonneg)
    if key not in _clean:
        x, w, bias = G.operands(case, nonneg=nonneg)
        xb, wb = _bounds(x, w)
        ref, m = G.emul64(case, x, w, bias, xb, wb, relu), G.mag(case, x, w, bias)
        ok, worst = G.check(G.restate32(case, x, w, bias, xb, wb, relu), ref, m, G.k_of(case))
        assert ok, (case, relu, worst)                 # the reference alone: every element inside the bound
        _clean[key] = (x, w, bias, xb, wb, ref, m, worst)
    return _clean[key]


def test_k_acc_is_measured_from_the_restatement():
    """Worst |restate32 - emul64| / (2^-24 mag) per case, bias on, ReLU off, exact bounds; the LOOSE cases at their
    loose bounds and the VARIANT_CASES with the non-negative input as well."""
    worst, seen = 0.0, set()
    for name, cases in G.GROUPS.items():
        lo, hi = math.inf, 0.0
        for case in cases:
            if case.geometry in seen:
                continue
            seen.add(case.geometry)
            w_ = _clean_case(case)[-1]
            print(f"  {case.id:44s} K {case.K:5d}: {w_:6.3f} x 2^-24   (cap 3K + 1 = {3 * case.K + 1})")
            assert math.isfinite(w_)
            lo, hi = min(lo, w_), max(hi, w_)
        print(f"{name}: {lo:.2f} - {hi:.2f}")
        worst = max(worst, hi)
        if name in G.VARIANT_CASES:
            w_ = _clean_case(G.VARIANT_CASES[name], nonneg=True)[-1]
            print(f"{name}: {G.VARIANT_CASES[name].id} with x >= 0: {w_:.3f}")
            worst = max(worst, w_)
    assert seen == {c.geometry for c in G.all_cases()}
    for case in G.LOOSE_CASES:
        x, w, bias = G.operands(case)
        for loose in G.LOOSE:
            xb, wb = _bounds(x, w, loose)
            w_ = G.ratio(G.restate32(case, x, w, bias, xb, wb), G.emul64(case, x, w, bias, xb, wb), G.mag(case, x, w, bias))
            print(f"loose: {case.id} 2^{loose}: {w_:.3f} x 2^-24")
            worst = max(worst, w_)
    print(f"worst {worst:.3f}; ACC_WORST = {G.ACC_WORST}, K_ACC = ceil(4 x ACC_WORST) = {G.K_ACC}")
    assert 0.8 * G.ACC_WORST <= worst <= G.ACC_WORST
    assert G.K_ACC == math.ceil(4 * G.ACC_WORST)


@pytest.mark.parametrize("nonneg", [False, True])
@pytest.mark.parametrize("group", G.MAIN_GROUPS)
def test_restatement_passes_with_relu(group, nonneg):
    case = G.VARIANT_CASES[group]
    print(f"{case.id} relu, x >= 0: {nonneg}: {_clean_case(case, relu=True, nonneg=nonneg)[-1]:.2f} x 2^-24")


def test_restatement_passes_without_bias():
    for case in (G.FILTER_CASES[2], G.TILE_CASES[1]):      # the pad-15 frame: mag = 0 there, the output exactly 0
        x, w, _ = G.operands(case)
        xb, wb = _bounds(x, w)
        ok, worst = G.check(G.restate32(case, x, w, None, xb, wb), G.emul64(case, x, w, None, xb, wb),
                            G.mag(case, x, w, None), G.k_of(case))
        assert ok, (case, worst)
    assert bool((G.mag(G.FILTER_CASES[2], *G.operands(G.FILTER_CASES[2])[:2], None) == 0).any())


# ---------------------------------------------------------------------------------------------------- 3. mutations
def _filter(k, s, p):
    return next(c for c in G.FILTER_CASES if (c.KH, c.KW, c.sh, c.sw, c.ph, c.pw) == (*k, *s, *p))


T64P = G.TILE_CASES[1]                 # forced 64 x 64, padded, Cout 33, three images of 5 x 7
# mutation -> (case, ReLU) it must be rejected on: the smallest cases of the tables that can show it
MUT_CASES = {
    "drop_lo_hi": [(G.K_CASES[1], False), (T64P, False), (G.K_CASES[5], False)],
    "drop_hi_lo": [(G.K_CASES[1], False), (T64P, False), (G.K_CASES[5], False)],
    "swap_kh_kw": [(_filter((1, 7), (1, 1), (0, 3)), False), (_filter((2, 4), (1, 1), (0, 0)), False), (T64P, False)],
    "swap_stride": [(_filter((3, 3), (1, 2), (1, 1)), False), (_filter((3, 3), (2, 1), (0, 0)), False)],
    "swap_pad": [(_filter((1, 7), (1, 1), (0, 3)), False), (_filter((7, 1), (1, 1), (3, 0)), False)],
    "tail_not_zero": [(G.K_CASES[0], False), (G.K_CASES[1], False), (G.K_CASES[3], False)],
    "pad_reads_clamped": [(T64P, False), (G.ONE_PIXEL[0], False), (_filter((1, 1), (1, 1), (15, 15)), False)],
    "bias_per_pixel": [(T64P, False), (G.K_CASES[1], False)],
    "relu_before_bias": [(T64P, True), (G.K_CASES[1], True)],
}
# ... and a case without the edge, on which the mutation changes nothing
MUT_BLIND = {
    "swap_kh_kw": G.K_CASES[2],                        # 1 x 1
    "swap_stride": T64P,                               # equal strides
    "swap_pad": T64P,                                  # equal pads
    "tail_not_zero": G.K_CASES[2],                     # K = 32: no entry beyond K
    "pad_reads_clamped": G.K_CASES[1],                 # unpadded
}


def test_every_mutation_has_cases():
    assert set(MUT_CASES) | {"image_stride_dense"} == set(G.MUTATIONS)
    table = {c.geometry for c in G.all_cases()}
    assert all(c.geometry in table for cs in MUT_CASES.values() for c, _ in cs)
    assert all(not c.pad and c.K % G.KC for c, _ in MUT_CASES["tail_not_zero"])
    assert all(c.pad for c, _ in MUT_CASES["pad_reads_clamped"])
    assert all(c.sh != c.sw for c, _ in MUT_CASES["swap_stride"]) and all(c.ph != c.pw for c, _ in MUT_CASES["swap_pad"])


@pytest.mark.parametrize("mut", sorted(MUT_CASES))
def test_mutation_is_caught(mut):
    for case, relu in MUT_CASES[mut]:
        x, w, bias, xb, wb, ref, m, _ = _clean_case(case, relu)
        ok, worst = G.check(G.restate32(case, x, w, bias, xb, wb, relu, mut=mut), ref, m, G.k_of(case))
        print(f"{mut} at {case.id}: worst {worst:.3g} x 2^-24 against k = {G.k_of(case)}")
        assert not ok, (mut, case, worst)
    if mut in MUT_BLIND:
        case = MUT_BLIND[mut]
        x, w, bias, xb, wb, _, _, _ = _clean_case(case)
        assert torch.equal(G.restate32(case, x, w, bias, xb, wb, mut=mut), G.restate32(case, x, w, bias, xb, wb)), (mut, case)


def slice_ok(case, buf, ref, m):
    """The GPU file's test_slices on a host buffer: the written channels inside their bounds, every other element
    bit-unchanged."""
    b, co = G.SLICE_BEFORE, case.Cout
    ok, worst = G.check(buf[:, b:b + co], ref, m, G.k_of(case))
    rest = torch.cat([buf[:, :b], buf[:, b + co:]], dim=1)
    return ok and bool((rest == G.GUARD).all()), worst


def test_image_stride_mutation_is_caught_where_a_tile_straddles_two_images():
    straddling, aligned = G.SLICE_CASES
    ohw = lambda c: c.out_hw[0] * c.out_hw[1]
    assert ohw(straddling) % straddling.route[1] and ohw(aligned) % aligned.route[1] == 0
    for case in G.SLICE_CASES:
        x, w, bias, xb, wb, ref, m, _ = _clean_case(case)
        y = G.restate32(case, x, w, bias, xb, wb)
        assert slice_ok(case, G.stored(case, y), ref, m)[0], case
        assert torch.equal(G.stored(case, y)[:, G.SLICE_BEFORE:G.SLICE_BEFORE + case.Cout], y)
        bad = slice_ok(case, G.stored(case, y, mut="image_stride_dense"), ref, m)[0]
        assert bad == (case is aligned), (case, bad)


# ---------------------------------------------------------------------------------------------------- 4. routes
@pytest.fixture(scope="module")
def tuning_lib():
    from disentangle_mlp_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load_tuning()
    yield lib
    lib.vg_debug_set_conv_general_tile(0, 0)


def _route(lib, case):
    out = (ctypes.c_int * 3)()
    assert lib.vg_debug_set_conv_general_tile(*(case.force or (0, 0))) == 0
    try:
        assert lib.vg_debug_conv_general_tile(case.Cout, case.npix, case.pad, out) == 0
    finally:
        lib.vg_debug_set_conv_general_tile(0, 0)
    return tuple(out)


_EVERY = tuple(c for cs in G.GROUPS.values() for c in cs)


def test_claimed_routes_are_the_librarys(tuning_lib):
    for case in _EVERY:
        assert _route(tuning_lib, case) == case.route, (case.id, _route(tuning_lib, case))
        assert case.force is None or case.route[:2] == case.force
        assert case.route[2] == case.pad


def test_both_sides_of_each_heuristic_switch(tuning_lib):
    routes = [c.route for c in G.HEURISTIC_CASES]
    assert all(c.force is None for c in G.HEURISTIC_CASES)
    assert routes == [(64, 64, 0), (64, 128, 0), (64, 64, 0), (128, 64, 0), (64, 64, 0), (128, 64, 0)]
    assert [c.npix for c in G.HEURISTIC_CASES[:2]] == [32640, 32768]
    assert [c.Cout for c in G.HEURISTIC_CASES[2:]] == [64, 65, 129, 193]
    out = (ctypes.c_int * 3)()
    for cout in (1, 8, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 2048):      # the restated cg_tile, around its switches
        tiles_m = -(-cout // G.tile_of(cout, 1)[0])
        edge = -(-256 // tiles_m) * 128                                    # the pixel count that fills the CUs with tn 128
        for npix in (1, 64, 65, edge - 128, edge - 127, edge, 1 << 20):
            if npix > 0:
                assert tuning_lib.vg_debug_conv_general_tile(cout, npix, 1, out) == 0
                assert tuple(out) == (*G.tile_of(cout, npix), 1), (cout, npix, tuple(out))


def test_tile_knob_takes_64_128_or_0_only(tuning_lib):
    lib, out = tuning_lib, (ctypes.c_int * 3)()
    assert lib.vg_debug_set_conv_general_tile(128, 64) == 0
    for bad in ((32, 0), (0, 256), (-1, 64), (64, 1)):
        assert lib.vg_debug_set_conv_general_tile(*bad) == -1
    assert lib.vg_debug_conv_general_tile(1, 1, 0, out) == 0 and tuple(out) == (128, 64, 0)      # a refused call changed nothing
    assert lib.vg_debug_set_conv_general_tile(0, 128) == 0                                     # one side forced
    assert lib.vg_debug_conv_general_tile(65, 81, 3, out) == 0 and tuple(out) == (128, 128, 1)
    assert lib.vg_debug_set_conv_general_tile(0, 0) == 0
    assert lib.vg_debug_conv_general_tile(65, 81, 0, out) == 0 and tuple(out) == (128, 64, 0)
    assert lib.vg_debug_conv_general_tile(65, 81, 0, None) == -1
    assert lib.vg_debug_conv_general_tile(0, 81, 0, out) == -1 and lib.vg_debug_conv_general_tile(65, 0, 0, out) == -1
    assert lib.vg_debug_conv_general_tile(65, 1 << 31, 0, out) == -1


def instantiations():
    """(tm, tn, pad) of every conv_general_kernel<...> the launch macro of conv_general.hip can reach, read from the
    source: a new instantiation shows up here and fails the coverage test until a case reaches it."""
    src = open(os.path.join(CSRC, "conv_general.hip")).read()
    pads = {p == "true" for p in re.findall(r"conv_general_kernel<TM_, TN_, (true|false)>", src)}
    tiles = {(int(a), int(b)) for a, b in re.findall(r"VG_CG_LAUNCH\((\d+), (\d+)\);", src)}
    assert pads == {True, False} and len(tiles) == 4, (pads, tiles)
    return {(tm, tn, int(p)) for (tm, tn) in tiles for p in pads}


def test_the_tables_reach_every_instantiation():
    assert instantiations() == {(tm, tn, p) for (tm, tn) in G.TILES for p in (0, 1)}
    assert {c.route for c in G.TILE_CASES} == instantiations()
    for route in instantiations():                         # each at every channel count and every pixel count of its tile
        mine = [c for c in G.TILE_CASES if c.route == route]
        assert {c.Cout for c in mine} == set(G.TILE_COUTS)
        assert {c.npix for c in mine} == {route[1] - 1, route[1], route[1] + 1, 105}
    assert {c.route for c in G.HEURISTIC_CASES} == {(64, 64, 0), (64, 128, 0), (128, 64, 0)}
    assert {c.K for c in G.K_CASES} == {1, 27, 32, 33, 64, 2048}
    assert {(c.KH, c.KW) for c in G.FILTER_CASES} == {(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1), (2, 4), (4, 2), (15, 15)}
    assert {(c.sh, c.sw) for c in G.FILTER_CASES} == {(1, 1), (2, 2), (1, 2), (2, 1)}
    assert {(c.ph, c.pw) for c in G.FILTER_CASES} == {(0, 0), (1, 1), (0, 3), (3, 0), (2, 2), (15, 15)}
    for k in {(c.KH, c.KW) for c in G.FILTER_CASES}:       # every filter with a stride above 1 and with a pad
        assert any((c.KH, c.KW) == k and (c.sh, c.sw) != (1, 1) for c in G.FILTER_CASES), k
        assert any((c.KH, c.KW) == k and c.pad for c in G.FILTER_CASES), k
    assert len(G.FILTER_CASES) <= 40
    assert [c.out_hw for c in G.ONE_PIXEL] == [(1, 1), (1, 1), (1, 7), (7, 1)] and [c.pad for c in G.ONE_PIXEL[:2]] == [1, 0]
    assert all(c.out_hw[0] * c.out_hw[1] == 42 and c.B == 3 for c in G.IMPULSE_CASES)
    assert [c.npix for c in G.NONFINITE_C] == [65, 65] and [c.pad for c in G.NONFINITE_C] == [1, 0]
