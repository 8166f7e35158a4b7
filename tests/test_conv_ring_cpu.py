"""CPU: the references of tests/_ring_refs.py for the fp16x3 5x5 convolution kernels (csrc/conv_ring.hip and, second table,
csrc/conv_bf16split.hip) -- no GPU, no kernel; the library is asked host-only questions (route, workspace, statistics).

1. emul64 stays within the documented split model of ref64 (tests/test_gemm_cpu.py has the derivation): per element
     |emul64 - ref64| <= C_REL 2^-24 mag + C_ABS 2^-40 (Px sum |w| + Pw sum |x|),
   Px / Pw the powers of two above the two bounds, the sums over the element's taps; at exact bounds and at bounds loose
   by 2^1 and 2^5, without and with an affine on load (the fp64-activated input of ref64 against the fp32 one of emul64:
   one more 2^-24 mag for the rounding of the activated input to fp32, 2 for the fma's product and sum).
2. K_ACC is measured from restate32 against emul64 over every case of the GPU file (R.ACC_WORST, R.K_ACC), and the
   unmutated restatement passes the GPU file's check with every element inside the bound.
3. Every mutation of R.MUTATIONS applied to the restatement is rejected by that check, on the smallest case that can
   show it.
4. The routes the case table claims are the library's (vg_debug_ring_route: the launch's own code), and agree with the
   public workspace and statistics queries -- for the table's cases and, test_one_plan_sizes_what_it_routes, over a sweep
   of shapes, planes and forced variants: the sizes are the formulas on the route's own tile and split.
"""
import ctypes
import math

import pytest
import torch

import _gemm_refs as G
import _ring_refs as R

C_REL = 12.0 * (1 + 2.0 ** -9)
C_ABS = 1 + 2.0 ** -9
PLANES = 2 | 0x100      # VG_PLANES_F16


def _bounds(x, w, affine=None, loose=0):
    return R.bound_of(R.activated(x, affine)) * 2.0 ** loose, R.bound_of(w) * 2.0 ** loose


# ---------------------------------------------------------------------------------------------------- 1. the split model
@pytest.mark.parametrize("act", [None, R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU])
@pytest.mark.parametrize("case", [R.RING_FWD[1], R.RING_TR[2], R.RING_TR_SPLIT[0], R.X_FWD[4], R.X_TR[2]], ids=lambda c: c.id)
def test_split_is_within_the_documented_model(case, act):
    x, w, bias = R.operands(case)
    tr, S = case.mode == R.TR, case.stride
    affine = None if act is None else R.affine_of(case, act)
    ref = R.ref64(x, w, bias, tr, affine, S)
    m = R.mag(x, w, bias, tr, affine, S)
    xa = R.activated(x, affine)
    sum_w = R._conv64(torch.ones_like(xa).double(), w.double().abs(), tr, S)
    sum_x = R._conv64(xa.double().abs(), torch.ones_like(w).double(), tr, S)
    extra = 0.0 if act is None else 3.0
    for loose in (0, 1, 5):
        xb, wb = _bounds(x, w, affine, loose)
        res = (R.emul64(x, w, bias, xb, wb, tr, affine, S) - ref).abs()
        model = (C_REL + extra) * R.U * m + C_ABS * 2.0 ** -40 * (G.pow2_bound(xb) * sum_w + G.pow2_bound(wb) * sum_x)
        over = float((res / model).max())
        print(f"{case.id} act {act} loose 2^{loose}: residual {float((res / (R.U * m)).max()):7.2f} x 2^-24 mag, {over:.3f} of the model")
        assert over <= 1.0, (case, act, loose, over)


# ---------------------------------------------------------------------------------------------------- 2. K_ACC
_clean = {}


def _clean_case(case, act=None):
    """(operands, bounds, emul64, mag) of a case, after the unmutated restatement passed the check on it."""
    key = (case, act)
    if key not in _clean:
        x, w, bias = R.operands(case)
        affine = None if act is None else R.affine_of(case, act)
        xb, wb = _bounds(x, w, affine)
        tr = case.mode == R.TR
        ref, m = R.emul64(x, w, bias, xb, wb, tr, affine, case.stride), R.mag(x, w, bias, tr, affine, case.stride)
        ok, worst = R.check(R.restate32(case, x, w, bias, xb, wb, affine), ref, m, R.k_of(case, affine is not None))
        assert ok, (case, act, worst)                  # the reference alone: every element inside the bound
        _clean[key] = (x, w, bias, affine, xb, wb, ref, m, worst)
    return _clean[key]


def test_k_acc_is_measured_from_the_restatement():
    """Worst |restate32 - emul64| / (2^-24 mag) per case, bias on, exact bounds (bounds loose by 2^1 and 2^5 at the fusion
    cases, where the GPU file hands them in)."""
    worst = 0.0
    for case in R.all_cases():
        w_ = _clean_case(case)[-1]
        print(f"{case.id:34s} splits {case.ksplit}: {w_:5.2f} x 2^-24   (cap 3K + splits >= {3 * R.reduction_length(case, 1, 1) + case.ksplit})")
        assert math.isfinite(w_)
        worst = max(worst, w_)
    for case in R.FUSION_CASES[:2]:
        x, w, bias = R.operands(case)
        tr = case.mode == R.TR
        for loose in (1, 5):
            xb, wb = _bounds(x, w, None, loose)
            w_ = R.ratio(R.restate32(case, x, w, bias, xb, wb), R.emul64(x, w, bias, xb, wb, tr), R.mag(x, w, bias, tr))
            print(f"{case.id:34s} loose 2^{loose}: {w_:5.2f} x 2^-24")
            worst = max(worst, w_)
    print(f"worst {worst:.3f}; ACC_WORST = {R.ACC_WORST}, K_ACC = ceil(4 x ACC_WORST) = {R.K_ACC}")
    assert 0.8 * R.ACC_WORST <= worst <= R.ACC_WORST
    assert R.K_ACC == math.ceil(4 * R.ACC_WORST)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU])
@pytest.mark.parametrize("case", R.FUSION_CASES[:2], ids=lambda c: c.id)
def test_restatement_passes_with_an_affine(case, act):
    print(f"{case.id} act {act}: {_clean_case(case, act)[-1]:.2f} x 2^-24")


# ---------------------------------------------------------------------------------------------------- 3. mutations
# (case, activation of the affine or None): the smallest cases that can show each
MUT_CASES = {
    "drop_lo_hi": [(R.RING_FWD[0], None), (R.RING_TR[0], None), (R.RING_FWD_SPLIT[0], None)],
    "drop_hi_lo": [(R.RING_FWD[0], None), (R.RING_TR[0], None), (R.RING_FWD_SPLIT[0], None)],
    "bias_every_split": [(R.RING_FWD_SPLIT[0], None), (R.RING_TR_SPLIT[0], None)],
    "bias_no_split": [(R.RING_FWD[0], None), (R.RING_FWD_SPLIT[0], None), (R.RING_TR_SPLIT[0], None)],
    "skip_last_chunk_of_last_split": [(R.RING_FWD_SPLIT[1], None), (R.RING_FWD_SPLIT[3], None), (R.RING_TR_SPLIT[0], None)],
    "chunk_buffer_parity": [(R.RING_TR[7], None)],
    "pad_before_act": [(R.RING_FWD[1], R.ACT_RELU), (R.RING_TR[2], R.ACT_LRELU), (R.RING_TR[2], R.ACT_NONE)],
    "tap_shift": [(R.RING_FWD[1], None), (R.RING_TR[1], None)],
    "class_swap": [(R.RING_TR[1], None)],
    "second_class_from_first_filter": [(R.RING_TR[1], None), (R.RING_PAIRED[0], None)],      # (the smallest paired case)
    "tile_remap": [(R.RING_FWD[1], None), (R.RING_TR[2], None), (R.RING_PAIRED[0], None)],
    "cout_row_off_by_one": [(R.RING_FWD[8 + 2], None), (R.RING_TR[1], None)],
    "image_pair_leak": [(R.RING_FWD_SPLIT[2], None), (R.RING_TR_SPLIT[2], None)],
}


def test_every_mutation_has_cases():
    assert set(MUT_CASES) == set(R.MUTATIONS)
    assert all(c in R.all_cases() for cs in MUT_CASES.values() for c, _ in cs)
    assert all(c.ksplit > 1 for m in ("bias_every_split", "skip_last_chunk_of_last_split", "image_pair_leak") for c, _ in MUT_CASES[m])
    assert all(c.B % 2 == 1 and c.route[2] == 2 for c, _ in MUT_CASES["image_pair_leak"])
    assert all(c.Cin == 48 and c.mode == R.TR for c, _ in MUT_CASES["chunk_buffer_parity"])


@pytest.mark.parametrize("mut", sorted(MUT_CASES))
def test_mutation_is_caught(mut):
    for case, act in MUT_CASES[mut]:
        x, w, bias, affine, xb, wb, ref, m, _ = _clean_case(case, act)
        ok, worst = R.check(R.restate32(case, x, w, bias, xb, wb, affine, mut=mut), ref, m, R.k_of(case, affine is not None))
        print(f"{mut} at {case.id} (splits {case.ksplit}): worst {worst:.3g} x 2^-24 against k <= {float(R.k_of(case).max()):.0f}")
        assert not ok, (mut, case, worst)


# ---------------------------------------------------------------------------------------------------- 4. routes
@pytest.fixture(scope="module")
def tuning_lib():
    from disentangle_mlp_amd import _lib
    lib = _lib.load_tuning()
    yield lib
    lib.vg_debug_set_conv_ring_tile(-1)
    lib.vg_debug_set_conv_bf16split_tile(-1)


def _queries(lib, case):
    name = "convT5x5" if case.mode == R.TR else "conv5x5"
    shape = (case.B, case.Cin, case.H, case.W, case.Cout, case.stride, PLANES)
    return (getattr(lib, f"vg_{name}_fwd_bf16split_workspace_bytes")(*shape),
            getattr(lib, f"vg_{name}_fwd_bf16split_stats_floats")(*shape))


@pytest.mark.parametrize("case", R.RING_CASES, ids=lambda c: c.id)
def test_claimed_ring_routes_are_the_librarys(tuning_lib, case):
    lib = tuning_lib
    assert lib.vg_conv5x5_bf16split_fusable(int(case.mode == R.TR), case.Cin, case.Cout, 2) == 1, "not a ring shape"
    lib.vg_debug_set_conv_ring_tile(-1 if case.force is None else case.force)
    try:
        out = (ctypes.c_int * 6)()
        assert lib.vg_debug_ring_route(case.mode, case.B, case.Cin, case.H, case.W, case.Cout, PLANES, out) == 0
        ws, st = _queries(lib, case)
    finally:
        lib.vg_debug_set_conv_ring_tile(-1)
    assert tuple(out) == case.route, (case.id, tuple(out))
    variant, ksplit, NB, TH, TW, paired = case.route
    OH, OW = case.out_hw
    ybytes = 4 * case.B * case.Cout * OH * OW
    assert ws == (ksplit * ybytes if ksplit > 1 else 0)                   # ksplit = bytes / output bytes
    th, tw = (case.H, case.W) if case.mode == R.TR else (OH, OW)          # the tile space
    tiles = -(-case.B // NB) * -(-th // TH) * -(-tw // TW)
    wp = 2 if variant in (0, 2) else 4                                    # wavefront rows of a tile: one slot each
    assert st == (0 if ksplit > 1 else tiles * wp * (4 if case.mode == R.TR else 1) * case.Cout * 2)
    assert not (paired and case.mode == R.FWD)


def test_one_plan_sizes_what_it_routes(tuning_lib):
    """The statistics and workspace sizes are those of the route's own tile and split (one host plan per launch), over 640
    ring shapes: every forced variant and the heuristic, both modes, fp16 and three bf16 planes, tile-ragged and whole
    images, one and 128 images.  Every expected value is the formula on the route's words."""
    lib, cdiv = tuning_lib, lambda a, b: -(-a // b)
    seen, out = set(), (ctypes.c_int * 6)()
    try:
        for force in (-1, 0, 1, 2, 3):
            lib.vg_debug_set_conv_ring_tile(force)
            for tr in (0, 1):
                name = "convT5x5" if tr else "conv5x5"
                for planes in (PLANES, 3):
                    for B in (3, 128):
                        for Cin in (32, 256):
                            for H, W in ((8, 8), (16, 16), (17, 9), (32, 64)):
                                for Cout in (65, 257):
                                    shape = (B, Cin, H, W, Cout)
                                    assert lib.vg_conv5x5_bf16split_fusable(tr, Cin, Cout, 2) == 1
                                    assert lib.vg_debug_ring_route(tr, *shape, planes, out) == 0, (force, tr, planes, shape)
                                    variant, ksplit, NB, TH, TW, paired = out
                                    ws = getattr(lib, f"vg_{name}_fwd_bf16split_workspace_bytes")(*shape, 2, planes)
                                    st = getattr(lib, f"vg_{name}_fwd_bf16split_stats_floats")(*shape, 2, planes)
                                    tsh, tsw = (H, W) if tr else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)      # the tile space
                                    YH, YW = (2 * H, 2 * W) if tr else (tsh, tsw)
                                    wp = 2 if variant in (0, 2) else 4
                                    slots = cdiv(B, NB) * cdiv(tsh, TH) * cdiv(tsw, TW) * wp * (4 if tr else 1)
                                    assert variant in (0, 1, 2, 3) and ksplit in (1, 2, 4, 8)
                                    assert st == (0 if ksplit > 1 else slots * Cout * 2), (force, tr, planes, shape, tuple(out), st)
                                    assert ws == (0 if ksplit == 1 else ksplit * B * Cout * YH * YW * 4), (force, tr, planes, shape, tuple(out), ws)
                                    assert not paired or (tr and planes == PLANES), (force, tr, planes, shape, tuple(out))
                                    seen.add((tr, planes, variant, ksplit > 1, paired))
    finally:
        lib.vg_debug_set_conv_ring_tile(-1)
    for tr in (0, 1):
        for planes in (PLANES, 3):
            got = {s[2] for s in seen if s[:2] == (tr, planes)}
            assert got == ({0, 1, 2} if (not tr and planes == 3) else {0, 1, 2, 3}), (tr, planes, got)      # (3: no forward tile with bf16 planes)
            assert any(s[3] for s in seen if s[:2] == (tr, planes)), "no K-split case"
    assert any(s[4] for s in seen), "no paired case"


def test_ring_route_refuses_what_the_kernel_does_not_take(tuning_lib):
    out = (ctypes.c_int * 6)()
    assert tuning_lib.vg_debug_ring_route(0, 2, 24, 8, 8, 8, PLANES, out) == -1          # Cin % 16
    assert tuning_lib.vg_debug_ring_route(2, 2, 16, 8, 8, 8, PLANES, out) == -1          # mode
    assert tuning_lib.vg_debug_ring_route(0, 2, 16, 8, 8, 8, PLANES, None) == -1


def test_the_table_reaches_what_it_is_for():
    """Every tile variant, geometry and split count of the ring, paired and not, is claimed by some case."""
    fwd = {c.route for c in R.RING_FWD + R.RING_FWD_SPLIT}
    tr = {c.route for c in R.RING_TR + R.RING_TR_SPLIT + R.RING_PAIRED}
    assert {r[0] for r in fwd} == {0, 1, 2, 3} == {r[0] for r in tr}
    assert {r[2:5] for r in fwd} == {(2, 8, 8), (1, 8, 16), (1, 16, 16)} == {r[2:5] for r in tr}
    assert {r[1] for r in fwd} == {1, 2, 4, 8} == {r[1] for r in tr}
    assert {(r[0], r[2:5]) for r in tr if r[5]} == {(2, (2, 8, 8)), (3, (1, 16, 16)), (2, (1, 8, 16)), (1, (1, 8, 16))}
    assert (0, 1, 2, 8, 8, 0) in tr                      # the 256-cout tile on 8-wide images
    parts = lambda c: [min(-(-c.Cin // 16 // c.ksplit), c.Cin // 16 - s * -(-c.Cin // 16 // c.ksplit)) for s in range(c.ksplit)]
    assert parts(R.RING_FWD_SPLIT[1]) == [3, 2] and parts(R.RING_FWD_SPLIT[3]) == [3, 3, 3, 2]


@pytest.mark.parametrize("case", R.X_FWD_SPLIT + R.X_FWD[:3] + R.X_TR[:3], ids=lambda c: c.id)
def test_claimed_split_counts_of_the_second_table(tuning_lib, case):
    tuning_lib.vg_debug_set_conv_bf16split_tile(-1)
    assert tuning_lib.vg_conv5x5_bf16split_fusable(int(case.mode == R.TR), case.Cin, case.Cout, case.stride) == 0, "a ring shape"
    ws, st = _queries(tuning_lib, case)
    OH, OW = case.out_hw
    assert st == 0 and ws == (case.ksplit * 4 * case.B * case.Cout * OH * OW if case.ksplit > 1 else 0), (case.id, ws)
