"""GPU: the three weight-gradient kernel families against the fp64 oracle, plan by plan.

  vg_conv5x5_wgrad                 exact fp32 (csrc/conv_wgrad.hip)
  vg_conv5x5_wgrad_bf16split       fp16x3 / bf16x6 / bf16x3 (csrc/wgrad_bf16split.hip), the default for Cin >= 32
  vg_conv5x5_thin_wgrad_bf16split  Cin <= 3 (csrc/conv_thin_wgrad.hip)

Every test runs through the tuning library and asks it (vg_debug_wgrad_*_plan: the launch's own planning code) which
instantiation, split and reducer the launch it is about to make uses; the coverage tests then compare what the case
tables reach with the instantiations written in the three dispatch switches of the sources.

References: oracle.ops.conv5x5_grads / convT5x5_grads in fp64 on the CPU.  Tolerances: CONV_TOL = 3e-6 relative L2 (and
50 x that of the largest reference magnitude per element) for fp32, fp16x3 and bf16x6; 2e-5 for bf16x3."""
import ctypes
import math
import os
import re

import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu

CONV_TOL = 3e-6
BF16X3_TOL = 2e-5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "disentangle_mlp_amd", "csrc")
KNOB_DEFAULTS = {"tm": -1, "target": -1, "ks": 2, "cit": 5, "vec4": 1, "th": 0}
KNOB_IDS = {"tm": 0, "target": 1, "ks": 2, "cit": 3, "vec4": 4, "th": 5}
RED_SUM4, RED_16, RED_4, RED_SUM1 = 0, 1, 2, 3          # vg_debug_wgrad_plan's reducer codes
PLANES = {"fp32": 0, "bf16x3": 2, "bf16x6": 3, "fp16x3": 2 | 0x100}
SPLIT_TOL = {"fp16x3": CONV_TOL, "bf16x6": CONV_TOL, "bf16x3": BF16X3_TOL}


# ------------------------------------------------------------------------------------------------ fixtures, helpers
@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


def set_knobs(lib, **kw):
    for name, default in KNOB_DEFAULTS.items():
        assert lib.vg_debug_set_wgrad(KNOB_IDS[name], kw.get(name, default)) == 0


@pytest.fixture
def tuning(H):
    """The ops through libvaegan_hip_tuning.so for one test; all six weight-gradient knobs and the arithmetic are back
    on their defaults afterwards."""
    from disentangle_mlp_amd import _lib
    prev = H.CONV_ARITH
    with _lib.use_tuning() as lib:
        try:
            set_knobs(lib)
            yield lib
        finally:
            set_knobs(lib)
            H.CONV_ARITH = prev


def rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).norm() / max(ref.norm(), 1e-30))


def assert_close(a, ref, tol, what=""):
    assert tuple(a.shape) == tuple(ref.shape), (what, a.shape, ref.shape)
    e = rel_l2(a, ref)
    assert math.isfinite(e) and e <= tol, f"{what}: rel L2 {e:.3e} > {tol:.1e}"
    m = float((a.detach().cpu().double() - ref.double()).abs().max())
    assert m <= 50 * tol * float(ref.abs().max()) + 1e-30, f"{what}: max abs err {m:.3e}"
    return e


def out_hw(Hs, Ws, S):
    return (Hs - 1) // S + 1, (Ws - 1) // S + 1


def operands(shape, seed, x_mag=1.0, gy_mag=1.0):
    B, Cin, Cout, Hs, Ws, S = shape
    g = torch.Generator().manual_seed(seed)
    OH, OW = out_hw(Hs, Ws, S)
    return torch.randn(B, Cin, Hs, Ws, generator=g) * x_mag, torch.randn(B, Cout, OH, OW, generator=g) * gy_mag


def activate(v, scale, shift, act):
    """fp64 act(v * scale[c] + shift[c]); act 0 none, 1 ReLU, 2 LeakyReLU(0.2)."""
    v = v.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return v if act == 0 else (v.clamp(min=0) if act == 1 else torch.where(v > 0, v, 0.2 * v))


def oracle_gw(x, gy, S):
    return O.conv5x5_grads(x, torch.zeros(gy.shape[1], x.shape[1], 5, 5), gy, S)[1]


def _ints(n):
    return (ctypes.c_int * n)()


def ws_ptr(H, nbytes):
    """Address of the scratch the next launch on this stream gets for ``nbytes``."""
    return H.workspace(max(int(nbytes), 1), torch.device("cuda", torch.cuda.current_device())).data_ptr()


def plan_fp32(lib, shape, gy=0, dw=0, ws=0):
    B, Cin, Cout, Hs, Ws, S = shape
    o = _ints(9)
    assert lib.vg_debug_wgrad_plan(B, Cin, Hs, Ws, Cout, S, gy, dw, ws, o) == 0
    return dict(zip(("tw", "tm", "cit", "ks", "splits", "vec4", "reducer", "chunks", "cps"), o))


def plan_split(lib, shape, arith):
    B, Cin, Cout, Hs, Ws, S = shape
    o = _ints(9)
    assert lib.vg_debug_wgrad_split_plan(B, Cin, Hs, Ws, Cout, S, PLANES[arith], o) == 0, (shape, "not taken")
    return dict(zip(("th", "wco", "mtiles", "ntiles", "units", "upw", "wgs", "pieces", "chunks"), o))


def plan_thin(lib, shape, planes, dw=0, ws=0):
    B, Cin, Cout, Hs, Ws, S = shape
    o = _ints(6)
    assert lib.vg_debug_wgrad_thin_plan(B, Cin, Hs, Ws, Cout, S, planes, dw, ws, o) == 0, (shape, "not taken")
    return dict(zip(("mt", "rb", "bands", "upw", "wgs", "reducer"), o))


def pieces_per_tile(p):
    """Partial slabs of every output tile of a split-kernel plan (wx_reduce_kernel's first / last)."""
    return [((t + 1) * p["chunks"] - 1) // p["upw"] - (t * p["chunks"]) // p["upw"] + 1
            for t in range(p["mtiles"] * p["ntiles"])]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# --------------------------------------------------------------------------- 1. every plan of the exact-fp32 kernel
def fp32_instantiations():
    """(S, TW, TM, KS, CIT) of every conv5x5_wgrad_kernel<WCfg<...>> the dispatch switch of conv_wgrad.hip can launch,
    read from the switch itself: a new instantiation shows up here and fails the coverage test until a shape reaches it."""
    src = _source("conv_wgrad.hip")
    forms = set()
    for args in re.findall(r"launch_w<WCfg<S, TW, ([0-9, ]+)>>", src):
        a = [int(v) for v in args.split(",")]
        forms.add((a[0], a[1] if len(a) > 1 else 1, a[2] if len(a) > 2 else 5))
    tws = {int(v) for v in re.findall(r"dispatch_tm<S, (\d+)>", src)}
    strides = {int(v) for v in re.findall(r"dispatch_tw<(\d)>\(A", src)}
    assert len(forms) >= 5 and len(tws) >= 4 and strides == {1, 2}, (forms, tws, strides)
    return {(s, tw, tm, ks, cit) for s in strides for tw in tws for (tm, ks, cit) in forms}


# (B, Cin, Cout, H, W, stride).  The first eight: one per (stride, pixel-tile width), Cout = 130 / Cin = 21 so that every
# row-tile form is reachable (130 is off the 32-, 64- and 128-row tiles, 21 off the 5- and the 10-channel column tile),
# output width a multiple of 4 (both gy load paths).  Then the scalar-only and single-image edges.
FP32_SHAPES = [
    (5, 21, 130, 11, 8, 1),      # TW 8:  OH 11 off the 8-row chunk
    (7, 21, 130, 13, 15, 2),     # TW 8, stride 2: OW 8, OH 7
    (5, 21, 130, 6, 16, 1),      # TW 16: OH 6 off the 4-row chunk
    (5, 21, 130, 10, 24, 2),     # TW 16, stride 2: OW 12 off the tile, OH 5
    (3, 21, 130, 5, 32, 1),      # TW 32: OH 5 off the 2-row chunk
    (5, 21, 130, 6, 56, 2),      # TW 32, stride 2: OW 28 off the tile, OH 3
    (3, 21, 130, 3, 72, 1),      # TW 64: OW 72, two tiles across, the second partial
    (3, 21, 130, 5, 136, 2),     # TW 64, stride 2: OW 68
    (1, 3, 33, 9, 7, 1),         # B = 1, Cin < 5, Cout 33, OW 7: scalar gy loads, off the tile
    (5, 7, 65, 7, 13, 1),        # Cout 65, Cin 7, OW 13
    (3, 12, 65, 9, 21, 2),       # stride 2, OW 11, OH 5, Cin 12
    (2, 9, 33, 5, 54, 2),        # OW 27 in the 32-pixel tile
    (1, 5, 33, 2, 256, 1),       # 256 pixels across: four tiles
    (1, 6, 40, 3, 256, 2),       # 128 pixels across at stride 2: two tiles
    (2, 4, 70, 3, 130, 1),       # OW 130: three tiles, the last two pixels wide, scalar loads
]


def fp32_runs(lib, shape):
    """The knob settings a shape is run with, each with the plan the dispatcher reports for it: every reachable
    row-tile form x both gy load paths at a split whose last slab is short (where the chunk count allows one), and the
    heuristic form at the one-slab, one-chunk-per-slab and heuristic splits."""
    runs, seen = [], set()

    def add(**kn):
        set_knobs(lib, **kn)
        p = plan_fp32(lib, shape)
        key = tuple(sorted(p.items()))
        if key not in seen:
            seen.add(key)
            runs.append((kn, p))

    OW = out_hw(shape[3], shape[4], shape[5])[1]
    for tm, ks, cit in sorted({f[2:] for f in fp32_instantiations()}):
        form = dict(tm=tm, ks=ks, cit=cit)
        set_knobs(lib, **form)
        p = plan_fp32(lib, shape)
        if (p["tm"], p["ks"], p["cit"]) != (tm, ks, cit):
            continue                       # the knob is ignored for this shape (tm above the plan's, cit 10 needs Cin >= 20)
        target = None
        for t in range(2, 2048):
            lib.vg_debug_set_wgrad(KNOB_IDS["target"], t)
            q = plan_fp32(lib, shape)
            if q["splits"] > 1 and q["chunks"] % q["cps"]:
                target = t
                break
        for vec4 in ((1, 0) if OW % 4 == 0 else (1,)):
            add(vec4=vec4, **({"target": target} if target else {}), **form)
    add(target=1)
    add(target=1 << 20)
    add()
    set_knobs(lib)
    return runs


def split_kind(p):
    return "one" if p["splits"] == 1 else ("ragged" if p["chunks"] % p["cps"] else
                                           ("chunks" if p["splits"] == p["chunks"] else "even"))


@pytest.mark.parametrize("shape", FP32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_every_plan(H, tuning, shape):
    """vg_conv5x5_wgrad under every plan a shape can be given, each against the fp64 oracle at CONV_TOL; the plan asked
    for is the plan reported for the very pointers of the launch."""
    lib = tuning
    H.CONV_ARITH = "fp32"
    B, Cin, Cout, Hs, Ws, S = shape
    x, gy = operands(shape, 100)
    ref = oracle_gw(x, gy, S)
    xd, gd = x.cuda(), gy.cuda()
    runs = fp32_runs(lib, shape)
    assert runs
    for kn, p in runs:
        set_knobs(lib, **kn)
        dw = torch.full((Cout, Cin, 5, 5), float("nan"), device="cuda")
        ws = ws_ptr(H, lib.vg_conv5x5_wgrad_workspace_bytes(B, Cin, Hs, Ws, Cout, S))
        assert plan_fp32(lib, shape, gd.data_ptr(), dw.data_ptr(), ws) == p, (kn, p)
        got = H.conv5x5_wgrad(xd, gd, S, out=dw)
        e = assert_close(got, ref, CONV_TOL, f"fp32 wgrad {shape} {p}")
        print(f"fp32 {shape} {p}: {e:.2e}")


def test_fp32_plans_cover_the_dispatch_switch(tuning):
    """What FP32_SHAPES reach (the same enumeration the test above runs) is every instantiation of the switch, with
    both gy load paths, and every (stride, TW) sees a one-slab, a slab-per-chunk and a short-last-slab split."""
    lib = tuning
    covered, kinds = set(), {}
    for shape in FP32_SHAPES:
        for _, p in fp32_runs(lib, shape):
            covered.add((shape[5], p["tw"], p["tm"], p["ks"], p["cit"], p["vec4"]))
            kinds.setdefault((shape[5], p["tw"]), set()).add(split_kind(p))
    full = {inst + (v,) for inst in fp32_instantiations() for v in (0, 1)}
    assert covered == full, (sorted(full - covered), sorted(covered - full))
    for key in {(i[0], i[1]) for i in fp32_instantiations()}:
        assert {"one", "chunks", "ragged"} <= kinds.get(key, set()), (key, kinds.get(key))


# ---------------------------------------------------------------- 2. the split kernel, three arithmetics, th 1 and 2
def split_instantiations():
    """(S, planes, fp16, WCO, TH) of every conv5x5_wgrad_split8_kernel<W8<...>> of wgrad_bf16split.hip's switches."""
    src = _source("wgrad_bf16split.hip")
    tiles = {(int(a), int(b)) for a, b in re.findall(r"launch_wx<W8<S, NP, (\d), (\d), F16>>", src)}
    outer = {(int(s), int(n), bool(f)) for s, n, f in re.findall(r"launch_wx_by_cout<(\d), (\d)(, true)?>\(A", src)}
    assert len(tiles) >= 4 and len(outer) >= 6, (tiles, outer)
    return {(s, n, f, wco, th) for (s, n, f) in outer for (wco, th) in tiles}


SPLIT_KEY = {"fp16x3": (2, True), "bf16x6": (3, False), "bf16x3": (2, False)}

# (B, Cin, Cout, H, W, stride), the th values forced.  Output widths are multiples of 8 (the kernel's condition).
SPLIT_SHAPES = [
    ((1, 32, 40, 7, 8, 1), (1,)),           # B = 1, Cout off 32, odd OH; units < 256
    ((15, 33, 130, 8, 16, 2), (1, 2)),      # B = 15, Cout 130: 256-row tile (wco 8), Cin off the 5-channel column tile
    ((17, 37, 128, 6, 16, 1), (1, 2)),      # B = 17: two image groups, the second one image wide; wco 4
    ((16, 32, 33, 4, 16, 2), (1, 2)),       # B = 16 exactly; stride 2 with wco 4
    ((33, 65, 260, 13, 8, 1), (1,)),        # B = 33, Cout 260 (two 256-row tiles), odd OH; upw 4, shares straddle tiles
    ((33, 48, 130, 12, 16, 1), (1, 2)),     # stride 1 with wco 8, even OH, upw > 1 for th 1
    ((17, 64, 200, 20, 16, 2), (1, 2)),     # stride 2 with wco 8 and upw > 1
]


def split_runs(lib, arith):
    out = []
    for shape, ths in SPLIT_SHAPES:
        for th in ths:
            set_knobs(lib, th=th)
            out.append((shape, th, plan_split(lib, shape, arith)))
    set_knobs(lib)
    return out


def _mags(arith):
    """fp16x3: operands far from 1 (x ~ 3e3, gy ~ 1e-5) so that the power-of-two scales do real work."""
    return (3e3, 1e-5) if arith == "fp16x3" else (1.0, 1.0)


@pytest.mark.parametrize("arith", ["fp16x3", "bf16x6", "bf16x3"])
def test_split_every_plan(H, tuning, arith):
    lib = tuning
    H.CONV_ARITH = arith
    refs = {}
    for shape, th, p in split_runs(lib, arith):
        B, Cin, Cout, Hs, Ws, S = shape
        assert p["th"] == th and p["wco"] == (8 if Cout > 128 else 4), (shape, th, p)
        x, gy = operands(shape, 200, *_mags(arith))
        if shape not in refs:
            refs[shape] = oracle_gw(x, gy, S)
        ref = refs[shape]
        set_knobs(lib, th=th)
        got = H.conv5x5_wgrad(x.cuda(), gy.cuda(), S)
        e = assert_close(got, ref, SPLIT_TOL[arith], f"{arith} wgrad {shape} th {th} {p}")
        print(f"{arith} {shape} {p}: {e:.2e}")


@pytest.mark.parametrize("arith", ["fp16x3", "bf16x6", "bf16x3"])
def test_split_plans_cover_the_dispatch_switch(tuning, arith):
    """Every (stride, wco, th) of the arithmetic's instantiations is reached, and the work split is seen in each of its
    regimes: fewer units than workgroup slots, several units per workgroup, a last share that is short, shares that
    straddle two tiles so that the tiles of one launch have different numbers of partial slabs."""
    lib = tuning
    runs = split_runs(lib, arith)
    np_, f16 = SPLIT_KEY[arith]
    covered = {(s[5], np_, f16, p["wco"], p["th"]) for s, _, p in runs}
    full = {i for i in split_instantiations() if i[1] == np_ and i[2] == f16}
    assert len(full) == 8 and covered == full, (sorted(full - covered), sorted(covered - full))
    plans = [p for _, _, p in runs]
    assert any(p["units"] < 256 and p["upw"] == 1 for p in plans)
    assert any(p["upw"] > 1 for p in plans)
    assert any(p["upw"] > 1 and p["units"] % p["upw"] for p in plans)
    assert any(p["chunks"] % p["upw"] and len(set(pieces_per_tile(p))) > 1 for p in plans)
    assert all(max(pieces_per_tile(p)) == p["pieces"] for p in plans)
    assert {s[0] for s, _, _ in runs} >= {1, 15, 16, 17, 33}
    assert len({tuple(sorted(kv.items())) for kv in plans}) == len(plans)            # every forced th gave another plan


@pytest.mark.parametrize("arith", ["fp16x3", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("th", [1, 2])
def test_split_operand_affine(H, tuning, arith, th):
    """in_affine on x, and on gy (the transposed layers' weight gradient), with act none / ReLU / LeakyReLU, applied on
    load by both chunk heights: against the oracle of the materialised operand (zero padding pads the ACTIVATED x)."""
    lib = tuning
    H.CONV_ARITH = arith
    shape = (17, 35, 70, 8, 16, 2)
    B, Cin, Cout, Hs, Ws, S = shape
    set_knobs(lib, th=th)
    assert plan_split(lib, shape, arith)["th"] == th
    xm, gm = _mags(arith)
    x, gy = operands(shape, 210, xm, gm)
    g = torch.Generator().manual_seed(211)
    for on_gy in (False, True):
        C = Cout if on_gy else Cin
        scale, shift = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g) * (gm if on_gy else xm)
        for act in (0, 1, 2):
            xa = x.double() if on_gy else activate(x, scale, shift, act)
            ga = activate(gy, scale, shift, act) if on_gy else gy.double()
            ref = oracle_gw(xa, ga, S)
            got = H.conv5x5_wgrad(x.cuda(), gy.cuda(), S, in_affine=(scale.cuda(), shift.cuda(), act), affine_on_gy=on_gy)
            e = assert_close(got, ref, SPLIT_TOL[arith], f"{arith} th {th} affine on {'gy' if on_gy else 'x'} act {act}")
            print(f"{arith} th {th} affine on {'gy' if on_gy else 'x'} act {act}: {e:.2e}")


# -------------------------------------------------------------------------------------------- 3. the thin kernel
def thin_instantiations():
    src = _source("conv_thin_wgrad.hip")
    sm = {(int(s), int(m)) for s, m in re.findall(r"launch_tw<(\d), (\d)>\(A", src)}
    nps = {int(n) for n in re.findall(r"conv_thin_wgrad_kernel<S, MT, (\d)>", src)}
    assert len(sm) >= 4 and nps >= {2, 3}, (sm, nps)
    return {(s, m, n) for (s, m) in sm for n in nps}


THIN_SHAPES = [
    (130, 1, 33, 40, 16, 1),     # MT 2 (Cout 33), two bands (32 + 8 rows), B * bands = 260 > 256: two units per workgroup
    (3, 2, 50, 80, 32, 2),       # stride 2, MT 2 (Cout 50), bands 32 + 8
    (5, 3, 20, 37, 32, 1),       # MT 1, Cout off 32, bands 32 + 5
    (2, 3, 32, 70, 64, 2),       # stride 2, MT 1, three bands (16 + 16 + 3)
    (2, 3, 63, 20, 16, 1),       # Cout 63, one band
]


@pytest.mark.parametrize("arith", ["fp16x3", "bf16x3"])
@pytest.mark.parametrize("shape", THIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_thin_every_plan(H, tuning, arith, shape):
    """vg_conv5x5_thin_wgrad_bf16split, three planes (the default arithmetic) and two (bf16x3): plain, and with the
    BatchNorm + activation of the wide operand applied on load."""
    lib = tuning
    H.CONV_ARITH = arith
    B, Cin, Cout, Hs, Ws, S = shape
    tol = SPLIT_TOL[arith]
    p = plan_thin(lib, shape, H._thin_planes())
    x, gy = operands(shape, 300)
    got = H.conv5x5_wgrad(x.cuda(), gy.cuda(), S)
    e = assert_close(got, oracle_gw(x, gy, S), tol, f"thin wgrad {shape} {p}")
    print(f"thin {arith} {shape} {p}: {e:.2e}")
    g = torch.Generator().manual_seed(301)
    scale, shift = 0.5 + torch.rand(Cout, generator=g), torch.randn(Cout, generator=g)
    for act in (1, 2):
        ref = oracle_gw(x, activate(gy, scale, shift, act), S)
        got = H.conv5x5_wgrad(x.cuda(), gy.cuda(), S, in_affine=(scale.cuda(), shift.cuda(), act), affine_on_gy=True)
        e = assert_close(got, ref, tol, f"thin wgrad {shape}, affine on gy, act {act}")
        print(f"thin {arith} {shape} affine act {act}: {e:.2e}")


def test_thin_plans_cover_the_dispatch_switch(H, tuning):
    lib = tuning
    covered, plans = set(), []
    for planes in (3, 2):
        for shape in THIN_SHAPES:
            p = plan_thin(lib, shape, planes)
            covered.add((shape[5], p["mt"], planes))
            plans.append((shape, p))
    assert covered == thin_instantiations(), sorted(thin_instantiations() ^ covered)
    assert {s[1] for s, _ in plans} == {1, 2, 3}
    assert any(p["bands"] > 1 and out_hw(s[3], s[4], s[5])[0] % p["rb"] for s, p in plans)       # ragged last band
    assert any(s[0] * p["bands"] > 256 and p["upw"] > 1 for s, p in plans)
    assert any(32 < s[2] < 64 for s, _ in plans)


# --------------------------------------------------------------------- 4. accumulate and out=, every reducer
# (family / arithmetic, shape, out misaligned to 4 (mod 16) bytes, the reducer the plan must report or None)
ACC_CASES = [
    ("fp32", (2, 8, 16, 8, 8, 1), False, RED_SUM4),
    ("fp32", (70, 4, 8, 8, 8, 1), False, RED_16),            # 70 slabs of 800 floats
    ("fp32", (70, 4, 8, 8, 8, 1), True, RED_16),
    ("fp32", (3, 3, 3, 8, 8, 2), False, RED_4),              # 225 floats: not a multiple of 4
    ("fp32", (66, 41, 64, 8, 8, 1), False, RED_4),           # 66 slabs of 65600 floats: too many workgroups for <16>
    ("fp32", (17, 8, 16, 8, 8, 1), False, RED_SUM4),         # 17 slabs: groups of 8, 8 and 1
    ("fp32", (2, 8, 16, 8, 8, 1), True, RED_SUM1),           # out 4 bytes into a 16-byte line: slab_sum4's order, scalar
    ("fp32", (17, 8, 16, 8, 8, 1), True, RED_SUM1),
    ("fp32", (5, 21, 130, 13, 15, 2), True, RED_4),
    ("fp16x3", (17, 37, 128, 6, 16, 1), False, None),        # wx_reduce_kernel
    ("fp16x3", (17, 37, 128, 6, 16, 1), True, None),
    ("fp16x3", (33, 65, 260, 13, 8, 1), True, None),        # tiles with 10 and with 11 partial slabs
    ("bf16x6", (17, 37, 128, 6, 16, 1), True, None),
    ("bf16x6", (15, 33, 130, 8, 16, 2), False, None),
    ("bf16x3", (15, 33, 130, 8, 16, 2), True, None),
    ("thin", (5, 3, 20, 37, 32, 1), False, RED_SUM4),
    ("thin", (130, 1, 33, 40, 16, 1), False, RED_16),        # 130 slabs
    ("thin", (3, 1, 33, 40, 16, 1), False, RED_4),           # 825 floats
    ("thin", (5, 3, 20, 37, 32, 1), True, RED_SUM1),
    ("thin", (3, 1, 33, 40, 16, 1), True, RED_4),
    ("thin", (130, 1, 33, 40, 16, 1), True, RED_16),
]


@pytest.mark.parametrize("family,shape,misaligned,reducer", ACC_CASES,
                         ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-{'off4' if c[2] else 'aligned'}" for c in ACC_CASES])
def test_accumulate_and_out(H, tuning, family, shape, misaligned, reducer):
    """accumulate=True into ``out`` gives the bits of ``prev + wgrad`` (include/vaegan_hip.h: "same bits"); without it
    an ``out`` full of NaN comes back finite and with the bits of the plain call; with ``out`` a view one float into a
    flat buffer -- how a trainer's flat gradient buffer hands it out: 4-byte aligned, not 16 -- its neighbours stay, and
    the bits are those of the aligned call (the order of the slab sum depends on the shape alone: slab_sum1_kernel adds
    in slab_sum4_kernel's order; before it existed a misaligned ``out`` went to wgrad_reduce_kernel<4>, whose order is
    another one, and this test failed for the thin kernel's ten slabs)."""
    lib = tuning
    H.CONV_ARITH = "fp16x3" if family == "thin" else family
    B, Cin, Cout, Hs, Ws, S = shape
    n = Cout * Cin * 25
    x, gy = operands(shape, 400)
    xd, gd = x.cuda(), gy.cuda()
    g = torch.Generator().manual_seed(401)
    flat_init = torch.randn(n + 8, generator=g).cuda()
    off = 1 if misaligned else 4

    def view(flat):
        v = flat[off:off + n].view(Cout, Cin, 5, 5)
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 if misaligned else 0) and v.data_ptr() % 4 == 0
        return v

    if family == "fp32":
        ws = ws_ptr(H, lib.vg_conv5x5_wgrad_workspace_bytes(B, Cin, Hs, Ws, Cout, S))
        p = plan_fp32(lib, shape, gd.data_ptr(), view(flat_init).data_ptr(), ws)
        assert p["reducer"] == reducer, p
    elif family == "thin":
        assert Cin <= 3
        ws = ws_ptr(H, lib.vg_conv5x5_thin_wgrad_bf16split_workspace_bytes(B, Cin, Hs, Ws, Cout, S, H._thin_planes()))
        p = plan_thin(lib, shape, H._thin_planes(), view(flat_init).data_ptr(), ws)
        assert p["reducer"] == reducer, p
    else:
        assert plan_split(lib, shape, family)["pieces"] >= 1 and Cin >= 32

    plain = H.conv5x5_wgrad(xd, gd, S)
    assert_close(plain, oracle_gw(x, gy, S), BF16X3_TOL if family == "bf16x3" else CONV_TOL, "plain")
    assert bool(torch.isfinite(plain).all())
    # out= without accumulate: whatever out held is overwritten
    flat = flat_init.clone()
    view(flat).fill_(float("nan"))
    got = H.conv5x5_wgrad(xd, gd, S, out=view(flat))
    assert got.data_ptr() == view(flat).data_ptr()
    assert torch.equal(got, plain), "out= prefilled with NaN"
    assert torch.equal(flat[:off], flat_init[:off]) and torch.equal(flat[off + n:], flat_init[off + n:])
    # accumulate: the second use of a filter before one backward
    flat = flat_init.clone()
    prev = view(flat).clone()
    got = H.conv5x5_wgrad(xd, gd, S, out=view(flat), accumulate=True)
    assert torch.equal(got, prev + plain), f"accumulate: max diff {float((got - (prev + plain)).abs().max()):.3e}"
    assert torch.equal(flat[:off], flat_init[:off]) and torch.equal(flat[off + n:], flat_init[off + n:])


def test_accumulate_cases_reach_every_reducer():
    fam = {(c[0] if c[0] in ("fp32", "thin") else "split", c[3]) for c in ACC_CASES}
    assert fam >= {("fp32", RED_SUM4), ("fp32", RED_SUM1), ("fp32", RED_16), ("fp32", RED_4), ("split", None),
                   ("thin", RED_SUM4), ("thin", RED_SUM1), ("thin", RED_16), ("thin", RED_4)}
    assert {c[0] for c in ACC_CASES} >= {"fp32", "fp16x3", "bf16x6", "bf16x3", "thin"}
    assert all(any(c[0] == f and c[2] for c in ACC_CASES) for f in ("fp32", "fp16x3", "bf16x6", "bf16x3", "thin"))


# ------------------------------------------------------------------------ 5. stale scratch, run-to-run bits
# (family / arithmetic, the ragged shape, a larger launch of the same family)
STALE_CASES = [
    ("fp32", (17, 7, 33, 7, 13, 1), (20, 12, 70, 9, 16, 1)),
    ("fp32", (17, 21, 130, 13, 15, 2), (20, 24, 140, 14, 16, 2)),
    ("fp16x3", (17, 33, 130, 7, 16, 1), (33, 40, 140, 9, 16, 1)),
    ("bf16x6", (17, 33, 130, 14, 16, 2), (33, 40, 140, 18, 16, 2)),
    ("bf16x3", (17, 35, 40, 5, 8, 1), (33, 40, 140, 9, 16, 1)),
    ("thin", (17, 3, 33, 37, 16, 1), (40, 3, 64, 41, 32, 1)),
    ("thin", (17, 2, 50, 70, 32, 2), (40, 3, 64, 82, 64, 2)),
]


@pytest.mark.parametrize("family,shape,larger", STALE_CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in STALE_CASES])
def test_scratch_is_fully_written_before_it_is_read(H, tuning, family, shape, larger):
    """The slabs and the re-laid-out gy (zero-padded to 16 images, 128 channels) live in the per-stream scratch, which
    holds whatever an earlier launch left.  With every byte of it 0xFF (each float a NaN), and again after a larger
    launch of the same family, the result is finite and keeps its bits: nothing is summed that was not written."""
    H.CONV_ARITH = "fp16x3" if family == "thin" else family
    S = shape[5]
    x, gy = operands(shape, 500)
    xd, gd = x.cuda(), gy.cuda()
    first = H.conv5x5_wgrad(xd, gd, S).clone()
    assert_close(first, oracle_gw(x, gy, S), BF16X3_TOL if family == "bf16x3" else CONV_TOL, "first run")
    scratch = H.workspace(1, xd.device)
    assert scratch.numel() >= 1 << 20
    scratch.fill_(0xFF)
    assert bool(torch.isnan(scratch[:4096].view(torch.float32)).all())
    again = H.conv5x5_wgrad(xd, gd, S)
    assert bool(torch.isfinite(again).all()), "reads scratch it did not write"
    assert torch.equal(again, first)
    xl, gl = operands(larger, 501)
    big = H.conv5x5_wgrad(xl.cuda() * 1e3, gl.cuda() * 1e3, larger[5])
    assert bool(torch.isfinite(big).all())
    assert H.workspace(1, xd.device).numel() >= 1
    third = H.conv5x5_wgrad(xd, gd, S)
    assert torch.equal(third, first), "result depends on what the scratch held"


# --------------------------------------------------------- 6. the benchmarked launches (B = 128), element by element
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
# (transposed, Cin, Cout, H, stride, the activation of the producer's BatchNorm applied on load or None): the trainer's
# chains -- encoder Conv-BN-ReLU, discriminator Conv-BN-LeakyReLU, decoder ConvT-BN-ReLU; a chain's first layer reads
# its input as it is.  model.py:450-456, 389-398, 495-507 of the reference.
BENCH_LAYERS = [
    (False, 3, 64, 64, 2, None), (False, 64, 128, 32, 2, ACT_RELU), (False, 128, 256, 16, 2, ACT_RELU),
    (False, 3, 32, 64, 1, None), (False, 32, 128, 64, 2, ACT_LRELU), (False, 128, 256, 32, 2, ACT_LRELU),
    (False, 256, 256, 16, 2, ACT_LRELU),
    (True, 256, 256, 8, 2, None), (True, 256, 128, 16, 2, ACT_RELU), (True, 128, 32, 32, 2, ACT_RELU),
    (True, 32, 3, 64, 1, ACT_RELU),
]
CO_EDGES = (0, 1, 31, 32, 63, 64, 127, 128, -2, -1)
CI_EDGES = (0, 4, 5, 9, 10, 31, 32, -1)


def _clip(edges, n):
    return sorted({(e + n) if e < 0 else e for e in edges if -n <= e < n})


@pytest.mark.parametrize("transposed,Cin,Cout,Hs,stride,act", BENCH_LAYERS,
                         ids=[f"{'convT' if c[0] else 'conv'}{c[1]}-{c[2]}at{c[3]}s{c[4]}" for c in BENCH_LAYERS])
def test_benchmarked_launch_channel_crops(H, transposed, Cin, Cout, Hs, stride, act):
    """The eleven weight gradients of a training iteration at the benchmarked batch, default arithmetic, heuristic plan,
    with the operand transform the trainer applies; once plain, once as the second, accumulating use.  gw[co, ci]
    depends on x[:, ci] and gy[:, co] alone, so the fp64 oracle on channel crops is the exact reference of
    gw[co_idx][:, ci_idx]; the index sets straddle every tile edge (32 / 64 / 128 rows, 5 / 10 channel column tiles).
    Bound: max(CONV_TOL, e32), e32 = the error of the oracle's own plain fp32 evaluation of the same crop against fp64
    (the reductions have up to 524288 terms: "fp32-equivalent" = no worse than fp32 itself).

    Measured on an MI355X (relative L2 of the crop; plain and accumulating run agree to the digits shown):

      layer                          kernel     e32        bound
      conv  3->64   @64 s2            3.6e-07    1.5e-06    3.0e-06
      conv  64->128 @32 s2            5.5e-07    9.3e-07    3.0e-06
      conv  128->256 @16 s2           3.5e-07    4.8e-07    3.0e-06
      conv  3->32   @64 s1            7.5e-07    3.3e-06    3.3e-06
      conv  32->128 @64 s2            1.1e-06    2.1e-06    3.0e-06
      conv  128->256 @32 s2           8.2e-07    1.4e-06    3.0e-06
      conv  256->256 @16 s2           4.5e-07    5.4e-07    3.0e-06
      convT 256->256 @8 s2            4.1e-07    5.3e-07    3.0e-06
      convT 256->128 @16 s2           6.7e-07    9.7e-07    3.0e-06
      convT 128->32 @32 s2            8.8e-07    1.5e-06    3.0e-06
      convT 32->3   @64 s1            8.5e-07    3.7e-06    3.7e-06
    """
    B = 128
    gen = torch.Generator(device="cuda").manual_seed(600)
    s = stride
    if transposed:
        # layer input (B, Cin, H, W) is the wide "gy" operand; the gradient of its output plays x
        a = torch.randn(B, Cout, s * Hs, s * Hs, device="cuda", generator=gen)       # operand in the x slot
        b = torch.randn(B, Cin, Hs, Hs, device="cuda", generator=gen)                # operand in the gy slot
        rows, cols = Cin, Cout
    else:
        a = torch.randn(B, Cin, Hs, Hs, device="cuda", generator=gen)
        oh = (Hs - 1) // s + 1
        b = torch.randn(B, Cout, oh, oh, device="cuda", generator=gen)
        rows, cols = Cout, Cin
    aff = None
    if act is not None:
        C = Cin                                                                     # the layer's input channels
        scale = 0.5 + torch.rand(C, device="cuda", generator=gen)
        shift = torch.randn(C, device="cuda", generator=gen)
        aff = (scale, shift, act)
    kw = dict(in_affine=aff, affine_on_gy=transposed) if aff is not None else {}
    gw = H.conv5x5_wgrad(a, b, s, **kw)
    assert gw.shape == (rows, cols, 5, 5)
    second = H.conv5x5_wgrad(a, b, s, out=gw.clone(), accumulate=True, **kw)
    assert torch.equal(second, gw + gw), "accumulating second use"

    co, ci = _clip(CO_EDGES, rows), _clip(CI_EDGES, cols)
    ac, bc = a[:, ci].cpu().double(), b[:, co].cpu().double()
    if aff is not None:
        if transposed:
            bc = activate(bc, scale[co].cpu(), shift[co].cpu(), act)
        else:
            ac = activate(ac, scale[ci].cpu(), shift[ci].cpu(), act)
    if transposed:      # ConvTranspose2d: x = layer input (bc), gy = output gradient (ac); weight (Cin, Cout, 5, 5)
        w0 = torch.zeros(len(co), len(ci), 5, 5)
        ref = O.convT5x5_grads(bc, w0, ac, s)[1]
        ref32 = O.convT5x5_grads(bc, w0, ac, s, dtype=torch.float32)[1]
    else:
        w0 = torch.zeros(len(co), len(ci), 5, 5)
        ref = O.conv5x5_grads(ac, w0, bc, s)[1]
        ref32 = O.conv5x5_grads(ac, w0, bc, s, dtype=torch.float32)[1]
    e32 = rel_l2(ref32, ref)
    bound = max(CONV_TOL, e32)
    crop = gw[co][:, ci]
    crop2 = second[co][:, ci]
    e1, e2 = rel_l2(crop, ref), rel_l2(crop2, 2 * ref)
    name = f"{'convT' if transposed else 'conv'} {Cin}->{Cout} @{Hs} s{s}"
    print(f"WGRAD-B128 {name:28s} kernel {e1:.2e} / {e2:.2e}  e32 {e32:.2e}  bound {bound:.2e}")
    assert_close(crop, ref, bound, name)
    assert_close(crop2, 2 * ref, bound, name + ", accumulated")
