"""The fp16x3 5x5 convolution kernels per element: csrc/conv_ring.hip at every tile variant, geometry, pairing and K split,
its affine on load and statistics epilogue, and -- second table -- csrc/conv_bf16split.hip at every forced tile.

Every launch goes through the C ABI (vg_conv5x5_fwd_bf16split / vg_convT5x5_fwd_bf16split) of the tuning build with the
two bounds handed in explicitly (ConvFusion.in_amax, the pack's w_amax): the output sits NaN-filled in the middle of a
guard-filled buffer, workspace and statistics buffers likewise, and the guards must be intact afterwards.  A ring case
first asserts the route it claims (vg_debug_ring_route: the launch's own code).  Then tests/_ring_refs.py's check: every
element finite and |got - emul64| <= k 2^-24 mag, no element excluded; k, the references and where K_ACC comes from
(the CPU restatement, tests/test_conv_ring_cpu.py) are described there.  The printed figure is the worst element's
share of its bound; it is a record and feeds nothing."""
import ctypes

import pytest
import torch

import _ring_refs as R

pytestmark = pytest.mark.gpu

GUARD = -12345.5
FRONT, BACK = 1024, 4096        # guard floats in front of / behind every buffer the kernel writes
PLANES = 2 | 0x100              # VG_PLANES_F16
BAD_ARG, NO_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    prev, ops.CONV_ARITH = ops.CONV_ARITH, "fp16x3"
    yield ops
    ops.CONV_ARITH = prev


@pytest.fixture
def tuning(H):
    """The tuning build (tile-forcing knobs, the route query) for one test; the knobs are back on the heuristic afterwards."""
    from disentangle_mlp_amd import _lib
    with _lib.use_tuning() as lib:
        try:
            yield lib
        finally:
            lib.vg_debug_set_conv_ring_tile(-1)
            lib.vg_debug_set_conv_bf16split_tile(-1)


class Guarded:
    """n floats filled with ``fill`` between two guard zones."""

    def __init__(self, n, fill=float("nan")):
        self.n = n
        self.buf = torch.full((FRONT + n + BACK,), GUARD, dtype=torch.float32, device="cuda")
        self.view = self.buf[FRONT:FRONT + n]
        self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:FRONT] == GUARD).all()) and bool((self.buf[FRONT + self.n:] == GUARD).all())


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(lib, H, case, x, w, bias, xb, wb, affine=None, stats=False, workspace="need", stats_floats=None):
    """One launch of ``case``; returns (status, y on the host or None, statistics (slots, Cout, 2) on the host or None).
    ``stats``: ask for the statistics epilogue (True: a buffer of the size the library asks for, an int: of that many
    floats; ``stats_floats``: the size DECLARED to the kernel instead of the true one).  ``workspace``: "need" -- what the
    library asks for --, None, or a number of bytes."""
    from disentangle_mlp_amd import _lib
    tr = case.mode == R.TR
    name = "convT5x5" if tr else "conv5x5"
    shape = (case.B, case.Cin, case.H, case.W, case.Cout)
    lib.vg_debug_set_conv_ring_tile(-1 if (case.force is None or not case.ring) else case.force)
    lib.vg_debug_set_conv_bf16split_tile(-1 if (case.force is None or case.ring) else case.force)
    if case.ring:       # the route this case is in the table for, from the launch's own code
        out = (ctypes.c_int * 6)()
        assert lib.vg_debug_ring_route(case.mode, *shape, PLANES, out) == 0
        assert tuple(out) == case.route, (case.id, tuple(out))
    st = H._stream()
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    pk = torch.empty(lib.vg_conv5x5_packed_bf16split_bytes(case.Cout, case.Cin, PLANES) // 4, dtype=torch.float32, device="cuda")
    bounds = torch.tensor([xb, wb], dtype=torch.float32, device="cuda")
    _lib.check(lib.vg_conv5x5_pack_bf16split(wd.data_ptr(), pk.data_ptr(), case.Cout, case.Cin, int(tr), case.stride, PLANES,
                                             bounds[1:].data_ptr(), st), "vg_conv5x5_pack_bf16split")
    need = getattr(lib, f"vg_{name}_fwd_bf16split_workspace_bytes")(*shape, case.stride, PLANES)
    OH, OW = case.out_hw
    assert need == (case.ksplit * 4 * case.B * case.Cout * OH * OW if case.ksplit > 1 else 0), (case.id, need)
    ws_bytes = need if workspace == "need" else (workspace or 0)
    ws = Guarded(ws_bytes // 4) if ws_bytes else None
    f = _lib.ConvFusion()
    f.in_amax = bounds.data_ptr()
    if affine is not None:
        sc, sh = _dev(affine[0]), _dev(affine[1])
        f.in_scale, f.in_shift, f.in_act = sc.data_ptr(), sh.data_ptr(), affine[2]
    sb = None
    if stats:
        n = getattr(lib, f"vg_{name}_fwd_bf16split_stats_floats")(*shape, case.stride, PLANES) if stats is True else stats
        sb = Guarded(n)
        f.stats, f.stats_floats = sb.view.data_ptr(), n if stats_floats is None else stats_floats
    y = Guarded(case.B * case.Cout * OH * OW)
    rc = getattr(lib, f"vg_{name}_fwd_bf16split")(xd.data_ptr(), pk.data_ptr(), _ptr(bd), y.view.data_ptr(), *shape, case.stride,
                                                   PLANES, None if ws is None else ws.view.data_ptr(), ws_bytes, ctypes.byref(f), st)
    torch.cuda.synchronize()
    assert y.intact(), f"{case.id}: wrote outside the output"
    assert ws is None or ws.intact(), f"{case.id}: wrote outside the workspace"
    assert sb is None or sb.intact(), f"{case.id}: wrote outside the statistics buffer"
    if rc != 0:
        assert bool(torch.isnan(y.view).all()), f"{case.id}: a refused launch wrote to the output"
        return rc, None, None
    return rc, y.view.view(case.B, case.Cout, OH, OW).cpu(), None if sb is None else sb.view.view(-1, case.Cout, 2).cpu()


_refs = {}


def references(case, act=None, loose=0):
    """(x, w, bias, affine, x bound, w bound, emul64, mag) of a case's operands: computed once per shape, shared among the
    tests (and the forced variants of a shape), never written to."""
    key = (case._replace(force=None, route=()), act, loose)
    if key not in _refs:
        x, w, bias = R.operands(case)
        affine = None if act is None else R.affine_of(case, act)
        xb, wb = R.bound_of(R.activated(x, affine)) * 2.0 ** loose, R.bound_of(w) * 2.0 ** loose
        tr = case.mode == R.TR
        _refs[key] = (x, w, bias, affine, xb, wb, R.emul64(x, w, bias, xb, wb, tr, affine, case.stride),
                      R.mag(x, w, bias, tr, affine, case.stride))
    return _refs[key]


def judge(case, y, ref, m, affine=False, what=""):
    """Every element inside its bound; prints the worst element's share of its bound."""
    k = R.k_of(case, affine)
    ok, worst = R.check(y, ref, m.expand_as(ref), k.expand_as(ref))
    share = R.ratio(y, ref, m * k) if worst == worst else float("nan")
    print(f"{case.id} {what}: worst element at {share:.3f} of its bound (k <= {float(k.max()):.0f}; {worst:.2f} x 2^-24 mag)")
    assert ok, (case.id, what, worst)


def run_case(lib, H, case, act=None, loose=0, stats=False):
    x, w, bias, affine, xb, wb, ref, m = references(case, act, loose)
    rc, y, st = launch(lib, H, case, x, w, bias, xb, wb, affine, stats)
    assert rc == 0, (case.id, rc)
    judge(case, y, ref, m, affine is not None, f"act {act} loose 2^{loose}" + (" + statistics" if stats else ""))
    if stats:
        ok, worst = R.stats_ok(st, y)
        print(f"{case.id} statistics: {worst:.3f} of 64 x 2^-24 sum |y|")
        assert ok, (case.id, worst)
    return y, st


# ---------------------------------------------------------------------------------------------------- 1. every route
@pytest.mark.parametrize("case", R.RING_CASES, ids=lambda c: c.id)
def test_ring_case(H, tuning, case):
    run_case(tuning, H, case)


@pytest.mark.parametrize("loose", [1, 5])
@pytest.mark.parametrize("case", R.FUSION_CASES, ids=lambda c: c.id)
def test_loose_bounds(H, tuning, case, loose):
    run_case(tuning, H, case, loose=loose)


# ---------------------------------------------------------------------------------------------------- 2. fusion
@pytest.mark.parametrize("what", ["none", "relu", "lrelu+stats", "stats"])
@pytest.mark.parametrize("case", R.FUSION_CASES, ids=lambda c: c.id)
def test_fusion(H, tuning, case, what):
    """The affine on load with each activation and shifts of both signs (zero padding pads the ACTIVATED tensor: a
    non-zero act(shift) in the halo would show at every border element), the statistics epilogue, both together."""
    act = {"none": R.ACT_NONE, "relu": R.ACT_RELU, "lrelu+stats": R.ACT_LRELU, "stats": None}[what]
    run_case(tuning, H, case, act=act, stats=what.endswith("stats"))


def test_refused_launches(H, tuning):
    split, plain = R.RING_TR_SPLIT[0], R.RING_FWD[1]
    x, w, bias, _, xb, wb, _, _ = references(split)
    assert launch(tuning, H, split, x, w, bias, xb, wb, stats=4096)[0] == BAD_ARG                 # statistics of a K split
    assert launch(tuning, H, split, x, w, bias, xb, wb, workspace=None)[0] == NO_WORKSPACE
    need = split.ksplit * 4 * split.B * split.Cout * split.out_hw[0] * split.out_hw[1]
    assert launch(tuning, H, split, x, w, bias, xb, wb, workspace=need - 4)[0] == NO_WORKSPACE
    x, w, bias, _, xb, wb, _, _ = references(plain)
    need = tuning.vg_conv5x5_fwd_bf16split_stats_floats(plain.B, plain.Cin, plain.H, plain.W, plain.Cout, 2, PLANES)
    assert need > 0
    assert launch(tuning, H, plain, x, w, bias, xb, wb, stats=True, stats_floats=need - 1)[0] == BAD_ARG
    assert launch(tuning, H, plain, x, w, bias, xb, wb, stats=True, stats_floats=need)[0] == 0


# ---------------------------------------------------------------------------------------------------- 3. one pixel
@pytest.mark.parametrize("case", R.PIXEL_CASES, ids=lambda c: c.id)
def test_one_pixel(H, tuning, case):
    """Image 1 of the batch is zero except a single 1.0 -- at each corner in turn and next to a tile seam (the last
    pixel of the first tile where the image has a second one): its output is that input channel's filter where the image
    holds it and exactly 0 everywhere else.  The bound handed in is 8 x the true maximum.  Per element (the derivation of
    tests/test_convT_quad_gpu.py::test_single_corner_pixel): 1.0 times a power of two is exact in the hi plane; a filter
    value's hi + lo planes drop at most 2^-23 of it (2^-39 of the filter's bound once lo is an fp16 subnormal), the fp32
    accumulations round by 2^-24 each: |y - w| <= 2^-21 |w| + 2^-38 max |w|."""
    x0, w, _ = R.operands(case)
    _v, _k, NB, TH, TW, _p = case.route
    s_in = 1 if case.mode == R.TR else 2                      # input pixels per pixel of the tile space
    seam = (min(case.H - 2, s_in * TH - 1), min(case.W - 2, s_in * TW - 1))
    tr, ci = case.mode == R.TR, 5
    wb = R.bound_of(w)
    for (r, c) in [(0, 0), (0, case.W - 1), (case.H - 1, 0), (case.H - 1, case.W - 1), seam]:
        x = x0.clone()
        x[1] = 0.0
        x[1, ci, r, c] = 1.0
        xb = 8.0 * R.bound_of(x)
        rc, y, _ = launch(tuning, H, case, x, w, None, xb, wb)
        assert rc == 0
        judge(case, y, R.emul64(x, w, None, xb, wb, tr), R.mag(x, w, None, tr), what=f"pixel ({r}, {c})")
        ref = R.ref64(x, w, None, tr)[1]
        zero = ref == 0
        assert int((~zero).sum()) > 0 and bool((y[1][zero] == 0).all()), (case.id, r, c, "a non-zero where the filter does not reach")
        err = (y[1].double() - ref).abs()
        assert bool((err <= 2.0 ** -21 * ref.abs() + 2.0 ** -38 * wb).all()), (case.id, r, c, float(err.max()))


# ---------------------------------------------------------------------------------------------------- 4. repeat
@pytest.mark.parametrize("case", R.REPEAT_CASES, ids=lambda c: c.id)
def test_two_runs_are_bit_identical(H, tuning, case):
    x, w, bias, _, xb, wb, _, _ = references(case)
    a, b = (launch(tuning, H, case, x, w, bias, xb, wb)[1] for _ in range(2))
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 5. conv_bf16split.hip
def _by_variant(cases):
    vs = sorted({c.force for c in cases})
    return [pytest.param([c for c in cases if c.force == v], id=f"v{v}") for v in vs]


@pytest.mark.parametrize("cases", _by_variant(R.X_FWD))
def test_stride1_forward_every_tile(H, tuning, cases):
    """Widths 8, 16, 32 (the three pixel-tile geometries) and a ragged 13 x 9, Cout 1 / 33 / 130, odd batch."""
    for case in cases:
        run_case(tuning, H, case)


@pytest.mark.parametrize("case", R.X_FWD_SPLIT, ids=lambda c: c.id)
def test_stride1_forward_k_split(H, tuning, case):
    run_case(tuning, H, case)


@pytest.mark.parametrize("cases", _by_variant(R.X_TR))
def test_thin_transposed_every_tile(H, tuning, cases):
    """Stride 1 and stride 2 (Cout <= 64: the layers the ring does not take), variants 0 - 5."""
    for case in cases:
        run_case(tuning, H, case)
