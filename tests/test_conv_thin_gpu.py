"""The kernels of the 3-channel edge layers per element, at every launch edge: csrc/conv_thin_fwd.hip
(vg_conv5x5_thin_bf16split: Cin <= 3 forward, stride 1 and 2, statistics epilogue), csrc/conv_thin_mfma.hip
(vg_convT5x5_s1_thin_bf16split: 32 -> (<= 3) transposed, affine on load) and csrc/conv_thin.hip (the exact-fp32 VALU
kernel behind vg_convT5x5_fwd at stride 1 and Cout <= 4).

Every launch goes through the C ABI of the product library, on torch's current stream: the output sits NaN-filled in the
middle of a guard-filled buffer, the statistics buffer likewise, and the guards must be intact afterwards; a refused
launch leaves the output all NaN.  Then tests/_thin_refs.py's check: every element finite and |got - emul64| <= k 2^-24
mag, no element excluded; k, the references, the one-pixel bound, the statistics contract and where K_ACC comes from (the
CPU restatements, tests/test_conv_thin_cpu.py) are described there.  The printed figure is the worst element's share of
its bound; it is a record and feeds nothing."""
import pytest
import torch

import _thin_refs as T

pytestmark = pytest.mark.gpu

GUARD = -12345.5
FRONT, BACK = 1024, 4096        # guard floats in front of / behind every buffer the kernel writes


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    prev, ops.CONV_ARITH = ops.CONV_ARITH, "fp16x3"
    yield ops
    ops.CONV_ARITH = prev


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


def launch(H, case, x, w, bias, affine=None, stats=False, stats_short=0, act=None, no_shift=False):
    """One launch of ``case``; returns (status, y on the host or None, statistics (slots, Cout, 2) on the host or None).
    ``stats``: ask the forward kernel for its statistics epilogue, in a buffer of the size the library asks for, DECLARED
    ``stats_short`` floats shorter.  ``affine``: (scale, shift, act) of the transposed kernel; ``act`` overrides the
    activation, ``no_shift`` hands the scale in alone."""
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    st = H._stream()
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    OH, OW = case.out_hw
    y = Guarded(case.B * case.Cout * OH * OW)
    sb = None
    if case.kind == T.FWD:
        n = 0
        if stats:
            n = lib.vg_conv5x5_thin_bf16split_stats_floats(*case.shape, case.stride)
            assert n == len(T.slot_regions(case)) * case.Cout * 2, (case.id, n)
            sb = Guarded(n)
        rc = lib.vg_conv5x5_thin_bf16split(xd.data_ptr(), wd.data_ptr(), _ptr(bd), y.view.data_ptr(), *case.shape, case.stride,
                                           case.planes, None if sb is None else sb.view.data_ptr(), n - stats_short, st)
    elif case.kind == T.TR:
        sc = sh = None
        if affine is not None:
            sc, sh = _dev(affine[0]), _dev(affine[1])
            act = affine[2] if act is None else act
        rc = lib.vg_convT5x5_s1_thin_bf16split(xd.data_ptr(), wd.data_ptr(), _ptr(bd), y.view.data_ptr(), *case.shape, case.planes,
                                               _ptr(sc), None if no_shift else _ptr(sh), act or 0, st)
    else:
        assert lib.vg_convT5x5_s1_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout) == 0      # the MFMA kernel refuses it
        rc = lib.vg_convT5x5_fwd(xd.data_ptr(), wd.data_ptr(), _ptr(bd), y.view.data_ptr(), *case.shape, 1, st)
    torch.cuda.synchronize()
    assert y.intact(), f"{case.id}: wrote outside the output"
    assert sb is None or sb.intact(), f"{case.id}: wrote outside the statistics buffer"
    if rc != 0:
        assert bool(torch.isnan(y.view).all()), f"{case.id}: a refused launch wrote to the output"
        assert sb is None or bool(torch.isnan(sb.view).all()), f"{case.id}: a refused launch wrote statistics"
        return rc, None, None
    return rc, y.view.view(case.B, case.Cout, OH, OW).cpu(), None if sb is None else sb.view.view(-1, case.Cout, 2).cpu()


_refs = {}


def references(case, with_bias=True, act=None):
    """(x, w, bias, affine, emul64, mag) of a case's operands: computed once, shared among the tests, never written to."""
    key = (case, with_bias, act)
    if key not in _refs:
        x, w, bias = T.operands(case)
        bias = bias if with_bias else None
        affine = None if act is None else T.affine_of(case, act)
        _refs[key] = (x, w, bias, affine, T.emul64(case, x, w, bias, affine), T.mag(case, x, w, bias, affine))
    return _refs[key]


def judge(case, y, ref, m, affine=False, what=""):
    """Every element inside its bound; prints and returns the worst element's share of its bound."""
    k = T.k_of(case, affine)
    ok, worst = T.check(y, ref, m, torch.full_like(m, k))
    share = worst / k
    print(f"{case.id} {what}: worst element at {share:.3f} of its bound (k = {k}; {worst:.2f} x 2^-24 mag)")
    assert ok, (case.id, what, worst)
    return share


# ---------------------------------------------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("case", T.FWD_CASES, ids=lambda c: c.id)
def test_forward_case(H, case):
    """With and without bias, with and without statistics; the statistics pointer does not change a bit of the output."""
    for with_bias in (True, False):
        x, w, bias, _, ref, m = references(case, with_bias)
        rc, y, _ = launch(H, case, x, w, bias)
        assert rc == 0, (case.id, rc)
        judge(case, y, ref, m, what="bias" if with_bias else "no bias")
        rc, ys, st = launch(H, case, x, w, bias, stats=True)
        assert rc == 0 and torch.equal(y.view(torch.int32), ys.view(torch.int32)), (case.id, "the statistics pointer changed the output")
        assert st is not None and bool(torch.isfinite(st).all()), (case.id, "a statistics slot was not written")


@pytest.mark.parametrize("case", T.TRANSPOSED + T.VALU_CASES, ids=lambda c: c.id)
def test_transposed_case(H, case):
    for with_bias in (True, False):
        x, w, bias, _, ref, m = references(case, with_bias)
        rc, y, _ = launch(H, case, x, w, bias)
        assert rc == 0, (case.id, rc)
        judge(case, y, ref, m, what="bias" if with_bias else "no bias")


# ---------------------------------------------------------------------------------------------------- 2. statistics
@pytest.mark.parametrize("case", T.FWD_CASES, ids=lambda c: c.id)
def test_statistics_per_slot(H, case):
    """Every slot written, and each within VG_STATS_SLOT_DEPTH x 2^-24 of its sum of magnitudes, for y and for y^2, against
    fp64 sums of the device's own output over the slot's region."""
    x, w, bias, _, _, _ = references(case)
    rc, y, st = launch(H, case, x, w, bias, stats=True)
    assert rc == 0
    ok, worst = T.slots_ok(case, st, y)
    print(f"{case.id} statistics: worst slot at {worst:.3f} of 16 x 2^-24 sum |y| ({st.shape[0]} slots)")
    assert ok, (case.id, worst)


# ---------------------------------------------------------------------------------------------------- 3. affine on load
@pytest.mark.parametrize("act", [T.ACT_NONE, T.ACT_RELU, T.ACT_LRELU])
@pytest.mark.parametrize("case", T.AFFINE_CASES, ids=lambda c: c.id)
def test_affine_on_load(H, case, act):
    """Shifts of both signs: zero padding pads the ACTIVATED tensor, a non-zero act(shift) in the halo would show at every
    border element."""
    x, w, bias, affine, ref, m = references(case, True, act)
    rc, y, _ = launch(H, case, x, w, bias, affine)
    assert rc == 0
    judge(case, y, ref, m, affine=True, what=f"act {act}")


# ---------------------------------------------------------------------------------------------------- 4. one pixel
@pytest.mark.parametrize("case", T.PIXEL_CASES, ids=lambda c: c.id)
def test_one_pixel(H, case):
    """Image 1 of the batch is zero except the single full-mantissa value, no bias: inside the footprint the one-pixel
    bound of tests/_thin_refs.py, everywhere else exactly 0."""
    w = T.operands(case)[1]
    worst = 0.0
    for place in T.pixel_places(case):
        x = T.pixel_input(case, place)
        rc, y, _ = launch(H, case, x, w, None)
        assert rc == 0
        judge(case, y, T.emul64(case, x, w, None), T.mag(case, x, w, None), what=f"pixel {place}")
        ok, share = T.pixel_judge(case, y[1], T.ref64(case, x, w, None)[1])
        print(f"{case.id} pixel {place}: {share:.3f} of the one-pixel bound ({T.pixel_bound(case) / T.U:.2f} x 2^-24 |w v|)")
        assert ok, (case.id, place, share)
        worst = max(worst, share)
    print(f"{case.id}: worst one-pixel share {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- 5. a NaN pixel
@pytest.mark.parametrize("case", T.PIXEL_CASES, ids=lambda c: c.id)
def test_nan_pixel(H, case):
    """One NaN in otherwise random data (data, not a fault): the output is NaN exactly where ref64 is, everywhere else
    finite and inside the bound."""
    x0, w, bias = T.operands(case)
    for place in T.pixel_places(case):
        x = x0.clone()
        x[1, T.pixel_channel(case), place[0], place[1]] = float("nan")
        rc, y, _ = launch(H, case, x, w, bias)
        assert rc == 0
        nan = torch.isnan(T.ref64(case, x, w, bias))
        assert 0 < int(nan.sum()) <= 25 * case.Cout and not bool(nan[0].any())
        assert torch.equal(torch.isnan(y), nan), (case.id, place, "NaN elsewhere than where the pixel reaches")
        clean = torch.nan_to_num(x, nan=0.0)
        ref = T.emul64(case, clean, w, bias)
        judge(case, torch.where(nan, ref.float(), y), ref, T.mag(case, clean, w, bias), what=f"NaN at {place}")


# ---------------------------------------------------------------------------------------------------- 6. powers of two
@pytest.mark.parametrize("case", T.SCALING_CASES, ids=lambda c: c.id)
def test_power_of_two_scaling(H, case):
    """y(2^k x, s w) = 2^k s y(x, w) bit for bit, k = -40 and 40, s = 1 and 2^-30: the planes span the full fp32 range."""
    x, w = T.scaling_operands(case)
    m = T.mag(case, x, w, None)
    rc, y0, _ = launch(H, case, x, w, None)
    assert rc == 0
    judge(case, y0, T.emul64(case, x, w, None), m, what="unscaled")
    for k in (-40, 40):
        for s in (1.0, 2.0 ** -30):
            xs, ws = x * 2.0 ** k, w * s
            px, pw = T.planes3(xs, case.planes), T.planes3(ws, case.planes)
            assert all(torch.equal(a, b * 2.0 ** k) for a, b in zip(px, T.planes3(x, case.planes)))      # the planes scale exactly
            least = min(float(p.abs()[p != 0].min()) for p in px) * min(float(p.abs()[p != 0].min()) for p in pw)
            assert least > 2.0 ** -120 and float(m.max()) * 2.0 ** k * s < 2.0 ** 120, (case.id, k, s, least)
            rc, y, _ = launch(H, case, xs, ws, None)
            assert rc == 0
            assert torch.equal(y.view(torch.int32), (y0 * 2.0 ** k * s).view(torch.int32)), (case.id, k, s)


# ---------------------------------------------------------------------------------------------------- 7. repeat
@pytest.mark.parametrize("case", T.REPEAT_CASES, ids=lambda c: c.id)
def test_two_runs_are_bit_identical(H, case):
    x, w, bias, _, _, _ = references(case)
    stats = case.kind == T.FWD
    (_, ya, sa), (_, yb, sb) = (launch(H, case, x, w, bias, stats=stats) for _ in range(2))
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    assert not stats or torch.equal(sa.view(torch.int32), sb.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 8. the ops wrappers
@pytest.mark.parametrize("case", T.OPS_CASES, ids=lambda c: c.id)
def test_ops_wrappers_return_the_bits_of_the_direct_launch(H, case):
    x, w, bias, _, _, _ = references(case)
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    if case.kind == T.FWD:
        route = H.route_conv("conv_fwd", *case.shape, case.stride, want_stats=True)
        assert route.family == H.THIN and route.stats_floats == len(T.slot_regions(case)) * case.Cout * 2
        _, y, st = launch(H, case, x, w, bias, stats=True)
        yo, so = H.conv5x5_fwd(xd, wd, bd, case.stride, want_stats=True)
        assert torch.equal(so.cpu().view(-1, case.Cout, 2).view(torch.int32), st.view(torch.int32))
    elif case.kind == T.TR:
        affine = T.affine_of(case, T.ACT_LRELU)
        route = H.route_conv("convT_fwd", *case.shape, 1, affine="x")
        assert route.family == H.THIN and route.affine_on_load
        _, y, _ = launch(H, case, x, w, bias, affine)
        yo = H.convT5x5_fwd(xd, wd, bd, 1, in_affine=(_dev(affine[0]), _dev(affine[1]), affine[2]))
    else:
        assert H.route_conv("convT_fwd", *case.shape, 1).family == H.FP32_PLAIN
        _, y, _ = launch(H, case, x, w, bias)
        yo = H.convT5x5_fwd(xd, wd, bd, 1)
    assert torch.equal(yo.cpu().view(torch.int32), y.view(torch.int32)), case.id


# ---------------------------------------------------------------------------------------------------- 9. refusals
@pytest.mark.parametrize("what,case,kw,shape_ok", T.REFUSED_FWD + T.REFUSED_TR, ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_refused_launch(H, what, case, kw, shape_ok):
    """One past each limit: the host-only query and the launch agree, and the refused launch writes nothing."""
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    x, w, bias = T.operands(case)
    affine = T.affine_of(case, T.ACT_RELU) if "act" in kw else None
    if case.kind == T.FWD:
        assert lib.vg_conv5x5_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout, case.stride) == int(shape_ok)
        assert (lib.vg_conv5x5_thin_bf16split_stats_floats(*case.shape, case.stride) > 0) == shape_ok
    else:
        assert lib.vg_convT5x5_s1_thin_bf16split_ok(case.Cin, case.H, case.W, case.Cout) == int(shape_ok)
    assert launch(H, case, x, w, bias, affine, **kw)[0] == T.BAD_ARG, what
    if shape_ok:                      # the same launch without the one thing refused is taken
        good = case._replace(planes=3)
        assert launch(H, good, x, w, bias, affine, stats=kw.get("stats", False))[0] == 0, what
