"""The general fp16x3 forward convolution (csrc/conv_general.hip) per element: every instantiation (TM, TN in {64, 128},
padded and not) forced at every channel-count and pixel-count edge, both sides of the heuristic's switches, every filter
shape, stride pair and pad class, reduction lengths 1 ... 2048, one output pixel, channel slices, the bound slot, a single
1.0, non-finite inputs, two runs, an input off a 16-byte boundary.

Every launch goes through the C ABI (vg_conv_general_pack / vg_conv_general_fwd) of the tuning build with the two bounds
handed in explicitly (the pack's w_amax, x_amax): the output sits NaN-filled in the middle of a guard-filled buffer, the
pack likewise, and the guards must be intact afterwards.  A case first asserts the route it claims
(vg_debug_conv_general_tile: the launch's own cg_tile).  Then tests/_general_refs.py's check: every element finite and
|got - emul64| <= k 2^-24 mag, no element excluded; k, the references and where K_ACC comes from (the CPU restatement,
tests/test_conv_general_refs_cpu.py, which also shows which mistakes the check rejects) are described there.  The printed
figure is the worst element's share of its bound; it is a record and feeds nothing."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _general_refs as G

pytestmark = pytest.mark.gpu

GUARD = G.GUARD
FRONT, BACK = 1024, 4096        # guard floats in front of / behind every buffer a kernel writes
BAD_ARG = -1


@pytest.fixture
def tuning():
    """The tuning build (the tile knob, the route query) for one test; the knob is back on the heuristic afterwards."""
    from disentangle_mlp_amd import _lib
    with _lib.use_tuning() as lib:
        try:
            yield lib
        finally:
            lib.vg_debug_set_conv_general_tile(0, 0)


class Guarded:
    """n floats filled with ``fill`` between two guard zones (the view starts 4096 bytes into the allocation)."""

    def __init__(self, n, fill=float("nan")):
        self.n = n
        self.buf = torch.full((FRONT + n + BACK,), GUARD, dtype=torch.float32, device="cuda")
        self.view = self.buf[FRONT:FRONT + n]
        self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:FRONT] == GUARD).all()) and bool((self.buf[FRONT + self.n:] == GUARD).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def launch(lib, case, x, w, bias, xb, wb, relu=False, slot=None, sliced=False, x_shift=0, fwd_args=None):
    """One pack and one launch of ``case``; returns (status, y on the host or None).  ``slot``: a Guarded of one float
    for y_amax (None: NULL).  ``sliced``: y is channels [SLICE_BEFORE, + Cout) of a GUARD-filled (B, Cout + SLICE_EXTRA,
    OH, OW) buffer and the whole buffer comes back.  ``x_shift``: x starts that many floats behind a 16-byte boundary.
    ``fwd_args``: overrides of vg_conv_general_fwd's geometry arguments (refused launches)."""
    from disentangle_mlp_amd import _lib
    assert lib.vg_debug_set_conv_general_tile(*(case.force or (0, 0))) == 0
    out = (ctypes.c_int * 3)()          # the route this case is in the table for, from the launch's own code
    assert lib.vg_debug_conv_general_tile(case.Cout, case.npix, case.pad, out) == 0
    assert tuple(out) == case.route, (case.id, tuple(out))
    st = _stream()
    xbuf = torch.zeros(x.numel() + 8, dtype=torch.float32, device="cuda")
    off = (-(xbuf.data_ptr() // 4) % 4 + x_shift) % 8
    xd = xbuf[off:off + x.numel()].view(x.shape)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4 * x_shift
    wd = w.cuda().contiguous()
    bd = None if bias is None else bias.cuda().contiguous()
    bounds = torch.tensor([xb, wb], dtype=torch.float32, device="cuda")
    nbytes = lib.vg_conv_general_packed_bytes(case.Cout, case.Cin, case.KH, case.KW)
    assert nbytes and nbytes % 16 == 0
    pk = Guarded(nbytes // 4)
    assert pk.view.data_ptr() % 16 == 0
    _lib.check(lib.vg_conv_general_pack(wd.data_ptr(), pk.view.data_ptr(), case.Cout, case.Cin, case.KH, case.KW,
                                        bounds[1:].data_ptr(), st), "vg_conv_general_pack")
    OH, OW = case.out_hw
    total = case.Cout + (G.SLICE_EXTRA if sliced else 0)
    y = Guarded(case.B * total * OH * OW, GUARD if sliced else float("nan"))
    full = y.view.view(case.B, total, OH, OW)
    before = G.SLICE_BEFORE if sliced else 0
    mine = full[:, before:before + case.Cout]
    mine.fill_(float("nan"))
    a = dict(B=case.B, Cin=case.Cin, H=case.H, W=case.W, Cout=case.Cout, KH=case.KH, KW=case.KW, sh=case.sh, sw=case.sw,
             ph=case.ph, pw=case.pw, ystride=total * OH * OW)
    a.update(fwd_args or {})
    rc = lib.vg_conv_general_fwd(xd.data_ptr(), pk.view.data_ptr(), None if bd is None else bd.data_ptr(), mine.data_ptr(),
                                 a["B"], a["Cin"], a["H"], a["W"], a["Cout"], a["KH"], a["KW"], a["sh"], a["sw"], a["ph"],
                                 a["pw"], a["ystride"], int(relu), bounds.data_ptr(), None if slot is None else slot.view.data_ptr(),
                                 st)
    torch.cuda.synchronize()
    assert y.intact(), f"{case.id}: wrote outside the output"
    assert pk.intact(), f"{case.id}: the pack kernel wrote outside the pack"
    assert slot is None or slot.intact(), f"{case.id}: wrote outside the bound slot"
    if rc != 0:
        assert bool(torch.isnan(mine).all()), f"{case.id}: a refused launch wrote to the output"
        return rc, None
    return rc, full.cpu()


_refs = {}


def references(case, loose=0, bias=True, relu=False, nonneg=False):
    """(x, w, bias or None, x bound, w bound, emul64, mag) of a case's operands: computed once per shape, shared among
    the tests (and the forced tiles of a shape), never written to."""
    key = (case.geometry, loose, bias, relu, nonneg)
    if key not in _refs:
        x, w, b = G.operands(case, nonneg=nonneg)
        b = b if bias else None
        xb, wb = G.bound_of(x) * 2.0 ** loose, G.bound_of(w) * 2.0 ** loose
        _refs[key] = (x, w, b, xb, wb, G.emul64(case, x, w, b, xb, wb, relu), G.mag(case, x, w, b))
    return _refs[key]


def judge(case, y, ref, m, what=""):
    """Every element inside its bound; prints the worst element's share of its bound."""
    k = G.k_of(case)
    ok, worst = G.check(y, ref, m, k)
    share = G.ratio(y, ref, m * k) if worst == worst else float("nan")
    print(f"{case.id} {what}: worst element at {share:.3f} of its bound (k = {k}; {worst:.2f} x 2^-24 mag)")
    assert ok, (case.id, what, worst)


def run_case(lib, case, **kw):
    x, w, b, xb, wb, ref, m = references(case, **kw)
    rc, y = launch(lib, case, x, w, b, xb, wb, relu=kw.get("relu", False))
    assert rc == 0, (case.id, rc)
    judge(case, y, ref, m, " ".join(f"{k} {v}" for k, v in kw.items()))
    return y


# ---------------------------------------------------------------------------------------------------- 1. every route and edge
@pytest.mark.parametrize("case", [c for g in G.MAIN_GROUPS for c in G.GROUPS[g]], ids=lambda c: c.id)
def test_case(tuning, case):
    run_case(tuning, case)


@pytest.mark.parametrize("variant", ["relu", "nobias", "relu-nobias", "nonneg-relu"])
@pytest.mark.parametrize("group", G.MAIN_GROUPS)
def test_case_variants(tuning, group, variant):
    """ReLU on, bias NULL, both, and the non-negative input of the network, on one case of every group (without a bias
    the frame of the pad-15 case is exactly 0: its bound there is 0)."""
    run_case(tuning, G.VARIANT_CASES[group], relu="relu" in variant, bias="nobias" not in variant, nonneg="nonneg" in variant)


@pytest.mark.parametrize("loose", G.LOOSE)
@pytest.mark.parametrize("case", G.LOOSE_CASES, ids=lambda c: c.id)
def test_loose_bounds(tuning, case, loose):
    run_case(tuning, case, loose=loose)


def test_refused_launches_leave_the_output_alone(tuning):
    case = G.TILE_CASES[1]
    x, w, b, xb, wb, _, _ = references(case)
    OH, OW = case.out_hw
    for bad in (dict(sh=3), dict(sw=0), dict(ph=16), dict(ystride=case.Cout * OH * OW - 1), dict(B=0), dict(KH=16), dict(H=1, ph=0)):
        assert launch(tuning, case, x, w, b, xb, wb, fwd_args=bad)[0] == BAD_ARG, bad
    assert launch(tuning, case, x, w, b, xb, wb)[0] == 0


# ---------------------------------------------------------------------------------------------------- 2. slices
@pytest.mark.parametrize("case", G.SLICE_CASES, ids=lambda c: c.id)
def test_slices(tuning, case):
    """Channels [5, 5 + Cout) of a (B, Cout + 12, OH, OW) buffer through y_image_stride: the written channels inside
    their bounds, every other element of the buffer bit-unchanged (the guards around it are launch's)."""
    x, w, b, xb, wb, ref, m = references(case)
    rc, full = launch(tuning, case, x, w, b, xb, wb, sliced=True)
    assert rc == 0
    lo, hi = G.SLICE_BEFORE, G.SLICE_BEFORE + case.Cout
    judge(case, full[:, lo:hi], ref, m, "slice")
    rest = torch.cat([full[:, :lo], full[:, hi:]], dim=1)
    assert torch.equal(_bits(rest), _bits(torch.full_like(rest, GUARD))), f"{case.id}: a neighbouring channel changed"
    rc, alone = launch(tuning, case, x, w, b, xb, wb)
    assert rc == 0 and torch.equal(_bits(alone), _bits(full[:, lo:hi]))


# ---------------------------------------------------------------------------------------------------- 3. the bound slot
@pytest.mark.parametrize("case", [G.TILE_CASES[1], G.TILE_CASES[-16 + 4], G.K_CASES[1]], ids=lambda c: c.id)
def test_bound_slot(tuning, case):
    """y_amax is an atomic maximum on the bit pattern: afterwards the slot holds max(what it held, max |y|) -- the
    bit-exact max |y| of the device's own output from an empty slot and from one pre-filled below it, the pre-filled
    value above it.  NULL: the same output bits, nothing else written."""
    x, w, b, xb, wb, ref, m = references(case)
    rc, y0 = launch(tuning, case, x, w, b, xb, wb)
    assert rc == 0
    judge(case, y0, ref, m, "y_amax NULL")
    top = y0.abs().max()
    assert float(top) > 0
    for name, pre in (("empty", 0.0), ("above", 2.0 * float(top)), ("below", 0.5 * float(top))):
        slot = Guarded(1, pre)
        rc, y = launch(tuning, case, x, w, b, xb, wb, slot=slot)
        assert rc == 0 and torch.equal(_bits(y), _bits(y0)), name
        want = torch.maximum(top, torch.tensor(pre, dtype=torch.float32)).reshape(1)
        assert torch.equal(_bits(slot.view.cpu()), _bits(want)), (case.id, name, float(slot.view), float(top))


# ---------------------------------------------------------------------------------------------------- 4. a single 1.0
@pytest.mark.parametrize("case", G.IMPULSE_CASES, ids=lambda c: c.id)
def test_impulse(tuning, case):
    """Image 1 of the batch is zero except a single 1.0 -- at each corner in turn and at the input pixel under the last
    pixel of the first pixel tile (output pixel tn - 1 of the batch lies in image 1): its output is that input channel's
    filter where the window reaches the pixel and exactly 0 everywhere else.  No bias; the bound handed in is 8 x the
    true maximum.  Per element (the derivation of tests/test_conv_ring_gpu.py::test_one_pixel): 1.0 times a power of two
    is exact in the hi plane; a filter value's hi + lo planes drop at most 2^-23 of it (2^-39 of the filter's bound once
    lo is an fp16 subnormal), the fp32 accumulations round by 2^-24 each: |y - w| <= 2^-21 |w| + 2^-38 max |w|."""
    x0, w, _ = G.operands(case)
    OH, OW = case.out_hw
    r = case.route[1] - 1 - OH * OW                  # output pixel tn - 1, inside image 1
    assert 0 <= r < OH * OW
    seam = (r // OW * case.sh, r % OW * case.sw)
    assert seam[0] < case.H and seam[1] < case.W
    ci, wb = 1, G.bound_of(w)
    for (row, col) in [(0, 0), (0, case.W - 1), (case.H - 1, 0), (case.H - 1, case.W - 1), seam]:
        x = x0.clone()
        x[1] = 0.0
        x[1, ci, row, col] = 1.0
        xb = 8.0 * G.bound_of(x)
        rc, y = launch(tuning, case, x, w, None, xb, wb)
        assert rc == 0
        judge(case, y, G.emul64(case, x, w, None, xb, wb), G.mag(case, x, w, None), f"pixel ({row}, {col})")
        ref = G.ref64(case, x, w, None)[1]
        zero = ref == 0
        assert int((~zero).sum()) > 0 and bool((y[1][zero] == 0).all()), (case.id, row, col, "a non-zero where the filter does not reach")
        err = (y[1].double() - ref).abs()
        assert bool((err <= 2.0 ** -21 * ref.abs() + 2.0 ** -38 * wb).all()), (case.id, row, col, float(err.max()))


# ---------------------------------------------------------------------------------------------------- 5. non-finite inputs
def _last(case, b):
    return (b, case.Cin - 1, case.H - 1, case.W - 1)


NONFINITE = [                                                                   # (case, position of the element)
    (G.NONFINITE_A, (1, 0, 0, 0)),               # padded: every out-of-image tap of image 1 reads this address and selects 0
    (G.NONFINITE_A, _last(G.NONFINITE_A, 1)),
    (G.NONFINITE_A, _last(G.NONFINITE_A, 2)),    # the last element of x
    (G.NONFINITE_B, (1, 0, 0, 0)),               # unpadded, K = 27: the table's five entries beyond K read tap (0, 0) of channel 0
    (G.NONFINITE_C[0], _last(G.NONFINITE_C[0], 4)),      # npix = tn + 1: the columns beyond npix re-read the last pixel
    (G.NONFINITE_C[1], _last(G.NONFINITE_C[1], 4)),
]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case,pos", NONFINITE, ids=lambda v: v.id if isinstance(v, G.Case) else "at" + "_".join(map(str, v)))
def test_nonfinite_stays_local(tuning, case, pos, value):
    """One NaN (or inf: its lo plane is inf - inf) in x, ReLU off, the bound taken from the finite part: the outputs that
    are not finite are exactly those whose window contains the element -- a clamped read that is multiplied by zero
    instead of being replaced by it would spread it -- and every other element passes the per-element check against
    the references of x with that element set to 0."""
    x0, w, b = G.operands(case)
    clean = x0.clone()
    clean[pos] = 0.0
    x = clean.clone()
    x[pos] = value
    xb, wb = G.bound_of(clean), G.bound_of(w)
    rc, y = launch(tuning, case, x, w, b, xb, wb)
    assert rc == 0
    mark = torch.zeros_like(x0, dtype=torch.float64)
    mark[pos] = 1.0
    hit = F.conv2d(mark, torch.ones(1, case.Cin, case.KH, case.KW, dtype=torch.float64), None, stride=(case.sh, case.sw),
                   padding=(case.ph, case.pw)) > 0
    hit = hit.expand_as(y)
    assert int(hit.sum()) > 0
    assert torch.equal(~torch.isfinite(y), hit), (case.id, pos, int((~torch.isfinite(y)).sum()), int(hit.sum()))
    ref, m = G.emul64(case, clean, w, b, xb, wb), G.mag(case, clean, w, b)
    judge(case, torch.where(hit, ref.float(), y), ref, m, f"{value} at {pos}, the finite elements")


# ---------------------------------------------------------------------------------------------------- 6. repeat, alignment
@pytest.mark.parametrize("case", G.REPEAT_CASES, ids=lambda c: c.id)
def test_two_runs_are_bit_identical(tuning, case):
    x, w, b, xb, wb, _, _ = references(case)
    runs = []
    for _ in range(2):
        slot = Guarded(1, 0.0)
        rc, y = launch(tuning, case, x, w, b, xb, wb, relu=True, slot=slot)
        assert rc == 0
        runs.append((y, slot.view.cpu()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize("case", [G.TILE_CASES[1], G.K_CASES[1]], ids=lambda c: c.id)
def test_x_base_alignment(tuning, case):
    """The same x one float behind a 16-byte boundary (a view into a larger tensor): the same bits."""
    x, w, b, xb, wb, ref, m = references(case)
    rc0, y0 = launch(tuning, case, x, w, b, xb, wb)
    rc1, y1 = launch(tuning, case, x, w, b, xb, wb, x_shift=1)
    assert rc0 == 0 and rc1 == 0
    judge(case, y1, ref, m, "x one float off")
    assert torch.equal(_bits(y0), _bits(y1))
