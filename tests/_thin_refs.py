"""References for the kernels of the 3-channel edge layers, with the seeded operands, the case tables and the mutations
the CPU and the GPU tests share.  A plain module: nothing here touches a GPU.

  FWD   csrc/conv_thin_fwd.hip   vg_conv5x5_thin_bf16split       Cin <= 3 forward, stride 1 / 2, statistics epilogue
  TR    csrc/conv_thin_mfma.hip  vg_convT5x5_s1_thin_bf16split   32 -> (<= 3) transposed, stride 1, affine on load
  VALU  csrc/conv_thin.hip       vg_convT5x5_fwd (stride 1, Cout <= 4): the exact-fp32 fmaf kernel

  planes3    the kernels' split (take_bf16_plane, common.hpp): NP successive round-to-nearest bf16 planes of the fp32
             residual.
  emul64     the fp64 sum of the plane products the kernel forms (filter plane + input plane < NP: six for NP = 3, three
             for NP = 2) as fp64 convolutions of the planes, plus bias; the transposed kernel's input is `activated`
             (tests/_ring_refs.py).  For the VALU kernel emul64 is ref64: fp32 operands, no planes.
  ref64      the plain fp64 convolution;  mag  the same convolution of |x| and |w|, plus |bias|.
  restate32  the same products accumulated in fp32 in each kernel's order (below).  It also takes MUTATIONS.

Split model (tests/test_conv_thin_cpu.py holds emul64 to ref64 by it).  A bf16 plane keeps 8 significand bits, so
|w1| <= 2^-8 |w| and |w2| <= 2^-16 |w| (strictly less: by a factor 1 + 2^-8 each), and three planes are the fp32 number
exactly.  NP = 3 drops w1 x2 + w2 x1 + w2 x2 <= (2^-24 + 2^-24 + 2^-32) / (1 + 2^-8)^3 |x||w|:
|emul64 - ref64| <= 2^-23 mag.  NP = 2 drops w1 x1 and the two residuals (w - w0 - w1) x, w (x - x0 - x1), each
<= 2^-16 |x||w|: 3 x 2^-16 mag.

The kernels' orders.
  FWD   per output row 5 NP (NP + 1) / 2 MFMA steps of 16 reduction indices: sum = NP - 1 .. 0, filter plane pa = sum .. 0
        (input plane sum - pa), kh = 0 .. 4, alternating between two accumulators d / d1; a step's indices are k-block 0:
        channel 0, kw 0..4, channel 1, kw 0..2; k-block 1: channel 2, kw 0..4, channel 1, kw 3, 4 and the zero tap
        "kw = 5"; channels >= Cin are zero.  Then d + d1, then + bias.  Each step is a sequential sum over its 16 indices
        into the accumulator (the MFMA's own order is not known).
  TR    per output row and filter column kw an element D[iw][co, kw]: one accumulator per product class (plane index sum)
        over the five kh, within a kh the order written in the source (classes 2 1 2 0 2 1 / 1 0 1), each step a
        sequential sum over the 32 channels; the classes added smallest first; then bias + sum over kw, in kw order, of
        the anti-diagonal D[ow + 2 - kw][co, kw] (zero outside the image: the halo columns of the row buffer).
  VALU  the fmaf chain in the order chunk of 8 channels, channel, kh, kw, then + bias.  The fmaf is formed through fp64:
        the product of two fp32 numbers is exact there, the sum is rounded once to fp64 and once more to fp32 (a double
        rounding: it can differ from the device's single one by an fp32 ulp of the partial sum in rare ties-after-
        rounding; the check's factor 4 covers it).

The check of both test files is _gemm_refs.check: every element finite and |got - emul64| <= k 2^-24 mag, no element
excluded, k = k_of(case): min(K_ACC[kernel], cap) + 2 with an affine on load (one fp32 ulp of difference in the activated
input moves an element by at most 2 x 2^-24 mag, as in _ring_refs.k_of).  `cap` counts the fp32 additions on an
element's path:
  FWD   5 NP (NP + 1) / 2 steps of 16 indices, the merge d + d1, the bias: 482 (NP = 3), 242 (NP = 2);
  TR    the longest class chain (NP products x 5 kh x 32 channels), NP - 1 class additions, 5 for bias + sum over kw:
        487 (NP = 3), 326 (NP = 2);
  VALU  25 Cin fmaf and the bias.
ACC_WORST[kernel] is the worst |restate32 - emul64| / (2^-24 mag) over every case of the kernel's table, as
tests/test_conv_thin_cpu.py::test_k_acc_is_measured_from_the_restatement measures it:

    pytest -s tests/test_conv_thin_cpu.py -k k_acc

K_ACC = ceil(4 ACC_WORST): the factor 4 is the project's margin for the unknown summation order and rounding inside the
MFMA (tests/_gemm_refs.py, tests/_ring_refs.py).  Nothing here is taken from a kernel run.

One pixel (`pixel_bound`).  An image that is zero except one value v whose three planes are all non-zero (PIXEL_VALUE):
every MFMA step then holds at most one non-zero term, so an output element inside the footprint is a sum of the NP (NP +
1) / 2 exact products w_pa v_pb (two bf16 numbers: 16 significand bits) and no other term.  Roundings on its path -- an
addition into a zero accumulator, and of zero, is exact:
  FWD   the products of one tap fall on steps 5 i + kh, i = 0 .. : alternately on d and d1.  NP = 3: three each, two
        roundings each, one for d + d1: 5.  NP = 2: two and one, one rounding, one for the merge: 2.
  TR    class 2 takes three products (2 roundings), class 1 two (1), class 0 one (0), two class additions: 5; NP = 2: 1 +
        1 = 2.  Of the five kw terms one is non-zero.
  VALU  one fmaf into zero: 1, and nothing is dropped.
Each rounding is at most 2^-24 of a partial sum, and a partial sum of plane products is at most (1 + 2^-8)^2 |w v| <
(1 + 2^-6) |w v|.  With the dropped products of the split model:
    |y - w v| <= (roundings (1 + 2^-6) 2^-24 + dropped) |w v|,   dropped = 2^-23 (NP = 3), 3 x 2^-16 (NP = 2), 0 (VALU).
A dropped w0 v2 of PIXEL_VALUE is 2^-17 |w v|, 128 x 2^-24: eighteen times the NP = 3 bound; w1 v1 and w2 v0 depend on
the filter value (9 - 17 bounds over a footprint of the cases' filters, tests/test_conv_thin_cpu.py).

Statistics (`slot_regions`, `slots_ok`).  Slot ((b bands + band) strips + strip) of the forward kernel is the fp32 sum
of y (and of y^2) over rows RB band .. (RB = 8, at stride 2: 4) and columns 32 strip .. + 32 of image b.  The contract
vg_bn_finalize_stats relies on is VG_STATS_SLOT_DEPTH = 16 (common.hpp): no term goes through more than 16 roundings, so
per slot and channel |slot[c][0] - sum y| <= 16 x 2^-24 sum |y| over that region, in fp64 from the device's own output,
and the same with y^2 for slot[c][1].
"""
import functools
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from _gemm_refs import U, _spread, check, ratio                                   # noqa: F401  (re-exported to the tests)
from _ring_refs import ACT_LRELU, ACT_NONE, ACT_RELU, activated, affine_of        # noqa: F401

FWD, TR, VALU = 0, 1, 2
KERNEL = {FWD: "fwd", TR: "tr", VALU: "valu"}
STATS_DEPTH = 16                     # VG_STATS_SLOT_DEPTH of common.hpp: the contract itself
PIXEL_VALUE = 1 + 2.0 ** -9 + 2.0 ** -17 + 2.0 ** -22       # planes 1, 2^-9 + 2^-16, -(2^-17 - 2^-22)

# measured by tests/test_conv_thin_cpu.py (see above); the test fails if a measurement leaves [0.8 ACC_WORST, ACC_WORST]
#   FWD   stride 1: 0.92 - 2.112 (2 x 1 x 8 x 32 -> 33: the worst), stride 2: 0.99 - 1.72
#   TR    0.22 - 0.585 (1 x 32 x 33 x 128 -> 3, two planes: the worst): the 800 terms of an element cancel, and the
#         roundings follow the partial sums, not mag
#   VALU  0.03 (1 x 1 x 1 x 1) - 4.461 (3 x 32 x 33 x 66 -> 1: the worst)
ACC_WORST = {FWD: 2.12, TR: 0.59, VALU: 4.47}
K_ACC = {k: math.ceil(4 * v) for k, v in ACC_WORST.items()}


class Case(NamedTuple):
    """One launch: the kernel, the shape of x (B, Cin, H, W), the output channels, the stride and the planes (VALU: 0)."""
    kind: int
    B: int
    Cin: int
    H: int
    W: int
    Cout: int
    stride: int = 1
    planes: int = 3

    @property
    def id(self):
        p = f"-p{self.planes}" if self.planes else ""
        return f"{KERNEL[self.kind]}{self.stride}-{self.B}x{self.Cin}x{self.H}x{self.W}-{self.Cout}{p}"

    @property
    def shape(self):
        return (self.B, self.Cin, self.H, self.W, self.Cout)

    @property
    def out_hw(self):
        S = self.stride
        return ((self.H - 1) // S + 1, (self.W - 1) // S + 1)

    @property
    def transposed(self):
        return self.kind != FWD

    # ---- the launch geometry the case claims
    @property
    def rows_per_band(self):
        return {FWD: 8 if self.stride == 1 else 4, TR: 16, VALU: 16}[self.kind]

    @property
    def bands(self):
        return -(-self.out_hw[0] // self.rows_per_band)

    @property
    def strips(self):
        """Wavefront columns (FWD: 32 output pixels, TR: 16) or 64-column tiles (VALU) across a row."""
        return -(-self.out_hw[1] // {FWD: 32, TR: 16, VALU: 64}[self.kind])

    @property
    def groups(self):
        return -(-self.Cout // 32) if self.kind == FWD else 1

    @property
    def waves(self):
        return self.strips * self.groups if self.kind != VALU else 4


def _table(kind, stride, shapes, two_planes=()):
    """planes = 3 on every shape; planes = 2 as well on the shapes whose index is in ``two_planes``."""
    out = [Case(kind, *s, stride, 3 if kind != VALU else 0) for s in shapes]
    return tuple(out + [out[i]._replace(planes=2) for i in two_planes])


# ------------------------------------------------------------------------------------------------ the case tables
# the smallest shapes that reach each edge; (B, Cin, H, W, Cout)
FWD1 = _table(FWD, 1, (                # 8-row bands, strips = W / 32, groups = ceil(Cout / 32), waves = strips x groups
    (1, 3, 1, 32, 1),
    (3, 3, 9, 32, 32),                 # two bands, the second one row, full group
    (2, 1, 8, 32, 33),                 # Cin 1, second group of one channel
    (2, 2, 13, 64, 31),                # Cin 2, two strips, partial group
    (2, 3, 17, 96, 40),                # three strips, two 64-column staging pieces
    (1, 3, 5, 64, 128),                # eight waves by groups
    (1, 3, 3, 256, 32),                # eight waves by strips
), two_planes=(1, 5))
FWD2 = _table(FWD, 2, (                # 4-row bands; W even, W / 2 a multiple of 32
    (1, 3, 1, 64, 1),
    (3, 3, 7, 64, 64),
    (2, 3, 9, 64, 70),                 # short last band, partial third group
    (2, 1, 16, 128, 33),               # even H
    (1, 2, 10, 256, 64),               # eight waves
), two_planes=(1, 4))
TRANSPOSED = _table(TR, 1, (           # Cin = 32, 16-row bands, W / 16 waves
    (1, 32, 1, 16, 1),
    (3, 32, 5, 16, 3),
    (2, 32, 16, 32, 2),                # exactly one band
    (2, 32, 17, 48, 3),                # one-row second band, three waves
    (2, 32, 21, 64, 1),
    (1, 32, 33, 128, 3),               # three bands, eight waves
), two_planes=(1, 5, 0, 2))           # (0 and 2: launch_thin_mfma<1, 2> and <2, 2>, which no other case reaches)
VALU_CASES = _table(VALU, 1, (         # 16 x 64 tile, 8-channel chunks
    (1, 1, 1, 1, 1),
    (2, 5, 17, 7, 3),                  # channel tail
    (2, 8, 16, 64, 4),                 # exact tile, Cout 4, 16-byte stores
    (1, 12, 21, 68, 2),                # full chunk then a tail; a 4-column second tile on the 16-byte path
    (1, 32, 5, 130, 3),                # three tiles across, scalar stores
    (3, 32, 33, 66, 1),
))
FWD_CASES = FWD1 + FWD2
TABLES = {FWD: FWD_CASES, TR: TRANSPOSED, VALU: VALU_CASES}
AFFINE_CASES = (TRANSPOSED[3], TRANSPOSED[1])
# one pixel / one NaN: image 1 of the batch, so B >= 2; every kernel, both strides, a second strip and a second band
PIXEL_CASES = (FWD1[3], FWD1[4], FWD2[2], FWD2[3], FWD1[7], TRANSPOSED[3], TRANSPOSED[4], TRANSPOSED[6],
               VALU_CASES[1], VALU_CASES[2], VALU_CASES[5])
SCALING_CASES = (FWD1[3], FWD2[2], FWD1[7], TRANSPOSED[3], TRANSPOSED[6])
REPEAT_CASES = (FWD1[6], TRANSPOSED[5], VALU_CASES[3])       # eight waves with statistics; three bands; a channel tail
OPS_CASES = (FWD1[4], FWD2[2], TRANSPOSED[3], VALU_CASES[4])  # (the VALU one: a width the MFMA kernel refuses)

BAD_ARG = -1
# what each entry point refuses: (what, Case, keyword changes of the launch, whether the shape query still says yes)
REFUSED_FWD = (
    ("Cin 4", Case(FWD, 1, 4, 8, 32, 32, 1), {}, False),
    ("W 48 at stride 1", Case(FWD, 1, 3, 8, 48, 32, 1), {}, False),
    ("W 66 at stride 2", Case(FWD, 1, 3, 8, 66, 32, 2), {}, False),
    ("W 63 at stride 2", Case(FWD, 1, 3, 8, 63, 32, 2), {}, False),
    ("nine waves: 3 strips x 3 groups", Case(FWD, 1, 3, 8, 96, 65, 1), {}, False),
    ("nine waves: 9 strips", Case(FWD, 1, 3, 8, 288, 32, 1), {}, False),
    ("planes 1", Case(FWD, 1, 3, 8, 32, 32, 1, 1), {}, True),
    ("planes 4", Case(FWD, 1, 3, 8, 32, 32, 1, 4), {}, True),
    ("statistics one float short", Case(FWD, 2, 3, 9, 64, 33, 1), {"stats": True, "stats_short": 1}, True),
)
REFUSED_TR = (
    ("Cin 16", Case(TR, 1, 16, 8, 32, 3), {}, False),
    ("Cin 48", Case(TR, 1, 48, 8, 32, 3), {}, False),
    ("W 24", Case(TR, 1, 32, 8, 24, 3), {}, False),
    ("W 144", Case(TR, 1, 32, 8, 144, 3), {}, False),
    ("Cout 4", Case(TR, 1, 32, 8, 32, 4), {}, False),
    ("in_act 3", Case(TR, 1, 32, 8, 32, 3), {"act": 3}, True),
    ("a scale without a shift", Case(TR, 1, 32, 8, 32, 3), {"act": ACT_RELU, "no_shift": True}, True),
    ("planes 1", Case(TR, 1, 32, 8, 32, 3, 1, 1), {}, True),
)


def all_cases():
    return FWD_CASES + TRANSPOSED + VALU_CASES


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(case, seed=0):
    """x (B, Cin, H, W), w ([Cout, Cin, 5, 5] forward, [Cin, Cout, 5, 5] transposed), bias (Cout): full-mantissa
    normals.  The filter's output channels (and the bias with them) spread over four decades in a seeded order: a store
    to the wrong channel plane cannot hide under a neighbour's magnitude.  (The planes are not part of the seed.)"""
    key = 0
    for v in (case.kind, *case.shape, case.stride):
        key = (key * 1009 + v) % 999983
    g = torch.Generator().manual_seed(1000003 * seed + key)
    x = torch.randn(case.B, case.Cin, case.H, case.W, generator=g)
    sp = _spread(case.Cout, 4, g)
    w = torch.randn(case.Cout, case.Cin, 5, 5, generator=g) * 0.05 * sp[:, None, None, None]
    bias = torch.randn(case.Cout, generator=g) * 0.1 * sp
    if case.transposed:
        w = w.transpose(0, 1).contiguous()
    return x, w, bias


@functools.lru_cache(maxsize=None)
def scaling_operands(case):
    """Operands of the power-of-two scaling test: no decade spread, magnitudes in [1, 2) (x) and [2^-4, 2^-3) (w) on a
    grid of 2^-20 of the leading bit, random signs -- all three planes are in use and no non-zero plane is below 2^-20
    of its element."""
    g = torch.Generator().manual_seed(4242 + case.Cin + 7 * case.W + case.Cout)

    def grid(*shape):
        m = 1.0 + torch.randint(0, 2 ** 20, shape, generator=g).double() * 2.0 ** -20
        return (m * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()

    x = grid(case.B, case.Cin, case.H, case.W)
    w = grid(*((case.Cin, case.Cout) if case.transposed else (case.Cout, case.Cin)), 5, 5) * 2.0 ** -4
    return x, w


def pixel_places(case):
    """(row, column) of the single pixel: each corner, the last pixel of the first strip / wavefront column / tile where
    the row has a second one, the last input row of the first band where the image has a second one."""
    H, W, S = case.H, case.W, case.stride
    places = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    strip_w = S * {FWD: 32, TR: 16, VALU: 64}[case.kind]
    if case.strips > 1:
        places.append((H // 2, strip_w - 1))
    if case.bands > 1:
        places.append((S * case.rows_per_band - 1, W // 2))
    return list(dict.fromkeys(places))


def pixel_channel(case):
    return min(13, case.Cin - 1)


def pixel_input(case, place, value=PIXEL_VALUE):
    """The case's x with image 1 zero except ``value`` at ``place`` of channel pixel_channel."""
    assert case.B >= 2
    x = operands(case)[0].clone()
    x[1] = 0.0
    x[1, pixel_channel(case), place[0], place[1]] = value
    return x


def pixel_judge(case, y1, ref1):
    """y1: image 1 of an output for a `pixel_input`, ref1: its ref64 (the filter times the value where the pixel reaches,
    0 elsewhere).  (ok, worst share of the one-pixel bound): exactly 0 outside the footprint, `pixel_bound` inside."""
    y1, inside = y1.detach().cpu().double(), ref1 != 0
    if not bool(torch.isfinite(y1).all()) or int(inside.sum()) == 0 or not bool((y1[~inside] == 0).all()):
        return False, float("nan")
    share = float(((y1 - ref1).abs()[inside] / (pixel_bound(case) * ref1.abs()[inside])).max())
    return share <= 1.0, share


# ------------------------------------------------------------------------------------------------ fp64 references
def planes3(v, NP):
    """NP successive bf16 planes (as fp32 tensors) of v: each the round-to-nearest-even bf16 of what is left."""
    r = v.float().clone()
    out = []
    for _ in range(NP):
        h = r.bfloat16().float()
        out.append(h)
        r = r - h
    return out


def _conv64(x, w, case):
    if case.transposed:
        return F.conv_transpose2d(x, w, None, stride=1, padding=2)
    return F.conv2d(x, w, None, stride=case.stride, padding=2)


def _plus_bias(r, bias, absolute=False):
    if bias is None:
        return r
    b = bias.double().abs() if absolute else bias.double()
    return r + b[None, :, None, None]


def ref64(case, x, w, bias, affine=None):
    return _plus_bias(_conv64(activated(x, affine, torch.float64), w.double(), case), bias)


def mag(case, x, w, bias, affine=None):
    return _plus_bias(_conv64(activated(x, affine).double().abs(), w.double().abs(), case), bias, absolute=True)


def emul64(case, x, w, bias, affine=None):
    xa = activated(x, affine)
    if case.kind == VALU:
        return _plus_bias(_conv64(xa.double(), w.double(), case), bias)
    NP = case.planes
    xp, wp = planes3(xa, NP), planes3(w, NP)
    r = 0
    for pw in range(NP):
        for px in range(NP - pw):
            r = r + _conv64(xp[px].double(), wp[pw].double(), case)
    return _plus_bias(r, bias)


def split_bound(case):
    """|emul64 - ref64| <= split_bound mag (the split model of the module docstring)."""
    return {0: 0.0, 2: 3 * 2.0 ** -16, 3: 2.0 ** -23}[case.planes if case.kind != VALU else 0]


def cap_of(case):
    """The fp32 additions on an element's path."""
    NP = case.planes
    if case.kind == FWD:
        return 5 * (NP * (NP + 1) // 2) * 16 + 2
    if case.kind == TR:
        return NP * 5 * 32 + (NP - 1) + 5
    return 25 * case.Cin + 1


def k_of(case, affine=False):
    return min(K_ACC[case.kind], cap_of(case)) + (2 if affine else 0)


def pixel_roundings(case):
    if case.kind == VALU:
        return 1
    return {3: 5, 2: 2}[case.planes]


def pixel_bound(case):
    """|y - w v| <= pixel_bound |w v| inside the footprint of the single pixel."""
    return pixel_roundings(case) * (1 + 2.0 ** -6) * U + split_bound(case)


# ------------------------------------------------------------------------------------------------ mutations
def _drops(NP):
    return tuple(f"drop_w{pw}x{px}" for pw in range(NP) for px in range(NP - pw))


MUTATIONS = {
    FWD: _drops(3) + (
        "zero_tap_let_through",          # "kw = 5" of channel 1 multiplied in: the next filter row's first tap, the pixel past the window
        "channel_not_zeroed",            # channels >= Cin read as channel Cin - 1 (the clamped addresses)
        "d1_forgotten",                  # the second accumulator is not added
        "band_last_row_off_by_one",      # a band's last output row takes its last input row one further down
        "wid_decode_swapped",            # strip = wid % groups, group = wid / groups
        "short_band_row_stored",         # the rows a short last band does not have are stored: into the next channel's plane
    ),
    TR: _drops(3) + (
        "bias_per_kw",
        "antidiagonal_off_by_one",
        "row_buffer_parity",             # row oh reads row oh - 1's buffer
        "halo_not_zero",                 # the row buffer's halo columns hold their neighbour's values
        "pad_before_act",                # padding holds act(shift) instead of 0
    ),
    VALU: (
        "tail_reads_previous_chunk",     # the channels past Cin of the last chunk: the previous chunk's patch, channel Cin - 1's taps
    ),
}


def _dropped(mut):
    return (int(mut[6]), int(mut[8])) if mut and mut.startswith("drop_w") else None


def restate32(case, x, w, bias, affine=None, mut=None):
    """The kernel's fp32 evaluation (module docstring) as a (B, Cout, OH, OW) fp32 tensor; `mut`: one of MUTATIONS[kind]."""
    assert mut is None or mut in MUTATIONS[case.kind], mut
    return {FWD: _restate_fwd, TR: _restate_tr, VALU: _restate_valu}[case.kind](case, x, w, bias, affine, mut)


def _restate_fwd(case, x, w, bias, affine, mut):
    assert affine is None
    f = torch.float32
    S, NP, (B, Cin, H, W, Cout) = case.stride, case.planes, case.shape
    OH, OW = case.out_hw
    RB, bands = case.rows_per_band, case.bands
    OHx = bands * RB                                            # with the rows a short last band does not have
    x3, w3 = torch.zeros(B, 3, H, W), torch.zeros(Cout, 3, 5, 5)
    x3[:, :Cin], w3[:, :Cin] = x, w
    nch = Cin
    if mut == "channel_not_zeroed":
        x3[:, Cin:], w3[:, Cin:] = x[:, Cin - 1:Cin], w[:, Cin - 1:Cin]
        nch = 3
    # row S oh + kh, column S ow + kw of the padded image is input pixel (S oh + kh - 2, S ow + kw - 2); rows past the
    # image are zero, as the staging leaves them
    xp = planes3(F.pad(x3, (2, 4, 2, S * OHx + 4 - H)), NP)
    wp = planes3(w3, NP)
    last_rows = torch.zeros(OHx, dtype=torch.bool)
    for band in range(bands):
        last_rows[min(RB, OH - band * RB) - 1 + band * RB] = True

    def patch(px, c, kh, kw):
        v = xp[px][:, c, kh:kh + S * (OHx - 1) + 1:S, kw:kw + S * (OW - 1) + 1:S]
        if mut == "band_last_row_off_by_one" and kh == 4:
            v = torch.where(last_rows[None, :, None], xp[px][:, c, kh + 1:kh + 1 + S * (OHx - 1) + 1:S, kw:kw + S * (OW - 1) + 1:S], v)
        return v[:, None]

    index16 = [(0, kw) for kw in range(5)] + [(1, kw) for kw in range(3)] + [(2, kw) for kw in range(5)] + [(1, 3), (1, 4), (1, 5)]
    d = [torch.zeros(B, Cout, OHx, OW, dtype=f) for _ in range(2)]
    n = 0
    for total in range(NP - 1, -1, -1):
        for pw in range(total, -1, -1):
            px = total - pw
            for kh in range(5):
                acc = d[n & 1]
                n += 1
                if (pw, px) == _dropped(mut):
                    continue
                for (c, kw) in index16:
                    if kw == 5:
                        if mut == "zero_tap_let_through" and Cin > 1:
                            acc.addcmul_(wp[pw][None, :, 1, (kh + 1) % 5, 0, None, None], patch(px, 1, kh, 5))
                    elif c < nch:                              # (a zero term leaves the accumulator as it is)
                        acc.addcmul_(wp[pw][None, :, c, kh, kw, None, None], patch(px, c, kh, kw))
    y = d[0] if mut == "d1_forgotten" else d[0] + d[1]
    if bias is not None:
        y = y + bias.float()[None, :, None, None]
    out = y[:, :, :OH].contiguous()
    if mut == "short_band_row_stored":
        rows = out.view(B * Cout * OH, OW)
        for b in range(B):
            for co in range(Cout):
                for oh in range(OH, OHx):
                    r = (b * Cout + co) * OH + oh
                    if r < rows.shape[0]:
                        rows[r] = y[b, co, oh]
    if mut == "wid_decode_swapped":
        good, out = out, torch.full_like(out, float("nan"))
        for wid in range(case.waves):
            strip, cg = wid % case.groups, wid // case.groups
            if strip < case.strips and cg < case.groups:
                out[:, cg * 32:cg * 32 + 32, :, strip * 32:strip * 32 + 32] = good[:, cg * 32:cg * 32 + 32, :, strip * 32:strip * 32 + 32]
    return out


TR_ORDER = {3: ((2, 0), (1, 0), (1, 1), (0, 0), (0, 2), (0, 1)),      # (input plane, filter plane) of a kh, as written
            2: ((1, 0), (0, 0), (0, 1))}


def _restate_tr(case, x, w, bias, affine, mut):
    f = torch.float32
    NP, (B, Cin, H, W, Cout) = case.planes, case.shape
    xa = activated(x, affine)
    if mut == "pad_before_act" and affine is not None:          # the halo goes through the affine and the activation too
        halo = activated(torch.zeros(1, Cin, 1, 1), affine).expand(B, Cin, H + 4, W + 4).clone()
        halo[:, :, 2:2 + H, 2:2 + W] = xa
        xa = halo
    else:
        xa = F.pad(xa, (2, 2, 2, 2))
    xp, wp = planes3(xa, NP), planes3(w, NP)
    # D[b][co][kw][oh][column iw + 2 of the row buffer]
    dc = [torch.zeros(B, Cout, 5, H, W + 4, dtype=f) for _ in range(NP)]
    for kh in range(5):                                          # input row oh + 2 - kh: row oh + 4 - kh of the padded image
        for (px, pw) in TR_ORDER[NP]:
            if (pw, px) == _dropped(mut):
                continue
            acc = dc[px + pw]
            for ci in range(Cin):
                acc.addcmul_(wp[pw][ci, :, kh, :][None, :, :, None, None], xp[px][:, ci, 4 - kh:4 - kh + H, :][:, None, None])
    D = dc[NP - 1]
    for c in range(NP - 2, -1, -1):
        D = D + dc[c]
    if mut == "halo_not_zero":
        D[..., 0], D[..., 1], D[..., W + 2], D[..., W + 3] = D[..., 2].clone(), D[..., 2].clone(), D[..., W + 1].clone(), D[..., W + 1].clone()
    if mut == "antidiagonal_off_by_one":
        D = F.pad(D[..., 1:], (0, 1))
    b32 = torch.zeros(Cout) if bias is None else bias.float()
    y = b32[None, :, None, None].expand(B, Cout, H, W)
    for kw in range(5):                                          # iw = ow + 2 - kw: column ow + 4 - kw
        y = y + D[:, :, kw, :, 4 - kw:4 - kw + W]
        if mut == "bias_per_kw" and kw:
            y = y + b32[None, :, None, None]
    if mut == "row_buffer_parity":
        y = torch.cat([torch.full_like(y[:, :, :1], float("nan")), y[:, :, :-1]], dim=2)
        y[:, :, ::16] = float("nan")                             # a band's first row: a buffer nobody wrote
    return y.contiguous()


def _restate_valu(case, x, w, bias, affine, mut):
    assert affine is None
    B, Cin, H, W, Cout = case.shape
    xp, wd = F.pad(x, (2, 2, 2, 2)).double(), w.double()
    acc = torch.zeros(B, Cout, H, W)

    def fma(acc, cx, cw, kh, kw):                                # iw = ow + 2 - kw: column ow + 4 - kw of the padded image
        v = xp[:, cx, 4 - kh:4 - kh + H, 4 - kw:4 - kw + W][:, None] * wd[cw, :, kh, kw][None, :, None, None]
        return (acc.double() + v).float()

    for c0 in range(0, Cin, 8):
        cmax = min(8, Cin - c0)
        for c in range(cmax if not (mut and c0) else 8):
            for kh in range(5):
                for kw in range(5):
                    acc = fma(acc, c0 + c, c0 + c, kh, kw) if c < cmax else fma(acc, c0 - 8 + c, Cin - 1, kh, kw)
    return acc if bias is None else acc + bias.float()[None, :, None, None]


# ------------------------------------------------------------------------------------------------ statistics
def slot_regions(case):
    """[(slot, image, row slice, column slice)] of the forward kernel's statistics slots."""
    assert case.kind == FWD
    RB = case.rows_per_band
    return [((b * case.bands + band) * case.strips + strip, b, slice(RB * band, RB * band + RB), slice(32 * strip, 32 * strip + 32))
            for b in range(case.B) for band in range(case.bands) for strip in range(case.strips)]


def slots_ok(case, stats, y):
    """stats: the device's (slots, Cout, 2) buffer; y: the device's output.  (ok, worst share of the bound): every slot
    finite and, per slot and channel, within 16 x 2^-24 of its sum of magnitudes, for y and for y^2."""
    s, yd = stats.detach().cpu().double(), y.detach().cpu().double()
    regions = slot_regions(case)
    if s.shape != (len(regions), case.Cout, 2) or not bool(torch.isfinite(s).all()):
        return False, float("nan")
    worst = 0.0
    for slot, b, rows, cols in regions:
        for j, v in enumerate((yd[b, :, rows, cols], yd[b, :, rows, cols] ** 2)):
            bound = (STATS_DEPTH * U * v.abs().sum(dim=(1, 2))).clamp_min(torch.finfo(torch.float64).tiny)
            worst = max(worst, float(((s[slot, :, j] - v.sum(dim=(1, 2))).abs() / bound).max()))
    return worst <= 1.0, worst
