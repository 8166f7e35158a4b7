"""References for the general fp16x3 forward convolution -- csrc/conv_general.hip (vg_conv_general_pack,
vg_conv_general_fwd: every convolution of the FID Inception network) -- with the seeded operands, the case tables and the
mutations the CPU and the GPU tests share.  A plain module: nothing here touches a GPU (routes are asked of the tuning
library's host-only query by tests/test_conv_general_refs_cpu.py).  The arithmetic pieces are tests/_gemm_refs.py's
(bound_exp, scales, planes, ratio, check, U, _spread).

  emul64     the fp64 sum of the three plane products the kernel forms (w_hi x_hi + w_hi x_lo + w_lo x_hi; lo lo dropped)
             as three fp64 convolutions of the fp16 planes, times the two exact inverse scales, plus bias: what the kernel
             would return with an exact accumulator FOR THE BOUNDS IT WAS HANDED.
  ref64      the plain fp64 convolution plus bias.
  mag        the same convolution of |x| and |w|, plus |bias|.
  ReLU       is applied to the reference as well (`relu=True`): it is 1-Lipschitz, so an element's bound stays that of
             the pre-activation value.
  restate32  the same plane products accumulated in fp32 in the kernel's order: reduction index
             k = (kh KW + kw) Cin + ci as the pack's table holds it, zero padded to a multiple of 32; stages of 32, two
             halves of 16 per stage; per half w_lo x_hi, then w_hi x_lo, then w_hi x_hi, each a sequential sum over its
             16 indices (the MFMA's own order is not known); then x x_unscale x w_unscale, + bias[cout], ReLU.  Written
             out here: _gemm_refs.restate32 on im2col matrices has the same product order only with the filter as its A
             operand, and then it unscales in the other order and adds its bias along the other axis.  The activations
             are gathered as the kernel gathers them -- per table entry, per output pixel, an in-image test and a select
             -- so that the MUTATIONS can be made where the kernel would make them.

The per-element check is _gemm_refs.check: every element finite and |got - emul64| <= k 2^-24 mag, no element excluded,
k = k_of(case) = min(K_ACC, 3 K + 1): 3 K accumulations (K = Cin KH KW) and the bias addition; the two unscalings are
exact.

K_ACC.  ACC_WORST is the worst |restate32 - emul64| / (2^-24 mag) over every case of this file (`all_cases`; the LOOSE
cases at their loose bounds too), as tests/test_conv_general_refs_cpu.py::test_k_acc_is_measured_from_the_restatement
measures it:

    pytest -s tests/test_conv_general_refs_cpu.py -k k_acc

K_ACC = ceil(4 ACC_WORST): the factor 4 is for the unknown summation order and rounding inside the MFMA.  Nothing here
is taken from a kernel run.
"""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from _gemm_refs import U, _spread, check, planes, ratio, scales      # noqa: F401  (re-exported to the tests)

KC = 32                              # CG_KC: reduction indices per stage
GUARD = -12345.5                     # what a buffer holds around the channels a launch writes

# measured by tests/test_conv_general_refs_cpu.py (see above); the test fails if the measurement leaves
# [0.8 ACC_WORST, ACC_WORST]
#   TILE_CASES (K = 45): 2.05 - 5.59;  HEURISTIC_CASES (K = 1 / 3): 1.50 - 2.71;  FILTER_CASES (K = 3 .. 225): 1.66 - 6.33
#   (the padded 5 x 5; 15 x 15: 3.6 - 4.4);  K_CASES 1 / 27 / 32 / 33 / 64 / 2048: 1.41 / 3.89 / 3.37 / 7.001 (the worst) /
#   4.57 / 4.57;  ONE_PIXEL: 1.10 - 3.98;  SLICE, IMPULSE and NONFINITE cases: 3.30 - 4.47;  bounds loose by 2^1 / 2^5: 4.75,
#   6.33;  x >= 0 (VARIANT_CASES): 1.42 - 4.35
ACC_WORST = 7.1
K_ACC = math.ceil(4 * ACC_WORST)


class Case(NamedTuple):
    """One launch.  ``force``: the (tm, tn) tile forced through the tuning knob (None: the heuristic).  ``route``: the
    (tm, tn, pad) of the conv_general_kernel<tm, tn, pad> the launch is claimed to take, as
    vg_debug_conv_general_tile reports it."""
    B: int
    Cin: int
    H: int
    W: int
    Cout: int
    KH: int
    KW: int
    sh: int = 1
    sw: int = 1
    ph: int = 0
    pw: int = 0
    force: Optional[Tuple[int, int]] = None
    route: Tuple[int, int, int] = ()

    @property
    def id(self):
        s = (f"{self.B}x{self.Cin}x{self.H}x{self.W}-{self.Cout}-k{self.KH}x{self.KW}-s{self.sh}x{self.sw}"
             f"-p{self.ph}x{self.pw}")
        return s if self.force is None else f"{s}-t{self.force[0]}x{self.force[1]}"

    @property
    def out_hw(self):
        return (self.H + 2 * self.ph - self.KH) // self.sh + 1, (self.W + 2 * self.pw - self.KW) // self.sw + 1

    @property
    def K(self):
        return self.Cin * self.KH * self.KW

    @property
    def npix(self):
        return self.B * self.out_hw[0] * self.out_hw[1]

    @property
    def pad(self):
        return int(bool(self.ph or self.pw))

    @property
    def geometry(self):
        """The launch without the tile: what operands and references depend on."""
        return self._replace(force=None, route=())


def tile_of(Cout, npix):
    """cg_tile restated: 128 output channels unless padding Cout to 128 wastes more than a fifth over padding it to 64;
    128 pixels unless that leaves fewer workgroups than the 256 CUs.  The claims of the tables below come from here;
    tests/test_conv_general_refs_cpu.py holds them against the library's own answer."""
    p64, p128 = -(-Cout // 64) * 64, -(-Cout // 128) * 128
    tm = 128 if 5 * p128 <= 6 * p64 else 64
    return tm, (128 if -(-Cout // tm) * -(-npix // 128) >= 256 else 64)


def _case(B, Cin, H, W, Cout, k, s=(1, 1), p=(0, 0), force=None):
    c = Case(B, Cin, H, W, Cout, *k, *s, *p, force=force)
    return c._replace(route=(*(force or tile_of(Cout, c.npix)), c.pad))


# ------------------------------------------------------------------------------------------------ case tables
TILES = tuple((tm, tn) for tm in (64, 128) for tn in (64, 128))
TILE_COUTS = (1, 33, 64, 65, 129)
# (B, OH, OW) with B OH OW = tn - 1, tn, tn + 1 (B = 3 divides neither 64, 65, 127 nor 128: the batch follows the count)
NPIX_SHAPES = {64: ((3, 3, 7), (4, 4, 4), (5, 1, 13)), 128: ((1, 1, 127), (2, 8, 8), (3, 1, 43))}


def _tile_cases():
    """Every (tm, tn) forced, with pad 1 and without, Cin 5, 3 x 3: Cout 1 / 33 / 64 / 65 / 129 on B 3 with 5 x 7 output
    pixels per image (105 pixels: the first pixel tile ends inside image 1 at tn 64, holds all three images at tn 128),
    then Cout 33 with tn - 1, tn and tn + 1 pixels."""
    out = []
    for t in TILES:
        for pad in (1, 0):
            g = 0 if pad else 2          # input rows / columns the unpadded filter needs beyond the output's
            out += [_case(3, 5, 5 + g, 7 + g, co, (3, 3), p=(pad, pad), force=t) for co in TILE_COUTS]
            out += [_case(b, 5, oh + g, ow + g, 33, (3, 3), p=(pad, pad), force=t) for (b, oh, ow) in NPIX_SHAPES[t[1]]]
    return tuple(out)


TILE_CASES = _tile_cases()
HEURISTIC_CASES = (                               # force None; the routes written out, both sides of each switch
    _case(2, 1, 120, 136, 8, (1, 1))._replace(route=(64, 64, 0)),       # 32640 pixels = 255 tiles of 128: one short of the CUs
    _case(2, 1, 128, 128, 8, (1, 1))._replace(route=(64, 128, 0)),      # 32768 pixels = 256 tiles
    _case(1, 3, 9, 9, 64, (1, 1))._replace(route=(64, 64, 0)),
    _case(1, 3, 9, 9, 65, (1, 1))._replace(route=(128, 64, 0)),
    _case(1, 3, 9, 9, 129, (1, 1))._replace(route=(64, 64, 0)),         # 192 padded channels against 256
    _case(1, 3, 9, 9, 193, (1, 1))._replace(route=(128, 64, 0)),
)


def _f(k, s, p, hw, cin=3):
    return _case(2, cin, *hw, 33, k, s, p)


FILTER_CASES = (                                  # filter, strides, pads, (H, W): even extents leave a stride-2 window short
    _f((1, 1), (1, 1), (0, 0), (7, 9)),
    _f((1, 1), (2, 2), (0, 0), (8, 10)),          # stops one row and one column short
    _f((1, 1), (1, 1), (15, 15), (5, 6)),         # a frame of bias-only pixels, 15 wide
    _f((3, 3), (1, 1), (1, 1), (9, 11)),
    _f((3, 3), (2, 2), (0, 0), (9, 11)),
    _f((3, 3), (2, 2), (0, 0), (8, 10)),          # stops short
    _f((3, 3), (2, 2), (1, 1), (9, 8)),
    _f((3, 3), (1, 2), (1, 1), (7, 10)),
    _f((3, 3), (2, 1), (0, 0), (10, 7)),
    _f((3, 3), (1, 1), (2, 2), (5, 7)),           # a pad wider than the filter needs
    _f((5, 5), (1, 1), (2, 2), (9, 11)),
    _f((5, 5), (2, 2), (0, 0), (10, 12)),
    _f((5, 5), (2, 1), (2, 2), (9, 7)),
    _f((1, 7), (1, 1), (0, 3), (7, 13)),
    _f((1, 7), (1, 2), (0, 3), (6, 13)),
    _f((1, 7), (2, 2), (0, 0), (6, 12)),
    _f((7, 1), (1, 1), (3, 0), (13, 7)),
    _f((7, 1), (2, 1), (3, 0), (13, 6)),
    _f((7, 1), (1, 2), (0, 0), (12, 6)),
    _f((1, 3), (1, 1), (0, 3), (6, 7)),           # wider than needed, one way
    _f((1, 3), (2, 1), (0, 0), (8, 9)),
    _f((3, 1), (1, 1), (3, 0), (7, 6)),
    _f((3, 1), (1, 2), (1, 1), (9, 8)),
    _f((2, 4), (1, 1), (0, 0), (8, 9)),
    _f((2, 4), (2, 2), (1, 1), (9, 10)),
    _f((4, 2), (1, 1), (2, 2), (7, 8)),
    _f((4, 2), (2, 1), (0, 0), (9, 8)),
    _f((4, 2), (1, 2), (0, 3), (8, 7)),
    _f((15, 15), (1, 1), (0, 0), (17, 16), cin=1),
    _f((15, 15), (2, 2), (2, 2), (15, 14), cin=1),
    _f((15, 15), (1, 2), (3, 0), (11, 17), cin=1),
)
# reduction lengths 1, 27, 32, 33 (one real index in the second stage), 64, 2048 (64 stages): 8 x 8 output pixels
K_CASES = (
    _case(1, 1, 8, 8, 33, (1, 1)),
    _case(1, 3, 10, 10, 33, (3, 3)),
    _case(1, 32, 8, 8, 33, (1, 1)),
    _case(1, 33, 8, 8, 33, (1, 1)),
    _case(1, 64, 8, 8, 33, (1, 1)),
    _case(1, 2048, 8, 8, 33, (1, 1)),
)
ONE_PIXEL = (
    _case(1, 3, 1, 1, 33, (3, 3), p=(1, 1)),      # one output pixel, eight of its nine taps in the padding
    _case(1, 3, 3, 3, 33, (3, 3)),                # one output pixel, unpadded
    _case(1, 3, 3, 9, 33, (3, 3)),                # one output row
    _case(2, 3, 9, 3, 33, (3, 3)),                # one output column
)
SLICE_BEFORE, SLICE_EXTRA = 5, 12                 # channels [5, 5 + Cout) of a (B, Cout + 12, OH, OW) buffer
SLICE_CASES = (
    _case(3, 5, 5, 7, 33, (3, 3), p=(1, 1)),      # 35 pixels per image: the first tile of 64 ends inside image 1
    _case(2, 3, 8, 8, 65, (1, 7), p=(0, 3)),      # 64 pixels per image: every tile inside one image
)
IMPULSE_CASES = (                                 # 42 output pixels per image: pixel 63 lies in image 1
    _case(3, 3, 6, 13, 33, (1, 7), (1, 2), (0, 3)),
    _case(3, 3, 13, 6, 33, (7, 1), (2, 1), (3, 0)),
    _case(3, 3, 7, 10, 33, (2, 4)),
)
# non-finite inputs: (a) padded 3 x 3, (b) unpadded with K = 27 (five table entries beyond K), (c) npix = tn + 1
NONFINITE_A = _case(3, 5, 5, 7, 33, (3, 3), p=(1, 1))
NONFINITE_B = _case(3, 3, 7, 9, 33, (3, 3))
NONFINITE_C = (_case(5, 5, 1, 13, 33, (3, 3), p=(1, 1), force=(64, 64)), _case(5, 5, 3, 15, 33, (3, 3), force=(64, 64)))
REPEAT_CASES = (TILE_CASES[-16 + 2], K_CASES[5], FILTER_CASES[-2])      # 128 x 128 padded, Cout 64; 64 stages; 15 x 15
LOOSE = (1, 5)                                    # bounds loose by 2^1 and 2^5 ...
LOOSE_CASES = (TILE_CASES[1], FILTER_CASES[10])   # ... on a forced padded tile and the padded 5 x 5
GROUPS = {"tile": TILE_CASES, "heuristic": HEURISTIC_CASES, "filter": FILTER_CASES, "k": K_CASES, "one_pixel": ONE_PIXEL,
          "slice": SLICE_CASES, "impulse": IMPULSE_CASES, "nonfinite": (NONFINITE_A, NONFINITE_B) + NONFINITE_C}
MAIN_GROUPS = ("tile", "heuristic", "filter", "k", "one_pixel")      # test_case of the GPU file
# one case per group that also runs with ReLU, without bias, and with the non-negative input
VARIANT_CASES = {"tile": TILE_CASES[1], "heuristic": HEURISTIC_CASES[3], "filter": FILTER_CASES[2], "k": K_CASES[3],
                 "one_pixel": ONE_PIXEL[0]}


def all_cases():
    seen, out = set(), []
    for cs in GROUPS.values():
        for c in cs:
            if c.geometry not in seen:            # the forced tiles of one shape share the arithmetic
                seen.add(c.geometry)
                out.append(c)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ operands
def bound_of(t):
    return float(t.abs().max())


@functools.lru_cache(maxsize=None)
def _operands(geometry, seed, nonneg):
    c = geometry
    key = 0
    for v in c[:11]:
        key = (key * 1000003 + int(v)) % 2147483629
    g = torch.Generator().manual_seed(1000003 * seed + key)
    x = torch.randn(c.B, c.Cin, c.H, c.W, generator=g)
    sp = _spread(c.Cout, 4, g)
    w = torch.randn(c.Cout, c.Cin, c.KH, c.KW, generator=g) * 0.05 * sp[:, None, None, None]
    bias = torch.randn(c.Cout, generator=g) * 0.1 * sp
    return (x.abs() if nonneg else x), w, bias


def operands(case, seed=0, nonneg=False):
    """x (B, Cin, H, W), w (Cout, Cin, KH, KW), bias (Cout): full-mantissa normals.  The filter's output channels (and
    the bias with them) spread over four decades in a seeded order: a store to the wrong channel row cannot hide under
    a neighbour's magnitude.  ``nonneg``: |x|, what the network (a ReLU in front of every layer but the first) feeds the
    kernel.  Shared and never written to: clone before changing one."""
    return _operands(case.geometry, seed, nonneg)


# ------------------------------------------------------------------------------------------------ fp64 references
def _conv64(case, x, w):
    return F.conv2d(x, w, None, stride=(case.sh, case.sw), padding=(case.ph, case.pw))


def _finish(r, bias, relu, absolute=False):
    if bias is not None:
        r = r + (bias.double().abs() if absolute else bias.double())[None, :, None, None]
    return torch.relu(r) if relu else r


def emul64(case, x, w, bias, x_bound, w_bound, relu=False):
    xh, xl = (p.double() for p in planes(x, x_bound))
    wh, wl = (p.double() for p in planes(w, w_bound))
    r = _conv64(case, xh, wh) + _conv64(case, xl, wh) + _conv64(case, xh, wl)
    return _finish(r * scales(x_bound)[1] * scales(w_bound)[1], bias, relu)


def ref64(case, x, w, bias, relu=False):
    return _finish(_conv64(case, x.double(), w.double()), bias, relu)


def mag(case, x, w, bias):
    return _finish(_conv64(case, x.double().abs(), w.double().abs()), bias, False, absolute=True)


def k_of(case):
    return min(K_ACC, 3 * case.K + 1)


# ------------------------------------------------------------------------------------------------ the kernel's order
MUTATIONS = (
    "drop_lo_hi",              # the w_lo x_hi product is dropped
    "drop_hi_lo",              # the w_hi x_lo product is dropped
    "swap_kh_kw",              # the table's two fields exchanged: tap (kw, kh) of the image meets filter tap (kh, kw)
    "swap_stride",             # the window steps by (stride_w, stride_h)
    "swap_pad",                # the window starts at (-pad_w, -pad_h)
    "tail_not_zero",           # the table's entries beyond K (tap (0, 0) of channel 0, unpadded kernel) meet a non-zero filter value
    "pad_reads_clamped",       # an out-of-image tap contributes the clamped read x[b][0][0][0] instead of 0
    "image_stride_dense",      # a pixel tile that straddles two images steps to the next one by Cout OH OW, not y_image_stride
    "bias_per_pixel",          # bias indexed by the column of the tile
    "relu_before_bias",
)


def table(case):
    """The pack's table: (ci, kh, kw) of reduction index k < K."""
    return [(k % case.Cin, (k // case.Cin) // case.KW, (k // case.Cin) % case.KW) for k in range(case.K)]


def _gather(case, xp, ci, kh, kw, mut):
    """Plane xp (B, Cin, H, W) at tap (kh, kw) of channel ci for every output pixel, (B, OH, OW): the in-image test and
    the select of load_stage."""
    OH, OW = case.out_hw
    sh, sw, ph, pw = case.sh, case.sw, case.ph, case.pw
    if mut == "swap_kh_kw":
        kh, kw = kw, kh
    if mut == "swap_stride":
        sh, sw = sw, sh
    if mut == "swap_pad":
        ph, pw = pw, ph
    ih = torch.arange(OH) * sh - ph + kh
    iw = torch.arange(OW) * sw - pw + kw
    ok = ((ih >= 0) & (ih < case.H))[:, None] & ((iw >= 0) & (iw < case.W))[None, :]
    v = xp[:, ci][:, ih.clamp(0, case.H - 1)][:, :, iw.clamp(0, case.W - 1)]
    out = xp[:, 0, 0, 0][:, None, None].expand_as(v) if mut == "pad_reads_clamped" else torch.zeros_like(v)
    return torch.where(ok[None], v, out)


def restate32(case, x, w, bias, x_bound, w_bound, relu=False, mut=None, tn=None):
    """The kernel's fp32 evaluation (see the module docstring) as a (B, Cout, OH, OW) fp32 tensor; `mut`: one of
    MUTATIONS (image_stride_dense is `stored`'s).  ``tn``: the pixel tile, for bias_per_pixel (the case's route by
    default)."""
    assert mut is None or (mut in MUTATIONS and mut != "image_stride_dense"), mut
    f = torch.float32
    B, Cout, K = case.B, case.Cout, case.K
    OH, OW = case.out_hw
    xh, xl = (p.float() for p in planes(x, x_bound))
    wh, wl = (p.float().permute(0, 2, 3, 1).reshape(Cout, K) for p in planes(w, w_bound))      # [cout][k]
    tab = table(case)
    products = [(wl, xh), (wh, xl), (wh, xh)]
    if mut == "drop_lo_hi":
        products = products[1:]
    if mut == "drop_hi_lo":
        products = [products[0], products[2]]
    acc = torch.zeros(B, Cout, OH, OW, dtype=f)
    kpad = -(-K // KC) * KC
    for k0 in range(0, kpad, 16):
        for pw_, px in products:
            for k in range(k0, min(k0 + 16, kpad)):
                if k < K:
                    acc.addcmul_(pw_[None, :, k, None, None], _gather(case, px, *tab[k], mut)[:, None])
                elif mut == "tail_not_zero" and not case.pad:
                    # the unpadded kernel's read for these entries, against the pack's clamped read of the filter
                    acc.addcmul_(pw_[None, :, K - 1, None, None], _gather(case, px, 0, 0, 0, None)[:, None])
                # else: a zero filter value (and, padded, a zero activation): the sum does not move
    y = acc * torch.tensor(scales(x_bound)[1], dtype=f) * torch.tensor(scales(w_bound)[1], dtype=f)
    if mut == "relu_before_bias" and relu:
        y = torch.relu(y)
    if bias is not None:
        if mut == "bias_per_pixel":
            col = torch.arange(B * OH * OW) % (tn or case.route[1])
            y = y + bias.float()[col % Cout].view(B, 1, OH, OW)
        else:
            y = y + bias.float()[None, :, None, None]
    if relu and mut != "relu_before_bias":
        y = torch.relu(y)
    return y


def stored(case, y, before=SLICE_BEFORE, extra=SLICE_EXTRA, mut=None, tn=None):
    """y (B, Cout, OH, OW) as the epilogue stores it into channels [before, before + Cout) of a GUARD-filled
    (B, Cout + extra, OH, OW) buffer through y_image_stride = (Cout + extra) OH OW: pixel n of the batch goes to
    image n / (OH OW).  `mut` image_stride_dense: inside a pixel tile, the images after the tile's first one are
    reached with the dense stride Cout OH OW."""
    assert mut in (None, "image_stride_dense")
    B, Cout = case.B, case.Cout
    ohw = case.out_hw[0] * case.out_hw[1]
    total, tn = Cout + extra, tn or case.route[1]
    buf = torch.full((B * total * ohw,), GUARD, dtype=torch.float32)
    n = torch.arange(B * ohw)
    nb, nr = n // ohw, n % ohw
    off = nb * (total * ohw)
    if mut:
        first = (n // tn * tn) // ohw             # the image of the tile's first pixel
        off = first * (total * ohw) + (nb - first) * (Cout * ohw)
    addr = (before * ohw + off + nr)[None, :] + (torch.arange(Cout) * ohw)[:, None]      # [cout][pixel]
    buf[addr.reshape(-1)] = y.permute(1, 0, 2, 3).reshape(-1)
    return buf.view(B, total, *case.out_hw)
