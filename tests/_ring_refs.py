"""References for the fp16x3 5x5 convolution kernels -- csrc/conv_ring.hip (every stride-2 forward convolution, the
stride-2 transposed ones with more than 64 output channels) and, second table, csrc/conv_bf16split.hip (stride 1, the
thin transposed layers) -- with the seeded operands, the case tables and the mutations the CPU and the GPU tests share.
A plain module: nothing here touches a GPU (routes and split counts are asked of the library's host-only queries by
tests/test_conv_ring_cpu.py).  The arithmetic pieces are tests/_gemm_refs.py's (bound_exp, scales, planes, slab_sum32,
ratio, check, U).

  activated  the input as the kernel reads it: act(fma(x, scale[c], shift[c])) in fp32, slope 1 / 0 / 0.2 (the fma
             through fp64: exact product, one rounding of the sum, one to fp32); zero padding pads THIS tensor.
  emul64     the fp64 sum of the three plane products the kernel forms (w_hi x_hi + w_hi x_lo + w_lo x_hi; lo lo
             dropped) as three fp64 convolutions of the fp16 planes, times the two exact inverse scales, plus bias: what
             the kernel would return with an exact accumulator FOR THE BOUNDS IT WAS HANDED.
  ref64      the plain fp64 convolution of the fp64-activated input.
  mag        the same convolution of |activated| and |w|, plus |bias|.
  restate32  the same plane products accumulated in fp32 in the kernel's order (ring_body, bf16split_body): chunks of 16
             channels from c_begin to c_end; per chunk the pack's steps of 16 reduction indices (`steps_of`: the ring's
             forward form 8 channels x 2 taps with the step-12 pairing; every other form 16 channels x 1 tap, taps row
             by row, the transposed classes one after the other); within a step w_lo x_hi, then w_hi x_lo, then
             w_hi x_hi, each a sequential sum over its 16 indices (the MFMA's own order is not known); then
             x x_unscale x w_unscale; bias with split 0 only; slabs summed by slab_sum32.  It also takes MUTATIONS.

The per-element check of both files is _gemm_refs.check: every element finite and |got - emul64| <= k 2^-24 mag, no
element excluded, k = k_of(case): min(K_ACC, 3 K + ksplit), K the element's reduction length (25 Cin forward,
taps of its parity class x Cin transposed), + 2 with an affine on load (one fp32 ulp of difference in the activated
input -- the device's fma against the double rounding above -- moves an element by at most 2 x 2^-24 mag).

K_ACC.  ACC_WORST is the worst |restate32 - emul64| / (2^-24 mag) over every case of this file (`all_cases`), as
tests/test_conv_ring_cpu.py::test_k_acc_is_measured_from_the_restatement measures it:

    pytest -s tests/test_conv_ring_cpu.py -k k_acc

K_ACC = ceil(4 ACC_WORST): the factor 4 is for the unknown summation order and rounding inside the MFMA.  Nothing here
is taken from a kernel run.

Statistics.  A slot is the fp32 sum of at most 64 values of acc + bias (FP x 32 pixels of one wavefront row); any order
of n additions errs by at most (n - 1) 2^-24 sum |v|.  Per channel, with the slot sums added in fp64 and against fp64
sums of the device's own output: |sum_slots stats[:, c, 0] - sum y[:, c]| <= 64 x 2^-24 sum |y[:, c]|, the same with
y^2 for stats[:, c, 1] (`stats_ok`).
"""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from _gemm_refs import U, _spread, check, planes, ratio, scales, slab_sum32      # noqa: F401  (re-exported to the tests)

FWD, TR = 0, 1                       # CONV_FWD / CONV_TR of conv_tile.hpp: the `mode` of vg_debug_ring_route
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
SLOPE = {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: 0.2}
STATS_N = 64                         # values per statistics slot, at most

# measured by tests/test_conv_ring_cpu.py (see above); the test fails if the measurement leaves [0.8 ACC_WORST, ACC_WORST]
#   ring forward, unsplit (K = 400): 5.8 - 9.0 (the one-pixel case 0.2);  transposed, unsplit (K = 64 .. 144 per class): 1.4 - 7.8;
#   K splits 2 / 4 / 8: 3.3 - 4.3 / 2.0 - 2.3 / 1.5;  the paired cases (most elements): 9.2 - 10.16 (128 x 16 x 16 x 16 -> 72: the
#   worst);  conv_bf16split.hip's table: 4.9 - 8.7
ACC_WORST = 10.2
K_ACC = math.ceil(4 * ACC_WORST)


class Case(NamedTuple):
    """One launch.  ``force``: the tile variant forced through the tuning knob (None: the heuristic).  ``route``: what the
    launch is claimed to take -- ring: (variant, ksplit, NB, TH, TW, paired) as vg_debug_ring_route reports it;
    conv_bf16split.hip: (ksplit,)."""
    mode: int
    B: int
    Cin: int
    H: int
    W: int
    Cout: int
    force: Optional[int] = None
    route: Tuple[int, ...] = ()
    stride: int = 2
    ring: bool = True

    @property
    def id(self):
        s = f"{'tr' if self.mode else 'fwd'}{self.stride}-{self.B}x{self.Cin}x{self.H}x{self.W}-{self.Cout}"
        return s if self.force is None else f"{s}-v{self.force}"

    @property
    def ksplit(self):
        return self.route[1] if self.ring else self.route[0]

    @property
    def out_hw(self):
        S = self.stride
        return (S * self.H, S * self.W) if self.mode == TR else ((self.H - 1) // S + 1, (self.W - 1) // S + 1)


def _ring(mode, shape, route, force=None):
    return Case(mode, *shape, force=force, route=route)


# ------------------------------------------------------------------------------------------------ ring cases
# route = (variant, ksplit, NB, TH, TW, paired)
RING_FWD = (
    _ring(FWD, (1, 16, 2, 2, 1), (2, 1, 2, 8, 8, 0)),                 # one pixel
    _ring(FWD, (3, 16, 9, 13, 33), (2, 1, 2, 8, 8, 0)),               # two-image 8 x 8 tile, odd batch, overhang both ways
    _ring(FWD, (2, 16, 17, 33, 129), (0, 1, 1, 8, 16, 0)),            # variant 0, 8 x 16 tile, one column and one row into the second
    _ring(FWD, (2, 16, 8, 8, 257), (0, 1, 2, 8, 8, 0)),               # two cout tiles
    _ring(FWD, (256, 16, 32, 32, 8), (3, 1, 1, 16, 16, 0)),           # variant 3 by the heuristic
) + tuple(_ring(FWD, (2, 16, 32, 32, 72), (v, 1, 1, 16 if v == 3 else 8, 16, 0), force=v) for v in range(4)) \
  + tuple(_ring(FWD, (2, 16, 16, 16, 72), (1 if v == 3 else v, 1, 2, 8, 8, 0), force=v) for v in range(4))
RING_FWD_SPLIT = (                                                    # 16 x 16 inputs
    _ring(FWD, (2, 64, 16, 16, 72), (2, 2, 2, 8, 8, 0)),
    _ring(FWD, (2, 80, 16, 16, 72), (2, 2, 2, 8, 8, 0)),              # parts 3 + 2
    _ring(FWD, (1, 128, 16, 16, 72), (2, 4, 2, 8, 8, 0)),
    _ring(FWD, (1, 176, 16, 16, 72), (2, 4, 2, 8, 8, 0)),             # parts 3, 3, 3, 2
    _ring(FWD, (1, 256, 16, 16, 136), (0, 8, 2, 8, 8, 0)),            # variant 0
)
RING_TR = (
    _ring(TR, (1, 16, 1, 1, 65), (2, 1, 2, 8, 8, 0)),                 # one pixel
    _ring(TR, (3, 16, 5, 7, 72), (2, 1, 2, 8, 8, 0)),                 # small ragged image
    _ring(TR, (3, 16, 9, 17, 72), (2, 1, 1, 8, 16, 0)),               # overhang on the 8 x 16 tile
    _ring(TR, (2, 16, 8, 8, 129), (0, 1, 2, 8, 8, 0)),                # 256-cout tile on 8-wide images: fp16 planes only
    _ring(TR, (2, 16, 8, 8, 257), (0, 1, 2, 8, 8, 0)),                # two cout tiles
    _ring(TR, (2, 16, 16, 16, 72), (3, 1, 1, 16, 16, 0)),             # variant 3
    _ring(TR, (2, 16, 24, 24, 72), (1, 1, 1, 8, 16, 0)),              # falls to variant 1
    _ring(TR, (2, 48, 8, 8, 72), (2, 1, 2, 8, 8, 0)),                 # three chunks
)
RING_TR_SPLIT = (                                                     # 8 x 8 inputs
    _ring(TR, (2, 64, 8, 8, 72), (2, 2, 2, 8, 8, 0)),
    _ring(TR, (2, 128, 8, 8, 72), (2, 4, 2, 8, 8, 0)),
    _ring(TR, (1, 256, 8, 8, 72), (2, 8, 2, 8, 8, 0)),
)
RING_PAIRED = (
    _ring(TR, (256, 16, 8, 8, 72), (2, 1, 2, 8, 8, 1)),
    _ring(TR, (256, 48, 8, 8, 72), (2, 1, 2, 8, 8, 1)),               # three chunks
    _ring(TR, (128, 16, 16, 16, 72), (3, 1, 1, 16, 16, 1)),           # variant 3
    _ring(TR, (64, 16, 16, 16, 72), (2, 1, 1, 8, 16, 1), force=2),
    _ring(TR, (64, 16, 16, 16, 72), (1, 1, 1, 8, 16, 1), force=1),
    _ring(TR, (254, 16, 8, 8, 72), (2, 1, 2, 8, 8, 0)),               # unpaired, one tile short
)
RING_CASES = RING_FWD + RING_FWD_SPLIT + RING_TR + RING_TR_SPLIT + RING_PAIRED
# fusion (affine on load, statistics): one unsplit forward case, one unpaired and one paired transposed case
FUSION_CASES = (RING_FWD[1], RING_TR[2], RING_PAIRED[0])
# one pixel: forward and transposed at each tile geometry (2 x 8 x 8, 8 x 16, 16 x 16)
PIXEL_CASES = (RING_FWD[1], RING_FWD[2], RING_FWD[5 + 3], RING_TR[1], RING_TR[2], RING_TR[5])
REPEAT_CASES = (RING_FWD_SPLIT[3], RING_TR_SPLIT[1], RING_PAIRED[1])

# ------------------------------------------------------------------------------------------------ conv_bf16split.hip cases
# route = (ksplit,).  Variants: 0 128 x 128, 1 64 x 128, 2 64 x 64, 3 32 x 128, 4 32 x 256 (transposed), 5 128 x 128 along cout;
# the pixel-tile geometry follows the width (>= 32, >= 16, below).
X_SIZES = ((8, 8), (16, 16), (32, 32), (13, 9))                       # (H, W): widths 8, 16, 32 and a ragged one
X_COUTS = (1, 33, 130)
X_FWD = tuple(Case(FWD, 3, 16, h, w, co, force=v, route=(1,), stride=1, ring=False)
              for v in (0, 1, 2, 3, 5) for (h, w) in X_SIZES for co in X_COUTS)
X_FWD_SPLIT = (                                                       # fwd_ksplit: Cout > 64, 8 x 8
    Case(FWD, 2, 128, 8, 8, 72, route=(4,), stride=1, ring=False),
    Case(FWD, 2, 176, 8, 8, 72, route=(4,), stride=1, ring=False),      # parts 3, 3, 3, 2
    Case(FWD, 2, 256, 8, 8, 130, route=(8,), stride=1, ring=False),
)
X_TR = tuple(Case(TR, 3, 16, h, w, co, force=v, route=(1,), stride=s, ring=False)
             for v in range(6) for s in (1, 2) for (h, w, co) in ((8, 8, 33), (13, 9, 1), (9, 33, 64))) \
    + (Case(TR, 3, 32, 16, 16, 130, force=0, route=(1,), stride=1, ring=False),)      # stride 1 takes any Cout; two chunks
X_CASES = X_FWD + X_FWD_SPLIT + X_TR


def all_cases():
    return RING_CASES + X_CASES


# ------------------------------------------------------------------------------------------------ operands
def bound_of(t):
    return float(t.abs().max())


@functools.lru_cache(maxsize=None)
def operands(case, seed=0):
    """x (B, Cin, H, W), w ([Cout, Cin, 5, 5] forward, [Cin, Cout, 5, 5] transposed), bias (Cout): full-mantissa
    normals.  The filter's output channels (and the bias with them) spread over four decades in a seeded order: a store
    to the wrong channel row cannot hide under a neighbour's magnitude."""
    g = torch.Generator().manual_seed(1000003 * seed + hash(case[:6] + (case.stride,)) % 999983)
    x = torch.randn(case.B, case.Cin, case.H, case.W, generator=g)
    sp = _spread(case.Cout, 4, g)
    w = torch.randn(case.Cout, case.Cin, 5, 5, generator=g) * 0.05 * sp[:, None, None, None]
    bias = torch.randn(case.Cout, generator=g) * 0.1 * sp
    if case.mode == TR:
        w = w.transpose(0, 1).contiguous()
    return x, w, bias


def affine_of(case, act, seed=0):
    """(scale, shift, act): per input channel, scales around 1 and shifts of both signs, large enough that act(shift) is
    far from 0 -- padding done before the activation would show."""
    g = torch.Generator().manual_seed(77 + 13 * seed + case.Cin + act)
    scale = 0.5 + torch.rand(case.Cin, generator=g)
    shift = torch.randn(case.Cin, generator=g)
    shift = shift + 0.25 * shift.sign()
    shift[0], shift[1] = abs(shift[0]), -abs(shift[1])
    return scale, shift, act


def _act(v, slope):
    return v * torch.where(v > 0, torch.ones((), dtype=v.dtype), torch.tensor(slope, dtype=v.dtype))


def activated(x, affine, dtype=torch.float32):
    """The input as the kernel reads it (dtype fp32), or the fp64-activated input of ref64."""
    if affine is None:
        return x.to(dtype)
    scale, shift, act = affine
    v = x.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    if dtype == torch.float32:
        return _act(v.float(), float(torch.tensor(SLOPE[act], dtype=torch.float32)))
    return _act(v, float(torch.tensor(SLOPE[act], dtype=torch.float32)))


# ------------------------------------------------------------------------------------------------ fp64 references
def _conv64(x, w, transposed, stride):
    if transposed:
        return F.conv_transpose2d(x, w, None, stride=stride, padding=2, output_padding=stride - 1)
    return F.conv2d(x, w, None, stride=stride, padding=2)


def _plus_bias(r, bias, absolute=False):
    if bias is None:
        return r
    b = bias.double().abs() if absolute else bias.double()
    return r + b[None, :, None, None]


def emul64(x, w, bias, x_bound, w_bound, transposed, affine=None, stride=2):
    xh, xl = (p.double() for p in planes(activated(x, affine), x_bound))
    wh, wl = (p.double() for p in planes(w, w_bound))
    r = _conv64(xh, wh, transposed, stride) + _conv64(xl, wh, transposed, stride) + _conv64(xh, wl, transposed, stride)
    return _plus_bias(r * scales(x_bound)[1] * scales(w_bound)[1], bias)


def ref64(x, w, bias, transposed, affine=None, stride=2):
    return _plus_bias(_conv64(activated(x, affine, torch.float64), w.double(), transposed, stride), bias)


def mag(x, w, bias, transposed, affine=None, stride=2):
    return _plus_bias(_conv64(activated(x, affine).double().abs(), w.double().abs(), transposed, stride), bias, absolute=True)


# ------------------------------------------------------------------------------------------------ the kernels' order
def class_taps(S, r):
    return (5 - r + S - 1) // S


def classes_of(mode, S):
    """Output-parity classes (R, SS), in the kernels' order; the forward form is one class."""
    return [(0, 0)] if mode == FWD else [(r, s) for r in range(S) for s in range(S)]


def steps_of(case, R=0, SS=0):
    """The K steps of one 16-channel chunk: a list of steps, each 16 (channel within the chunk, kh, kw) in k order
    (k-block 0, then 1).  The ring's forward form: 8 channels x 2 consecutive taps, step 12 pairs tap 24 of both halves
    (pack_bf16split_body); every other form: the taps of the class row by row, 16 channels each."""
    if case.ring and case.mode == FWD:
        out = []
        for s in range(25):
            st = []
            for kb in range(2):
                half = 0 if s < 12 else (kb if s == 12 else 1)
                tap = 2 * s + kb if s < 12 else (24 if s == 12 else 2 * (s - 13) + kb)
                st += [(half * 8 + j, tap // 5, tap % 5) for j in range(8)]
            out.append(st)
        return out
    if case.mode == FWD:
        return [[(c, kh, kw) for c in range(16)] for kh in range(5) for kw in range(5)]
    S = case.stride
    return [[(c, R + S * a, SS + S * b) for c in range(16)] for a in range(class_taps(S, R)) for b in range(class_taps(S, SS))]


def reduction_length(case, R=0, SS=0):
    if case.mode == FWD:
        return 25 * case.Cin
    return class_taps(case.stride, R) * class_taps(case.stride, SS) * case.Cin


def k_of(case, affine=False):
    """The factor k of the check, as a tensor broadcastable to the output (the transposed classes differ in K)."""
    H, W = case.out_hw
    k = torch.empty(1, 1, H, W, dtype=torch.float64)
    S = case.stride if case.mode == TR else 1
    for (R, SS) in classes_of(case.mode, case.stride):
        k[..., R::S, SS::S] = min(K_ACC, 3 * reduction_length(case, R, SS) + case.ksplit) + (2 if affine else 0)
    return k


MUTATIONS = (
    "drop_lo_hi",                        # the w_lo x_hi product is dropped
    "drop_hi_lo",                        # the w_hi x_lo product is dropped
    "bias_every_split",
    "bias_no_split",
    "skip_last_chunk_of_last_split",     # the shorter part
    "chunk_buffer_parity",               # chunk n reads chunk n - 1's patch (the transposed double buffer)
    "pad_before_act",                    # padding holds act(shift) instead of 0
    "tap_shift",                         # one tap one pixel off
    "class_swap",                        # parities (0, 1) and (1, 0) exchanged
    "second_class_from_first_filter",    # the paired body's second accumulator fed class 1's taps
    "tile_remap",                        # two pixel tiles exchanged, as a wrong XCD remap would
    "cout_row_off_by_one",               # in the second 32-row fragment
    "image_pair_leak",                   # NB = 2: the missing second image of an odd batch is stored into the next slot
)


def _patch(xp, mode, S, c, kh, kw, H, W, OH, OW, dw=0):
    """The (B, OH or H, OW or W) view of the padded planes xp (pad 2 + 1) that tap (kh, kw) of channel c multiplies;
    ``dw``: the view one column off (tap_shift)."""
    if mode == FWD:
        return xp[:, c, 1 + kh:1 + kh + S * (OH - 1) + 1:S, 1 + kw + dw:1 + kw + dw + S * (OW - 1) + 1:S]
    a, b = kh // S, kw // S                                   # input pixel i + 2 // S - a of class row i
    return xp[:, c, 3 + 2 // S - a:3 + 2 // S - a + H, 3 + 2 // S - b + dw:3 + 2 // S - b + dw + W]


def restate32(case, x, w, bias, x_bound, w_bound, affine=None, mut=None):
    """The kernel's fp32 evaluation (see the module docstring) as a (B, Cout, OH, OW) fp32 tensor; `mut`: one of
    MUTATIONS."""
    assert mut is None or mut in MUTATIONS, mut
    f = torch.float32
    mode, S, B, Cin, H, W, Cout = case.mode, case.stride, case.B, case.Cin, case.H, case.W, case.Cout
    OH, OW = case.out_hw
    ksplit, nchunks = case.ksplit, Cin // 16
    cps = -(-nchunks // ksplit)
    xa = activated(x, affine)
    if mut == "pad_before_act" and affine is not None:       # the halo goes through the affine and the activation too
        halo = activated(torch.zeros(1, Cin, 1, 1), affine).expand(B, Cin, H + 6, W + 6).clone()
        halo[:, :, 3:3 + H, 3:3 + W] = xa
        xa = halo
    else:
        xa = F.pad(xa, (3, 3, 3, 3))
    xh, xl = (p.float() for p in planes(xa, x_bound))
    wh, wl = (p.float() for p in planes(w if mode == FWD else w.transpose(0, 1), w_bound))      # [Cout][Cin][5][5]
    ux, uw = (torch.tensor(scales(b)[1], dtype=f) for b in (x_bound, w_bound))
    products = [(wl, xh), (wh, xl), (wh, xh)]
    if mut == "drop_lo_hi":
        products = products[1:]
    if mut == "drop_hi_lo":
        products = [products[0], products[2]]
    out = torch.empty(B, Cout, OH, OW, dtype=f)
    classes = classes_of(mode, S)
    for (R, SS) in classes:
        steps = steps_of(case, R, SS)
        wsteps = steps
        if mut == "second_class_from_first_filter" and (R, SS) == (1, 1):
            wsteps = steps_of(case, 0, 0)[:len(steps)]        # the first class's filter stream, the second class's patch
        shape = (B, Cout, H, W) if mode == TR else (B, Cout, OH, OW)
        slabs = []
        for split in range(ksplit):
            c_begin, c_end = split * cps, min((split + 1) * cps, nchunks)
            if mut == "skip_last_chunk_of_last_split" and split == ksplit - 1:
                c_end -= 1
            acc = torch.zeros(shape, dtype=f)
            for ch in range(c_begin, c_end):
                xch = ch - 1 if (mut == "chunk_buffer_parity" and ch > c_begin) else ch
                for si, st in enumerate(steps):
                    for pw, px in products:
                        for ki, (c, kh, kw) in enumerate(st):
                            wc, wkh, wkw = wsteps[si][ki]
                            dw = 1 if (mut == "tap_shift" and si == len(steps) - 1 and ki >= 8) else 0
                            acc.addcmul_(pw[None, :, ch * 16 + wc, wkh, wkw, None, None],
                                         _patch(px, mode, S, xch * 16 + c, kh, kw, H, W, OH, OW, dw)[:, None])
            acc = acc * ux * uw
            with_bias = bias is not None and mut != "bias_no_split" and (split == 0 or mut == "bias_every_split")
            slabs.append(acc + bias.float()[None, :, None, None] if with_bias else acc)
        if mut == "image_pair_leak" and ksplit > 1 and B % 2:
            for split in range(ksplit - 1, 0, -1):            # image B of slab s - 1 is image 0 of slab s
                slabs[split][0] = slabs[split - 1][B - 1]
        y = slabs[0] if ksplit == 1 else slab_sum32(slabs, (B * Cout * OH * OW) % 4 == 0)
        if mode == TR:
            out[:, :, R::S, SS::S] = y
        else:
            out = y
    if mut == "class_swap":
        a, b = out[:, :, 0::2, 1::2].clone(), out[:, :, 1::2, 0::2].clone()
        out[:, :, 0::2, 1::2], out[:, :, 1::2, 0::2] = b, a
    if mut == "tile_remap":
        swap_tiles(case, out)
    if mut == "cout_row_off_by_one" and Cout > 33:
        out[:, 33:64] = out[:, 32:63].clone()[:, :out[:, 33:64].shape[1]]
    return out


def swap_tiles(case, out):
    """Exchanges (in place) the outputs of two pixel tiles from the middle of the grid: the tiles of two image groups at
    the same place when the batch has more than one group, else two neighbouring tiles of the image."""
    _v, _k, NB, TH, TW, _p = case.route
    S = 2 if case.mode == TR else 1                           # output pixels per tile pixel
    groups = -(-case.B // NB)
    if groups >= 2:
        g1, g2 = groups // 2 - 1, groups // 2
        n = min(NB, case.B - g2 * NB)
        a, b = out[g1 * NB:g1 * NB + n, :, :S * TH, :S * TW], out[g2 * NB:g2 * NB + n, :, :S * TH, :S * TW]
    else:
        assert out.shape[3] >= 2 * S * TW, case
        a, b = out[:, :, :S * TH, :S * TW], out[:, :, :S * TH, S * TW:2 * S * TW]
    t = a.clone()
    a.copy_(b)
    b.copy_(t)


# ------------------------------------------------------------------------------------------------ statistics
def stats_ok(stats, y):
    """stats: the device's (slots, Cout, 2) buffer; y: the device's output.  (ok, worst ratio to the bound), per channel,
    for the sum and the sum of squares (see the module docstring)."""
    s = stats.detach().cpu().double()
    yd = y.detach().cpu().double()
    if not bool(torch.isfinite(s).all()):
        return False, float("nan")
    worst = 0.0
    for j, v in enumerate((yd, yd * yd)):
        want, m = v.sum(dim=(0, 2, 3)), v.abs().sum(dim=(0, 2, 3))
        r = (s[:, :, j].sum(0) - want).abs() / (STATS_N * U * m).clamp_min(torch.finfo(torch.float64).tiny)
        worst = max(worst, float(r.max()))
    return worst <= 1.0, worst
