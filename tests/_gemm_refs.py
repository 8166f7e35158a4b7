"""References for the Linear fp16x3 GEMM (csrc/gemm_split.hip: vg_gemm_nt_f16x3 and its grouped form) and the seeded
operands, shapes and mutations the CPU and the GPU tests share.  A plain module: nothing here touches a GPU (the split
count of a shape is asked of the library's host-only workspace query, `ksplit_of`).

    C[m][n] = sum_k A(m, k) B(n, k) (+ bias[n])

Every function takes the operands as the (rows, K) fp32 matrices the GEMM multiplies (`as_matrix` of what a layout
stores) and the bounds the kernel is handed, as Python floats.

  planes     the kernel's operand preparation restated: the exponent clamp of f16_bound_exp (common.hpp), the exact
             power-of-two scale applied in fp32, fp16 hi = rne(v), lo = rne(v - hi).  The CPU's half conversion keeps
             subnormals, as the MFMA does.
  emul64     the fp64 sum of the three plane products the kernel forms (hi hi, hi lo, lo hi; lo lo dropped), times the
             two exact inverse scales, plus bias: what the kernel would return with an exact accumulator FOR THE BOUNDS
             IT WAS HANDED.  The GPU tests compare with this, so that only the accumulation is left to a tolerance.
  ref64      the plain fp64 product.  tests/test_gemm_cpu.py holds emul64 to it by the documented split model.
  mag        |A| |B|^T (+ |bias|) in fp64: the per-element magnitude every bound is taken against.
  restate32  the same plane products accumulated in fp32 in the kernel's order: per 32-index stage two 16-index steps,
             within a step A_lo B_hi, A_hi B_lo, A_hi B_hi, each a sequential sum over its 16 indices (the MFMA's own
             order is not known); under a K split the per-slab partial sums, each unscaled (times ua, then ub, as the
             epilogue does), the bias with slab 0, then the slab sum in the order of vg_internal_wgrad_reduce
             (conv_wgrad.hip: slab order below 64 slabs when M N % 4 == 0, else per-wavefront strided partials and a
             pairwise tree).  It also takes the MUTATIONS below.

The per-element check of both files is `check`: every element finite and |got - emul64| <= k 2^-24 mag, k = k_acc(K,
ksplit).

K_ACC.  ACC_WORST is the worst |restate32 - emul64| / (2^-24 mag) over every shape of this file (`all_shapes`), as
tests/test_gemm_cpu.py::test_k_acc_is_measured_from_the_restatement measures it:

    pytest -s tests/test_gemm_cpu.py -k k_acc

K_ACC = ceil(4 ACC_WORST): the factor 4 is for the unknown summation order and rounding inside the MFMA.  Per shape it
is capped at 3 K + ksplit, the deterministic worst case (3 K additions into the accumulator, ksplit more in the slab
sum and the bias).  Nothing here is taken from a kernel run.
"""
import functools
import math

import torch

from _loss_refs import U      # 2^-24

LAYOUTS = ("fwd", "dgrad", "wgrad", "atbc")      # atbc: A strided / B contiguous (gemm_nt_f16x3_kernel<true, false>)
GKC, TILE = 32, 128           # reduction indices per stage, rows / columns of an output tile (gemm_split.hip)

# measured by tests/test_gemm_cpu.py (see above); the test fails if the measurement leaves [0.8 ACC_WORST, ACC_WORST]
#   K = 32 .. 224 unsplit: 2.7 - 5.9;  ragged tiles at K = 96 / 512: 0.4 - 8.1;  2, 4, 8, 16, 32 splits of 8 stages:
#   4.1, 3.4, 4.8, 7.1, 9.69 (128 x 128, K = 8192: the worst)
ACC_WORST = 9.7
K_ACC = math.ceil(4 * ACC_WORST)


def k_acc(K, ksplit):
    return min(K_ACC, 3 * K + ksplit)


# ------------------------------------------------------------------------------------------------ shapes of the edges
STAGE_KS = (32, 64, 96, 128, 160, 192, 224)              # nst 1..7, no K split
STAGE_MN = (40, 72)                                      # one partial tile
SPLIT_KS = (512, 768, 1024, 1280, 2048, 4096, 8192)
SPLIT_MNS = ((128, 128), (130, 136))                     # one tile, four tiles
SPLIT_COVER = {(2, 8), (2, 12), (4, 8), (4, 10), (8, 8), (16, 8), (32, 8)}      # (splits, stages per split) of SPLIT_KS
# every M of {1, 127, 128, 129} and N of {1, 3, 127, 128, 129, 257} with a whole (128) and with a ragged partner
RAGGED_MN = ((1, 128), (127, 128), (129, 128), (128, 1), (128, 3), (128, 127), (128, 129), (128, 257),
             (1, 3), (129, 1), (127, 127), (129, 129), (127, 257))
RAGGED_KS = (96, 512)                                    # unsplit, split in two
SMALL = (40, 72, 96)                                     # bounds, zero operands, clamps, non-finite data, pointers
SMALL_SPLIT = (130, 136, 1024)
ENTRY_SHAPES = ((129, 72, 96), (128, 128, 1024))         # the GEMMs behind ops.linear_fwd / _dgrad / _wgrad
LOOSE = (1, 5, 10)                                       # bounds loose by 2^1, 2^5, 2^10
GROUP_SCALES = (1.0, 1e3, 1e-3)                          # grouped entry: group 0 is neither the largest nor the smallest


def all_shapes():
    """Every (M, N, K) the GPU file launches."""
    s = [(*STAGE_MN, K) for K in STAGE_KS]
    s += [(M, N, K) for (M, N) in SPLIT_MNS for K in SPLIT_KS]
    s += [(M, N, K) for (M, N) in RAGGED_MN for K in RAGGED_KS]
    s += [SMALL, SMALL_SPLIT, *ENTRY_SHAPES]
    return sorted(set(s))


@functools.lru_cache(maxsize=None)
def ksplit_of(M, N, K):
    """Splits of the reduction, from the library's host-side workspace query (the heuristic is not restated)."""
    from disentangle_mlp_amd import _lib
    need = _lib.load().vg_gemm_nt_f16x3_workspace_bytes(M, N, K)
    assert need % (4 * M * N) == 0, (M, N, K, need)
    return max(need // (4 * M * N), 1)


# ------------------------------------------------------------------------------------------------ operands
def strides_of(layout, M, N, K, a_pitch=None, b_pitch=None):
    """(a_row_stride, a_k_stride, b_row_stride, b_k_stride); a pitch is the stored row length when wider than needed."""
    at, bt = layout in ("wgrad", "atbc"), layout in ("dgrad", "wgrad")
    a = (1, a_pitch or M) if at else (a_pitch or K, 1)
    b = (1, b_pitch or N) if bt else (b_pitch or K, 1)
    return (*a, *b)


def as_stored(layout, t, which):
    """The (rows, K) matrix as the layout stores it: transposed where the row index is the contiguous one."""
    tr = layout in ("wgrad", "atbc") if which == "A" else layout in ("dgrad", "wgrad")
    return t.t().contiguous() if tr else t.contiguous()


def as_matrix(layout, t, which):
    """The stored operand as the (rows, K) matrix the GEMM multiplies."""
    tr = layout in ("wgrad", "atbc") if which == "A" else layout in ("dgrad", "wgrad")
    return t.t() if tr else t


def _spread(n, decades, g):
    """n factors from 1 down to 10^-decades, evenly spaced in the exponent, in a seeded order; 1 is always among them."""
    if n == 1 or decades == 0:
        return torch.ones(n)
    e = torch.linspace(0.0, -float(decades), n)[torch.randperm(n, generator=g)]
    return (10.0 ** e.double()).float()


@functools.lru_cache(maxsize=None)
def matrices(M, N, K, seed=0, decades=4, a_mul=1.0, b_mul=1.0):
    """A (M, K), B (N, K), bias (N): full-mantissa normals.  The rows of A spread over `decades` decades and its
    reduction columns over two more, the rows of B over two: rows of very different magnitude share one bound."""
    g = torch.Generator().manual_seed(1000003 * seed + 8191 * M + 131 * N + K)
    A = torch.randn(M, K, generator=g) * _spread(M, decades, g)[:, None] * _spread(K, min(decades, 2), g)[None, :]
    B = torch.randn(N, K, generator=g) * 0.05 * _spread(N, min(decades, 2), g)[:, None]
    bias = torch.randn(N, generator=g) * 0.1 * float(a_mul) * float(b_mul)
    return A * float(a_mul), B * float(b_mul), bias


def operands(layout, M, N, K, seed=0, **kw):
    """(A as stored, B as stored, bias, strides) of one layout; `as_matrix` gives the matrices back."""
    A, B, bias = matrices(M, N, K, seed, **kw)
    return as_stored(layout, A, "A"), as_stored(layout, B, "B"), bias, strides_of(layout, M, N, K)


def bound_of(t):
    return float(t.abs().max())


# ------------------------------------------------------------------------------------------------ the arithmetic
def bound_exp(bound):
    """f16_bound_exp: the biased fp32 exponent of the bound, clamped to [15, 254] (0 / subnormal: 15; inf / NaN: 254)."""
    bits = int(torch.tensor(bound, dtype=torch.float32).view(torch.int32)) & 0x7fffffff
    return min(max(bits >> 23, 15), 254)


def scales(bound):
    """(f16_scale_of, f16_unscale_of): 2^(14 - E) and 2^(E - 14) for a bound in [2^E, 2^(E + 1)), exact."""
    e = bound_exp(bound)
    return 2.0 ** (141 - e), 2.0 ** (e - 141)


def pow2_bound(bound):
    """2^(E + 1): the power of two the scaled operand is kept under 2^15 of."""
    return 2.0 ** (bound_exp(bound) - 126)


def planes(x, bound):
    """(hi, lo) fp16 planes of x scaled by the bound's power of two, as piece() / split_planes16 form them."""
    v = x.float() * torch.tensor(scales(bound)[0], dtype=torch.float32)
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi, lo


def ref64(A, B, bias=None):
    r = A.double() @ B.double().t()
    return r if bias is None else r + bias.double()


def mag(A, B, bias=None):
    r = A.double().abs() @ B.double().abs().t()
    return r if bias is None else r + bias.double().abs()


def emul64(A, B, bias, a_bound, b_bound):
    ah, al = (p.double() for p in planes(A, a_bound))
    bh, bl = (p.double() for p in planes(B, b_bound))
    r = (al @ bh.t() + ah @ bl.t() + ah @ bh.t()) * scales(a_bound)[1] * scales(b_bound)[1]
    return r if bias is None else r + bias.double()


def slab_sum32(slabs, n_is_vec):
    """vg_internal_wgrad_reduce restated on a list of fp32 slabs: in slab order (slab_sum4 / slab_sum1), or -- 64 slabs
    and more, or M N % 4 != 0 -- NW wavefronts' strided partial sums joined by a pairwise tree (wgrad_reduce_kernel)."""
    ks = len(slabs)
    if ks < 64 and n_is_vec:
        s = torch.zeros_like(slabs[0])
        for v in slabs:
            s = s + v
        return s
    nw = 16 if (ks >= 64 and -(-slabs[0].numel() // 64) < 1024) else 4
    red = [torch.zeros_like(slabs[0]) for _ in range(nw)]
    for k, v in enumerate(slabs):
        red[k % nw] = red[k % nw] + v
    w = nw // 2
    while w >= 2:
        for i in range(w):
            red[i] = red[i] + red[i + w]
        w //= 2
    return red[0] + red[1]


MUTATIONS = (
    "drop_lo_hi",           # 1  the A_lo B_hi product is dropped
    "drop_hi_lo",           # 2  the A_hi B_lo product is dropped
    "group_scale0",         # 3  group g is scaled with group 0's bound (and unscaled with its own)
    "group_bound0",         # 3' group g is scaled AND unscaled with group 0's bound
    "bias_every_split",     # 4
    "bias_no_split",        # 5
    "skip_last_stage",      # 6  of the last split
    "last_stage_twice",     # 7  of the last split
    "slab_unwritten",       # 8  one (tile, split) slab never written: NaN, as the tests leave the workspace
    "slab_twice",           # 9  one (tile, split) slab summed twice
    "pad_leak",             # 10 rows >= M (clamped re-reads of row M - 1) are not zeroed and land in row M - 1
    "row_off_by_one",       # 11 rows of the second row tile stored one row late
    "col_off_by_one",       # 11 columns of the second column tile stored one column late
)
NEEDS_SPLIT = {"bias_every_split", "slab_unwritten", "slab_twice"}
NEEDS_BIAS = {"bias_every_split", "bias_no_split"}


def restate32(A, B, bias, a_bound, b_bound, ksplit=1, mut=None, a_unscale_bound=None):
    """The kernel's fp32 evaluation (see the module docstring) as an (M, N) fp32 tensor; `mut`: one of MUTATIONS
    (the group mutations are the caller's: they are a choice of `a_bound` / `a_unscale_bound`)."""
    assert mut is None or mut in MUTATIONS, mut
    M, K = A.shape
    N = B.shape[0]
    assert K % (GKC * ksplit) == 0
    kper = K // ksplit
    f = torch.float32
    # [k within the split][split][row][1] and [..][1][column]: all slabs advance together, each in its own order
    def cols(p, rows):
        return p.float().reshape(rows, ksplit, kper).permute(2, 1, 0).contiguous()
    ah, al = (cols(p, M).unsqueeze(3) for p in planes(A, a_bound))
    bh, bl = (cols(p, N).unsqueeze(2) for p in planes(B, b_bound))
    products = [(al, bh), (ah, bl), (ah, bh)]
    if mut == "drop_lo_hi":
        products = products[1:]
    if mut == "drop_hi_lo":
        products = [products[0], products[2]]
    last = torch.zeros(ksplit, 1, 1)
    last[-1] = 1.0
    acc = torch.zeros(ksplit, M, N, dtype=f)

    def step(k0, only_last=False, but_last=False):
        for pa, pb in products:
            for k in range(k0, k0 + 16):
                a = pa[k]
                if only_last:
                    a = a * last
                if but_last:
                    a = a * (1.0 - last)
                acc.addcmul_(a, pb[k])      # the product of two fp16 numbers is exact in fp32: one rounding, the sum's

    for k0 in range(0, kper, 16):
        step(k0, but_last=(mut == "skip_last_stage" and k0 >= kper - GKC))
    if mut == "last_stage_twice":
        step(kper - GKC, only_last=True)
        step(kper - 16, only_last=True)
    if mut == "pad_leak" and M % TILE:
        acc[:, M - 1] *= float(1 + TILE - M % TILE)
    ua = torch.tensor(scales(a_bound if a_unscale_bound is None else a_unscale_bound)[1], dtype=f)
    ub = torch.tensor(scales(b_bound)[1], dtype=f)
    slabs = [acc[s] * ua * ub for s in range(ksplit)]
    if bias is not None and mut != "bias_no_split":
        for s in range(ksplit if mut == "bias_every_split" else 1):
            slabs[s] = slabs[s] + bias.float()[None, :]
    if ksplit == 1:
        out = slabs[0]
    else:
        m0, n0 = (M - 1) // TILE * TILE, (N - 1) // TILE * TILE      # the last tile
        if mut == "slab_unwritten":
            slabs[ksplit // 2][m0:, n0:] = float("nan")
        if mut == "slab_twice":
            again = torch.zeros(M, N, dtype=f)
            again[m0:, n0:] = slabs[ksplit // 2][m0:, n0:]
            slabs.insert(ksplit // 2 + 1, again)
        out = slab_sum32(slabs, (M * N) % 4 == 0)
    if mut == "row_off_by_one" and M > TILE:
        out = torch.cat([out[:TILE], out[TILE - 1:M - 1]])
    if mut == "col_off_by_one" and N > TILE:
        out = torch.cat([out[:, :TILE], out[:, TILE - 1:N - 1]], dim=1)
    return out


# ------------------------------------------------------------------------------------------------ the check
def ratio(got, ref, m):
    """Worst |got - ref| / (2^-24 mag) over the elements (nan if any element of got is not finite)."""
    g = got.detach().cpu().double()
    if not bool(torch.isfinite(g).all()):
        return float("nan")
    tiny = torch.finfo(torch.float64).tiny
    return float(((g - ref).abs() / (U * m).clamp_min(tiny)).max())


def check(got, ref, m, k):
    """(ok, worst ratio): every element finite and |got - ref| <= k 2^-24 mag, no element excluded."""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape == m.shape, (g.shape, ref.shape, m.shape)
    w = ratio(g, ref, m)
    ok = bool(torch.isfinite(g).all()) and not bool(((g - ref).abs() > k * U * m).any())
    return ok, w
