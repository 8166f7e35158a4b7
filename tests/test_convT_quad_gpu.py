"""The quad form of the stride-2 transposed convolution with <= 32 output channels (conv_bf16split.hip, tile variant 6:
one workgroup = one 8 x 32 input tile and all four output-parity classes) against fp64 and, bit for bit, against the
per-class kernel it replaces (variant 4).  fp16x3 unless a test says otherwise.

Bound against fp64: relative L2 <= 3e-6, the CONV_TOL tests/test_kernels_gpu.py holds this kernel family to."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 3e-6
GUARD = -12345.5
FRONT, BACK = 1024, 4096        # guard floats in front of / behind the output


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    prev, ops.CONV_ARITH = ops.CONV_ARITH, "fp16x3"
    yield ops
    ops.CONV_ARITH = prev


@pytest.fixture
def tuning(H):
    """The tuning build (the tile-forcing knob) for one test; the knob is back on the heuristic afterwards."""
    from disentangle_mlp_amd import _lib
    with _lib.use_tuning() as lib:
        try:
            yield lib
        finally:
            lib.vg_debug_set_conv_bf16split_tile(-1)


def ref64(x, w, bias):
    return torch.nn.functional.conv_transpose2d(x.double(), w.double(), None if bias is None else bias.double(), stride=2,
                                                padding=2, output_padding=1)


def rel_l2(a, ref):
    return float((a.detach().cpu().double() - ref).norm() / max(float(ref.norm()), 1e-30))


def operands(B, Cin, Cout, Hs, Ws, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, Hs, Ws, generator=g)
    w = torch.randn(Cin, Cout, 5, 5, generator=g) * 0.05
    return x, w, (torch.randn(Cout, generator=g) if bias else None)


def guarded_convT(H, x, w, bias, amax=None, skew=0):
    """vg_convT5x5_fwd_bf16split of the active library into the middle of a guard-filled buffer (``skew`` floats further
    in: 1 leaves the output 4-byte aligned only); returns (whole buffer, the output's view of it).  ``amax``: the bound
    of max |x| handed to the kernel instead of the measured one."""
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    B, Cin, Hs, Ws = x.shape
    Cout = w.shape[1]
    n = B * Cout * 4 * Hs * Ws
    buf = torch.full((FRONT + skew + n + BACK,), GUARD, dtype=torch.float32, device="cuda")
    y = buf[FRONT + skew:FRONT + skew + n]
    xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
    bd = None if bias is None else bias.cuda()
    pk = H._packed_filter(lib, wd, Cout, Cin, H.PACK_SPLIT, True, 2)
    f = _lib.ConvFusion()
    slot = H.amax_of(xd) if amax is None else torch.tensor([amax], dtype=torch.float32, device="cuda")
    f.in_amax = slot.data_ptr()
    assert lib.vg_convT5x5_fwd_bf16split_workspace_bytes(B, Cin, Hs, Ws, Cout, 2, H._planes()) == 0
    _lib.check(lib.vg_convT5x5_fwd_bf16split(xd.data_ptr(), pk.data_ptr(), H._ptr(bd), y.data_ptr(), B, Cin, Hs, Ws, Cout, 2,
                                             H._planes(), None, 0, ctypes.byref(f), H._stream()), "vg_convT5x5_fwd_bf16split")
    torch.cuda.synchronize()
    return buf, y.view(B, Cout, 2 * Hs, 2 * Ws)


def both_variants(H, lib, x, w, bias, amax=None, skew=0):
    """Variant 6 (quad), then variant 4 (per class) on the same operands: the buffers are equal bit for bit, the guards
    intact; returns the quad output."""
    n = x.shape[0] * w.shape[1] * 4 * x.shape[2] * x.shape[3]
    out = {}
    for variant in (6, 4):
        lib.vg_debug_set_conv_bf16split_tile(variant)
        buf, y = guarded_convT(H, x, w, bias, amax, skew)
        assert bool((buf[:FRONT + skew] == GUARD).all()) and bool((buf[FRONT + skew + n:] == GUARD).all()), \
            f"variant {variant} wrote outside the output"
        out[variant] = (buf, y)
    assert torch.equal(out[6][0], out[4][0]), "quad and per-class kernels differ"
    return out[6][1]


# ------------------------------------------------------------------ 1. the production route
@pytest.mark.parametrize("B,Cin,Cout", [(8, 16, 32), (8, 32, 32), (8, 16, 20), (8, 32, 20), (16, 16, 20), (16, 32, 32)])
def test_production_route(H, B, Cin, Cout):
    """The heuristic's own choice (no switch), the product library, 64 x 64 inputs, one and two chunks of channels, a
    full and a partial cout fragment.  B = 8 is 32 768 input pixels, where the 256-pixel tiles begin (128 quad
    workgroups: the per-class kernel measured faster there and keeps the launch); B = 16 gives the quad kernel's grid a
    workgroup per CU, from where dispatch_x sends the launch to it."""
    x, w, bias = operands(B, Cin, Cout, 64, 64, seed=B + Cin + Cout)
    y = H.convT5x5_fwd(x.cuda(), w.cuda(), bias.cuda(), 2)
    ref = ref64(x, w, bias)
    assert tuple(y.shape) == tuple(ref.shape)
    e = rel_l2(y, ref)
    print(f"production route B {B} Cin {Cin} Cout {Cout}: rel L2 {e:.3e}")
    assert e <= TOL, f"rel L2 {e:.3e} > {TOL:.1e}"


# ------------------------------------------------------------------ 2. edges, quad against per-class
@pytest.mark.parametrize("Cout", [32, 20, 1])
@pytest.mark.parametrize("Hs,Ws", [(8, 32), (9, 33), (5, 7)])
@pytest.mark.parametrize("B", [1, 3])
def test_edges_bit_identical(H, tuning, B, Hs, Ws, Cout):
    """One tile exactly, partial tiles both ways, an image smaller than a tile; full, partial and single-channel cout
    fragments.  A store for a channel >= Cout or a pixel beyond the image would land in the next image or the guard."""
    x, w, bias = operands(B, 16, Cout, Hs, Ws, seed=100 * B + Hs + Cout)
    y = both_variants(H, tuning, x, w, bias)
    e = rel_l2(y, ref64(x, w, bias))
    print(f"edges B {B} {Hs}x{Ws} Cout {Cout}: rel L2 {e:.3e}")
    assert e <= TOL, f"rel L2 {e:.3e} > {TOL:.1e}"


def test_output_aligned_to_4_bytes_only(H, tuning):
    """An output that starts 4 bytes off an 8-byte boundary takes the 4-byte stores: same bits, same guards."""
    x, w, bias = operands(2, 16, 20, 9, 33, seed=7)
    y = both_variants(H, tuning, x, w, bias, skew=1)
    assert rel_l2(y, ref64(x, w, bias)) <= TOL
    assert torch.equal(y, both_variants(H, tuning, x, w, bias, skew=0))


def test_bf16x3_planes_share_the_kernel(H, tuning):
    """The opt-in 2-plane bf16 arithmetic instantiates the same quad body: same bits as its per-class kernel, and the
    2e-5 that tests/test_kernels_gpu.py holds bf16x3 to."""
    x, w, bias = operands(3, 32, 20, 9, 33, seed=5)
    prev, H.CONV_ARITH = H.CONV_ARITH, "bf16x3"
    try:
        y = both_variants(H, tuning, x, w, bias)
    finally:
        H.CONV_ARITH = prev
    e = rel_l2(y, ref64(x, w, bias))
    print(f"bf16x3 quad: rel L2 {e:.3e}")
    assert e <= 2e-5, f"rel L2 {e:.3e} > 2.0e-05"


# ------------------------------------------------------------------ 3. one pixel: the filter itself
@pytest.mark.parametrize("corner", [(0, 0), (0, 32), (8, 0), (8, 32)])
def test_single_corner_pixel(H, tuning, corner):
    """One image of the batch is zero except a single 1.0 at a corner pixel: its output is that input channel's filter
    (where the image holds it) and exactly 0 everywhere else -- a patch element staged at the wrong place, or a masked
    one let through, shows as a non-zero there.  The bound handed in is 8 x the true maximum.
    Per element: 1.0 times a power of two is exact in the hi plane; a filter value's hi + lo planes drop at most 2^-23 of
    it (2^-39 of the filter's bound once lo is an fp16 subnormal), and the three fp32 accumulations round by 2^-24 each:
    |y - w| <= 2^-21 |w| + 2^-38 max |w|."""
    Hs, Ws, B, Cin, Cout, ci = 9, 33, 3, 16, 20, 5
    x, w, _ = operands(B, Cin, Cout, Hs, Ws, seed=11, bias=False)
    x[1] = 0.0
    x[1, ci, corner[0], corner[1]] = 1.0
    y = both_variants(H, tuning, x, w, None, amax=8.0 * float(x.abs().max())).cpu()
    ref = ref64(x, w, None)
    assert rel_l2(y, ref) <= TOL
    zero = ref[1] == 0
    assert int((~zero).sum()) > 0 and bool((y[1][zero] == 0).all()), "a non-zero where the filter does not reach"
    err = (y[1].double() - ref[1]).abs()
    assert bool((err <= 2.0 ** -21 * ref[1].abs() + 2.0 ** -38 * float(w.abs().max())).all()), float(err.max())
