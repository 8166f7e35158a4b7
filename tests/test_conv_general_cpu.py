"""CPU: the host side of the general forward convolution (csrc/conv_general.hip) -- the pack-size query against the
layout include/vaegan_hip.h documents, and argument validation, which happens before any launch (no device here)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def documented_bytes(cout, cin, kh, kw):
    """[nsteps][2 planes][4 k-blocks][CoutP] 16-byte units, the k -> (ci, kh << 16 | kw) table (8 bytes per padded
    reduction index), a 16-byte trailer; nsteps = ceil(K / 32), CoutP = Cout rounded up to 128."""
    nsteps = (cin * kh * kw + 31) // 32
    coutp = (cout + 127) // 128 * 128
    return nsteps * 2 * 4 * coutp * 16 + nsteps * 32 * 8 + 16


@pytest.mark.parametrize("cout,cin,kh,kw", [
    (32, 3, 3, 3),        # K = 27: one padded step
    (64, 48, 5, 5),       # K = 1200 -> 1216
    (192, 80, 3, 3),      # K = 720 -> 736, Cout 192 -> 256
    (192, 768, 1, 1), (192, 160, 7, 1), (384, 384, 1, 3), (320, 2048, 1, 1), (1, 1, 1, 1)])
def test_pack_size_is_the_documented_layout(lib, cout, cin, kh, kw):
    assert lib.vg_conv_general_packed_bytes(cout, cin, kh, kw) == documented_bytes(cout, cin, kh, kw)


def test_no_workspace_query_exists(lib):
    """The reduction is never split over workgroups, so the ABI has no workspace for this kernel."""
    from disentangle_mlp_amd import _lib
    assert not [n for n in _lib.SIGNATURES if n.startswith("vg_conv_general") and "workspace" in n]


def test_pack_size_rejects_bad_filters(lib):
    q = lib.vg_conv_general_packed_bytes
    assert q(0, 3, 3, 3) == 0 and q(32, 0, 3, 3) == 0 and q(32, 3, 0, 3) == 0 and q(32, 3, 3, 0) == 0
    assert q(32, 3, 16, 3) == 0                      # filter extents: 1..15
    assert q(-1, 3, 3, 3) == 0
    assert q(64, 1 << 30, 3, 3) == 0                 # K beyond the 32-bit index range


def test_bad_arguments_are_rejected_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                    # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15

    def fwd(x=p, packed=p, bias=p, y=p, B=1, Cin=3, H=8, W=8, Cout=4, KH=3, KW=3, sh=1, sw=1, ph=0, pw=0, ystride=None,
            relu=1, x_amax=p, y_amax=None):
        OH, OW = (H + 2 * ph - KH) // max(sh, 1) + 1, (W + 2 * pw - KW) // max(sw, 1) + 1
        return lib.vg_conv_general_fwd(x, packed, bias, y, B, Cin, H, W, Cout, KH, KW, sh, sw, ph, pw,
                                       Cout * OH * OW if ystride is None else ystride, relu, x_amax, y_amax, None)

    assert fwd(x=None) == -1 and fwd(packed=None) == -1 and fwd(y=None) == -1 and fwd(x_amax=None) == -1
    assert fwd(packed=p + 4) == -1                   # the pack is read in 16-byte units
    assert fwd(KH=0) == -1 and fwd(KW=0) == -1       # kernel extent 0
    assert fwd(sh=3) == -1 and fwd(sw=3) == -1 and fwd(sh=0) == -1
    assert fwd(ph=-1) == -1 and fwd(H=2) == -1       # filter larger than the padded image
    assert fwd(B=0) == -1 and fwd(Cin=0) == -1 and fwd(Cout=0) == -1
    assert fwd(ystride=4 * 6 * 6 - 1) == -1          # images of y would overlap
    # sizes beyond the 32-bit index range: output pixels of the batch, elements of one input image, of one output image
    assert fwd(B=1 << 20, H=1024, W=1024, KH=1, KW=1) == -1
    assert fwd(Cin=1 << 12, H=1024, W=1024, KH=1, KW=1) == -1
    assert fwd(Cout=1 << 12, H=1024, W=1024, KH=1, KW=1) == -1
    assert fwd(H=1 << 14, W=8, KH=1, KW=1) == -1     # image extents: <= 8192
    assert lib.vg_conv_general_pack(None, p, 4, 3, 3, 3, p, None) == -1
    assert lib.vg_conv_general_pack(p, None, 4, 3, 3, 3, p, None) == -1
    assert lib.vg_conv_general_pack(p, p, 4, 3, 3, 3, None, None) == -1
    assert lib.vg_conv_general_pack(p, p, 4, 3, 0, 3, p, None) == -1
    assert lib.vg_conv_general_pack(p, p + 4, 4, 3, 3, 3, p, None) == -1


def test_op_refuses_cpu_tensors():
    import torch
    from disentangle_mlp_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv_general_pack(torch.zeros(4, 3, 3, 3))
    meta = ops.ConvGeneralMeta(4, 3, 3, 3, 1, 1, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv2d_bias_act(torch.zeros(1, 3, 8, 8), torch.zeros(16, dtype=torch.uint8), meta)


def test_cpu_tensors_keep_the_unfold_lowering(monkeypatch):
    """A CPU tensor never reaches the HIP library, whatever the switch says."""
    import torch
    from disentangle_mlp_amd import inception
    monkeypatch.setattr(inception, "CONV_LOWERING", "hip")
    monkeypatch.setattr(inception, "_ops", lambda: pytest.fail("the CPU path loaded the HIP ops"))
    m = inception._ConvBN(3, 8, 3, stride=2).eval()
    x = torch.rand(2, 3, 9, 9, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = torch.relu(m.bn(m.conv(x)))
        got = m(x)
    assert float((got - want).abs().max()) <= 1e-5
