"""MI355X: the four kernels of csrc/fid_front.hip against the torch CPU functions the reference itself calls, evaluated
in fp64 -- ``F.max_pool2d``, ``F.avg_pool2d(count_include_pad=False)``, ``F.interpolate(mode="bilinear",
align_corners=False)``, ``F.adaptive_avg_pool2d`` -- and the batch quantiser against the per-image writer
(``ops.image_grid_u8``, itself pinned bit-exact against the restated torchvision 0.2.1 arithmetic).

Tolerances: max pooling, the quantiser, the identity resize and every emitted bound are bit-exact.  Average pooling:
8 fp32 additions and one division, each within 2^-24 of a partial sum bounded by 9 max|x| / count: ~6e-7 max|x|,
stated as 1e-6 max|x|.  Global average: the same bound (a per-lane chain and a 6-level tree of partial means).
Resize: not fixed in advance -- the fp32 rounding of the source coordinate dominates and ATen has the same one, so the
kernel must stay within twice the error ATen's own fp32 evaluation shows against fp64 (+ 1e-6)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


def record(key, value):
    """Measured figures go to the JSON-lines file VG_FID_RECORD names (the profile run sets it); printed always."""
    print(f"[fid_front] {key}: {value}")
    path = os.environ.get("VG_FID_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({key: value}) + "\n")


def _normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _unaligned(x):
    """x on the device as a contiguous view that starts one float behind a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


MODES = {"max_s2": ("max", 2, 0), "avg_s1": ("avg", 1, 1), "max_s1": ("max", 1, 1)}
POOL_CASES = [(shape, m, kind) for shape in ((2, 5, 7, 9), (1, 3, 3, 3)) for m in MODES for kind in ("plain",)]
POOL_CASES += [((2, 4, 35, 35), "max_s2", "plain"), ((1, 2, 8, 8), "avg_s1", "plain"), ((1, 2, 8, 8), "max_s1", "plain")]
POOL_CASES += [((1, 3, 5, 6), m, "negative") for m in MODES]           # a zero-padded max / a pad-counting average show here
POOL_CASES += [((1, 3, 7, 9), m, "unaligned") for m in MODES]          # base 4 bytes behind a 16-byte boundary, W = 9


@pytest.mark.parametrize("shape,mode_key,kind", POOL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_pool3x3(shape, mode_key, kind):
    from disentangle_mlp_amd import ops
    mode, stride, pad = MODES[mode_key]
    x = _normal(shape, 11)
    if kind == "negative":
        x = -x.abs() - 0.5
    xd = _unaligned(x) if kind == "unaligned" else x.cuda()
    x64 = x.double()
    want = F.max_pool2d(x64, 3, stride, pad) if mode == "max" else \
        F.avg_pool2d(x64, 3, stride, pad, count_include_pad=False)
    B, C, OH, OW = want.shape
    if shape == (1, 3, 3, 3) and stride == 2:
        assert (OH, OW) == (1, 1)
    off, total = 2, C + 5
    first = None
    for s0 in (0.0, 1e6):                              # the slot: empty, and already above every |out|
        out = torch.full((B, total, OH, OW), SENTINEL, dtype=torch.float32, device="cuda")
        slot = torch.full((1,), s0, dtype=torch.float32, device="cuda")
        view = ops.pool3x3(xd, stride, pad, mode, out, off, slot)
        got = out.cpu()
        assert view.data_ptr() == out[:, off:off + C].data_ptr() and ops.amax_of(view) is slot
        untouched = torch.cat([got[:, :off], got[:, off + C:]], 1)
        assert torch.equal(untouched, torch.full_like(untouched, SENTINEL))            # bit-unchanged
        y = got[:, off:off + C]
        if mode == "max":
            assert torch.equal(y.double(), want)
        else:
            err = float((y.double() - want).abs().max())
            assert err <= 1e-6 * float(x.abs().max()), err
        assert float(slot) == max(s0, float(y.abs().max()))                           # exactly
        first = y if first is None else first
        assert torch.equal(first, y)
    if kind == "negative":
        assert float(first.max()) < 0


def test_pool3x3_without_out_and_rejections():
    from disentangle_mlp_amd import ops
    x = _normal((2, 3, 6, 5), 2).cuda()
    y = ops.pool3x3(x, 2, 0, "max")
    assert torch.equal(y.cpu(), F.max_pool2d(x.cpu(), 3, 2)) and float(ops.amax_of(y)) == float(y.abs().max())
    with pytest.raises(RuntimeError):
        ops.pool3x3(x, 3, 0, "max")
    with pytest.raises(RuntimeError):
        ops.pool3x3(x, 1, 1, "max", torch.empty(2, 3, 6, 5, device="cuda"), 1)     # the slice does not fit
    with pytest.raises(RuntimeError):
        ops.pool3x3(x[:, :, :2].contiguous(), 1, 0, "avg")                                     # smaller than the window


@pytest.mark.parametrize("hw", [(64, 64), (32, 32), (299, 299), (300, 200), (1, 1)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_resize_bilinear_u8(hw):
    from disentangle_mlp_amd import ops
    H, W = hw
    img = torch.randint(0, 256, (2, H, W, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    y = ops.resize_bilinear_u8(img.cuda(), (299, 299), 2.0, -1.0)
    got = y.cpu()
    v = img.permute(0, 3, 1, 2)
    ref64 = 2 * F.interpolate(v.double() / 255, size=(299, 299), mode="bilinear", align_corners=False) - 1
    ref32 = 2 * F.interpolate(v.float() / 255, size=(299, 299), mode="bilinear", align_corners=False) - 1
    e_ref = float((ref32.double() - ref64).abs().max())
    e_kernel = float((got.double() - ref64).abs().max())
    record(f"resize_{H}x{W}_to_299", {"e_ref_aten_fp32_vs_fp64": e_ref, "e_kernel_vs_fp64": e_kernel})
    assert got.shape == (2, 3, 299, 299)
    assert e_kernel <= 2 * e_ref + 1e-6, (e_kernel, e_ref)
    if hw == (299, 299):
        assert torch.equal(got, 2 * (v.float() / 255) - 1)                          # in == out: the identity, bit for bit
    assert float(ops.amax_of(y)) == float(got.abs().max())


def test_resize_takes_other_output_sizes_and_scales():
    from disentangle_mlp_amd import ops
    img = torch.randint(0, 256, (1, 9, 5, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    y = ops.resize_bilinear_u8(img.cuda(), (13, 7), 1.0, 0.0).cpu()
    v = img.permute(0, 3, 1, 2)
    ref64 = F.interpolate(v.double() / 255, size=(13, 7), mode="bilinear", align_corners=False)
    ref32 = F.interpolate(v.float() / 255, size=(13, 7), mode="bilinear", align_corners=False)
    assert float((y.double() - ref64).abs().max()) <= 2 * float((ref32.double() - ref64).abs().max()) + 1e-6


@pytest.mark.parametrize("B,C,H,W", [(5, 3, 16, 12), (3, 1, 16, 12), (3, 3, 5, 7)], ids=["rgb", "grey", "odd"])
def test_quantize_each_u8_is_the_per_image_writer(B, C, H, W):
    from disentangle_mlp_amd import ops
    x = _normal((B, C, H, W), 21)
    x[1] = 0.37                                             # max == min: only the 1e-5 keeps the division finite
    x[2].view(-1)[5] = x[2].max()                           # a second value exactly at the maximum
    xd = x.cuda()
    got = ops.quantize_each_u8(xd)
    assert got.shape == (B, H, W, 3) and got.dtype == torch.uint8
    for i in range(B):
        assert torch.equal(got[i], ops.image_grid_u8(xd[i], normalize=True)), i
    assert int(got[1].max()) == 0 and int(got[2].max()) == 254           # (max - min) / (max - min + 1e-5) < 1: trunc
    un = ops.quantize_each_u8(_unaligned(x))                              # the scalar path: same bytes
    assert torch.equal(un, got)


@pytest.mark.parametrize("shape,kind", [((3, 7, 64), "plain"), ((2, 2048, 64), "plain"), ((2, 5, 35), "unaligned")],
                         ids=["3x7x64", "2x2048x64", "2x5x35_unaligned"])
def test_global_avg_pool(shape, kind):
    from disentangle_mlp_amd import ops
    x = _normal(shape, 31) + 0.25
    xd = _unaligned(x) if kind == "unaligned" else x.cuda()
    a, b = ops.global_avg_pool(xd), ops.global_avg_pool(xd)
    want = F.adaptive_avg_pool2d(x.double().unsqueeze(-1), (1, 1)).reshape(shape[0], shape[1])
    err = float((a.cpu().double() - want).abs().max())
    assert a.shape == shape[:2] and err <= 1e-6 * float(x.abs().max()), err
    assert torch.equal(a, b)                                              # fixed summation order
    if kind == "unaligned":
        assert torch.equal(a, ops.global_avg_pool(x.cuda()))              # ... which the alignment does not change
