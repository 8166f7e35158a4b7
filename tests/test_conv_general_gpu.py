"""MI355X: the general fp16x3 forward convolution (csrc/conv_general.hip, ops.conv2d_bias_act) on every distinct
convolution of the FID Inception network, against relu(F.conv2d) in fp64 on the CPU.  Tolerance: relative L2 <= 3e-6,
the project's figure for every fp16x3 convolution; the fp32 CPU convolution itself stays at
0.7e-7 ... 2.5e-7 on these shapes, so the fp64 reference is far inside it.
The kernel's edges -- every forced tile, tails, borders, non-finite inputs, per element -- are tests/test_conv_general_elem_gpu.py's."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CONV_TOL = 3e-6


@functools.lru_cache(maxsize=None)
def network_convolutions():
    """(cin, cout, kernel, stride, padding, (H, W)) of every distinct convolution, collected from the product's module
    tree with forward hooks on one 1 x 3 x 299 x 299 CPU forward."""
    from disentangle_mlp_amd import inception
    model = inception.InceptionV3([3], resize_input=False, weights=inception._FidInception().state_dict())
    seen, hooks = [], []

    def hook(mod, args, out):
        c = mod.conv
        key = (c.in_channels, c.out_channels, tuple(c.kernel_size), tuple(c.stride), tuple(c.padding), tuple(args[0].shape[2:]))
        if key not in seen:
            seen.append(key)

    for mod in model.modules():
        if isinstance(mod, inception._ConvBN):
            hooks.append(mod.register_forward_hook(hook))
    with torch.no_grad():
        model(torch.rand(1, 3, 299, 299, generator=torch.Generator().manual_seed(0)))
    for h in hooks:
        h.remove()
    return tuple(seen)


def _id(c):
    return f"{c[0]}-{c[1]}-k{c[2][0]}x{c[2][1]}-s{c[3][0]}-p{c[4][0]}x{c[4][1]}-{c[5][0]}x{c[5][1]}"


@pytest.fixture(scope="module")
def ops():
    from disentangle_mlp_amd import ops
    return ops


def make(conv, B, seed):
    """He-scaled random filter, a bias, a non-negative input (what oracle.inception.random_fid_inception feeds a layer)."""
    cin, cout, k, _, _, hw = conv
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, *k, generator=g) * (2.0 / (cin * k[0] * k[1])) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    x = torch.rand(B, cin, *hw, generator=g)
    return x, w, b


def reference(x, w, b, conv, relu=True):
    y = F.conv2d(x.double(), w.double(), b.double(), stride=conv[3], padding=conv[4])
    return torch.relu(y) if relu else y


def launch(ops, x, w, b, conv, **kw):
    packed, meta = ops.conv_general_pack(w.cuda(), conv[3], conv[4])
    return ops.conv2d_bias_act(x if x.is_cuda else x.cuda(), packed, meta, b.cuda(), **kw)


def rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm())


def test_the_network_has_the_expected_variety():
    convs = network_convolutions()
    kernels = {c[2] for c in convs}
    assert {(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1)} <= kernels
    assert {c[0] for c in convs} >= {3, 32, 48, 80, 96, 160, 192, 288, 384, 448, 768, 1280, 2048}
    assert {c[5][0] for c in convs} >= {299, 149, 147, 73, 35, 17, 8}


@pytest.mark.parametrize("conv", network_convolutions(), ids=_id)
def test_every_convolution_of_the_network(ops, conv):
    x, w, b = make(conv, 3, 11)
    got = launch(ops, x, w, b, conv).cpu()
    want = reference(x, w, b, conv)
    assert got.shape == want.shape
    e = rel_l2(got, want)
    print(f"conv_general {_id(conv)}: rel L2 {e:.3e}")
    assert e <= CONV_TOL, e


SLICE_CASES = [c for c in network_convolutions() if c[:3] in ((288, 64, (1, 1)), (64, 96, (3, 3)), (160, 192, (1, 7)),
                                                              (1280, 192, (1, 1)))]


@pytest.mark.parametrize("conv", SLICE_CASES, ids=_id)
def test_channel_slice_leaves_the_other_channels_alone(ops, conv):
    x, w, b = make(conv, 3, 12)
    alone = launch(ops, x, w, b, conv)
    before, after = 5, 7
    total = before + conv[1] + after
    out = torch.full((3, total) + tuple(alone.shape[2:]), -1234.5, device="cuda")
    sentinel = out.clone()
    view = launch(ops, x, w, b, conv, out=out, out_channel_offset=before)
    assert view.data_ptr() == out[:, before:].data_ptr()
    assert torch.equal(out[:, before:before + conv[1]], alone)
    assert torch.equal(out[:, :before], sentinel[:, :before]) and torch.equal(out[:, before + conv[1]:], sentinel[:, before + conv[1]:])
    # `out` given as the slice itself
    out2 = sentinel.clone()
    launch(ops, x, w, b, conv, out=out2[:, before:before + conv[1]])
    assert torch.equal(out2, out)


def test_output_bound_is_the_exact_maximum_and_accumulates(ops):
    convs = network_convolutions()
    c1 = next(c for c in convs if c[:3] == (192, 64, (1, 1)))
    c2 = next(c for c in convs if c[:3] == (192, 48, (1, 1)))
    x, w1, b1 = make(c1, 3, 13)
    _, w2, b2 = make(c2, 3, 14)
    xd = x.cuda()
    y1 = launch(ops, xd, w1, b1, c1)
    s1 = ops.amax_of(y1)
    assert torch.equal(s1, y1.abs().max().reshape(1))
    slot = ops.new_amax_slot(xd.device)
    ya = launch(ops, xd, w1, b1, c1, amax=slot)
    yb = launch(ops, xd, 3 * w2, b2, c2, amax=slot)
    assert torch.equal(slot, torch.maximum(ya.abs().max(), yb.abs().max()).reshape(1))
    slot2 = ops.new_amax_slot(xd.device)
    launch(ops, xd, 3 * w2, b2, c2, amax=slot2)
    launch(ops, xd, w1, b1, c1, amax=slot2)
    assert torch.equal(slot2, slot)


def test_a_bound_that_is_too_small_is_loud(ops):
    """Loud, not wrong: with a bound 2^4 below the data the scaled input overflows fp16 and the output is inf / NaN.
    ReLU off: the activation passes NaN through, but turns -inf into a number times zero."""
    conv = next(c for c in network_convolutions() if c[:3] == (64, 96, (3, 3)))
    x, w, b = make(conv, 3, 15)
    xd = x.cuda()
    ops.set_amax(xd, (xd.abs().max() / 16).reshape(1))
    y = launch(ops, xd, w, b, conv, relu=False)
    assert not bool(torch.isfinite(y).all())
    xd2 = x.cuda()                                   # the honest bound: finite and right
    y2 = launch(ops, xd2, w, b, conv, relu=False)
    assert rel_l2(y2.cpu(), reference(x, w, b, conv, relu=False)) <= CONV_TOL


REPEAT_CASES = [(next(c for c in network_convolutions() if c[:3] == (1280, 448, (1, 1))), 50),      # underfilled 8 x 8 grid
                (next(c for c in network_convolutions() if c[:3] == (448, 384, (3, 3))), 50),
                (next(c for c in network_convolutions() if c[:3] == (128, 128, (7, 1))), 7),
                (next(c for c in network_convolutions() if c[:3] == (3, 32, (3, 3))), 2)]


@pytest.mark.parametrize("conv,B", REPEAT_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_two_runs_are_bit_identical(ops, conv, B):
    x, w, b = make(conv, B, 16)
    xd = x.cuda()
    packed, meta = ops.conv_general_pack(w.cuda(), conv[3], conv[4])
    bd = b.cuda()
    y1 = ops.conv2d_bias_act(xd, packed, meta, bd)
    s1 = ops.amax_of(y1)
    y2 = ops.conv2d_bias_act(xd, packed, meta, bd)
    assert torch.equal(y1, y2) and torch.equal(s1, ops.amax_of(y2))
    assert torch.equal(s1, y2.abs().max().reshape(1))


# one launch per spatial stage at the extractor's batch
FULL_SIZE = [next(c for c in network_convolutions() if c[:3] == k and c[5][0] == hw) for k, hw in (
    ((3, 32, (3, 3)), 299), ((32, 64, (3, 3)), 147), ((80, 192, (3, 3)), 73), ((48, 64, (5, 5)), 35),
    ((160, 160, (1, 7)), 17), ((768, 192, (1, 1)), 17), ((448, 384, (3, 3)), 8), ((2048, 320, (1, 1)), 8))]


@pytest.mark.parametrize("conv", FULL_SIZE, ids=_id)
def test_full_size_launch_against_fp64_crops(ops, conv):
    """B = 50 (what InceptionFeatureExtractor launches): the four corner crops of the first and the last image against
    the fp64 convolution of the input region they depend on."""
    B = 50
    cin, cout, k, s, p, (H, W) = conv
    g = torch.Generator(device="cuda").manual_seed(17)
    xd = torch.rand(B, cin, H, W, device="cuda", generator=g)
    _, w, b = make(conv, 1, 18)
    y = launch(ops, xd, w, b, conv)
    OH, OW = y.shape[2:]
    ch, cw = min(6, OH), min(6, OW)
    worst = 0.0
    for img in (0, B - 1):
        xp = F.pad(xd[img:img + 1].cpu().double(), (p[1], p[1], p[0], p[0]))
        for oh0 in (0, OH - ch):
            for ow0 in (0, OW - cw):
                region = xp[:, :, oh0 * s[0]:(oh0 + ch - 1) * s[0] + k[0], ow0 * s[1]:(ow0 + cw - 1) * s[1] + k[1]]
                want = torch.relu(F.conv2d(region, w.double(), b.double(), stride=s))
                got = y[img:img + 1, :, oh0:oh0 + ch, ow0:ow0 + cw].cpu()
                assert got.shape == want.shape
                worst = max(worst, rel_l2(got, want))
    print(f"conv_general B=50 {_id(conv)}: worst crop rel L2 {worst:.3e}")
    assert worst <= CONV_TOL, worst
    assert torch.equal(ops.amax_of(y), y.abs().max().reshape(1))
