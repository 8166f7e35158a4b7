"""GPU: the bounds of max |tensor| that the fp16x3 arithmetic scales every convolution / big-Linear operand by
(common.hpp, "split arithmetics"), each against the exact maximum of what its consumer reads.  A bound below the data
overflows the fp16 hi plane (inf / NaN out); one far above it drops significand bits of the smaller elements.

(a) producers that emit an exact maximum: equal to max |output| bit for bit;  (b) the coefficient-only bound of the
BatchNorm finalize kernels on hand-made statistics slots, including channels whose computed variance cancels to 0;
(c) the same through the fused BatchNorm -> convolution layer;  (d) every bound a real training iteration hands out."""
import math

import numpy as np
import pytest
import torch

from disentangle_mlp_amd import _lib, functional as HF, ops
from oracle import ops as O

pytestmark = pytest.mark.gpu

CONV_TOL = 3e-6              # relative L2 of an fp16x3 convolution against fp64 (tests/test_kernels_gpu.py)
USELESS = 2.0 ** 16          # a bound this far above the largest element leaves even that element short of 22 bits
# 1e4 + 2^-10: its fp32 square is 3.5 below the exact one, the same for every element -- sums of them cancel in ANY order
C4 = 10000.0009765625
ACTS = {0: lambda v: v, 1: lambda v: v.clamp(min=0), 2: lambda v: torch.where(v > 0, v, 0.2 * v)}


@pytest.fixture(autouse=True)
def fp16x3():
    prev = ops.CONV_ARITH
    ops.CONV_ARITH = "fp16x3"
    yield
    ops.CONV_ARITH = prev


def _slot():
    return torch.zeros(1, device="cuda")


def _absmax(x):
    slot = _slot()
    assert _lib.load().vg_absmax(x.data_ptr(), x.numel(), slot.data_ptr(), None) == 0
    return slot


def _exact_max(t):
    """max |t| (a NaN anywhere: NaN), on the host in fp64 -- every fp32 value is exact there."""
    return float(t.detach().double().abs().max().cpu())


def _assert_exact(bound, t, what):
    b, m = float(bound), _exact_max(t)
    if math.isnan(m):
        assert math.isnan(b), (what, b)
    else:
        assert b == m, (what, b, m)


# ------------------------------------------------------------------------------------------- (a) exact producers
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4097, 2048 * 256 * 16 + 4099])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_absmax_sizes_offsets_and_where_the_maximum_sits(n, off):
    """vg_absmax: tails of every length, 16-byte aligned and unaligned views (offsets of 1-3 floats take the scalar
    path), a grid capped at 2048 workgroups (the largest n), the (negative) maximum at the first / last element."""
    g = torch.Generator(device="cuda").manual_seed(n * 4 + off)
    base = torch.randn(n + off, device="cuda", generator=g)
    x = base[off:]
    assert (x.data_ptr() % 16 == 0) == (off == 0)
    _assert_exact(_absmax(x), x, "random")
    for pos in sorted({0, n - 1, n // 2}):
        y = x.clone() if off == 0 else base.clone()[off:]
        y[pos] = -1e3 - pos
        _assert_exact(_absmax(y), y, f"maximum at {pos}")


def test_absmax_special_values():
    n = 4097
    z = torch.full((n,), -0.0, device="cuda")
    b = _absmax(z)
    assert float(b) == 0.0 and not math.copysign(1.0, float(b)) < 0
    sub = torch.full((n,), 1e-40, device="cuda")
    sub[1234] = -3e-39
    assert float(_absmax(sub)) == float(np.float32(3e-39))
    for v in (float("inf"), float("-inf")):
        x = torch.randn(n, device="cuda")
        x[77] = v
        assert float(_absmax(x)) == float("inf")
    x = torch.randn(n, device="cuda")
    x[4096] = float("nan")
    x[5] = float("inf")
    assert math.isnan(float(_absmax(x)))
    _assert_exact(_absmax(x[1:]), x[1:], "NaN, unaligned view")


def test_absmax_multi_many_entries_shared_slots_and_unaligned():
    """vg_absmax_multi: 31 entries (two launches of <= 24), sizes from 1 element to past the 64-workgroup cap of an
    entry, unaligned entries, and several entries accumulating into one slot."""
    g = torch.Generator(device="cuda").manual_seed(5)
    sizes = [1, 2, 3, 5, 7, 64, 100, 1023, 4097, 65536, 64 * 256 * 16 + 5, 3 * 64 * 256 * 16 + 1] * 3
    sizes = sizes[:31]
    bufs = [torch.randn(s + 3, device="cuda", generator=g) * (1 + i) for i, s in enumerate(sizes)]
    xs = [b[i % 4:][:s] for i, (b, s) in enumerate(zip(bufs, sizes))]      # offsets 0-3 floats
    for i, x in enumerate(xs):
        x[(i * 7919) % x.numel()] = -(100.0 + i)            # a negative maximum somewhere in each
    nslots = 9
    slots = torch.zeros(nslots, device="cuda")
    owner = [(i * 5) % nslots for i in range(len(xs))]
    arr = (_lib.AbsmaxEntry * len(xs))()
    for i, x in enumerate(xs):
        arr[i] = _lib.AbsmaxEntry(x.data_ptr(), x.numel(), slots[owner[i]:owner[i] + 1].data_ptr())
    assert _lib.load().vg_absmax_multi(arr, len(xs), None) == 0
    got = slots.cpu()
    for s in range(nslots):
        ref = max([_exact_max(x) for i, x in enumerate(xs) if owner[i] == s], default=0.0)
        assert float(got[s]) == ref, (s, float(got[s]), ref)


AFFINE_SHAPES = [(5, 7, 1, 1), (4, 6, 1, 3), (3, 5, 3, 4), (7, 9, 8, 12), (3, 4, 16, 16), (2, 3, 64, 64)]


@pytest.mark.parametrize("shape", AFFINE_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_absmax_affine_and_affine_act_bound(shape, act):
    """vg_absmax_affine (ops.amax_of with in_affine) == max |vg_affine_act(...)| on the same coefficients, bit for bit
    (both fmaf); vg_affine_act's own y_amax == max |y|.  HW = 1 / 3: scalar kernels; 12, 96: vector kernel with a
    non-power-of-two HW / 4; 256, 4096: the shift path; partial last chunks; negative scales."""
    B, C, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(B * C * H * W + act)
    x = torch.randn(B, C, H, W, device="cuda", generator=g) * 3
    sc = torch.randn(C, device="cuda", generator=g)                   # about half negative
    sh = torch.randn(C, device="cuda", generator=g)
    bound = ops.amax_of(x, (sc, sh, act))
    y = ops.affine_act(x, sc, sh, act)
    assert ops.known_amax(y) is not None
    _assert_exact(ops.known_amax(y), y, "vg_affine_act y_amax")
    _assert_exact(bound, y, "vg_absmax_affine")
    ref = ACTS[act](x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).abs().max()
    assert abs(float(bound) - float(ref)) <= 2.0 ** -23 * float(ref)


@pytest.mark.parametrize("shape", [(4, 8, 5, 5), (8, 16, 16, 16), (2, 3, 7, 3), (16, 64, 8, 8)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_act_fwd_bound(shape, act):
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + act)
    C = shape[1]
    x = torch.randn(*shape, device="cuda", generator=g) * 2 + 1
    gamma, beta = torch.randn(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
    y, _, _ = ops.bn_act_fwd(x, gamma, beta, None, None, 1e-5, 0.1, act)
    _assert_exact(ops.known_amax(y), y, "vg_bn_act_fwd y_amax")


@pytest.mark.parametrize("shape", [(8, 128, 8, 8), (16, 128, 32, 32), (4, 64, 16, 16), (3, 5, 7, 5), (128, 32, 64, 64)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_bn_act_bwd_bound(shape, accumulate):
    """gx_amax of every dispatch path of vg_bn_act_bwd: one-pass <2> and <8>, two-pass for C < 128, odd HW and a large
    per-channel count; with and without accumulate_param_grads."""
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + accumulate)
    C = shape[1]
    x = torch.randn(*shape, device="cuda", generator=g)
    gy = torch.randn(*shape, device="cuda", generator=g)
    gamma, beta = torch.randn(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
    for act in (0, 1, 2):
        _, mean, invstd = ops.bn_act_fwd(x, gamma, beta, None, None, 1e-5, 0.1, act)
        acc = (torch.ones(C, device="cuda"), torch.ones(C, device="cuda")) if accumulate else None
        gx, _, _ = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, act, True, accumulate_into=acc)
        _assert_exact(ops.known_amax(gx), gx, f"vg_bn_act_bwd gx_amax, act {act}")


@pytest.mark.parametrize("kind", [ops.EW_LRELU, ops.EW_TANH, ops.EW_SIGMOID])
def test_act_bwd_bound(kind, monkeypatch):
    monkeypatch.setattr(ops, "LINEAR_SPLIT", True)
    g = torch.Generator(device="cuda").manual_seed(40 + kind)
    pre = torch.randn(7, 129, device="cuda", generator=g) * 3          # 903 elements: not a multiple of 4
    y = {ops.EW_LRELU: torch.where(pre > 0, pre, 0.2 * pre), ops.EW_TANH: torch.tanh(pre),
         ops.EW_SIGMOID: torch.sigmoid(pre)}[kind].contiguous()
    gy = torch.randn(7, 129, device="cuda", generator=g) * 5
    gx = ops.act_bwd(gy, y, kind)
    _assert_exact(ops.known_amax(gx), gx, f"vg_act_bwd kind {kind}")


@pytest.mark.parametrize("case", ["two-pass", "producer's slots", "HW == 1"])
def test_batch_norm_act_hands_out_its_kernels_bound(case):
    """functional.batch_norm_act (BNActFn through autograd): the tensor the caller gets carries the exact max |out| its
    forward's kernel emitted -- vg_bn_act_fwd, or vg_affine_act behind the finalize of a convolution's slots --, and none
    on the HW == 1 path, where a consumer measures; backward runs and is finite."""
    g = torch.Generator(device="cuda").manual_seed(len(case))
    stats = None
    if case == "two-pass":
        x = torch.randn(4, 8, 4, 4, device="cuda", generator=g) * 2 + 1
    elif case == "HW == 1":
        x = torch.randn(8, 32, device="cuda", generator=g) * 2 + 1
    else:
        x0 = torch.randn(4, 16, 16, 16, device="cuda", generator=g)
        w0 = torch.randn(32, 16, 5, 5, device="cuda", generator=g) / 20
        x, stats = ops.conv5x5_fwd(x0, w0, None, 2, want_stats=True)
        assert stats is not None and stats.numel()
    C = x.shape[1]
    x.requires_grad_()
    gamma = torch.randn(C, device="cuda", generator=g).requires_grad_()
    beta = torch.randn(C, device="cuda", generator=g).requires_grad_()
    out = HF.batch_norm_act(x, gamma, beta, None, None, act=ops.ACT_LRELU, stats=stats)
    assert out.requires_grad
    if case == "HW == 1":
        assert ops.known_amax(out) is None
        _assert_exact(ops.amax_of(out), out, case)
    else:
        assert ops.known_amax(out) is not None
        _assert_exact(ops.known_amax(out), out, case)
    out.backward(torch.randn(out.shape, device="cuda", generator=g))
    for name, t in (("dx", x.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        assert t is not None and bool(torch.isfinite(t).all()), (case, name)


# ------------------------------------------------------------------ (b) the coefficient-only BatchNorm bound
def _fp32_slot_sums(v, k):
    """v: (C, n) fp32 values; slot j of channel c holds the fp32 sums of v[c, j*k:(j+1)*k] and of their (fp32-rounded)
    squares, added pairwise -- what a convolution epilogue writes: no term goes through more than 1 + log2(k) <= 9
    roundings (the slot contract, common.hpp VG_STATS_SLOT_DEPTH = 16).  Returns stats[nslots][C][2] on the GPU."""
    def tree(a):
        p = 1 << (a.shape[-1] - 1).bit_length()
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (p - a.shape[-1],), np.float32)], -1)
        while a.shape[-1] > 1:
            a = a[..., 0::2] + a[..., 1::2]
        return a[..., 0]
    a = v.numpy().astype(np.float32).reshape(v.shape[0], -1, k)
    st = np.stack([tree(a), tree(a * a)], axis=-1).transpose(1, 0, 2)      # [slot][C][2]
    return torch.from_numpy(np.ascontiguousarray(st)).cuda()


def _channels(n, g):
    """(name, values, gamma, beta, tight-case?) -- tight: |mean| <= 8 sigma, where the bound must stay ~|gamma| sqrt(n)."""
    def outlier(base, bump, at):
        v = torch.full((n,), base, dtype=torch.float64)
        v[at] += bump
        return v
    return [
        ("N(0,1)", torch.randn(n, generator=g, dtype=torch.float64), 1.3, 0.2),
        ("Samuelson extreme", outlier(0.0, 1000.0, n // 3), 1.0, 0.0),
        ("offset 50", 50 + torch.randn(n, generator=g, dtype=torch.float64), 0.9, -0.1),
        ("offset 7.5", 7.5 + torch.randn(n, generator=g, dtype=torch.float64), 1.1, 0.0),
        ("1e3, one +1", outlier(1e3, 1.0, n - 1), 1.0, 0.0),
        ("1e4, one +100", outlier(C4, 100.0, (n // 2 + 7) % n), 1.0, 0.0),
        ("constant 2", torch.full((n,), 2.0, dtype=torch.float64), 1.0, 0.25),
        ("gamma < 0, large beta", 3 * torch.randn(n, generator=g, dtype=torch.float64) - 2, -1.7, 40.0),
    ]


def _check_bn_bound(name, v, gamma, beta, scale, shift, bound, tight, report):
    """v: the channel's fp32 values (fp64 tensor); scale / shift / bound: what the kernel wrote.  Sound for every act
    (fp64 of the kernel's own coefficients, one fp32 ulp of slack for fma against separate rounding), tight where the
    statistics are well conditioned, never beyond 2^16 of the true maximum."""
    b, sc, sh = float(bound), float(scale), float(shift)
    n = v.numel()
    sigma, mu = float(v.std(unbiased=False)), float(v.mean())
    for act, f in ACTS.items():
        m = float(f(v * sc + sh).abs().max())
        assert b >= m * (1 - 2.0 ** -23), f"{name}, act {act}: bound {b} below max {m} (scale {sc}, shift {sh})"
        if m > 0:
            assert math.isfinite(b) and b <= USELESS * m, f"{name}, act {act}: bound {b} useless for max {m}"
            report.append(b / m)
    if tight and abs(mu) <= 8 * sigma:
        assert b <= 1.01 * (abs(gamma) * math.sqrt(n) + abs(beta)), f"{name}: bound {b} looser than 1.01 (|g| sqrt(n) + |b|)"
    return b


@pytest.mark.parametrize("n,k", [(16384, 256), (2, 1), (3, 3), (32768, 64), (32768, 4), (65536, 8)])
def test_bn_finalize_bound_is_sound_and_tight(n, k):
    """vg_bn_finalize_stats' act_amax from hand-made fp32 slots: <= 64 slots (one launch), 65..4096 (the wide kernel),
    > 4096 (two stages); vg_bn_stats' from a pass over the same tensor.  The 1e3 / 1e4 channels cancel: the computed
    variance is 0 while the true one is not, 1/std is 1/sqrt(eps), and their normalised outlier reaches 316 / 3.2e4.
    The Samuelson extreme (one nonzero element) is where the exact maximum reaches the bound: within 1 %."""
    g = torch.Generator().manual_seed(n + k)
    chans = _channels(n, g)
    C = len(chans)
    v32 = torch.stack([c[1] for c in chans]).float()                    # (C, n): the fp32 values
    v64 = v32.double()
    gamma = torch.tensor([c[2] for c in chans], dtype=torch.float32).cuda()
    beta = torch.tensor([c[3] for c in chans], dtype=torch.float32).cuda()
    stats = _fp32_slot_sums(v32, k)
    nslots = n // k
    B = min(n, 32)
    HW = n // B
    x = v32.view(C, B, HW).permute(1, 0, 2).contiguous().view(B, C, HW, 1).cuda()     # NCHW, channel c holds v32[c]
    ratios = []
    for how in ("slots", "pass"):
        per_channel = []
        for c, (name, _, gm, bt) in enumerate(chans):
            tight = name in ("N(0,1)", "Samuelson extreme", "offset 7.5", "gamma < 0, large beta")
            if how == "slots":
                mean, invstd, sc, sh, bound = ops.bn_finalize_stats(stats[:, c:c + 1].contiguous(), n, gamma[c:c + 1],
                                                                     beta[c:c + 1], None, None, 1e-5, 0.1, want_bound=True)
            else:
                mean, invstd, sc, sh, bound = ops.bn_stats(x[:, c:c + 1].contiguous(), gamma[c:c + 1], beta[c:c + 1],
                                                           None, None, 1e-5, 0.1, want_bound=True)
            b = _check_bn_bound(f"{how} n={n} slots={nslots} {name}", v64[c], gm, bt, sc, sh, bound,
                                tight, ratios)
            # the consumer's own fp32 arithmetic never exceeds it either
            y = ops.affine_act(x[:, c:c + 1].contiguous(), sc, sh, 0)
            assert float(y.abs().max()) <= b, (how, name)
            if name == "Samuelson extreme":                              # the bound really is at the edge
                assert _exact_max(y) >= 0.99 * b, (how, n, _exact_max(y), b)
            per_channel.append(b)
        # all channels in one launch: the maximum of the per-channel bounds (and the same coefficients)
        if how == "slots":
            out = ops.bn_finalize_stats(stats, n, gamma, beta, None, None, 1e-5, 0.1, want_bound=True)
        else:
            out = ops.bn_stats(x, gamma, beta, None, None, 1e-5, 0.1, want_bound=True)
        assert float(out[4]) == max(per_channel), (how, float(out[4]), per_channel)
    print(f"\nBN bound n={n} slots={nslots}: bound / true max in [{min(ratios):.4f}, {max(ratios):.1f}]")


# ------------------------------------------------------------------ (c) through the fused BatchNorm -> convolution
def _bn_conv_case(x, stats_in, seed, B_ref):
    """bn_act_conv (BNConvFn) on x with the given slots, forward + backward: everything finite, the output equal (fp64,
    image by image for the images in B_ref) to the convolution of act(x * scale + shift) with the kernel's own
    coefficients (the same slots through vg_bn_finalize_stats again: deterministic)."""
    # (bounds and finiteness only: the six gradients are compared with an fp64 reference in tests/test_fused_functions_gpu.py)
    g = torch.Generator(device="cuda").manual_seed(seed)
    Cin, Cout = x.shape[1], 256
    act = 2
    gamma = (1 + 0.1 * torch.randn(Cin, device="cuda", generator=g)).requires_grad_()
    beta = (0.1 * torch.randn(Cin, device="cuda", generator=g)).requires_grad_()
    w = (torch.randn(Cout, Cin, 5, 5, device="cuda", generator=g) / (Cin * 25) ** 0.5).requires_grad_()
    bias = torch.randn(Cout, device="cuda", generator=g).requires_grad_()
    xg = x.clone().requires_grad_()
    y, _ = HF.bn_act_conv(xg, gamma, beta, None, None, 1e-5, 0.1, act, w, bias, 2, stats_in=stats_in)
    gy = torch.randn(y.shape, device="cuda", generator=g)
    y.backward(gy)
    for name, t in (("y", y), ("dx", xg.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad), ("dw", w.grad),
                    ("dbias", bias.grad)):
        assert bool(torch.isfinite(t).all()), name
    count = x.numel() // Cin
    with torch.no_grad():
        if stats_in is not None:
            _, _, sc, sh, bound = ops.bn_finalize_stats(stats_in, count, gamma, beta, None, None, 1e-5, 0.1, want_bound=True)
        else:
            _, _, sc, sh, bound = ops.bn_stats(x, gamma, beta, None, None, 1e-5, 0.1, want_bound=True)
    a = ACTS[act](x[B_ref].double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    assert float(bound) >= float(a.abs().max()) * (1 - 2.0 ** -23)
    ref = O.conv5x5(a.cpu(), w.detach().cpu(), bias.detach().cpu(), 2)
    got = y.detach()[B_ref].cpu().double()
    err = float((got - ref).norm() / ref.norm())
    assert err <= CONV_TOL, f"rel L2 {err:.3e}"
    return float(bound), float(a.abs().max())


def test_fused_bn_conv_with_cancelling_slots():
    """Channels at 1e4 (C4) with one element at +100 (n = 32 * 16 * 16, 128 slots of 64: the wide finalize kernel): the
    slots' variance cancels to 0, the normalised outlier is ~3.2e4.  The bound the convolution (and, in backward, its
    weight gradient) scales the operand by must cover it: before, it was ~|gamma| sqrt(n) ~ 90 and the layer's output
    was inf."""
    B, Cin, Hs = 32, 128, 16
    x = torch.full((B, Cin, Hs, Hs), C4)
    x[5, :, 7, 9] += 100.0
    v = x.permute(1, 0, 2, 3).reshape(Cin, -1)
    stats = _fp32_slot_sums(v, 64)
    b, m = _bn_conv_case(x.cuda(), stats, 81, [5, 0])
    assert m > 1e4, m                          # the case does reach the cancellation (1/std ~ 1/sqrt(eps))
    print(f"\nfused BN-conv, cancelling slots: bound {b:.4g}, true max {m:.4g}")


def test_fused_bn_conv_with_real_epilogue_slots():
    """The same with the slots a convolution epilogue wrote: a mostly-zero input, a bias of 1e4, one nonzero pixel."""
    g = torch.Generator(device="cuda").manual_seed(82)
    B, Cin0, Cin, Hs = 128, 32, 128, 64           # the encoder's convs.2 launch (stride 2 -> 32 x 32): epilogue slots
    x0 = torch.zeros(B, Cin0, Hs, Hs, device="cuda")
    x0[3, :, 22, 41] = torch.randn(Cin0, device="cuda", generator=g)
    w0 = torch.randn(Cin, Cin0, 5, 5, device="cuda", generator=g) / (Cin0 * 25) ** 0.5
    b0 = torch.full((Cin,), 1e4, device="cuda")
    x, stats = ops.conv5x5_fwd(x0, w0, b0, 2, want_stats=True)
    assert stats is not None
    b, m = _bn_conv_case(x, stats, 83, [3, 0])
    print(f"\nfused BN-conv, epilogue slots: bound {b:.4g}, true max {m:.4g}")


# ------------------------------------------------------------------ (d) every bound of a real iteration
def _consumer_max(t, in_affine):
    t = t.detach()
    if in_affine is None:
        return t.abs().max().double()
    sc, sh, act = in_affine[:3]
    shp = (1, -1) + (1,) * (t.dim() - 2)
    return ACTS[int(act)](t.double() * sc.double().view(shp) + sh.double().view(shp)).abs().max()


@pytest.mark.parametrize("B", [16, 128])
def test_every_bound_of_a_training_iteration(B):
    """BetaVAEGANTrainer, eager, two iterations (the second reads the Linear-weight bounds HipAdam emitted): every bound
    ops.amax_of / ops.weight_bound hands out is compared with the exact maximum of what its consumer reads, recorded on
    the stream when the bound is handed out."""
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
    from oracle import steps as osteps
    recs = []
    measured = set()
    orig_amax, orig_wb = ops.amax_of, ops.weight_bound

    def amax_spy(t, in_affine=None):
        if in_affine is not None and len(in_affine) > 3 and in_affine[3] is not None:
            origin = "in_affine"
        else:
            known = ops.known_amax(t, in_affine)
            origin = "producer" if known is not None and known.data_ptr() not in measured else "measured"
        slot = orig_amax(t, in_affine)
        if origin == "measured":
            measured.add(slot.data_ptr())
        recs.append((origin, tuple(t.shape), slot.clone(), _consumer_max(t, in_affine)))
        return slot

    def wb_spy(w):
        ent = ops._weight_bound_entry(w)
        origin = "adam" if ent is not None and ent.emitted else "measured"
        slot = orig_wb(w)
        recs.append((origin, tuple(w.shape), slot.clone(), w.detach().abs().max().double()))
        return slot

    tr = BetaVAEGANTrainer(device="cuda:0", graph=False)
    batches = [osteps.synthetic_batch(B, seed=s) for s in (1234, 1235)]
    try:
        ops.amax_of, ops.weight_bound = amax_spy, wb_spy
        for b in batches:
            out = tr.step(*(b[k].cuda() for k in ("data", "noise", "eps2", "eps3")))
            assert all(math.isfinite(float(v)) for v in out.values())
    finally:
        ops.amax_of, ops.weight_bound = orig_amax, orig_wb
    torch.cuda.synchronize()
    worst, count = 0.0, {}
    for origin, shape, slot, m in recs:
        bnd, mx = float(slot), float(m)
        count[origin] = count.get(origin, 0) + 1
        assert bnd >= mx * (1 - 2.0 ** -23), (origin, shape, bnd, mx)
        if mx > 0:
            assert math.isfinite(bnd) and bnd <= USELESS * mx, (origin, shape, bnd, mx)
            worst = max(worst, bnd / mx)
    print(f"\naudit B={B}: {len(recs)} bounds checked {count}, largest bound / true max {worst:.2f}")
    # Deterministic counts, the same before and after the bounds' bookkeeping moved from ids and addresses to objects: a
    # changed one means an absmax launch (or a producer's bound) appeared or vanished.
    assert count == {16: dict(measured=51, producer=112, in_affine=76, adam=25),
                     128: dict(measured=79, producer=112, in_affine=76, adam=25)}[B], count
