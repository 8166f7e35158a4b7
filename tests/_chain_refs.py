"""fp64 reference for chains of [5x5 conv | transposed conv | train-mode BatchNorm + activation] and the seeded cases
the CPU and the GPU tests of the fused conv-BatchNorm Functions share (tests/test_chain_refs_cpu.py,
tests/test_fused_functions_gpu.py).  A plain module: nothing here touches a GPU or reads a file.

The reference is plain torch on the CPU with autograd, the operations as oracle/ops.py states them:
F.conv2d(padding=2, stride=s); F.conv_transpose2d(padding=2, stride=s, output_padding=s-1);
F.batch_norm(training=True, momentum, eps) on cloned running buffers; relu / leaky_relu(0.2).  `run` evaluates a case
in ``dtype`` (fp64: the reference; fp32: the same chain as an honest fp32 evaluation, whose distance from fp64 the CPU
test records next to every ceiling below).

Ceilings -- none of them new, all relative L2 with the max-abs guard of `rel_err` / tests/test_kernels_gpu.py:
  CONV_TOL 3e-6   convolution outputs against fp64 (test_kernels_gpu.CONV_TOL); gw / gb of a chain's last convolution,
                  whose gy is exact
  STAT_TOL 3e-6   running statistics (test_bn_shapes, test_bn_coefficients_from_stats_and_from_pass); the saved batch
                  mean and 1/std, which the running statistics are an affine function of
  BN_TOL   2e-5   gx / dgamma / dbeta of a BatchNorm (test_bn_shapes) and every gradient that passes through a
                  BatchNorm backward: the loosest link

Units near zero.  A pre-activation whose sign differs between fp32 and fp64 moves a ReLU / LeakyReLU gradient by a
whole unit.  No case has one: every fp64 pre-activation of every BatchNorm is farther than MARGIN * max |pre| (over
its channel) from zero -- `margin` measures it, the CPU test asserts it for every case, the GPU test again before it
compares anything.  A case that violates it gets another seed; no element is ever masked.
"""
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

CONV_TOL, STAT_TOL, BN_TOL = 3e-6, 3e-6, 2e-5
MARGIN = 2.0 ** -14
ACTS = {"none": 0, "relu": 1, "lrelu": 2}      # VG_ACT_*


class Conv(NamedTuple):
    cin: int
    cout: int
    stride: int
    transposed: bool = False


class BN(NamedTuple):
    c: int
    act: str
    eps: float = 1e-5
    momentum: float = 0.1
    running: bool = True        # False: running_mean = running_var = None


class Route(NamedTuple):
    """What ops.route_conv must say of a convolution layer's launches under the split arithmetics (fp16x3, bf16x6);
    under "fp32" every launch is an FP32_* family, applies nothing on load and leaves no statistics."""
    family: str                 # forward launch: "split" | "thin"
    affine_on_load: bool        # forward launch, asked with the producing BatchNorm as the operand's affine
    stats: bool                 # forward launch: stats_floats > 0
    wgrad: Optional[str] = None # layers that read a BatchNorm: family of the weight gradient, which applies the affine on
                                # load ("split" | "thin") or takes the operand materialised ("fp32_plain")


class Case(NamedTuple):
    name: str
    shape: Tuple[int, ...]      # of the chain's input
    layers: tuple
    seed: int
    routes: tuple = ()          # one Route per Conv layer, in order
    uses: int = 1               # inputs that go through the same layers before one backward


# Shapes: the smallest that reach each path.
# * Channels 16 / 32: a ring launch (conv_ring.hip) splits K only from 64 input channels on (a split needs >= 2 chunks of
#   16 channels per part), so a stride-2 convolution of 16 or 32 input channels leaves its statistics slots at ANY batch
#   -- batches 2..4 here; the "batch 8 is K-split" of test_fused_conv_bn_equals_two_pass_batchnorm is about the model's
#   64..256-channel layers.
# * The split weight gradient (wgrad_bf16split.hip: the one that applies the affine on load) takes whole 1 x 8 output
#   tiles only, i.e. an output width that is a multiple of 8.  Stride 2: a 16-wide BatchNorm input, so the producer in
#   front of it reads 8 x 32 images (4 x 16 after it, 2 x 8 at the end: the width leaves the 8..16 range, the tensors
#   stay the smallest there are).  Stride 1: 8 x 8.
# * A stride-1 forward convolution never fuses (vg_conv5x5_bf16split_fusable: stride 2 only): its BatchNorm is
#   materialised by ops._materialize in forward and read on load by the weight gradient in backward.
# * A transposed convolution fuses on the ring kernel only, which takes stride 2 and more than 64 output channels: 80 is
#   the smallest ragged count above that.  The thin 32 -> 3 transposed kernel needs W % 16 == 0 (conv_thin_mfma.hip)
#   and any H: 8 x 16 images.
# * "twice", "asked", "modules": a stride-2 layer on 8 x 8 -- the fused forward with the exact-fp32 weight gradient
#   (output width 4), which takes the BatchNorm materialised and, for "twice", adds into the first pass's tensor.
def _fwd(name, act, stride, seed, **bn):
    shape, second = ((2, 16, 8, 32), Route("split", True, True, "split")) if stride == 2 else \
        ((3, 16, 16, 16), Route("split", False, False, "split"))
    return Case(name, shape, (Conv(16, 32, 2), BN(32, act, **bn), Conv(32, 32, stride)), seed,
                (Route("split", False, True), second))


FWD_CASES = (
    _fwd("fwd_s2_relu", "relu", 2, 1),
    _fwd("fwd_s2_lrelu", "lrelu", 2, 2, eps=1e-3, momentum=0.3),
    _fwd("fwd_s2_none", "none", 2, 3, running=False),
    _fwd("fwd_s1_relu", "relu", 1, 8, running=False),
    _fwd("fwd_s1_lrelu", "lrelu", 1, 6),
    _fwd("fwd_s1_none", "none", 1, 9, eps=1e-3, momentum=0.3),
)
T_RING = Case("convT_ring", (2, 16, 4, 4), (Conv(16, 32, 2, True), BN(32, "relu"), Conv(32, 80, 2, True)), 16,
              (Route("split", False, False), Route("split", True, True, "split")))
T_THIN = Case("convT_thin", (2, 16, 2, 4),
              (Conv(16, 32, 2, True), BN(32, "relu", eps=1e-3, momentum=0.3), Conv(32, 32, 2, True), BN(32, "relu"),
               Conv(32, 3, 1, True)), 26,
              (Route("split", False, False), Route("split", False, False, "split"), Route("thin", True, False, "thin")))
LAST_BN_CASES = (
    Case("last_bn_conv", (4, 16, 16, 16), (Conv(16, 32, 2), BN(32, "lrelu", eps=1e-3, momentum=0.3)), 25,
         (Route("split", False, True),)),
    Case("last_bn_convT", (2, 32, 4, 4), (Conv(32, 80, 2, True), BN(80, "relu")), 28, (Route("split", False, True),)),
)
BN1D = Case("bn1d", (6, 40), (BN(40, "relu"),), 23)
ASKED = Case("asked", (4, 32, 8, 8), (BN(32, "lrelu"), Conv(32, 32, 2)), 33, (Route("split", True, True, "fp32_plain"),))
TWICE = Case("twice", (2, 16, 16, 16), (Conv(16, 32, 2), BN(32, "lrelu"), Conv(32, 32, 2)), 43,
             (Route("split", False, True), Route("split", True, True, "fp32_plain")), uses=2)
MODULES = Case("modules", (4, 16, 16, 16),
               (Conv(16, 32, 2), BN(32, "lrelu"), Conv(32, 32, 2), BN(32, "relu")), 57,
               (Route("split", False, True), Route("split", True, True, "fp32_plain")))
TINY = Case("tiny", (2, 2, 4, 4), (Conv(2, 3, 2), BN(3, "lrelu"), Conv(3, 2, 1)), 61)      # the CPU test's gradcheck

GPU_CASES = FWD_CASES + (T_RING, T_THIN) + LAST_BN_CASES + (BN1D, ASKED, TWICE, MODULES)
ALL_CASES = GPU_CASES + (TINY,)


def out_shape(case):
    shape = tuple(case.shape)
    for L in case.layers:
        if isinstance(L, Conv):
            B, _, H, W = shape
            s = L.stride
            shape = (B, L.cout, H * s, W * s) if L.transposed else (B, L.cout, (H - 1) // s + 1, (W - 1) // s + 1)
    return shape


def make_inputs(case):
    """Seeded fp32 inputs of a case: ``xs`` / ``gys`` (one per use), ``params`` (one dict per layer: w, b of a
    convolution -- filters scaled for unit-variance outputs --; gamma, beta and non-trivial running buffers rm, rv of a
    BatchNorm, None where the case runs without)."""
    g = torch.Generator().manual_seed(1000 + case.seed)

    def randn(*s):
        return torch.randn(*s, generator=g)
    params = []
    for L in case.layers:
        if isinstance(L, Conv):
            wshape = (L.cin, L.cout, 5, 5) if L.transposed else (L.cout, L.cin, 5, 5)
            params.append(dict(w=randn(*wshape) / (L.cin * 25 / (L.stride ** 2 if L.transposed else 1)) ** 0.5,
                               b=0.5 * randn(L.cout)))
        else:
            rm = 0.3 * randn(L.c) if L.running else None
            rv = 0.5 + torch.rand(L.c, generator=g) if L.running else None
            params.append(dict(gamma=1 + 0.2 * randn(L.c), beta=0.3 * randn(L.c), rm=rm, rv=rv))
    xs = [1.5 * randn(*case.shape) + 0.25 for _ in range(case.uses)]
    gys = [randn(*out_shape(case)) for _ in range(case.uses)]
    return dict(xs=xs, gys=gys, params=params)


def _act(z, act):
    return z if act == "none" else (F.relu(z) if act == "relu" else F.leaky_relu(z, 0.2))


def chain_forward(layers, x, params, bufs=None, taps=None):
    """The chain on ``x`` with ``params`` (one dict per layer, tensors of x's dtype).  ``bufs``: per BatchNorm layer a
    dict of running buffers rm / rv updated in place (None: batch statistics only).  ``taps``: a dict that receives,
    per BatchNorm layer index, the detached pre-activation and the batch mean and 1/std (`run` adds ``gin``, the
    gradient with respect to the BatchNorm's input, where a convolution produced it)."""
    t = x
    for i, (L, p) in enumerate(zip(layers, params)):
        if isinstance(L, Conv):
            if L.transposed:
                t = F.conv_transpose2d(t, p["w"], p["b"], stride=L.stride, padding=2, output_padding=L.stride - 1)
            else:
                t = F.conv2d(t, p["w"], p["b"], stride=L.stride, padding=2)
        else:
            b = bufs[i] if bufs is not None else dict(rm=None, rv=None)
            z = F.batch_norm(t, b["rm"], b["rv"], p["gamma"], p["beta"], True, L.momentum, L.eps)
            if taps is not None:
                dims = [0] + list(range(2, t.dim()))
                td = t.detach()
                taps[i] = dict(pre=z.detach(), mean=td.mean(dims),
                               invstd=(td.var(dims, unbiased=False) + L.eps).rsqrt())
                if t.requires_grad and not t.is_leaf:
                    t.retain_grad()
                    taps[i]["_in"] = t
            t = _act(z, L.act)
    return t


def run(case, inp, dtype=torch.float64, used=None):
    """The case in ``dtype`` with autograd: every use of the layers in order (running buffers go through all of them),
    loss = sum over the uses of <y, gy>; ``used[u]`` False: use u is run but its output does not reach the loss.
    Returns dict(ys, gxs -- None for an unused use --, grads: per layer {w, b} / {gamma, beta}, bufs: per layer
    {rm, rv} after the run (None for a convolution), taps: per use {layer index: pre, mean, invstd})."""
    used = [True] * case.uses if used is None else list(used)
    leaf = lambda t: t.detach().to(dtype).requires_grad_()          # noqa: E731
    params = [{k: leaf(v) for k, v in p.items() if k in ("w", "b", "gamma", "beta")} for p in inp["params"]]
    bufs = [None if isinstance(L, Conv) else
            {k: (None if p[k] is None else p[k].detach().to(dtype).clone()) for k in ("rm", "rv")}
            for L, p in zip(case.layers, inp["params"])]
    xs = [leaf(x) for x in inp["xs"]]
    ys, taps, loss = [], [], 0.0
    for u, x in enumerate(xs):
        taps.append({})
        y = chain_forward(case.layers, x, params, bufs, taps[-1])
        ys.append(y.detach())
        if used[u]:
            loss = loss + (y * inp["gys"][u].to(dtype)).sum()
    loss.backward()
    for tp in taps:
        for tap in tp.values():
            if "_in" in tap:
                tap["gin"] = tap.pop("_in").grad      # gradient w.r.t. the BatchNorm's input (None: unused use)
    return dict(ys=ys, gxs=[x.grad for x in xs], grads=[{k: v.grad for k, v in p.items()} for p in params],
                bufs=bufs, taps=taps, loss=loss.detach())


def margin(ref):
    """min over every use, BatchNorm and channel of min |pre| / max |pre| (fp64 pre-activations of `run`)."""
    worst = float("inf")
    for taps in ref["taps"]:
        for tap in taps.values():
            a = tap["pre"].abs().transpose(0, 1).reshape(tap["pre"].shape[1], -1)
            worst = min(worst, float((a.min(1).values / a.max(1).values).min()))
    return worst


def rel_err(got, ref):
    """(relative L2, max |got - ref| / max |ref|) in fp64 on the CPU."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    d = got - ref
    return float(d.norm() / max(float(ref.norm()), 1e-300)), float(d.abs().max() / max(float(ref.abs().max()), 1e-300))


def last_conv(case):
    """Index of the convolution whose gy is the loss's own gradient (the chain ends in it), or None."""
    return len(case.layers) - 1 if isinstance(case.layers[-1], Conv) else None


def through_bn(case, i):
    """Whether the gradient of layer i's parameters has passed through a BatchNorm backward."""
    return any(isinstance(L, BN) for L in case.layers[i + (1 if isinstance(case.layers[i], Conv) else 0):])


def quantities(case, res):
    """Flat {name: (tensor, ceiling)} of everything `run` returns that a test compares: outputs and input gradients
    per use, parameter gradients and running buffers per layer, saved statistics per use and BatchNorm.  The bias of a
    convolution that feeds a BatchNorm is left out here: its gradient is analytically zero (rounding noise in any
    arithmetic, no relative error to speak of) and is judged on its own by the tests."""
    has_bn = any(isinstance(L, BN) for L in case.layers)
    q = {}
    for u in range(case.uses):
        q[f"y{u}"] = (res["ys"][u], CONV_TOL)
        if res["gxs"][u] is not None:
            q[f"gx{u}"] = (res["gxs"][u], BN_TOL if has_bn else CONV_TOL)
        for i, tap in res["taps"][u].items():
            q[f"mean{u}.{i}"] = (tap["mean"], STAT_TOL)
            q[f"invstd{u}.{i}"] = (tap["invstd"], STAT_TOL)
    for i, L in enumerate(case.layers):
        tol = BN_TOL if through_bn(case, i) else CONV_TOL
        for k, v in res["grads"][i].items():
            if k == "b" and shadowed(case, i):
                continue
            q[f"g{k}.{i}"] = (v, tol)
        if res["bufs"][i] is not None:
            for k, v in res["bufs"][i].items():
                if v is not None:
                    q[f"{k}.{i}"] = (v, STAT_TOL)
    return q


def shadowed(case, i):
    """Layer i is a convolution whose output goes straight into a BatchNorm (its bias gradient is analytically 0)."""
    return isinstance(case.layers[i], Conv) and i + 1 < len(case.layers) and isinstance(case.layers[i + 1], BN)


def check_routes(case, ops):
    """Asserts, host only, that under ops.CONV_ARITH as it is now every convolution of the case takes the route its
    `Route` states -- forward launch (family, affine on load, statistics) and, for a layer that reads a BatchNorm, the
    weight gradient -- and returns [(forward ConvRoute, weight-gradient ConvRoute or None)] per convolution."""
    split = ops.CONV_ARITH != "fp32"
    shape, out, prev_bn = tuple(case.shape), [], False
    convs = iter(case.routes)
    for L in case.layers:
        if not isinstance(L, Conv):
            prev_bn = True
            continue
        want = next(convs)
        B, _, H, W = shape
        s = L.stride
        full = (B, L.cin, H, W, L.cout, s)
        r = ops.route_conv("convT_fwd" if L.transposed else "conv_fwd", *full, affine="x" if prev_bn else None, want_stats=True)
        what = (case.name, ops.CONV_ARITH, L, r)
        if split:
            assert r.family == want.family, what
            assert r.affine_on_load == (want.affine_on_load and prev_bn), what
            assert (r.stats_floats > 0) == want.stats, what
            assert ops.conv_fusable(L.transposed, L.cin, L.cout, s) == (want.stats or (want.affine_on_load and want.family == "split")), what
        else:
            assert r.family.startswith("fp32") and not r.affine_on_load and r.stats_floats == 0, what
            assert not ops.conv_fusable(L.transposed, L.cin, L.cout, s), what
        shape = (B, L.cout, H * s, W * s) if L.transposed else (B, L.cout, (H - 1) // s + 1, (W - 1) // s + 1)
        rw = None
        if prev_bn:
            # a transposed layer's weight gradient is that of the convolution gy -> x: the layer's input is its "gy"
            wshape = (B, L.cout) + shape[2:] + (L.cin, s) if L.transposed else full
            rw = ops.route_conv("conv_wgrad", *wshape, affine="gy" if L.transposed else "x")
            what = (case.name, ops.CONV_ARITH, L, rw)
            if split:
                assert rw.family == want.wgrad and rw.affine_on_load == (want.wgrad != "fp32_plain"), what
            else:
                assert rw.family == "fp32_plain" and not rw.affine_on_load, what
        out.append((r, rw))
        prev_bn = False
    return out
