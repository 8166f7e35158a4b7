"""The autograd Functions of the fused conv-BatchNorm path -- functional.ConvStatsFn, BNConvFn, BNActFn(stats=...) and
model.run_conv_bn_chain over them -- against the fp64 chain reference of tests/_chain_refs.py, layer by layer.

The kernels underneath are each held to fp64 on their own (test_conv_input_affine_and_output_stats, test_bn_shapes,
test_wgrad_gpu.py, test_bounds_gpu.py); this file is about the composition: which operand the weight gradient reads the
BatchNorm through, which saved statistics the BatchNorm backward uses, what `needs_input_grad`, BIAS_GRAD_ZERO and the
`accumulate_param_grads` protocol make of the gradients, and how often a running statistic moves.

Every case (the table in _chain_refs.py) asserts before it launches that its convolutions take the kernel route the
table states (`check_routes`: family, affine on load, statistics slots, the weight gradient's family), and asserts the
near-zero condition (no fp64 pre-activation within 2^-14 max |pre| of zero) before it compares.  Every case runs in
three arithmetics: the default fp16x3, "fp32" (no kernel fuses: ops._materialize and the unfused fallbacks under the
same Functions) and "bf16x6".  No element is left out of a comparison and no bound depends on what was measured.

Ceilings (relative L2 with the max-abs guard of test_kernels_gpu.assert_close; _chain_refs.py says where each comes
from): y 3e-6; running statistics, saved mean / 1/std 3e-6; gx, dgamma, dbeta and gw / gb upstream of a BatchNorm 2e-5;
gw / gb of a chain's last convolution 3e-6.  The bias of a convolution that feeds a BatchNorm has an analytically zero
gradient: |gb[c]| <= 2e-5 * sum |g[c]| over the terms that cancel.  Each check prints its error before it asserts
(pytest -s); the worst per quantity and arithmetic is printed once at the end of the module.
"""
import math
from collections import defaultdict

import pytest
import torch

import _chain_refs as R
from test_losses_gpu import at_offset

pytestmark = pytest.mark.gpu

SOURCES = ("producer", "none", "empty")      # stats_in: the producing convolution's slots / None / an empty tensor
_ref, _worst = {}, defaultdict(float)


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


@pytest.fixture(scope="module")
def Fn():
    from disentangle_mlp_amd import functional
    return functional


@pytest.fixture(params=["default", "fp32", "bf16x6"])
def arith(request, H):
    """Every case three times: the product's default arithmetic (fp16x3), the exact fp32 kernels (nothing fuses) and
    bf16x6 -- as `conv_arith` of tests/test_kernels_gpu.py."""
    prev = H.CONV_ARITH
    if request.param != "default":
        H.CONV_ARITH = request.param
    yield H.CONV_ARITH
    H.CONV_ARITH = prev


@pytest.fixture(scope="module", autouse=True)
def worst_errors():
    yield
    print("\nworst error per quantity and arithmetic (relative L2):")
    for (kind, a), e in sorted(_worst.items()):
        print(f"  {kind:8s} {a:7s} {e:.2e}")


def ref_of(case, used=None):
    """(inputs, fp64 reference) of a case, computed once and never changed; the near-zero condition is asserted here,
    before anything is compared."""
    key = (case.name, None if used is None else tuple(used))
    if key not in _ref:
        inp = R.make_inputs(case)
        ref = R.run(case, inp, used=used)
        assert R.margin(ref) > R.MARGIN, (case.name, case.seed, R.margin(ref))
        _ref[key] = (inp, ref)
    return _ref[key]


def check(got, want, tol, what, arith):
    e, m = R.rel_err(got, want)
    kind = what.split()[-1].rstrip("0123456789.")
    _worst[(kind, arith)] = max(_worst[(kind, arith)], e)
    print(f"{what}: rel L2 {e:.2e}, max abs {m:.2e} of max |ref| (ceiling {tol:.0e})")
    assert math.isfinite(e) and e <= tol, f"{what}: rel L2 {e:.3e} > {tol:.1e}"
    assert m <= 50 * tol, f"{what}: max abs err {m:.3e} of max |ref|"


def leaves(inp, requires=lambda i, k: True):
    """The parameters on the device, one dict per layer: leaves for w, b, gamma, beta (requires(i, k): with gradient),
    fresh copies of the running buffers."""
    return [{k: (None if v is None else v.cuda().clone().requires_grad_(k not in ("rm", "rv") and requires(i, k)))
             for k, v in p.items()} for i, p in enumerate(inp["params"])]


def run_functions(Fn, H, case, x, P, source="producer", bias_grad=None):
    """The case's layers on x by the Functions, as model.run_conv_bn_chain strings them: a convolution behind a BatchNorm
    is ONE bn_act_conv call, a convolution without one a conv_with_stats call, a BatchNorm at the end batch_norm_act.
    ``source``: what a BatchNorm gets as statistics slots.  Returns (y, {BatchNorm layer index: the tensor whose grad_fn
    saved that BatchNorm's mean and 1/std})."""
    routes = iter(R.check_routes(case, H))

    def pick(stats, t):
        if source == "producer":
            return stats
        return None if source == "none" else t.new_empty(0)
    t, stats, pending, heads = x, None, None, {}
    for i, L in enumerate(case.layers):
        p = P[i]
        if isinstance(L, R.BN):
            pending = (i, L)
            continue
        bg = Fn.BIAS_GRAD_COMPUTE if bias_grad is None else bias_grad
        route = next(routes)[0]
        if pending is None:
            t, stats = Fn.conv_with_stats(t, p["w"], p["b"], L.stride, L.transposed, bg)
        else:
            j, N = pending
            q = P[j]
            t, stats = Fn.bn_act_conv(t, q["gamma"], q["beta"], q["rm"], q["rv"], N.eps, N.momentum, R.ACTS[N.act],
                                      p["w"], p["b"], L.stride, L.transposed, bg, pick(stats, t))
            heads[j], pending = t, None
        assert stats.numel() == route.stats_floats and not stats.requires_grad, (case.name, L, stats.shape, route)
    if pending is not None:
        j, N = pending
        q = P[j]
        t = Fn.batch_norm_act(t, q["gamma"], q["beta"], q["rm"], q["rv"], N.eps, N.momentum, R.ACTS[N.act],
                              pick(stats, t))
        heads[j] = t
    return t, heads


def saved_stats(heads):
    """{BatchNorm index: dict(mean, invstd)} from the Functions' saved tensors (read before backward frees them)."""
    out = {}
    for j, t in heads.items():
        sv = t.grad_fn.saved_tensors          # BNActFn / BNConvFn: (x, gamma, beta, mean, invstd, ...)
        out[j] = dict(mean=sv[3].clone(), invstd=sv[4].clone())
    return out


def result(case, ys, xs, P, taps):
    """What the Functions produced, in the layout of `_chain_refs.run`."""
    return dict(ys=ys, gxs=[x.grad for x in xs],
                grads=[{k: p[k].grad for k in p if k not in ("rm", "rv")} for p in P],
                bufs=[None if isinstance(L, R.Conv) else {k: p[k] for k in ("rm", "rv")} for L, p in zip(case.layers, P)],
                taps=taps)


def run_case(Fn, H, case, inp, source="producer", bias_grad=None, requires=lambda i, k: True, x_grad=True, ctx=None,
             used=None, extra_loss=None):
    """Forward of every use, one backward of sum <y, gy> over the used ones, inside ``ctx`` (e.g.
    accumulate_param_grads) when given."""
    import contextlib
    used = [True] * case.uses if used is None else used
    P = leaves(inp, requires)
    xs = [x.cuda().clone().requires_grad_(x_grad) for x in inp["xs"]]
    with (ctx() if ctx is not None else contextlib.nullcontext()):
        ys, taps, loss = [], [], None
        for u, x in enumerate(xs):
            y, heads = run_functions(Fn, H, case, x, P, source, bias_grad)
            taps.append(saved_stats(heads))
            ys.append(y)
            term = (y * inp["gys"][u].cuda()).sum() if used[u] else (extra_loss(y) if extra_loss is not None else None)
            if term is not None:
                loss = term if loss is None else loss + term
        loss.backward()
    torch.cuda.synchronize()
    return result(case, [y.detach() for y in ys], xs, P, taps)


def compare(case, got, ref, arith, label, absent=()):
    """Every quantity of the reference against what the Functions gave; ``absent``: names that must be None (autograd
    did not ask, or BIAS_GRAD_ZERO)."""
    qr, qg = R.quantities(case, ref), R.quantities(case, got)
    for name, (want, tol) in qr.items():
        if name in absent:
            assert name not in qg or qg[name][0] is None, f"{label} {name}: a gradient nobody asked for"
            continue
        assert name in qg and qg[name][0] is not None, f"{label}: {name} is missing"
        check(qg[name][0], want, tol, f"{case.name} [{arith}] {label} {name}", arith)
    # biases in front of a BatchNorm: analytically zero, |gb[c]| <= BN_TOL * sum of the |terms| that cancel
    for i, L in enumerate(case.layers):
        if not R.shadowed(case, i) or f"gb.{i}" in absent:
            continue
        gb = got["grads"][i]["b"]
        assert gb is not None, f"{label}: gb.{i} is missing"
        gins = [ref["taps"][u][i + 1]["gin"] for u in range(case.uses) if ref["taps"][u][i + 1].get("gin") is not None]
        mag = sum(g.abs().sum(dim=[0] + list(range(2, g.dim()))) for g in gins)
        ratio = float((gb.detach().cpu().double().abs() / mag).max())
        print(f"{case.name} [{arith}] {label} gb.{i} (analytically 0): max |gb| / sum |terms| = {ratio:.2e} (ceiling {R.BN_TOL:.0e})")
        assert ratio <= R.BN_TOL, (label, i, ratio)


# ------------------------------------------------------------------------------------ 1. BNConvFn, forward convolution
@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c.name)
def test_bn_conv_forward(H, Fn, arith, case):
    """conv -> [BatchNorm + act -> conv] with the second pair one BNConvFn: stride 2 (fused on load, statistics from the
    producer's epilogue) and stride 1 (materialised forward, read on load by the split weight gradient), none / ReLU /
    LeakyReLU, default and non-default eps / momentum, with and without running buffers.  y, gx, dgamma, dbeta, gw, gb,
    running statistics and the saved mean / 1/std against fp64 for the three sources of statistics -- the producer's
    slots, None, an empty tensor: all three meet the same reference.
    Guards functional.BNConvFn: the statistics finalize / pass choice (`stats_in.numel()`), `aff=` handed to
    `_conv_backward` (without it gw is the weight gradient against the raw x), the saved mean / invstd that
    `_bn_backward` reads, and the running buffers moving exactly once per call."""
    inp, ref = ref_of(case)
    for source in SOURCES:
        got = run_case(Fn, H, case, inp, source)
        compare(case, got, ref, arith, source)


# ------------------------------------------------------------------------------------ 2. BNConvFn, transposed
@pytest.mark.parametrize("case", (R.T_RING, R.T_THIN), ids=lambda c: c.name)
def test_bn_conv_transposed(H, Fn, arith, case):
    """The decoder's direction.  convT_ring: ConvT -> BN + ReLU -> ConvT(32 -> 80, stride 2) on the ring kernel, fused
    on load.  convT_thin: two such layers (64 output channels or fewer: materialised) and then BN + ReLU ->
    ConvT(32 -> 3, stride 1) on the THIN route (vg_convT5x5_s1_thin_bf16split_ok takes 8 x 16 images), whose weight
    gradient (conv_thin_wgrad.hip) reads the BatchNorm through its gy operand.
    Guards `affine_on_gy=tr` in functional._conv_backward: a transposed layer's weight gradient is that of the
    convolution gy -> x, so the layer's input -- and with it the BatchNorm -- sits in the gy slot; with the affine on
    the other operand gw of the consuming layers (gw.2, gw.4) misses fp64 by O(1)."""
    inp, ref = ref_of(case)
    got = run_case(Fn, H, case, inp)
    compare(case, got, ref, arith, "producer")


# ------------------------------------------------------------------------------------ 3. ConvStatsFn -> BNActFn(stats=)
@pytest.mark.parametrize("case", R.LAST_BN_CASES, ids=lambda c: c.name)
def test_last_batchnorm_of_a_chain(H, Fn, arith, case):
    """A chain's last BatchNorm, materialised: ConvStatsFn -> BNActFn with the producer's slots (finalize + affine_act,
    no statistics pass) and without (stats=None and an empty tensor: the two-pass kernel) against the same reference.
    Guards BNActFn.forward's `stats is not None` branch (count, the saved mean / invstd of the finalize kernel that the
    backward reads) and ConvStatsFn.backward."""
    inp, ref = ref_of(case)
    for source in SOURCES:
        got = run_case(Fn, H, case, inp, source)
        compare(case, got, ref, arith, source)


def test_batchnorm1d_through_batch_norm_act(H, Fn):
    """HW == 1 (BatchNorm1d, (B, C) input) through batch_norm_act with stats=None: no bound is emitted or adopted."""
    inp, ref = ref_of(R.BN1D)
    got = run_case(Fn, H, R.BN1D, inp, "none")
    compare(R.BN1D, got, ref, H.CONV_ARITH, "bn1d")


# ------------------------------------------------------------------------------------ 4. what autograd asks for
ASKS = {
    # name: (x requires grad, which parameters do, names that must come back as None)
    "first_layer": (False, lambda i, k: True, ("gx0",)),
    "relay": (True, lambda i, k: False, ("ggamma.0", "gbeta.0", "gw.1", "gb.1")),
    "bn_only": (False, lambda i, k: k in ("gamma", "beta"), ("gx0", "gw.1", "gb.1")),
}


@pytest.mark.parametrize("ask", list(ASKS))
def test_what_autograd_asks_for(H, Fn, arith, ask):
    """BNConvFn with x a plain input and the parameters trained (a first layer), with every parameter frozen and only x
    asked for (the discriminator relaying to the decoder), with only gamma / beta asked for: what was not asked for is
    None, the rest meets the reference.
    Guards the `need[0] or need_p` argument in BNConvFn.backward ("first_layer", "bn_only": with `need[0]` alone the
    data gradient is skipped and dgamma / dbeta come back None) and `need[3]`, `need[4]` next to it."""
    case = R.ASKED
    x_grad, requires, absent = ASKS[ask]
    inp, ref = ref_of(case)
    got = run_case(Fn, H, case, inp, requires=requires, x_grad=x_grad)
    compare(case, got, ref, arith, ask, absent=absent)


def test_bias_grad_zero_changes_nothing_else(H, Fn, arith):
    """bias_grad=BIAS_GRAD_ZERO: the bias gets no gradient at all, everything else is bit for bit BIAS_GRAD_COMPUTE."""
    case = R.ASKED
    inp, ref = ref_of(case)
    a = run_case(Fn, H, case, inp, bias_grad=Fn.BIAS_GRAD_COMPUTE)
    b = run_case(Fn, H, case, inp, bias_grad=Fn.BIAS_GRAD_ZERO)
    compare(case, a, ref, arith, "compute")
    compare(case, b, ref, arith, "zero", absent=("gb.1",))
    assert b["grads"][1]["b"] is None
    qa, qb = R.quantities(case, a), R.quantities(case, b)
    for name in qa:
        if name != "gb.1":
            assert torch.equal(qa[name][0], qb[name][0]), name


# ------------------------------------------------------------------------------------ 5. a layer used twice
@pytest.mark.parametrize("mode", ["autograd_sums", "accumulate_param_grads"])
def test_layer_used_twice_before_one_backward(H, Fn, arith, mode):
    """Two inputs through the same conv -> BN + LeakyReLU -> conv (shared w, bias, gamma, beta, running buffers), one
    backward: plainly (autograd adds the two parameter gradients) and under functional.accumulate_param_grads() (the
    second pass adds inside its kernels and hands autograd None).  Both meet the fp64 sum of the two uses; the running
    statistics have moved exactly twice, in order, as in the reference.
    Guards the `slot.prev` hand-over in functional._bn_backward (without `accumulate_into=slot.prev` the second pass's
    dgamma / dbeta are dropped: half the gradient), `out=slot.prev, accumulate=True` in `_conv_backward` (ConvStatsFn
    and BNConvFn both carry the context), and `_grad_slot.hand_over`.
    functional.deferred_wgrad() is not run here: it covers LinearFn / LinearGroupedFn only (`ctx.defer` is set nowhere
    else; a convolution's weight gradient is never batched over passes)."""
    case = R.TWICE
    inp, ref = ref_of(case)
    ctx = Fn.accumulate_param_grads if mode == "accumulate_param_grads" else None
    got = run_case(Fn, H, case, inp, ctx=ctx)
    compare(case, got, ref, arith, mode)


# ------------------------------------------------------------------------------------ 6. an output that is not used
class _Swallow(torch.autograd.Function):
    """A consumer that hands its input NO gradient (None, not zeros) -- what LinearGroupedFn does for a pass that got
    none: the producing node then runs its backward with gy = None."""

    @staticmethod
    def forward(ctx, y):
        return y.new_zeros(())

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("how", ["pruned", "gy_is_none"])
@pytest.mark.parametrize("mode", ["autograd_sums", "accumulate_param_grads"])
def test_output_that_does_not_reach_the_loss(H, Fn, arith, how, mode, monkeypatch):
    """Two uses of the same layers; only the second one's output reaches the loss.  "pruned": the first output is
    dropped (autograd never visits its nodes).  "gy_is_none": it feeds a consumer that returns no gradient, so
    BNConvFn.backward and ConvStatsFn.backward ARE called, with gy = None (set_materialize_grads(False)) -- the early
    returns.  Backward completes, the unused use contributes nothing (its x has no gradient, the shared parameters'
    gradients equal the single-use reference), and its forward still moved the running statistics (twice in all).
    Guards the `if gy is None: return (None,) * n` lines of BNConvFn.backward and ConvStatsFn.backward."""
    case = R.TWICE
    inp, ref = ref_of(case, used=(False, True))
    seen = defaultdict(list)
    for cls in (Fn.BNConvFn, Fn.ConvStatsFn):
        orig = cls.backward

        def spy(ctx, gy, _s, orig=orig, name=cls.__name__):
            seen[name].append(gy is None)
            return orig(ctx, gy, _s)
        monkeypatch.setattr(cls, "backward", staticmethod(spy))
    ctx = Fn.accumulate_param_grads if mode == "accumulate_param_grads" else None
    got = run_case(Fn, H, case, inp, ctx=ctx, used=[False, True],
                   extra_loss=_Swallow.apply if how == "gy_is_none" else None)
    want_calls = [True, False] if how == "gy_is_none" else [False]
    assert sorted(seen["BNConvFn"]) == sorted(want_calls) and sorted(seen["ConvStatsFn"]) == sorted(want_calls), dict(seen)
    assert got["gxs"][0] is None
    compare(case, got, ref, arith, f"{how} {mode}")


# ------------------------------------------------------------------------------------ 7. run_conv_bn_chain
def _chain_modules(M, H, case, inp):
    mods = []
    for L, p in zip(case.layers, inp["params"]):
        if isinstance(L, R.Conv):
            m = M.HipConv2d(L.cin, L.cout, L.stride)
            m.weight.data.copy_(p["w"]), m.bias.data.copy_(p["b"])
            mods.append(m)
        else:
            m = M.HipBatchNorm2d(L.c, R.ACTS[L.act])
            assert (m.eps, m.momentum) == (L.eps, L.momentum)
            m.weight.data.copy_(p["gamma"]), m.bias.data.copy_(p["beta"])
            m.running_mean.copy_(p["rm"]), m.running_var.copy_(p["rv"])
            mods += [m, M.FusedIntoBN(L.act)]
    return M.FusedChain(*mods).cuda().train()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "module_by_module"])
def test_chain_against_modules(H, Fn, arith, fused, monkeypatch):
    """A miniature FusedChain of the model's own classes -- conv, BN, placeholder, twice, ending in a BatchNorm -- run
    by model.run_conv_bn_chain and, with model.FUSE_CONV_BN = False, module by module: each against the fp64 reference
    (output, every parameter gradient, running buffers, num_batches_tracked == 1; the BatchNorm-shadowed biases get no
    gradient).  The fused run must take no statistics pass where the producing convolution left slots: under the split
    arithmetics both BatchNorms go through vg_bn_finalize_stats.
    Guards the `stats` argument of the final `flush` in run_conv_bn_chain (without it the last BatchNorm runs
    ops.bn_act_fwd: counted here), `bn._note_forward()` beside bn_act_conv, and the slots handed from layer to layer."""
    from disentangle_mlp_amd import model as M
    case = R.MODULES
    inp, ref = ref_of(case)
    routes = R.check_routes(case, H)
    net = _chain_modules(M, H, case, inp)
    calls = defaultdict(int)
    for name in ("bn_act_fwd", "bn_stats", "bn_finalize_stats"):
        def counted(*a, _f=getattr(H, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(H, name, counted)
    x = inp["xs"][0].cuda().requires_grad_()
    prev = M.FUSE_CONV_BN
    try:
        M.FUSE_CONV_BN = fused
        y = net(x)
        (y * inp["gys"][0].cuda()).sum().backward()
    finally:
        M.FUSE_CONV_BN = prev
    torch.cuda.synchronize()
    if not fused:
        assert dict(calls) == dict(bn_act_fwd=2), dict(calls)
    elif all(r.stats_floats > 0 for r, _ in routes):
        assert dict(calls) == dict(bn_finalize_stats=2), dict(calls)
    else:                                        # "fp32": no slots anywhere -- one pass for the inner BatchNorm, the
        assert dict(calls) == dict(bn_stats=1, bn_act_fwd=1), dict(calls)      # two-pass kernel for the last
    mods = [m for m in net if not isinstance(m, M.FusedIntoBN)]
    sd = net.state_dict()
    P = []
    for m in mods:
        if isinstance(m, M.HipConv2d):
            assert m.bias.grad is None                       # bn_shadowed: BIAS_GRAD_ZERO on both paths
            P.append(dict(w=m.weight, b=m.bias))
        else:
            P.append(dict(gamma=m.weight, beta=m.bias, rm=m.running_mean, rv=m.running_var))
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, (k, int(v))
    got = result(case, [y.detach()], [x], P, [{}])
    want = dict(ref, taps=[{}])                              # the modules do not expose their saved statistics
    compare(case, got, want, arith, "fused" if fused else "module by module", absent=("gb.0", "gb.2"))


# ------------------------------------------------------------------------------------ misaligned BatchNorm inputs
@pytest.mark.parametrize("shape", [(8, 16, 16, 16),      # two passes, two slices per channel (C < 128)
                                   (6, 128, 6, 6),       # backward in one pass <2>: B * HW = 216, not a power of two
                                   (40, 128, 16, 16)])   # backward in one pass <8>: 8192 < B * HW <= 32768
def test_batchnorm_inputs_off_a_16_byte_boundary(H, shape):
    """ops._req takes any contiguous view; bn.hip's BatchNorm entry points read x / gy with 16-byte loads whenever
    HW % 4 == 0 and take the alignment "on trust" (bn_partial_kernel).  x and gy at 1-3 floats from a 16-byte boundary
    must give the bits of the aligned call: y, mean, 1/std, running statistics, gx, dgamma, dbeta."""
    C = shape[1]
    g = torch.Generator().manual_seed(90)
    x, gy = (torch.randn(*shape, generator=g) * 2 + 0.5).cuda(), torch.randn(*shape, generator=g).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()

    def both(xv, gv):
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y, mean, invstd = H.bn_act_fwd(xv, gamma, beta, rm, rv, 1e-5, 0.1, 2)
        gx, dg, db = H.bn_act_bwd(gv, xv, gamma, beta, mean, invstd, 2)
        return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, gx=gx, dgamma=dg, dbeta=db)
    want = both(x, gy)
    for ox, og in ((1, 1), (2, 2), (3, 3), (1, 0), (0, 2)):
        got = both(at_offset(x, ox), at_offset(gy, og))
        for k, v in want.items():
            assert torch.equal(got[k], v), (shape, ox, og, k)
