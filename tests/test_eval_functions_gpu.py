"""The eval-mode autograd Functions -- functional.BNEvalConvFn (conv(act(BN_eval(x))), nothing materialised) and
BNEvalActFn (materialised) -- against the fp64 chain reference of tests/_eval_refs.py, in the three arithmetics.

Every case asserts first (host only) that its convolutions take the kernel route _chain_refs states, so the
affine-on-load kernels are what runs under the split arithmetics, and that no fp64 pre-activation lies within MARGIN of
zero.  Ceilings: those of test_fused_functions_gpu.py -- y 3e-6; gx, dgamma, dbeta and every gradient that passed through
a BatchNorm backward 2e-5; gw / gb of a chain's last convolution 3e-6 (relative L2 with the max-abs guard).  The bias of
a convolution in front of an eval BatchNorm has an ordinary, NON-zero gradient and is compared like the rest.
"""
import math

import pytest
import torch

import _eval_refs as E

pytestmark = pytest.mark.gpu
_ref = {}


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
    prev = H.CONV_ARITH
    if request.param != "default":
        H.CONV_ARITH = request.param
    yield H.CONV_ARITH
    H.CONV_ARITH = prev


def ref_of(case, uses=1):
    key = (case.name, uses)
    if key not in _ref:
        inp = E.eval_inputs(case, uses)
        ref = E.run(case, inp)
        assert ref["margin"] > E.MARGIN, (case.name, uses, ref["margin"])
        _ref[key] = (inp, ref)
    return _ref[key]


def check(got, want, tol, what):
    e, m = E.rel_err(got, want)
    print(f"{what}: rel L2 {e:.2e}, max abs {m:.2e} of max |ref| (ceiling {tol:.0e})")
    assert math.isfinite(e) and e <= tol, f"{what}: rel L2 {e:.3e} > {tol:.1e}"
    assert m <= 50 * tol, f"{what}: max abs err {m:.3e} of max |ref|"


def leaves(inp):
    return [{k: v.cuda().clone().requires_grad_(k not in ("rm", "rv")) for k, v in p.items()} for p in inp["params"]]


def run_functions(Fn, H, case, x, P, slots=True):
    """The layers on x as model.run_conv_bn_chain strings them in eval mode.  ``slots``: the BatchNorm gets the
    producing convolution's statistics slots (the bound without a pass over x) or none (`ops.amax_of` measures)."""
    routes = iter(E.check_routes(case, H))          # asserts the routes, host only
    t, stats, pending = x, None, None
    for i, L in enumerate(case.layers):
        p = P[i]
        if E.is_bn(L):
            pending = (i, L)
            continue
        route = next(routes)[0]
        if pending is None:
            t, stats = Fn.conv_with_stats(t, p["w"], p["b"], L.stride, L.transposed, Fn.BIAS_GRAD_COMPUTE)
        else:
            j, N = pending
            q = P[j]
            t, stats = Fn.bn_eval_act_conv(t, q["gamma"], q["beta"], q["rm"], q["rv"], N.eps, E.ACTS[N.act], p["w"], p["b"],
                                           L.stride, L.transposed, Fn.BIAS_GRAD_COMPUTE, stats if slots else None)
            pending = None
        assert stats.numel() == route.stats_floats and not stats.requires_grad, (case.name, L, stats.shape, route)
    if pending is not None:
        j, N = pending
        q = P[j]
        t = Fn.batch_norm_eval_act(t, q["gamma"], q["beta"], q["rm"], q["rv"], N.eps, E.ACTS[N.act])
    return t


def run_case(Fn, H, case, inp, slots=True, ctx=None, between=None):
    import contextlib
    P = leaves(inp)
    bufs0 = [{k: p[k].clone() for k in ("rm", "rv")} if "rm" in p else None for p in P]
    xs = [x.cuda().clone().requires_grad_() for x in inp["xs"]]
    with (ctx() if ctx is not None else contextlib.nullcontext()):
        ys = [run_functions(Fn, H, case, x, P, slots) for x in xs]
        loss = sum((y * gy.cuda()).sum() for y, gy in zip(ys, inp["gys"]))
        for p, b0 in zip(P, bufs0):          # the forward read the running buffers and left their bits alone
            if b0 is not None:
                assert torch.equal(p["rm"], b0["rm"]) and torch.equal(p["rv"], b0["rv"]), case.name
        if between is not None:
            between(P)
        loss.backward()
    torch.cuda.synchronize()
    return dict(ys=[y.detach() for y in ys], gxs=[x.grad for x in xs],
                grads=[{k: p[k].grad for k in p if k not in ("rm", "rv")} for p in P])


def compare(case, got, ref, label):
    qr, qg = E.quantities(case, ref), E.quantities(case, got)
    for name, (want, tol) in qr.items():
        assert qg[name][0] is not None, f"{label}: {name} is missing"
        check(qg[name][0], want, tol, f"{case.name} [{label}] {name}")


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.name)
def test_eval_chain(H, Fn, arith, case):
    """y, gx, gw, gb (non-zero: the BatchNorm behind it cancels nothing), dgamma, dbeta against fp64, with the
    producer's slots and without; the running buffers keep their bits (asserted in run_case)."""
    inp, ref = ref_of(case)
    for i, L in enumerate(case.layers[:-1]):
        if not E.is_bn(L) and E.is_bn(case.layers[i + 1]):
            assert float(ref["grads"][i]["b"].abs().max()) > 1e-3, "the reference's bias gradient is not zero in eval"
    for slots in (True, False):
        got = run_case(Fn, H, case, inp, slots)
        compare(case, got, ref, f"{arith} {'slots' if slots else 'measured'}")


@pytest.mark.parametrize("mode", ["autograd_sums", "accumulate_param_grads"])
def test_layer_used_twice_accumulates(H, Fn, arith, mode):
    """Two inputs through the same conv -> eval BN + LeakyReLU -> conv, one backward: autograd's sum, and the
    accumulate protocol (the second pass adds dgamma / dbeta / gw inside its kernels)."""
    case = E.FWD_CASES[1]
    inp, ref = ref_of(case, uses=2)
    got = run_case(Fn, H, case, inp, ctx=Fn.accumulate_param_grads if mode == "accumulate_param_grads" else None)
    compare(case, got, ref, f"{arith} {mode}")


@pytest.mark.parametrize("case", (E.FWD_CASES[0], E.LAST_BN_CASES[0], E.BN1D), ids=lambda c: c.name)
def test_buffers_moved_between_forward_and_backward(H, Fn, case):
    """A train-mode step between forward and backward moves the running buffers; the Functions saved their own
    coefficients and a copy of the running mean: the gradients keep their bits."""
    inp, _ = ref_of(case)

    def move(P):
        for p in P:
            if "rm" in p:
                p["rm"].mul_(1.7).add_(0.3)
                p["rv"].mul_(0.4).add_(0.2)
    a = run_case(Fn, H, case, inp)
    b = run_case(Fn, H, case, inp, between=move)
    for name, (t, _tol) in E.quantities(case, a).items():
        assert torch.equal(t, E.quantities(case, b)[name][0]), (case.name, name)
