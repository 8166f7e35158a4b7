"""CPU: the fp64 chain reference of tests/_chain_refs.py itself, and the condition every case of
tests/test_fused_functions_gpu.py rests on.

(a) no fp64 pre-activation of any BatchNorm of any case lies within 2^-14 max |pre| (over its channel) of zero -- the
    seeds in the case table were chosen here so that it holds; a new case that fails gets another seed;
(b) the helper's gradients against torch.autograd.gradcheck and against central differences of its own loss, on one
    tiny conv -> BN -> LeakyReLU -> conv chain;
(c) the same chains restated in torch float32 on the CPU against fp64, per quantity, so that it can be seen how much of
    each ceiling a plain fp32 evaluation already uses.  Worst over all cases, as measured here (pytest -s prints the
    table per case), as a fraction of the ceiling:
        y 4.9e-7 (16 % of 3e-6), running statistics and saved mean / 1/std 1.2e-7 (4 % of 3e-6), gx 5.2e-7 and
        dgamma / dbeta 5.9e-7 (3 % of 2e-5), gw / gb 4.2e-7 (14 % of 3e-6 for a chain's last convolution, 2 % of 2e-5
        upstream of a BatchNorm);
(d) host only: every case takes the kernel route its table entry states, in the three arithmetics of the GPU file.
"""
import pytest
import torch

import _chain_refs as R

_ref = {}


def ref_of(case):
    if case.name not in _ref:
        inp = R.make_inputs(case)
        _ref[case.name] = (inp, R.run(case, inp))
    return _ref[case.name]


@pytest.mark.parametrize("case", R.ALL_CASES, ids=lambda c: c.name)
def test_no_unit_near_zero(case):
    inp, ref = ref_of(case)
    m = R.margin(ref)
    print(f"{case.name}: min |pre| / max |pre| over every BatchNorm channel = {m:.3e} (needs > {R.MARGIN:.3e})")
    assert m > R.MARGIN, (case.name, case.seed, m)
    assert len(case.routes) == sum(isinstance(L, R.Conv) for L in case.layers) or case is R.TINY
    assert tuple(ref["ys"][0].shape) == R.out_shape(case)


def test_case_names_are_unique_and_buffers_move():
    assert len({c.name for c in R.ALL_CASES}) == len(R.ALL_CASES)
    inp, ref = ref_of(R.TWICE)
    i = 1
    rm0, rm2 = inp["params"][i]["rm"].double(), ref["bufs"][i]["rm"]
    m = [ref["taps"][u][i]["mean"] for u in range(2)]               # of the BatchNorm's input: what F.batch_norm averaged
    want = 0.9 * (0.9 * rm0 + 0.1 * m[0]) + 0.1 * m[1]              # updated exactly twice, in order
    assert float((rm2 - want).abs().max()) <= 1e-14
    assert inp["params"][i]["rm"].dtype == torch.float32            # the inputs themselves are left alone


def test_helper_gradients_on_a_tiny_chain():
    case = R.TINY
    inp, ref = ref_of(case)
    names = [(i, k) for i, p in enumerate(inp["params"]) for k in ("w", "b", "gamma", "beta") if k in p]

    def fwd(x, *flat):
        params = [dict() for _ in case.layers]
        for (i, k), t in zip(names, flat):
            params[i][k] = t
        return R.chain_forward(case.layers, x, params)
    leaves = [inp["xs"][0].double().requires_grad_()] + [inp["params"][i][k].double().requires_grad_() for i, k in names]
    assert torch.autograd.gradcheck(fwd, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)
    # what `run` returns under each name, against central differences of its loss along one random direction
    g = torch.Generator().manual_seed(7)
    dirs = dict(x=torch.randn(case.shape, generator=g, dtype=torch.float64))
    for i, k in names:
        dirs[(i, k)] = torch.randn(inp["params"][i][k].shape, generator=g, dtype=torch.float64)
    analytic = float((ref["gxs"][0] * dirs["x"]).sum()) + sum(float((ref["grads"][i][k] * dirs[(i, k)]).sum()) for i, k in names)

    def loss_at(h):
        moved = dict(xs=[inp["xs"][0].double() + h * dirs["x"]], gys=inp["gys"],
                     params=[{k: (v.double() + h * dirs[(i, k)] if (i, k) in dirs else v) for k, v in p.items()}
                             for i, p in enumerate(inp["params"])])
        return float(R.run(case, moved)["loss"])
    h = 1e-6
    numeric = (loss_at(h) - loss_at(-h)) / (2 * h)
    print(f"directional derivative: autograd {analytic!r}, central differences {numeric!r}")
    assert abs(numeric - analytic) <= 1e-7 * max(abs(analytic), 1.0)


@pytest.mark.parametrize("case", R.GPU_CASES, ids=lambda c: c.name)
def test_fp32_restatement_against_fp64(case):
    """The chain in torch float32 on the CPU: per quantity its distance from fp64, printed, and below the ceiling the
    GPU is held to (a ceiling that plain fp32 arithmetic missed could not be met by any fp32 kernel)."""
    inp, ref = ref_of(case)
    r32 = R.run(case, inp, dtype=torch.float32)
    q64, q32 = R.quantities(case, ref), R.quantities(case, r32)
    assert list(q64) == list(q32)
    for name, (want, tol) in q64.items():
        e, m = R.rel_err(q32[name][0], want)
        print(f"{case.name} {name}: fp32 restatement {e:.2e} rel L2, {m:.2e} max (ceiling {tol:.0e}: {100 * e / tol:.1f} %)")
        assert e <= tol and m <= 50 * tol, (case.name, name, e, m)


@pytest.mark.parametrize("arith", ["fp16x3", "fp32", "bf16x6"])
def test_every_case_reaches_its_route(arith):
    """Host only (ops.route_conv launches nothing): the routes the case table states, in the three arithmetics the GPU
    file runs, so that a case which would silently test a fallback fails here already."""
    from disentangle_mlp_amd import ops
    prev, ops.CONV_ARITH = ops.CONV_ARITH, arith
    try:
        for case in R.GPU_CASES:
            for r, rw in R.check_routes(case, ops):
                print(case.name, arith, r.family, r.affine_on_load, r.stats_floats, rw and (rw.family, rw.affine_on_load))
    finally:
        ops.CONV_ARITH = prev
