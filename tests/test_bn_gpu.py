"""The BatchNorm kernels of csrc/bn.hip through ops.bn_act_fwd / bn_act_bwd / bn_stats / bn_finalize_stats, every
output per element against the fp64 references of tests/_bn_refs.py, at every host-side dispatch edge: scalar and
16-byte plane loops with one and several slices in either pass, the ends of make_slicing, the one-pass backward at its
thresholds, BatchNorm1d off its 32-channel workgroups and 8 row-slices, the three regimes of the slot finalisation.

|got - ref| <= K 2^-24 magnitude per element, K per output from the fp32 restatement measured in
tests/test_bn_cpu.py (R.K) -- nothing here is measured from a kernel; "same bits" is torch.equal.  Every check prints
its worst ratio (pytest -s) before it asserts, and the module prints the worst per output at its end.

The backward is given the reference's saved statistics (rounded to fp32), so its reference does not depend on what the
forward kernel computed; the kink of ReLU / LeakyReLU is handled as _bn_refs describes.

Misaligned inputs: a contiguous view at 1-3 floats from a 16-byte boundary is a legal argument; the host side picks the
scalar loops (and the two-pass backward) for it.  y and gx are allocated by the operations themselves.
"""
import pytest
import torch

import _bn_refs as R
from test_losses_gpu import at_offset

pytestmark = pytest.mark.gpu

EPS = R.EPS
STATS = ("mean", "invstd", "scale", "shift")
WORST = {}


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    yield ops
    print("\noutput          worst on the device (2^-24)   K")
    for name in R.K:
        if name in WORST:
            print(f"{name:<16}{WORST[name]:>10.2f}{R.K[name]:>22.1f}")


def check(got, ref, name, what):
    """Per element: |got - ref[name]| <= K[name] 2^-24 magnitude (+ the kink allowance of a backward output)."""
    k = R.K[name]
    g = got.detach().cpu().double()
    r, mag, allow = ref[name].double(), ref[name + "_mag"].double(), ref.get(name + "_allow")
    assert g.shape == r.shape, (what, name, g.shape, r.shape)
    assert bool(torch.isfinite(g).all()), (what, name)
    w = R.ratio(g, r, mag, allow)
    WORST[name] = max(WORST.get(name, 0.0), w)
    print(f"{what} {name}: worst {w:.2f} x 2^-24 (K = {k})")
    bound = k * R.U * mag.expand_as(r) + (0 if allow is None else allow.double())
    bad = (g - r).abs() > bound
    assert not bool(bad.any()), (f"{what} {name}: {int(bad.sum())} of {bad.numel()} elements off by more than {k} x 2^-24 x "
                                 f"magnitude (worst {w:.2f}); first at {bad.nonzero()[0].tolist()}")


def dev(i, *names):
    return tuple(i[n].cuda() for n in names)


_fwd_ref, _bwd_ref = {}, {}


def fwd_ref(shape, act, mom):
    key = (shape, act, mom)
    if key not in _fwd_ref:
        i = R.bn_inputs(shape)
        _fwd_ref[key] = R.bn_fwd(i["x"], i["gamma"], i["beta"], act, EPS, mom, i["rm0"], i["rv0"])
    return _fwd_ref[key]


def saved(shape):
    """The reference's saved statistics as the backward receives them: fp32."""
    r = fwd_ref(shape, "none", 0.1)
    return r["mean"].float(), r["invstd"].float()


def bwd_ref(shape, act):
    key = (shape, act)
    if key not in _bwd_ref:
        i = R.bn_inputs(shape)
        mean, invstd = saved(shape)
        _bwd_ref[key] = R.bn_bwd(i["gy"], i["x"], i["gamma"], i["beta"], mean, invstd, act)
    return _bwd_ref[key]


# ----------------------------------------------------------------------------------------------------- forward
def run_fwd(H, shape, x=None):
    """Every activation, momentum 0.1 and 1.0, running statistics from random values; running_* = None gives the
    other outputs the same bits."""
    i = R.bn_inputs(shape)
    xd = i["x"].cuda() if x is None else x
    gamma, beta = dev(i, "gamma", "beta")
    for act, code in R.ACTS.items():
        for mom in (0.1, 1.0) if act == "lrelu" or x is not None else (0.1,):
            ref = fwd_ref(shape, act, mom)
            rm, rv = dev(i, "rm0", "rv0")
            y, mean, invstd = H.bn_act_fwd(xd, gamma, beta, rm, rv, EPS, mom, code)
            what = f"bn_act_fwd {shape} {act} momentum={mom}"
            check(y, ref, "y", what)
            check(mean, ref, "mean", what), check(invstd, ref, "invstd", what)
            check(rm, ref, "running_mean", what), check(rv, ref, "running_var", what)
            y2, mean2, invstd2 = H.bn_act_fwd(xd, gamma, beta, None, None, EPS, mom, code)
            assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(invstd2, invstd), \
                what + ": running_* = None changes another output"


@pytest.mark.parametrize("shape", list(R.SHAPES_2D))
def test_bn_fwd(H, shape):
    run_fwd(H, shape)


# ---------------------------------------------------------------------------------------------------- backward
def run_bwd(H, shape, gy=None, x=None, extras=True):
    i = R.bn_inputs(shape)
    C = shape[1]
    gyd = i["gy"].cuda() if gy is None else gy
    xd = i["x"].cuda() if x is None else x
    gamma, beta = dev(i, "gamma", "beta")
    mean, invstd = (t.cuda() for t in saved(shape))
    for act, code in R.ACTS.items():
        ref = bwd_ref(shape, act)
        what = f"bn_act_bwd {shape} {act}"
        gx, dgamma, dbeta = H.bn_act_bwd(gyd, xd, gamma, beta, mean, invstd, code)
        check(gx, ref, "gx", what), check(dgamma, ref, "dgamma", what), check(dbeta, ref, "dbeta", what)
        if not extras:
            continue
        # a second identical call: the reductions are fixed-order
        gx2, dgamma2, dbeta2 = H.bn_act_bwd(gyd, xd, gamma, beta, mean, invstd, code)
        assert torch.equal(gx2, gx) and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta), what + ": a second call differs"
        gx3, none_g, none_b = H.bn_act_bwd(gyd, xd, gamma, beta, mean, invstd, code, need_param_grads=False)
        assert none_g is None and none_b is None and torch.equal(gx3, gx), what + ": need_param_grads=False changes gx"
        g0, b0 = R.randn(C, seed=31).cuda(), R.randn(C, seed=32).cuda()
        acc_g, acc_b = g0.clone(), b0.clone()
        gx4, rg, rb = H.bn_act_bwd(gyd, xd, gamma, beta, mean, invstd, code, accumulate_into=(acc_g, acc_b))
        assert rg is acc_g and rb is acc_b and torch.equal(gx4, gx), what + ": accumulate_into changes gx"
        assert torch.equal(acc_g, dgamma + g0) and torch.equal(acc_b, dbeta + b0), what + ": accumulate_into does not add exactly"


@pytest.mark.parametrize("shape", list(R.SHAPES_2D))
def test_bn_bwd(H, shape):
    run_bwd(H, shape)


# -------------------------------------------------------------------------------------------------- BatchNorm1d
@pytest.mark.parametrize("shape", R.SHAPES_1D)
def test_bn1d(H, shape):
    run_fwd(H, shape)
    run_bwd(H, shape)


# ------------------------------------------------------------------------------------------- coefficients from x
def run_stats(H, shape, x=None):
    i = R.bn_inputs(shape)
    xd = i["x"].cuda() if x is None else x
    gamma, beta = dev(i, "gamma", "beta")
    for mom in (0.1, 1.0):
        ref = fwd_ref(shape, "none", mom)
        rm, rv = dev(i, "rm0", "rv0")
        out = H.bn_stats(xd, gamma, beta, rm, rv, EPS, mom)
        what = f"bn_stats {shape} momentum={mom}"
        for name, t in zip(STATS, out):
            check(t, ref, name, what)
        check(rm, ref, "running_mean", what), check(rv, ref, "running_var", what)
        out2 = H.bn_stats(xd, gamma, beta, None, None, EPS, mom)
        assert all(torch.equal(a, b) for a, b in zip(out, out2)), what + ": running_* = None changes another output"


@pytest.mark.parametrize("shape", list(R.TWO_PASS))
def test_bn_stats(H, shape):
    run_stats(H, shape)


# --------------------------------------------------------------------------------------- coefficients from slots
@pytest.mark.parametrize("nslots", list(R.SLOT_CASES))
def test_bn_finalize_stats(H, nslots):
    for C in R.SLOT_CASES[nslots]:
        i = R.slot_inputs(nslots, C)
        stats, gamma, beta = dev(i, "stats", "gamma", "beta")
        for mom in (0.1, 1.0):
            ref = R.bn_coefficients_from_slots(i["stats"], i["count"], i["gamma"], i["beta"], EPS, mom, i["rm0"], i["rv0"])
            rm, rv = dev(i, "rm0", "rv0")
            out = H.bn_finalize_stats(stats, i["count"], gamma, beta, rm, rv, EPS, mom)
            what = f"bn_finalize_stats slots={nslots} ({R.finalize_regime(nslots)}) C={C} momentum={mom}"
            for name, t in zip(STATS, out):
                check(t, ref, name, what)
            check(rm, ref, "running_mean", what), check(rv, ref, "running_var", what)
            # the channel with s2 / n < m^2: the clamp answers, 1 / sqrt(eps)
            c = i["clamped"]
            want = R.f32(EPS) ** -0.5
            assert abs(float(out[1][c]) - want) <= R.K["invstd"] * R.U * want, (what, float(out[1][c]), want)
            out2 = H.bn_finalize_stats(stats, i["count"], gamma, beta, None, None, EPS, mom)
            assert all(torch.equal(a, b) for a, b in zip(out, out2)), what + ": running_* = None changes another output"


# ------------------------------------------------------------------------------------------- misaligned inputs
@pytest.mark.parametrize("shape", R.MISALIGNED_SHAPES)
def test_bn_misaligned(H, shape):
    """x alone, and x and gy together, at 1-3 floats off a 16-byte boundary: the same references and tolerances as the
    aligned call (the scalar loops add in another order: equal bits are not promised)."""
    i = R.bn_inputs(shape)
    x, gy = dev(i, "x", "gy")
    for o in (1, 2, 3):
        print(f"-- x at +{o} floats")
        xo = at_offset(x, o)
        run_fwd(H, shape, x=xo)
        run_stats(H, shape, x=xo)
        run_bwd(H, shape, x=xo, extras=False)
        print(f"-- x and gy at +{o} floats")
        run_bwd(H, shape, gy=at_offset(gy, o), x=xo, extras=(o == 1))
    print("-- gy alone at +2 floats")
    run_bwd(H, shape, gy=at_offset(gy, 2), extras=False)
