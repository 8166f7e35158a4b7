"""The eval-mode BatchNorm kernels of csrc/bn.hip -- vg_bn_eval_coeffs and vg_bn_eval_act_bwd through
ops.bn_eval_coeffs / ops.bn_eval_act_bwd -- against fp64 computed here.

Coefficients: relative L2 <= 3e-6 (the project's figure for BatchNorm coefficients, _chain_refs.STAT_TOL); the running
buffers keep their bits.  Bound: never below the fp64 maximum of |act(scale x + shift)| -- for the coefficients the
kernel wrote and for the exact fp64 ones -- and finite; bound / true maximum is printed per case (a recorded figure, no
threshold).  Backward: gx, dgamma, dbeta relative L2 <= 2e-5 (_chain_refs.BN_TOL) with the max-abs guard of
`_chain_refs.rel_err`, after asserting that no fp64 pre-activation lies within MARGIN of zero (seeds picked on the CPU
so that it holds with no element left out); two runs give identical bits; the same on views off a 16-byte boundary.
"""
import math

import pytest
import torch

import _chain_refs as R
from test_losses_gpu import at_offset

pytestmark = pytest.mark.gpu

COEFF_TOL, BWD_TOL = R.STAT_TOL, R.BN_TOL
ACTS = R.ACTS
EPS = 1e-5


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


def check(got, want, tol, what):
    e, m = R.rel_err(got, want)
    print(f"{what}: rel L2 {e:.2e}, max abs {m:.2e} of max |ref| (ceiling {tol:.0e})")
    assert math.isfinite(e) and e <= tol, f"{what}: rel L2 {e:.3e} > {tol:.1e}"
    assert m <= 50 * tol, f"{what}: max abs err {m:.3e} of max |ref|"


def act64(pre, act):
    if act == "relu":
        return torch.relu(pre)
    return torch.where(pre > 0, pre, 0.2 * pre) if act == "lrelu" else pre


# ------------------------------------------------------------------------------------------------ coefficients
def coeff_inputs(C, seed=0):
    g = torch.Generator().manual_seed(4100 + 13 * C + seed)
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    rm = 2.0 * torch.randn(C, generator=g)
    rv = 0.2 + torch.rand(C, generator=g)
    for i, v in enumerate((0.0, 1e-12, 1e6)):          # variance 0, far below eps, huge
        rv[(i * 7) % C] = v
    return gamma, beta, rm, rv


def coeff_ref(gamma, beta, rm, rv, eps):
    is_ = 1.0 / torch.sqrt(rv.double() + float(torch.tensor(eps, dtype=torch.float32)))
    sc = gamma.double() * is_
    return sc, beta.double() - rm.double() * sc, is_


def slot_sums(x, k=4):
    """stats[nslots][C][2] of x (B, C, H, W): consecutive groups of k values of a channel, fp32 sums added pairwise, the
    squares rounded to fp32 first -- what a convolution epilogue leaves (as _bn_refs.slot_sums)."""
    C = x.shape[1]
    v = x.transpose(0, 1).reshape(C, -1).float()
    assert v.shape[1] % k == 0

    def tree(a):
        while a.shape[-1] > 1:
            a = a[..., 0::2] + a[..., 1::2]
        return a[..., 0]
    a = v.reshape(C, -1, k)
    return torch.stack([tree(a), tree(a * a)], -1).permute(1, 0, 2).contiguous()


@pytest.mark.parametrize("C", [1, 3, 33, 80, 2048])
def test_coefficients(H, C):
    """Without slots, and with hand-made slots (1 and several, both kernel geometries): same coefficients, same bits;
    nothing but scale / shift / invstd (and the bound slot) is written."""
    gamma, beta, rm, rv = coeff_inputs(C)
    want = coeff_ref(gamma, beta, rm, rv, EPS)
    dev = [t.cuda() for t in (gamma, beta, rm, rv)]
    keep = [t.clone() for t in dev]
    sc, sh, is_ = H.bn_eval_coeffs(*dev, EPS, ACTS["relu"])
    for name, got, ref in zip(("scale", "shift", "invstd"), (sc, sh, is_), want):
        check(got, ref, COEFF_TOL, f"bn_eval_coeffs C={C} {name}")
    g = torch.Generator().manual_seed(C)
    for nslots in (1, 5, 64, 65, 300):
        hw = 4 * nslots
        stats = slot_sums(torch.randn(1, C, hw, 1, generator=g)).cuda()
        assert stats.shape == (nslots, C, 2)
        out = H.bn_eval_coeffs(*dev, EPS, ACTS["lrelu"], stats=stats, count=hw, want_bound=True)
        assert torch.equal(out[0], sc) and torch.equal(out[1], sh) and torch.equal(out[2], is_), (C, nslots)
        if H.CONV_ARITH == "fp16x3":
            assert out[3] is not None and math.isfinite(float(out[3])), (C, nslots)
    for a, b in zip(dev, keep):
        assert torch.equal(a, b), "an input of bn_eval_coeffs was written"


@pytest.fixture
def fp16x3(H, monkeypatch):
    """The bound exists under the fp16 planes: these tests pin that arithmetic instead of depending on the default."""
    monkeypatch.setattr(H, "CONV_ARITH", "fp16x3")


def test_coefficients_with_slots_of_a_real_convolution(H, fp16x3):
    """Slots from conv5x5_fwd(..., want_stats=True): coefficients as without them, the bound holds for the convolution's
    output."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 16, 8, 32, generator=g).cuda()
    w = (torch.randn(32, 16, 5, 5, generator=g) / 20).cuda()
    b = (0.5 * torch.randn(32, generator=g)).cuda()
    y, stats = H.conv5x5_fwd(x, w, b, 2, want_stats=True)
    assert stats is not None and stats.numel() > 0, "the stride-2 16 -> 32 convolution leaves statistics slots under fp16x3"
    gamma, beta, rm, rv = coeff_inputs(32, seed=1)
    dev = [t.cuda() for t in (gamma, beta, rm, rv)]
    sc, sh, is_, bound = H.bn_eval_coeffs(*dev, EPS, ACTS["relu"], stats=stats, count=y.numel() // 32, want_bound=True)
    want = coeff_ref(gamma, beta, rm, rv, EPS)
    for name, got, ref in zip(("scale", "shift", "invstd"), (sc, sh, is_), want):
        check(got, ref, COEFF_TOL, f"conv slots {name}")
    sc0 = H.bn_eval_coeffs(*dev, EPS, ACTS["relu"])[0]
    assert torch.equal(sc0, sc)
    assert bound is not None
    true = float(act64(y.double().cpu() * sc.double().cpu().view(1, -1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1),
                       "relu").abs().max())
    print(f"real convolution: bound / true maximum = {float(bound) / true:.3f}")
    assert math.isfinite(float(bound)) and float(bound) >= true


# ------------------------------------------------------------------------------------------------------- bound
def bound_inputs(kind):
    g = torch.Generator().manual_seed({"random": 1, "cancel": 2, "constant": 3}[kind])
    x = 1.5 * torch.randn(2, 6, 8, 16, generator=g) + 0.25
    if kind == "cancel":
        x[:, 2] = 1e4 * 0.7 + 0.7 * torch.randn(2, 8, 16, generator=g)        # |mean| = 1e4 sigma
    if kind == "constant":
        x[:, 4] = 1.7
    return x.float().contiguous()


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("kind", ["random", "cancel", "constant"])
def test_bound_is_sound(H, fp16x3, kind, act):
    """bound >= the fp64 maximum of |act(scale x + shift)|, with the coefficients as written and with the exact ones, for
    random data, a channel whose variance is lost to cancellation, and a constant channel; finite."""
    x = bound_inputs(kind)
    C = x.shape[1]
    gamma, beta, rm, rv = coeff_inputs(C, seed=5)
    if kind != "random":
        rv = torch.full((C,), 1e-12)          # 1 / std = 1 / sqrt(eps): the data is stretched as far as it goes
    dev = [t.cuda() for t in (gamma, beta, rm, rv)]
    for k in (4, 64):
        stats = slot_sums(x, k).cuda()
        sc, sh, _is, bound = H.bn_eval_coeffs(*dev, EPS, ACTS[act], stats=stats, count=x.numel() // C, want_bound=True)
        written = act64(x.double() * sc.double().cpu().view(1, -1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1), act).abs().max()
        e_sc, e_sh, _ = coeff_ref(gamma, beta, rm, rv, EPS)
        exact = act64(x.double() * e_sc.view(1, -1, 1, 1) + e_sh.view(1, -1, 1, 1), act).abs().max()
        true = max(float(written), float(exact))
        b = float(bound)
        print(f"bound {kind} {act} slots of {k}: bound {b:.6g}, true maximum {true:.6g}, ratio {b / true:.3f}")
        assert math.isfinite(b), (kind, act, b)
        assert b >= true, (kind, act, k, b, true)


# ---------------------------------------------------------------------------------------------------- backward
# shape -> seed bump (a seed whose fp64 pre-activations came within MARGIN of zero got the next one; picked on the CPU)
BWD_SHAPES = {(1, 1, 1, 1): 0, (2, 3, 5, 7): 0, (2, 5, 4, 4): 0, (1, 32, 8, 8): 0, (4, 33): 0, (1, 2048): 0,
              (2, 2, 24, 24): 4}          # the last: two slices per channel (the partials + the finalize launch)


def bwd_inputs(shape):
    C = shape[1]
    g = torch.Generator().manual_seed(5200 + sum((i + 3) * d for i, d in enumerate(shape)) + BWD_SHAPES[shape])
    x = 1.5 * torch.randn(*shape, generator=g) + 0.25
    gy = torch.randn(*shape, generator=g) + 0.5
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    rm = 0.3 * torch.randn(C, generator=g)
    rv = 0.5 + torch.rand(C, generator=g)
    is_ = (1.0 / torch.sqrt(rv.double() + EPS)).float()
    sc = gamma * is_
    sh = beta - rm * sc
    return dict(x=x, gy=gy, scale=sc, shift=sh, mean=rm, invstd=is_)


def bwd_ref(i, act):
    """fp64 from the fp32 inputs as they are; also the near-zero margin of the pre-activations."""
    x, gy = i["x"].double(), i["gy"].double()
    v = (1, -1) + (1,) * (x.dim() - 2)
    sc, sh, mu, is_ = (i[k].double().view(v) for k in ("scale", "shift", "mean", "invstd"))
    pre = x * sc + sh
    d = torch.ones_like(pre) if act == "none" else torch.where(pre > 0, 1.0, 0.0 if act == "relu" else 0.2).double()
    g = gy * d
    dims = [0] + list(range(2, x.dim()))
    a = pre.abs().transpose(0, 1).reshape(x.shape[1], -1)
    margin = float((a.min(1).values / a.max(1).values).min())
    return dict(gx=g * sc, dbeta=g.sum(dims), dgamma=(g * (x - mu) * is_).sum(dims), margin=margin)


def test_backward_seeds_keep_clear_of_zero():
    """(Needs no kernel; kept here so that the seeds and the kernels' test cannot drift apart.)"""
    for shape in BWD_SHAPES:
        m = bwd_ref(bwd_inputs(shape), "relu")["margin"]
        assert m > R.MARGIN, (shape, m)


def run_bwd(H, shape, off=0):
    i = bwd_inputs(shape)
    d = {k: v.cuda() for k, v in i.items()}
    if off:
        d["x"], d["gy"] = at_offset(d["x"], off), at_offset(d["gy"], off)
    C = shape[1]
    args = (d["gy"], d["x"], d["scale"], d["shift"], d["mean"], d["invstd"])
    for act, code in ACTS.items():
        ref = bwd_ref(i, act)
        assert ref["margin"] > R.MARGIN, (shape, act, ref["margin"])          # before anything is compared
        what = f"bn_eval_act_bwd {shape} {act} +{off}"
        gx, dg, db = H.bn_eval_act_bwd(*args, code)
        check(gx, ref["gx"], BWD_TOL, what + " gx")
        check(dg, ref["dgamma"], BWD_TOL, what + " dgamma")
        check(db, ref["dbeta"], BWD_TOL, what + " dbeta")
        gx2, dg2, db2 = H.bn_eval_act_bwd(*args, code)
        assert torch.equal(gx2, gx) and torch.equal(dg2, dg) and torch.equal(db2, db), what + ": a second run differs"
        gx3, ng, nb = H.bn_eval_act_bwd(*args, code, need_param_grads=False)
        assert ng is None and nb is None and torch.equal(gx3, gx), what + ": need_param_grads=False changes gx"
        g0, b0 = torch.randn(C, generator=torch.Generator().manual_seed(31)).cuda(), torch.randn(
            C, generator=torch.Generator().manual_seed(32)).cuda()
        acc_g, acc_b = g0.clone(), b0.clone()
        gx4, rg, rb = H.bn_eval_act_bwd(*args, code, accumulate_into=(acc_g, acc_b))
        assert rg is acc_g and rb is acc_b and torch.equal(gx4, gx), what + ": accumulate_into changes gx"
        assert torch.equal(acc_g, dg + g0) and torch.equal(acc_b, db + b0), what + ": accumulate_into does not add exactly"
        if H.CONV_ARITH == "fp16x3" and gx.numel() // (shape[0] * C) > 1:          # (HW == 1: no bound is emitted)
            slot = H.known_amax(gx)
            assert slot is not None and float(slot) == float(gx.abs().max()), what + ": gx_amax"


@pytest.mark.parametrize("shape", list(BWD_SHAPES), ids=str)
def test_backward(H, shape):
    run_bwd(H, shape)


@pytest.mark.parametrize("shape", list(BWD_SHAPES), ids=str)
def test_backward_off_a_16_byte_boundary(H, shape):
    """x and gy at 1-3 floats from a 16-byte boundary: the scalar loops, same references and ceilings."""
    for off in (1, 2, 3):
        run_bwd(H, shape, off)


def test_backward_keeps_nan(H):
    """A NaN gradient stays a NaN under ReLU (a select would drop it where the unit is off); a NaN input gives a NaN
    gradient under ReLU / LeakyReLU; the other elements keep their bits."""
    shape = (2, 5, 4, 4)
    i = bwd_inputs(shape)
    d = {k: v.cuda() for k, v in i.items()}
    gx0, _, _ = H.bn_eval_act_bwd(d["gy"], d["x"], d["scale"], d["shift"], d["mean"], d["invstd"], ACTS["relu"])
    gy, x = d["gy"].clone(), d["x"].clone()
    off_unit = (gx0 == 0).nonzero()[0]
    gy[tuple(off_unit)] = float("nan")
    x[1, 4, 3, 3] = float("nan")
    gx, dg, db = H.bn_eval_act_bwd(gy, x, d["scale"], d["shift"], d["mean"], d["invstd"], ACTS["relu"])
    assert math.isnan(float(gx[tuple(off_unit)])) and math.isnan(float(gx[1, 4, 3, 3]))
    mask = torch.ones(shape, dtype=torch.bool, device="cuda")
    mask[tuple(off_unit)] = False
    mask[1, 4, 3, 3] = False
    assert torch.equal(gx[mask], gx0[mask])
    assert math.isnan(float(db[int(off_unit[1])])) and math.isnan(float(db[4]))
