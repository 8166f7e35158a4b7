"""Where the tolerances of tests/test_bn_gpu.py come from, and that its cases reach what they are named for (no GPU).

1. The fp64 references of tests/_bn_refs.py agree with the oracle's BatchNorm (oracle.ops.bn_act, torch autograd
   through F.batch_norm) to 1e-10, a count of 1 stated by hand.
2. The same functions in the kernel's precision mix (dtype=torch.float32, see _bn_refs) against fp64, element by
   element, on every case the GPU tests use: worst |err| / magnitude per output, in units of 2^-24.

   output          worst (2^-24)   recorded   K = max(4 x recorded, 2)
   y                  2.96           3.0         12.0
   mean               1.00           1.0          4.0
   invstd             0.99           1.0          4.0
   scale              1.81           1.9          7.6
   shift              3.10           3.3         13.2
   running_mean       2.22           2.3          9.2
   running_var        2.08           2.1          8.4
   gx                10.67          11.0         44.0
   dgamma             2.30           2.4          9.6
   dbeta              1.57           1.6          6.4

   "recorded" (FP32_WORST of _bn_refs.py) is the measured figure rounded up.  The factor 4 stands for what the
   restatement leaves out: the order of the fp64 sums and the device's fused multiply-adds; the floor of 2 for an
   output whose restatement happens to be exact.  Nothing here is measured from a kernel.
   test_fp32_restatement measures the column again, prints it (-s) and asserts that it stays within "recorded".
3. The kink set of ReLU / LeakyReLU (see _bn_refs) is all but empty in every case: at most 1e-5 of the elements, none
   in a case of fewer than 100 000 -- from the reference alone.
4. make_slicing / make_apply_slicing / the backward's path, restated in _bn_refs from bn.hip, give the slice counts
   and kernels each case is named for.
"""
import pytest
import torch

import _bn_refs as R
from oracle import ops as O


def close(a, b, tol=1e-10):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("shape", ((10, 5, 21, 21), (3, 7, 5, 1), (9, 33), (2, 31)))
@pytest.mark.parametrize("act", list(R.ACTS))
def test_refs_match_oracle(shape, act):
    i = R.bn_inputs(shape)
    C = shape[1]
    r = R.bn_fwd(i["x"], i["gamma"], i["beta"], act, rm0=torch.zeros(C), rv0=torch.ones(C))
    o = O.bn_act(i["x"], i["gamma"], i["beta"], act, eps=R.f32(R.EPS), momentum=R.f32(0.1))
    close(r["y"], o["y"].reshape(shape), 1e-9), close(r["running_mean"], o["rm"]), close(r["running_var"], o["rv"])
    # backward: fp64 autograd through F.batch_norm, upstream gradient gy; the saved statistics are the fp64 ones
    x = i["x"].double().requires_grad_()
    gm, bt = i["gamma"].double().requires_grad_(), i["beta"].double().requires_grad_()
    pre = torch.nn.functional.batch_norm(x, None, None, gm, bt, True, 0.1, R.f32(R.EPS))
    y = R._act(pre, act)
    close(r["y"], y.detach(), 1e-9)
    y.backward(i["gy"].double())
    b = R.bn_bwd(i["gy"], i["x"], i["gamma"], i["beta"], r["mean"], r["invstd"], act)
    scale = float(x.grad.abs().max())
    assert float((b["gx"] - x.grad).abs().max()) <= 1e-9 * scale
    close(b["dgamma"], gm.grad, 1e-9), close(b["dbeta"], bt.grad, 1e-9)


def test_refs_count_of_one():
    """One value per channel: mean = x, variance 0, invstd = 1 / sqrt(eps), y = act(beta), and the running variance
    takes the biased variance 0 -- the kernel's documented behaviour, which F.batch_norm refuses."""
    i = R.bn_inputs((1, 33))
    r = R.bn_fwd(i["x"], i["gamma"], i["beta"], "none", momentum=0.1, rm0=i["rm0"], rv0=i["rv0"])
    close(r["mean"], i["x"][0].double(), 1e-15)
    close(r["invstd"], torch.full((33,), R.f32(R.EPS) ** -0.5, dtype=torch.float64), 1e-15)
    close(r["y"][0], i["beta"].double(), 1e-12)
    close(r["running_var"], (1 - R.f32(0.1)) * i["rv0"].double(), 1e-15)
    close(r["running_mean"], (1 - R.f32(0.1)) * i["rm0"].double() + R.f32(0.1) * i["x"][0].double(), 1e-15)


def test_slot_reference_matches_pass_reference():
    """Coefficients from slots that hold exact sums are the coefficients from the values."""
    v = R.randn(5, 64, seed=5).double() * 2 + 0.5
    gamma, beta = 1 + 0.1 * R.randn(5, seed=6), 0.1 * R.randn(5, seed=7)
    a = v.view(5, 16, 4)
    stats = torch.stack([a.sum(-1), (a * a).sum(-1)], -1).permute(1, 0, 2).contiguous()
    s = R.bn_coefficients_from_slots(stats, 64.0, gamma, beta, rm0=torch.zeros(5), rv0=torch.ones(5))
    x = v.view(5, 8, 8).permute(1, 0, 2).reshape(8, 5, 2, 4)
    p = R.bn_coefficients_from_x(x, gamma, beta, rm0=torch.zeros(5), rv0=torch.ones(5))
    for name in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
        close(s[name], p[name], 1e-12)


def test_clamped_slot_channel():
    for nslots, Cs in R.SLOT_CASES.items():
        for C in Cs:
            i = R.slot_inputs(nslots, C)
            s = i["stats"].double()
            c = i["clamped"]
            m = s[:, c, 0].sum() / i["count"]
            assert float(s[:, c, 1].sum() / i["count"]) < 0.75 * float(m * m), (nslots, C)
            r = R.bn_coefficients_from_slots(i["stats"], i["count"], i["gamma"], i["beta"])
            assert abs(float(r["invstd"][c]) * R.f32(R.EPS) ** 0.5 - 1) <= 1e-15          # var clamped at 0: 1 / sqrt(eps)
            assert bool(torch.isfinite(torch.stack([r[k] for k in ("mean", "invstd", "scale", "shift")])).all())


# ------------------------------------------------------------------------- 2. fp32 against fp64, on the GPU tests' inputs
def _saved(ref):
    return ref["mean"].float(), ref["invstd"].float()


def restatement_and_kinks():
    """({output: worst |fp32 - fp64| / magnitude in units of 2^-24}, {(shape, act): (kink elements, elements)})"""
    worst, kinks = {}, {}

    def note(r32, r64, *names):
        for n in names:
            w = R.ratio(r32[n], r64[n], r64[n + "_mag"], r64.get(n + "_allow"))
            worst[n] = max(worst.get(n, 0.0), w)

    stat_names = ("mean", "invstd", "scale", "shift", "running_mean", "running_var")
    for shape in tuple(R.SHAPES_2D) + R.SHAPES_1D:
        i = R.bn_inputs(shape)
        for act in R.ACTS:
            for mom in (0.1, 1.0):
                a = (i["x"], i["gamma"], i["beta"], act)
                kw = dict(momentum=mom, rm0=i["rm0"], rv0=i["rv0"])
                r64 = R.bn_fwd(*a, **kw)
                note(R.bn_fwd(*a, dtype=torch.float32, **kw), r64, "y", *stat_names)
            mean, invstd = _saved(r64)
            b = (i["gy"], i["x"], i["gamma"], i["beta"], mean, invstd, act)
            b64 = R.bn_bwd(*b)
            note(R.bn_bwd(*b, dtype=torch.float32), b64, "gx", "dgamma", "dbeta")
            kinks[(shape, act)] = (int(b64["kink"].sum()), b64["kink"].numel())
    for nslots, Cs in R.SLOT_CASES.items():
        for C in Cs:
            i = R.slot_inputs(nslots, C)
            for mom in (0.1, 1.0):
                a = (i["stats"], i["count"], i["gamma"], i["beta"])
                kw = dict(momentum=mom, rm0=i["rm0"], rv0=i["rv0"])
                note(R.bn_coefficients_from_slots(*a, dtype=torch.float32, **kw), R.bn_coefficients_from_slots(*a, **kw),
                     *stat_names)
    return worst, kinks


@pytest.fixture(scope="module")
def measured():
    return restatement_and_kinks()


def test_fp32_restatement(measured):
    worst, _ = measured
    assert set(worst) == set(R.K)
    print("\noutput          worst (2^-24)   recorded   K")
    for name in R.K:
        print(f"{name:<16}{worst[name]:>10.2f}{R.FP32_WORST[name]:>14.1f}{R.K[name]:>8.1f}")
    for name, w in worst.items():
        assert w <= R.FP32_WORST[name], (name, w, R.FP32_WORST[name])      # the recorded column, which K derives from, is current
        assert R.K[name] == max(4 * R.FP32_WORST[name], 2.0)


def test_kink_share(measured):
    """A condition on the inputs, not a measurement of a kernel: the elements a ReLU / LeakyReLU case leaves unjudged."""
    _, kinks = measured
    over = [(shape, act, k, n) for (shape, act), (k, n) in kinks.items()
            if k > (1e-5 * n if act != "none" and n >= 100_000 else 0)]
    assert not over, over
    big = {s: kn for (s, a), kn in kinks.items() if a == "relu" and kn[1] >= 100_000}
    print("\nkink elements (of elements):", {s: kn for s, kn in big.items()})


# --------------------------------------------------------------------------------------- 4. the cases reach their paths
def _hw(shape):
    hw = 1
    for d in shape[2:]:
        hw *= d
    return hw


@pytest.mark.parametrize("shape", list(R.SHAPES_2D))
def test_cases_reach_their_paths(shape):
    ns_sums, ns_apply, path = R.SHAPES_2D[shape]
    B, C, HW = shape[0], shape[1], _hw(shape)
    assert R.make_slicing(B, C, HW)[0] == ns_sums
    assert R.make_apply_slicing(B, C, HW)[0] == ns_apply
    assert R.bwd_path(B, C, HW) == path
    total = B * HW
    for ns, per in (R.make_slicing(B, C, HW), R.make_apply_slicing(B, C, HW)):
        assert per % 4 == 0 and (ns - 1) * per < total <= ns * per
    assert ns_sums <= R.NS_MAX          # the partials of a channel fit the workspace


def test_named_edges():
    """What the cases are named for, beyond the counts."""
    S, A = R.make_slicing, R.make_apply_slicing
    # scalar loops with both passes sliced and ragged last slices
    assert 441 % 4 != 0 and 4410 % S(10, 5, 441)[1] != 0 and 4410 % A(10, 5, 441)[1] != 0
    # vector loops: a plane that is no power of two, ragged last slices
    assert 100 % 4 == 0 and 100 & 99 and 5000 % S(50, 3, 100)[1] != 0 and 5000 % A(50, 3, 100)[1] != 0
    assert 2048 // 2304 == 0 and S(2, 2304, 4)[0] == 1                       # ns clamped up to 1
    assert 2048 // 3 > R.NS_MAX and S(17, 3, 4096)[0] == R.NS_MAX          # ... and capped at 64
    # the one pass: its thresholds, C = 127 against 128, a ragged last vector on the division path
    assert R.bwd_path(1, 128, 4) == "one<2>" and R.bwd_path(1, 128, 2) == "two"
    assert R.bwd_path(32, 128, 256) == "one<2>" and R.bwd_path(683, 128, 12) == "one<8>"
    assert 32 * 256 == 8192 and 683 * 12 == 8196 and 128 * 256 == 32768 and 2731 * 12 == 32772
    assert R.bwd_path(128, 128, 256) == "one<8>" and R.bwd_path(2731, 128, 12) == "two"
    assert R.bwd_path(8, 127, 16) == "two" and R.bwd_path(8, 128, 16) == "one<2>"
    assert 12 & 11 and (8196 // 4) % R.ONE_NT != 0 and (4100 // 4) % R.ONE_NT != 0
    assert R.bwd_path(32, 128, 256, aligned=False) == "two"
    # the three regimes of the slot finalisation, each from both sides
    regimes = [R.finalize_regime(n) for n in R.SLOT_CASES]
    assert [R.finalize_regime(n) for n in (64, 65, 4096, 4097)] == ["small", "wide", "wide", "split"]
    assert {64, 65, 4096, 4097} <= set(R.SLOT_CASES) and set(regimes) == {"small", "wide", "split"}
    for n, Cs in R.SLOT_CASES.items():
        assert len(Cs) == 2 and set(Cs) <= {1, 7, 8, 9, 31, 32, 33, 70}
    for C in (1, 7, 8, 9, 31, 32, 33, 70):
        assert any(C in Cs for Cs in R.SLOT_CASES.values())
