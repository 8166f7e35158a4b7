"""GPU: the device-word twins of the augmentation kernels (vg_diff_augment_fwd_dev / _bwd_dev) and the controller of p
(vg_ada_update) -- DESIGN.md section 4.35.  Exact throughout: the twins against the value entry points bit for bit (and
against the fp64 reference of tests/_augment_refs.py at the tolerance tests/test_diff_augment_gpu.py derives), the
controller's eight words against the NumPy restatement of tests/_ada_refs.py after every call.

Shapes of the twins: (2, 3, 64, 64) is three 4096-element sum chunks per image with the chunk edge inside a plane,
(2, 4, 33, 31) an odd element count (image 1 off a 16-byte boundary), (3, 1, 2, 2) the smallest image there is.  Sizes of
the controller: 1, 63, 64, 65 (a lane, a wavefront and its edges), 257 and 1000 (past the 256-thread workgroup: a thread
takes more than one element)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import _ada_refs as A
import _augment_refs as R
from test_diff_augment_gpu import REL, _inputs

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 3, 8, 8), (5, 3, 16, 16), (3, 1, 2, 2), (2, 4, 33, 31), (2, 3, 64, 64)]
SIZES = (1, 63, 64, 65, 257, 1000)


def _word(value):
    return torch.tensor([value], dtype=torch.float32).cuda()


def _plants(p):
    """u7 at p, at its fp32 neighbours and at ALMOST_ONE -- kept inside [0, 1]."""
    lo, at, hi = A.neighbours(p)
    return [max(lo, 0.0), at, min(hi, 1.0), R.ALMOST_ONE]


# ---- the twins --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", sorted(R.POLICIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dev_twins_give_the_value_twins_bits(shape, policy):
    from disentangle_mlp_amd import ops
    B, C, H, W = shape
    x, gy, u = _inputs(*shape, seed=300 * policy + H + B)
    xd, gd = x.cuda(), gy.cuda()
    tol_f, tol_b = REL * (float(x.abs().max()) + 0.5), REL * float(gy.abs().max())
    for p in (0.0, 0.3, 1.0):
        plants = _plants(p)
        word = _word(p)
        for rnd in range(-(-len(plants) // B)):                        # every plant on some image, whatever B is
            u[:, 7] = torch.tensor([plants[(rnd * B + b) % len(plants)] for b in range(B)])
            ud = u.cuda()
            y, gx = ops.diff_augment_fwd(xd, ud, policy, p), ops.diff_augment_bwd(gd, ud, policy, p)
            yw, gxw = ops.diff_augment_fwd(xd, ud, policy, word), ops.diff_augment_bwd(gd, ud, policy, word)
            torch.cuda.synchronize()
            assert torch.equal(yw, y) and torch.equal(gxw, gx), (shape, policy, p, rnd)
            yw, gxw = yw.cpu(), gxw.cpu()
            ry, rgx = R.augment(x, u, policy, p), R.transpose(gy, u, policy, p)
            err_f, err_b = float((yw.double() - ry).abs().max()), float((gxw.double() - rgx).abs().max())
            if policy & R.COLOR:
                assert err_f <= tol_f and err_b <= tol_b, (shape, policy, p, rnd, err_f, tol_f, err_b, tol_b)
            else:                                                       # copies and zeros
                assert torch.equal(yw.double(), ry) and torch.equal(gxw.double(), rgx), (shape, policy, p, rnd)
            for b in range(B):
                if not R.is_open(u[b], p):                                       # bit copies under every policy
                    assert torch.equal(yw[b], x[b]) and torch.equal(gxw[b], gy[b]), (shape, policy, p, rnd, b)
        assert float(word) == float(F32(p))                             # the kernels only read the word


@pytest.mark.parametrize("policy", sorted(R.POLICIES))
def test_a_nan_word_closes_every_image(policy):
    from disentangle_mlp_amd import ops
    x, gy, u = _inputs(5, 3, 16, 16, seed=policy)
    u[:, 7] = torch.tensor([0.0, 0.5, R.ALMOST_ONE, 0.25, 0.75])
    xd, gd, ud, word = x.cuda(), gy.cuda(), u.cuda(), _word(NAN)
    assert torch.equal(ops.diff_augment_fwd(xd, ud, policy, word), xd)
    assert torch.equal(ops.diff_augment_bwd(gd, ud, policy, word), gd)
    # ... and a word outside [0, 1] is compared as it is: above every uniform opens everything, below 0 closes everything
    assert torch.equal(ops.diff_augment_fwd(xd, ud, policy, _word(2.0)), ops.diff_augment_fwd(xd, ud, policy, 1.0))
    assert torch.equal(ops.diff_augment_fwd(xd, ud, policy, _word(-1.0)), xd)


def test_autograd_function_takes_the_word_and_saves_u_only():
    from disentangle_mlp_amd import functional as F, ops
    x, gy, u = _inputs(4, 3, 16, 16, seed=9)
    u[:, 7] = torch.tensor([0.1, 0.4, 0.6, 0.9])
    xd, gd, ud, word = x.cuda().requires_grad_(), gy.cuda(), u.cuda(), _word(0.5)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = F.diff_augment(xd, ud, "cutout,color,translation", word)
    assert len(saved) == 1 and saved[0].data_ptr() == ud.data_ptr()    # u, never x, never the word
    word.fill_(0.75)                                                    # held by reference: the backward reads it when it runs
    y.backward(gd)
    assert torch.equal(y.detach(), ops.diff_augment_fwd(xd.detach(), ud, 7, 0.5))
    assert torch.equal(xd.grad, ops.diff_augment_bwd(gd, ud, 7, 0.75))
    assert ud.grad is None and word.grad is None


# ---- the controller -----------------------------------------------------------------------------------------------------------
def _vector(kind, n, threshold):
    lo, at, hi = A.neighbours(threshold)
    if kind == "above":
        v = [threshold + 1.0] * n
    elif kind == "below":
        v = [threshold - 1.0] * n
    elif kind == "ties":
        v = [at] * n
    elif kind == "near":                                                # fp32 neighbours on both sides, one more above
        v = [(hi, lo, hi, at, lo, hi, hi)[i % 7] for i in range(n)]
    elif kind == "special":
        v = [(NAN, INF, -INF, NAN, INF, threshold, INF)[i % 7] for i in range(n)]
    else:                                                               # "zeros": +-0, ties of a threshold 0 of either sign
        v = [(0.0, -0.0)[i % 2] for i in range(n)]
    return np.array(v, dtype=F32)


SEQUENCES = {"up_first": ("above", "above", "above", "above", "below", "ties", "near", "below", "special"),
             "down_first": ("below", "ties", "below", "near", "above", "above", "special", "above", "zeros")}


@pytest.mark.parametrize("interval", (1, 4))
@pytest.mark.parametrize("B", SIZES)
def test_controller_words_equal_the_restatement_after_every_call(B, interval):
    from disentangle_mlp_amd import ops
    rate = 0.7 / (B * interval)                                         # an adjustment moves p by about 0.7: both clamps are met
    seen_p, inexact = set(), False
    for threshold in (0.5, 0.0, -0.0):
        for name, kinds in SEQUENCES.items():
            state, st = ops.ada_state("cuda", 0.5), A.state(0.5)
            assert np.array_equal(state.cpu().numpy(), A.words(st))
            for k, kind in enumerate(kinds):
                # a different size in the last call of every other interval: the step is count * rate, not interval * B * rate
                n = B + 3 if (k % interval == interval - 1 and (k // interval) % 2 == 0) else B
                d = _vector(kind, n, threshold)
                if st["calls"] + 1 >= interval:
                    count = st["count"] + n
                    inexact |= Fraction(float(F32(count))) * Fraction(float(F32(rate))) != Fraction(float(F32(count) * F32(rate)))
                st = A.update(st, d, threshold, 0.6, rate, interval)
                ops.ada_update(torch.from_numpy(d).cuda(), state, threshold, 0.6, rate, interval)
                got = state.cpu().numpy()
                assert np.array_equal(got, A.words(st)), (B, interval, threshold, name, k, kind, got, A.words(st))
                seen_p.add(float(st["p"]))
            assert ops.ada_read(state) == {w: (float(st[w]) if w in ("p", "rt") else st[w]) for w in A.WORDS}
            assert st["adjustments"] == 9 // interval and st["calls"] == 9 % interval
    assert 0.0 in seen_p and 1.0 in seen_p                              # p was driven into both clamps
    assert len(seen_p) >= 3                                             # ... and stood between them
    if B in (63, 257, 1000):
        assert inexact                                                  # count * rate was rounded: what the no-FMA rule is for


def _fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, from exact rationals."""
    exact = Fraction(float(F32(a))) * Fraction(float(F32(b))) + Fraction(float(F32(c)))
    near = F32(float(exact))                                            # (a double first: off by at most one fp32 step)
    cands = (near, np.nextafter(near, F32(INF)), np.nextafter(near, F32(-INF)))
    return min(cands, key=lambda v: abs(Fraction(float(v)) - exact))


@pytest.mark.parametrize("count,rate,p0", [(257, 0.001, 0.5), (1000, 1.0 / 3000.0, 0.5)])
def test_the_step_is_a_rounded_product_and_a_rounded_sum_not_an_fma(count, rate, p0):
    from disentangle_mlp_amd import ops
    two = F32(p0) + F32(count) * F32(rate)
    assert two != _fma32(count, rate, p0) and 0 < two < 1               # the case can tell the two apart
    state = ops.ada_state("cuda", p0)
    ops.ada_update(torch.ones(count).cuda(), state, 0.0, 0.6, rate, 1)
    assert ops.ada_read(state)["p"] == float(two)
    # ... and downwards
    two = F32(p0) - F32(count) * F32(rate)
    state = ops.ada_state("cuda", p0)
    ops.ada_update(-torch.ones(count).cuda(), state, 0.0, 0.6, rate, 1)
    assert ops.ada_read(state)["p"] == float(two)


def test_a_tie_of_r_t_with_the_target_leaves_p():
    from disentangle_mlp_amd import ops
    state = ops.ada_state("cuda", 0.3)
    d = torch.tensor([1.0, 1.0, 1.0, -1.0]).cuda()
    ops.ada_update(d, state, 0.0, 0.5, 1 / 64, 1)                       # r_t = 2/4 == target
    assert ops.ada_read(state) == dict(p=float(F32(0.3)), sign_sum=0, count=0, calls=0, rt=0.5, adjustments=1)
    ops.ada_update(d, state, 0.0, 0.5, 3e38, 1)                         # ... also where count * rate overflows
    assert ops.ada_read(state)["p"] == float(F32(0.3))


# ---- one graph: forward + backward on the word, then the controller ---------------------------------------------------------
def _captured_run(captured):
    """Six iterations of [augment forward, backward on the word; controller] -- replays of one graph, or eager calls.
    Returns per iteration (y, gx, the eight words) on the host."""
    from disentangle_mlp_amd import ops
    B, policy, rate = 8, 7, 1.0 / 32.0                                   # interval 1: p moves by 8/32 = 0.25 per call
    x, gy, u = _inputs(B, 3, 16, 16, seed=21)
    u[:, 7] = torch.tensor([0.0, 0.2, 0.25, 0.3, 0.5, 0.7, 0.75, R.ALMOST_ONE])
    xd, gd, ud = x.cuda(), gy.cuda(), u.cuda()
    state = ops.ada_state("cuda", 0.25)
    word = state[0:1].view(torch.float32)
    d = torch.zeros(B).cuda()
    ops.diff_augment_fwd(xd, ud, policy, 1.0)                            # (the workspace exists)
    torch.cuda.synchronize()

    def body():
        y = ops.diff_augment_fwd(xd, ud, policy, word)
        gx = ops.diff_augment_bwd(gd, ud, policy, word)
        ops.ada_update(d, state, 0.0, 0.6, rate, 1)
        return y, gx

    if captured:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y, gx = body()
    out = []
    for sign in (1.0, 1.0, 1.0, -1.0, -1.0, 1.0):                         # p: 0.25 -> 0.5 -> 0.75 -> 1 -> 0.75 -> 0.5 -> 0.75
        d.fill_(sign)
        if captured:
            graph.replay()
        else:
            y, gx = body()
        torch.cuda.synchronize()
        out.append((y.cpu().clone(), gx.cpu().clone(), state.cpu().clone()))
    return x, gy, u, out


def test_one_graph_replays_a_moving_p_and_equals_eager():
    x, gy, u, cap = _captured_run(True)
    _, _, _, eager = _captured_run(False)
    _, _, _, again = _captured_run(True)
    st = A.state(0.25)
    opened = []
    for it, sign in enumerate((1.0, 1.0, 1.0, -1.0, -1.0, 1.0)):
        p_used = float(st["p"])                                         # the p the previous iteration left
        st = A.update(st, np.full(8, sign, dtype=F32), 0.0, 0.6, 1.0 / 32.0, 1)
        y, gx, words = cap[it]
        assert np.array_equal(words.numpy(), A.words(st)), it
        is_open = [R.is_open(u[b], p_used) for b in range(8)]
        opened.append(sum(is_open))
        for b in range(8):                                              # closed: bit copies; open: not a copy (policy 7 moves every image)
            assert torch.equal(y[b], x[b]) == (not is_open[b]) and torch.equal(gx[b], gy[b]) == (not is_open[b]), (it, b)
        for other in (eager, again):                                    # the eager twin, and a second captured run: the same bits
            assert all(torch.equal(a, b) for a, b in zip(cap[it], other[it])), it
    assert opened == [2, 4, 6, 8, 6, 4]                                 # p crossed the planted u7 in both directions
