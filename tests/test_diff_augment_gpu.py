"""GPU: vg_diff_augment_fwd / _bwd per element against the fp64 reference of tests/_augment_refs.py.

Shapes (B, C, H, W).  The sum pass gives a workgroup 4096 elements of an image (VG_DIFF_AUGMENT_SUM_CHUNK), so a
3 x 64 x 64 image already spans three chunks; (2, 3, 128, 128) spans twelve; (2, 3, 37, 39) spans two, the second one
partial, with an odd element count: image 1 starts off a 16-byte boundary and takes the element path of the sum where
image 0 takes the 16-byte path.  (2, 3, 7, 5): odd cut sizes, H != W, every image misaligned.  (3, 1, 8, 8): r = 1, k = 4.
(2, 4, 16, 24): not square -- a row / column swap shows.

Tolerance with the colour step: 256 * 2^-24 * (max|x| + 1/2) per element forward, 256 * 2^-24 * max|gy| backward --
derived, not measured: an output is formed by about a dozen fp32 roundings of intermediates no larger than
10 (max|x| + 1/2) (s <= 2, c <= 3/2, the means summed in fp64); a wrong pixel, factor or mean is off by 1e-2 .. 1 on
U(-1, 1) inputs.  Without the colour step, and for every image whose gate is closed, outputs and gradients are copies
and zeros: compared bit for bit.

The adjoint identity <gy, A x> = <A^T gy, x>, A x = fwd(x) - fwd(0), is evaluated in fp64 on the kernel's outputs per
image and compared to the same relative bound times sqrt(C H W), scaled by the magnitudes of the two factors:
256 * 2^-24 * sqrt(C H W) * (max|x| + 1/2) * max|gy|."""
import math

import pytest
import torch

import _augment_refs as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 64, 64), (5, 3, 64, 64), (3, 1, 8, 8), (2, 3, 7, 5), (2, 4, 16, 24), (2, 3, 128, 128), (2, 3, 37, 39)]
EXTREME_SHAPES = [(3, 64, 64), (1, 8, 8), (3, 7, 5), (4, 16, 24), (3, 37, 39)]      # (C, H, W): a batch of R.extreme_rows
REL = 256 * 2.0 ** -24


def _inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = 2 * torch.rand(B, C, H, W, generator=g) - 1
    gy = 2 * torch.rand(B, C, H, W, generator=g) - 1
    u = torch.rand(B, 8, generator=g)
    return x, gy, u


def _run(x, gy, u, policy, p):
    from disentangle_mlp_amd import ops
    xd, gd, ud = x.cuda(), gy.cuda(), u.cuda()
    y = ops.diff_augment_fwd(xd, ud, policy, p)
    gx = ops.diff_augment_bwd(gd, ud, policy, p)
    y0 = ops.diff_augment_fwd(torch.zeros_like(xd), ud, policy, p)
    torch.cuda.synchronize()
    return y.cpu(), gx.cpu(), y0.cpu()


def _check(x, gy, u, policy, p, what):
    y, gx, y0 = _run(x, gy, u, policy, p)
    ry, rgx = R.augment(x, u, policy, p), R.transpose(gy, u, policy, p)
    B, C, H, W = x.shape
    tol_f = REL * (float(x.abs().max()) + 0.5)
    tol_b = REL * float(gy.abs().max())
    err_f, err_b = float((y.double() - ry).abs().max()), float((gx.double() - rgx).abs().max())
    print(f"{what} policy {policy} p {p}: fwd err {err_f:.3e} (tol {tol_f:.3e}), bwd err {err_b:.3e} (tol {tol_b:.3e})")
    if policy & R.COLOR:
        assert err_f <= tol_f and err_b <= tol_b, (what, policy, p, err_f, tol_f, err_b, tol_b)
    else:                                               # copies and zeros
        assert torch.equal(y.double(), ry) and torch.equal(gx.double(), rgx), (what, policy, p)
    closed = [b for b in range(B) if not R.is_open(u[b], p)]
    for b in closed:                                    # bit copies under every policy
        assert torch.equal(y[b], x[b]) and torch.equal(gx[b], gy[b]), (what, policy, p, b)
    # adjoint identity on the kernel's own outputs, per image, in fp64
    lhs = (gy.double() * (y.double() - y0.double())).flatten(1).sum(1)
    rhs = (gx.double() * x.double()).flatten(1).sum(1)
    bound = REL * math.sqrt(C * H * W) * (float(x.abs().max()) + 0.5) * float(gy.abs().max())
    gap = float((lhs - rhs).abs().max())
    print(f"{what} policy {policy} p {p}: adjoint gap {gap:.3e} (bound {bound:.3e})")
    assert gap <= bound, (what, policy, p, gap, bound)
    return closed


@pytest.mark.parametrize("policy", sorted(R.POLICIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_rows_against_reference(shape, policy):
    x, gy, u = _inputs(*shape, seed=1000 * policy + shape[2] + shape[0])
    _check(x, gy, u, policy, 1.0, shape)
    u[:, 7] = torch.tensor([0.25, 0.75, 0.5, 0.1, 0.9])[:shape[0]]          # p = 0.5: open, closed, u7 == p (closed), ...
    closed = _check(x, gy, u, policy, 0.5, shape)
    assert closed == [b for b in (1, 2, 4) if b < shape[0]]


@pytest.mark.parametrize("policy", sorted(R.POLICIES))
@pytest.mark.parametrize("chw", EXTREME_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_extreme_rows_against_reference(chw, policy):
    """The largest shifts in all four directions, cut centres at 0 and n - 1 on both axes, s = 0, c at both ends, u7 on
    both sides of p = 0.5 and equal to it."""
    u = R.extreme_rows(0.5)
    x, gy, _ = _inputs(u.shape[0], *chw, seed=77 * policy + chw[1])
    closed = _check(x, gy, u, policy, 0.5, chw)
    assert closed == [9, 10]
    assert _check(x, gy, u, policy, 1.0, chw) == []
    H, W = chw[1:]
    rh, rw = R.radius(H), R.radius(W)
    assert [(R.shift_of(float(r[3]), H), R.shift_of(float(r[4]), W)) for r in u[:4]] == [(-rh, -rw), (rh, rw), (-rh, rw), (rh, -rw)]
    assert [R.pick(float(u[i][5]), R.cut_count(H)) for i in (2, 3)] == [0, R.cut_count(H) - 1]


@pytest.mark.parametrize("policy", sorted(R.POLICIES))
def test_p_zero_is_a_copy_of_everything(policy):
    x, gy, u = _inputs(3, 3, 7, 5, seed=policy)
    y, gx, _ = _run(x, gy, u, policy, 0.0)
    assert torch.equal(y, x) and torch.equal(gx, gy)


@pytest.mark.parametrize("policy", [1, 7])
@pytest.mark.parametrize("chw", [(3, 64, 64), (3, 7, 5), (3, 37, 39)], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_every_run_and_at_every_batch_index(chw, policy):
    x, gy, u = _inputs(5, *chw, seed=5)
    x[4], gy[4], u[4] = x[0], gy[0], u[0]
    y, gx, _ = _run(x, gy, u, policy, 1.0)
    y2, gx2, _ = _run(x, gy, u, policy, 1.0)
    assert torch.equal(y, y2) and torch.equal(gx, gx2)                       # two runs
    assert torch.equal(y[4], y[0]) and torch.equal(gx[4], gx[0])              # batch index 0 and 4
    y1, gx1, _ = _run(x[:1], gy[:1], u[:1], policy, 1.0)                       # ... and alone
    assert torch.equal(y1[0], y[0]) and torch.equal(gx1[0], gx[0])


def test_autograd_function_saves_u_only_and_matches_the_ops():
    from disentangle_mlp_amd import functional as F, ops
    x, gy, u = _inputs(4, 3, 64, 64, seed=9)
    xd, gd, ud = x.cuda().requires_grad_(), gy.cuda(), u.cuda()
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = F.diff_augment(xd, ud, "cutout,color,translation", 0.75)
    assert len(saved) == 1 and saved[0].data_ptr() == ud.data_ptr()           # u, never x
    y.backward(gd)
    assert torch.equal(y.detach(), ops.diff_augment_fwd(xd.detach(), ud, 7, 0.75))
    assert torch.equal(xd.grad, ops.diff_augment_bwd(gd, ud, 7, 0.75))
    assert ud.grad is None


def test_both_directions_replay_from_a_graph_with_fresh_uniforms():
    """No host read and no allocation inside: captured once, replayed with new rows of u, the bits of an eager call."""
    from disentangle_mlp_amd import ops
    x, gy, u = _inputs(4, 3, 64, 64, seed=11)
    xd, gd, ud = x.cuda(), gy.cuda(), u.cuda()
    ops.diff_augment_fwd(xd, ud, 7, 1.0)                                      # (the workspace exists)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    us = ud.clone()
    with torch.cuda.graph(graph):
        y = ops.diff_augment_fwd(xd, us, 7, 1.0)
        gx = ops.diff_augment_bwd(gd, us, 7, 1.0)
    for seed in (1, 2):
        fresh = torch.rand(4, 8, generator=torch.Generator().manual_seed(seed)).cuda()
        us.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, ops.diff_augment_fwd(xd, fresh, 7, 1.0)) and torch.equal(gx, ops.diff_augment_bwd(gd, fresh, 7, 1.0))
