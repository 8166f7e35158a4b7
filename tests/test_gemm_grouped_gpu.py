"""GPU: the grouped Linear GEMM (vg_gemm_nt_f16x3_grouped, csrc/gemm_split.hip) and what is built on it.

The grouped entry promises that every C_g is BIT FOR BIT what the single-call entry returns for A_g alone (same tiling,
K slicing, MFMA order per group, epilogue and slab sum), so bit identity is the check all the way up: the kernel, the
autograd Function and one trainer iteration.  The groups' magnitudes are three decades apart each, so that a group
scaled or unscaled by another group's bound cannot pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALES = (1e-3, 1.0, 1e3)
MS = (1, 5, 128, 130)          # below, at and just over one 128-row tile


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


def _operands(layout, M, N, K, G, seed):
    """A_g (G of them), B and the stride arguments of one layout; the tensors are stored as the layout reads them."""
    g = torch.Generator().manual_seed(seed)
    a_shape = (K, M) if layout == "wgrad" else (M, K)
    b_shape = (N, K) if layout == "fwd" else (K, N)
    As = [(torch.randn(a_shape, generator=g) * SCALES[i]).cuda() for i in range(G)]
    B = (torch.randn(b_shape, generator=g) * 0.02).cuda()
    strides = {"fwd": (K, 1, K, 1),           # both reductions contiguous
               "dgrad": (K, 1, 1, N),         # B's rows strided (the weight read as [k][n])
               "wgrad": (1, M, 1, N)}[layout]  # both operands strided
    return As, B, strides


def _bounds(ts):
    return [t.abs().max().reshape(1) for t in ts]


def _as_matrix(layout, t, which):
    """The operand as the (rows, K) matrix the GEMM multiplies."""
    if which == "A":
        return t.t() if layout == "wgrad" else t
    return t if layout == "fwd" else t.t()


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N,K", [(136, 64), (128, 1024)], ids=["nosplit", "ksplit"])
@pytest.mark.parametrize("layout", ["fwd", "dgrad", "wgrad"])
def test_grouped_is_bitwise_the_single_call(H, layout, N, K, bias):
    """G = 1, 2, 3 at M = 1, 5, 128, 130: N = 136, K = 64 (a ragged second column tile, no K split) and N = 128,
    K = 1024 (one column tile: the reduction is split over workgroups, slabs per group)."""
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    for M in MS:
        assert (lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K) > 0) == (K == 1024)
        As, B, st = _operands(layout, M, N, K, 3, seed=M + N + K)
        bv = torch.randn(N, generator=torch.Generator().manual_seed(7)).cuda() if bias else None
        am, bm = _bounds(As), _bounds([B])[0]
        single = [H._gemm_nt(As[i], B, bv, torch.empty(M, N, device="cuda"), M, N, K, *st, am[i], bm) for i in range(3)]
        for G in (1, 2, 3):
            # the groups in an order of their own: group 0 is not always the small one
            order = [(G - 1 - i) for i in range(G)]
            Cs = [torch.full((M, N), float("nan"), device="cuda") for _ in order]
            H._gemm_nt_grouped([As[i] for i in order], B, bv, Cs, M, N, K, *st, [am[i] for i in order], bm)
            for c, i in zip(Cs, order):
                assert torch.equal(c, single[i]), (layout, M, N, K, G, i, float((c - single[i]).abs().max()))


@pytest.mark.parametrize("layout", ["fwd", "dgrad", "wgrad"])
def test_grouped_vs_fp64(H, layout):
    """Every group against an fp64 matmul at the bound of the Linear GEMM's own test (test_kernels_gpu.py:
    test_linear_gemms_fp16x3_vs_fp64: relative L2 and worst element over the largest output <= 3e-6)."""
    M, N, K = 130, 136, 1024
    As, B, st = _operands(layout, M, N, K, 3, seed=3)
    bv = torch.randn(N, generator=torch.Generator().manual_seed(8)).cuda() * 1e-3
    Cs = [torch.empty(M, N, device="cuda") for _ in As]
    H._gemm_nt_grouped(As, B, bv, Cs, M, N, K, *st, _bounds(As), _bounds([B])[0])
    for i, (a, c) in enumerate(zip(As, Cs)):
        ref = _as_matrix(layout, a, "A").double() @ _as_matrix(layout, B, "B").double().t() + bv.double()
        rel = float((c.double() - ref).norm() / ref.norm())
        worst = float((c.double() - ref).abs().max() / ref.abs().max())
        print(layout, "group", i, "rel", rel, "worst", worst)
        assert rel <= 3e-6 and worst <= 3e-6, (layout, i, rel, worst)


@pytest.mark.parametrize("protocols", [False, True], ids=["plain", "deferred+accumulate"])
def test_grouped_linear_fn_is_bitwise_separate_calls(H, monkeypatch, protocols):
    """functional.linear_grouped against G separate functional.linear calls at M = 8 on a 64 x 32 weight forced onto the
    package's GEMM: outputs, input gradients, weight and bias gradient, with one input that requires no gradient --
    outside and inside deferred_wgrad() + accumulate_param_grads() (the trainers' discriminator phase)."""
    from contextlib import ExitStack
    from disentangle_mlp_amd import functional as F
    monkeypatch.setattr(H, "LINEAR_SPLIT_MIN_WEIGHTS", 0)
    monkeypatch.setattr(F, "DEFER_MIN_WEIGHTS", 0)
    assert H.linear_split_ok(32, 64 * 32) and H.linear_split_ok(64, 64 * 32)
    g = torch.Generator().manual_seed(21)
    x0 = [(torch.randn(8, 32, generator=g) * s).cuda() for s in SCALES]
    w0, b0 = (torch.randn(64, 32, generator=g) * 0.1).cuda(), torch.randn(64, generator=g).cuda()
    coef = [torch.randn(8, 64, generator=g).cuda() for _ in SCALES]
    calls = []
    real = H.linear_fwd_grouped
    monkeypatch.setattr(H, "linear_fwd_grouped", lambda xs, w, b: calls.append(len(xs)) or real(xs, w, b))
    res = []
    for grouped in (False, True):
        xs = [x.clone().requires_grad_(i != 1) for i, x in enumerate(x0)]
        w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        with ExitStack() as stack:
            if protocols:
                stack.enter_context(F.accumulate_param_grads())
                stack.enter_context(F.deferred_wgrad())
            ys = F.linear_grouped(xs, w, b) if grouped else [F.linear(x, w, b) for x in xs]
            torch.autograd.backward([(y * c).sum() for y, c in zip(ys, coef)])
        assert xs[1].grad is None
        res.append([y.detach() for y in ys] + [xs[0].grad, xs[2].grad, w.grad, b.grad])
    assert calls == [3]
    for i, (a, b_) in enumerate(zip(*res)):
        assert torch.equal(a, b_), (i, float((a - b_).abs().max()))


def test_detached_group_takes_no_part_in_the_backward(H, monkeypatch):
    """A group made as under no_grad: its output needs no gradient and the frozen-weight phase's other groups get theirs."""
    from disentangle_mlp_amd import functional as F
    monkeypatch.setattr(H, "LINEAR_SPLIT_MIN_WEIGHTS", 0)
    g = torch.Generator().manual_seed(22)
    x0 = [torch.randn(8, 32, generator=g).cuda() for _ in range(3)]
    w, b = (torch.randn(64, 32, generator=g) * 0.1).cuda(), torch.randn(64, generator=g).cuda()      # frozen
    xs = [x0[0]] + [x.clone().requires_grad_(True) for x in x0[1:]]
    ys = F.linear_grouped(xs, w, b, detached=(True, False, False))
    assert not ys[0].requires_grad and ys[1].requires_grad and ys[2].requires_grad
    ((ys[1] - ys[0]) ** 2).sum().backward()               # the sim loss's shape: only group 1 gets a gradient
    ref = x0[1].clone().requires_grad_(True)
    with torch.no_grad():
        y0 = F.linear(x0[0], w, b)
    ((F.linear(ref, w, b) - y0) ** 2).sum().backward()
    assert torch.equal(ys[0], y0) and torch.equal(xs[1].grad, ref.grad) and xs[2].grad is None


def test_trainer_iteration_grouped_is_bitwise_per_pass(H, monkeypatch):
    """One beta-VAE-GAN iteration at batch 4 with the discriminator's passes grouped (2 in phase 1, 3 in phase 2)
    against the same iteration pass by pass (model.GROUP_PASSES): all nine losses and every parameter and buffer."""
    from disentangle_mlp_amd import model, trainer
    from oracle import steps as osteps
    b = {k: v.cuda() for k, v in osteps.synthetic_batch(4).items()}
    fwd, dgrad = [], []
    real_f, real_d = H.linear_fwd_grouped, H.linear_dgrad_grouped
    monkeypatch.setattr(H, "linear_fwd_grouped", lambda xs, w, bias: fwd.append(len(xs)) or real_f(xs, w, bias))
    monkeypatch.setattr(H, "linear_dgrad_grouped", lambda gys, w: dgrad.append(len(gys)) or real_d(gys, w))
    runs = []
    for grouped in (False, True):
        monkeypatch.setattr(model, "GROUP_PASSES", grouped)
        tr = trainer.BetaVAEGANTrainer(beta=25.0)
        out = tr.step(b["data"], b["noise"], b["eps2"], b["eps3"])
        state = {**{"eg." + k: v for k, v in tr.netEG.state_dict().items()},
                 **{"d." + k: v for k, v in tr.netD.state_dict().items()}}
        runs.append(({k: v.clone() for k, v in out.items()}, {k: v.clone() for k, v in state.items()}))
        if not grouped:
            assert fwd == [] and dgrad == []
    assert fwd == [2, 3] and dgrad == [2, 2]
    assert len(runs[0][0]) == 9
    for part in (0, 1):
        for k in runs[0][part]:
            assert torch.equal(runs[0][part][k], runs[1][part][k]), k
