"""GPU: FactorVAE's kernels (csrc/factor_vae.hip) -- ``permute_dims`` against torch's stable argsort
and gather, bit for bit; the encoder phase's loss and the critic's loss against the fp64 restatements of
tests/_factor_refs.py; `model.LatentCritic` against torch.nn modules carrying the same weights.

Bound of every parity check, per tensor: max error over the reference's largest magnitude <= max(1e-6, 5 x the same figure
of the restatement evaluated in fp32) -- the project's convention (tests/test_reparam_klc_gpu.py::_check); each check prints
its figures before it asserts (``pytest -s``)."""
import numpy as np
import pytest
import torch

import _factor_refs as R

pytestmark = pytest.mark.gpu

KL = 37.25


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(what, got, r32, r64):
    e, b = R.rel_err(got, r64), R.bound(r32, r64)
    print(f"{what}: error {e:.3e}  bound {b:.3e}  (fp32 restatement {R.rel_err(r32, r64):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert e <= b, (what, e, b)


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


def _zu(B, D, seed=0):
    g = torch.Generator().manual_seed(100003 * B + D + seed)
    return torch.randn(B, D, generator=g).cuda(), torch.rand(B, D, generator=g).cuda()


def _argsort_gather(z, u):
    return z.gather(0, torch.argsort(u, dim=0, stable=True))


# ------------------------------------------------------------------ 1. permute_dims
# a single element; partial strips and partial row blocks; the LDS images of 256, 1024 and 2048 rows, at and across their edges
PERMUTE_SHAPES = [(1, 1), (2, 3), (63, 5), (64, 128), (65, 127), (128, 128), (257, 10), (1024, 128)]


@pytest.mark.parametrize("shape", PERMUTE_SHAPES, ids=str)
def test_permute_dims_is_the_stable_argsort_and_gather(H, shape):
    z, u = _zu(*shape)
    zp = H.permute_dims(z, u)
    assert torch.equal(_bits(zp), _bits(_argsort_gather(z, u)))
    assert torch.equal(zp.sort(0).values, z.sort(0).values)          # every column: a permutation of the input column
    assert torch.equal(_bits(H.permute_dims(z, u)), _bits(zp))       # the same bits on a second run


def test_permute_dims_at_the_stated_limit_and_beyond(H):
    top = H.PERMUTE_MAX_BATCH
    assert top >= 1024
    z, u = _zu(top, 3)
    zp = H.permute_dims(z, u)
    assert torch.equal(_bits(zp), _bits(_argsort_gather(z, u))) and torch.equal(zp.sort(0).values, z.sort(0).values)
    z, u = _zu(top + 1, 3)
    with pytest.raises(ValueError, match=f"above {top}"):
        H.permute_dims(z, u)
    with pytest.raises(RuntimeError, match="one shape"):
        H.permute_dims(z[:4], u[:5])


@pytest.mark.parametrize("shape", [(65, 127), (300, 17)], ids=str)
def test_permute_dims_breaks_ties_by_row_index(H, shape):
    z, u = _zu(*shape)
    q = torch.floor(u * 4) / 4                                        # four values: every column is mostly ties
    zp = H.permute_dims(z, q)
    assert torch.equal(_bits(zp), _bits(_argsort_gather(z, q))) and torch.equal(zp.sort(0).values, z.sort(0).values)
    assert torch.equal(_bits(H.permute_dims(z, torch.full_like(u, 0.5))), _bits(z))      # constant: the identity
    assert torch.equal(_bits(zp.cpu()), _bits(R.permute_dims(z.cpu(), q.cpu())))        # ... and the counting restatement


def test_permute_dims_orders_special_values_as_torch_sort_does(H):
    """-0 ties with +0, a subnormal is above 0, the infinities are the ends, every NaN is last and ties with every NaN: the
    order of torch's stable CPU sort (the uniforms of a trainer hold none of these; the kernel's ranks stay a permutation)."""
    g = torch.Generator().manual_seed(9)
    values = torch.tensor([float("-inf"), -1.0, -0.0, 0.0, 1e-40, 1.0, float("inf"), float("nan"), -float("nan")])
    u = values[torch.randint(len(values), (130, 19), generator=g)]
    z = torch.randn(130, 19, generator=g)
    want = z.gather(0, torch.argsort(u, dim=0, stable=True))
    zp = H.permute_dims(z.cuda(), u.cuda()).cpu()
    assert torch.equal(_bits(zp), _bits(want)) and torch.equal(zp.sort(0).values, z.sort(0).values)
    finite = torch.nan_to_num(u, nan=float("inf"))                    # (without NaNs: the counting restatement too)
    assert torch.equal(_bits(H.permute_dims(z.cuda(), finite.cuda()).cpu()), _bits(R.permute_dims(z, finite)))


def test_permute_dims_in_a_graph_replay_and_through_functional(H):
    from disentangle_mlp_amd import functional as Fn
    z, u = _zu(128, 128)
    want = H.permute_dims(z, u)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = H.permute_dims(z, u)
    graph.replay()
    assert torch.equal(_bits(out), _bits(want))
    u.copy_(torch.rand(128, 128, generator=torch.Generator().manual_seed(5)))      # the replay reads the inputs as they are now
    graph.replay()
    assert torch.equal(_bits(out), _bits(_argsort_gather(z, u))) and not torch.equal(out, want)
    zg = z.clone().requires_grad_(True)
    zp = Fn.permute_dims(zg, u)
    assert not zp.requires_grad and torch.equal(_bits(zp), _bits(out))             # a sample: no gradient flows


# ------------------------------------------------------------------ 2. the encoder phase's loss
_tc_cache = {}


def _tc_refs(B):
    if B not in _tc_cache:
        logits = R.make_logits(B)
        _tc_cache[B] = (logits, *(R.factor_tc(logits, KL, R.BETA, R.GAMMA, dtype=dt) for dt in (torch.float64, torch.float32)))
    return _tc_cache[B]


@pytest.mark.parametrize("B", R.ROWS)
def test_factor_tc_against_the_fp64_restatement(H, B):
    logits, r64, r32 = _tc_refs(B)
    dev, kl = logits.cuda(), torch.full((), KL, device="cuda")
    out4 = H.factor_tc_fwd(dev, kl, R.BETA, R.GAMMA)
    for n, name in enumerate(("loss", "kl", "tc")):
        _check(f"B={B} {name}", out4[n], r32[name], r64[name])
    print(f"B={B} rows with l0 > l1: {float(out4[3]):g}  reference {r64['first']}")
    assert float(out4[3]) == r64["first"] and float(out4[1]) == KL
    gloss = torch.full((), R.GLOSS, device="cuda")
    glogits, gkl = H.factor_tc_bwd(dev, gloss, R.BETA, R.GAMMA)
    _check(f"B={B} glogits", glogits, r32["glogits"], r64["glogits"])
    _check(f"B={B} gkl", gkl, r32["gkl"], r64["gkl"])
    assert torch.equal(glogits[:, 0], -glogits[:, 1]) and bool((glogits[:, 0] == glogits[0, 0]).all())      # the constant +-gamma*gloss
    # device words: the same bits, and read at every launch
    bw, gw = torch.full((1,), R.BETA, device="cuda"), torch.full((1,), R.GAMMA, device="cuda")
    assert torch.equal(_bits(H.factor_tc_fwd(dev, kl, bw, gw)), _bits(out4))
    a, b = H.factor_tc_bwd(dev, gloss, bw, gw)
    assert torch.equal(_bits(a), _bits(glogits)) and torch.equal(_bits(b), _bits(gkl))
    assert torch.equal(_bits(H.factor_tc_fwd(dev, kl, R.BETA, R.GAMMA)), _bits(out4))          # ... and run to run
    gw.fill_(0.0)
    zero = H.factor_tc_fwd(dev, kl, bw, gw)
    assert float(zero[0]) == np.float32(R.BETA) * np.float32(KL) and torch.equal(_bits(zero[1:]), _bits(out4[1:]))
    assert float(H.factor_tc_bwd(dev, gloss, bw, gw)[0].abs().max()) == 0.0
    if B == R.ROWS[0]:
        with pytest.raises(TypeError, match="both"):
            H.factor_tc_fwd(dev, kl, bw, R.GAMMA)
        with pytest.raises(TypeError, match="both"):
            H.factor_tc_bwd(dev, gloss, R.BETA, gw)
        with pytest.raises(RuntimeError, match="logits"):
            H.factor_tc_fwd(torch.zeros(4, 3, device="cuda"), kl, 1.0, 1.0)


def test_factor_tc_keeps_a_nan(H):
    logits = R.make_logits(65)
    logits[40, 1] = float("nan")
    out4 = H.factor_tc_fwd(logits.cuda(), torch.full((), KL, device="cuda"), R.BETA, R.GAMMA)
    assert bool(torch.isnan(out4[0])) and bool(torch.isnan(out4[2])) and float(out4[1]) == KL


# ------------------------------------------------------------------ 3. the critic phase's loss
_critic_cache = {}


def _critic_logits(B):
    return torch.cat([R.make_logits(B, 0), R.make_logits(B, 1)])      # the gaps in both halves: both classes saturate


def _critic_refs(B, div):
    if (B, div) not in _critic_cache:
        logits = _critic_logits(B)
        _critic_cache[(B, div)] = (logits, *(R.critic_loss(logits, div, dtype=dt) for dt in (torch.float64, torch.float32)))
    return _critic_cache[(B, div)]


@pytest.mark.parametrize("world", [1, 2], ids=["mean", "global-batch"])
@pytest.mark.parametrize("B", R.ROWS)
def test_factor_critic_loss_against_the_fp64_restatement(H, B, world):
    div = None if world == 1 else 2.0 * B * world
    logits, r64, r32 = _critic_refs(B, div)
    dev = logits.cuda()
    loss, glogits, acc = H.factor_critic_loss(dev, div)
    _check(f"B={B} loss", loss, r32["loss"], r64["loss"])
    _check(f"B={B} glogits", glogits, r32["glogits"], r64["glogits"])
    print(f"B={B} acc: {float(acc):.9g}  reference {r64['acc']:.9g}")
    assert float(acc) == float(np.float32(r64["acc"]))                # exact; the tie rows (gap 0) count as wrong
    # a saturated row: exactly 0, or exactly -+1/divisor, where the fp64 reference rounds to that
    ref, got = r64["glogits"], glogits.cpu()
    exact = (ref == 0) | (ref.abs() == 1.0 / (div if div is not None else 2.0 * B))
    print(f"B={B} saturated gradient elements: {int(exact.sum())} of {exact.numel()}")
    assert int(exact.sum()) >= (4 if B >= 9 else 0)
    assert torch.equal(got[exact].double(), ref[exact].float().double())
    assert torch.equal(got[:, 0], -got[:, 1])
    again = H.factor_critic_loss(dev, div)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, (loss, glogits, acc)))
    only = H.factor_critic_loss(dev, div, want_grad=False)
    assert only[1] is None and torch.equal(_bits(only[0]), _bits(loss)) and torch.equal(_bits(only[2]), _bits(acc))


def test_factor_critic_loss_ties_nan_and_bad_arguments(H):
    tie = torch.tensor([[0.5, 0.5], [1.0, 2.0], [3.0, 3.0], [2.0, 1.0]]).cuda()      # rows 0, 1: class 0; rows 2, 3: class 1
    loss, glogits, acc = H.factor_critic_loss(tie)
    assert float(acc) == 0.0                                          # two ties, two on the wrong side
    assert float(H.factor_critic_loss(tie.flip(0).contiguous())[2]) == 0.5
    logits = _critic_logits(65)
    logits[70, 0] = float("nan")
    loss, glogits, acc = H.factor_critic_loss(logits.cuda())
    assert bool(torch.isnan(loss)) and bool(torch.isnan(glogits[70]).all()) and bool(torch.isfinite(glogits[:70]).all())
    assert float(acc) == float(np.float32(R.critic_loss(logits)["acc"]))             # the NaN row is wrong, the others count
    with pytest.raises(RuntimeError, match="even"):
        H.factor_critic_loss(torch.zeros(3, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="logits"):
        H.factor_critic_loss(torch.zeros(4, device="cuda"))


# ------------------------------------------------------------------ 4. the Functions
def test_functions_equal_the_direct_calls(H):
    from disentangle_mlp_amd import functional as Fn
    logits = R.make_logits(65).cuda().requires_grad_(True)
    kl = torch.full((), KL, device="cuda", requires_grad=True)
    loss, parts = Fn.factor_tc(logits, kl, R.BETA, R.GAMMA)
    out4 = H.factor_tc_fwd(logits.detach(), kl.detach(), R.BETA, R.GAMMA)
    assert loss.requires_grad and not parts.requires_grad and parts.shape == (3,)
    assert torch.equal(_bits(loss), _bits(out4[0])) and torch.equal(_bits(parts), _bits(out4[1:]))
    (R.GLOSS * loss).backward()
    glogits, gkl = H.factor_tc_bwd(logits.detach(), torch.full((), R.GLOSS, device="cuda"), R.BETA, R.GAMMA)
    assert torch.equal(_bits(logits.grad), _bits(glogits)) and torch.equal(_bits(kl.grad), _bits(gkl))
    bw, gw = torch.full((1,), R.BETA, device="cuda"), torch.full((1,), R.GAMMA, device="cuda")
    assert torch.equal(_bits(Fn.factor_tc(logits, kl, bw, gw)[0]), _bits(loss))      # tensors are the words themselves
    # the critic's loss: forward and gradient from one launch, scaled by the upstream gradient
    x = _critic_logits(65).cuda().requires_grad_(True)
    loss, acc = Fn.factor_critic_loss(x, 260.0)
    want = H.factor_critic_loss(x.detach(), 260.0)
    assert not acc.requires_grad and torch.equal(_bits(loss), _bits(want[0])) and torch.equal(_bits(acc), _bits(want[2]))
    (2.0 * loss).backward()
    assert torch.equal(_bits(x.grad), _bits(2.0 * want[1]))


@pytest.mark.parametrize("mode", ["gz+gloss", "gloss", "gz"])
def test_reparam_critic_and_loss_compose_in_every_backward_mode(mode):
    """z and the KL from `reparam_kl`, the critic on z, `factor_tc` on its logits: what `VAE.forward_with_factor` puts
    together, with the decoder's gradient (gz) and the loss's (gloss) present or absent -- an absent one takes its whole
    term out, as in the other objectives' Functions."""
    from disentangle_mlp_amd import functional as Fn, model as M
    B, D = 65, 128
    g = torch.Generator().manual_seed(17)
    mu, lv, eps, gz = (torch.randn(B, D, generator=g) * s for s in (1.0, 0.3, 1.0, 1.0))
    critic = M.LatentCritic(D, 96, 2, generator=torch.Generator().manual_seed(3)).cuda()
    ref = {}
    for dt in (torch.float64, torch.float32):
        net = R.torch_critic(critic, dt)
        m, l = mu.to(dt, copy=True).requires_grad_(True), lv.to(dt, copy=True).requires_grad_(True)
        z = m + eps.to(dt) * torch.exp(0.5 * l)
        kl = -0.5 * (1 + l - m * m - torch.exp(l)).sum()
        logits = net(z)
        loss = R.BETA * kl + R.GAMMA * (logits[:, 0] - logits[:, 1]).sum()
        total = (R.GLOSS * loss if "gloss" in mode else 0) + ((z * gz.to(dt)).sum() if "gz" in mode else 0)
        ref[dt] = (loss.detach(), *torch.autograd.grad(total, (m, l)))
    m, l = mu.cuda().requires_grad_(True), lv.cuda().requires_grad_(True)
    for p in critic.parameters():
        p.requires_grad_(False)                                       # it only relays gradients
    z, kl = Fn.reparam_kl(m, l, eps.cuda(), 1.0)
    loss, parts = Fn.factor_tc(critic(z), kl, R.BETA, R.GAMMA)
    total = (R.GLOSS * loss if "gloss" in mode else 0) + ((z * gz.cuda()).sum() if "gz" in mode else 0)
    total.backward()
    r64, r32 = ref[torch.float64], ref[torch.float32]
    _check(f"[{mode}] loss", loss.detach(), r32[0], r64[0])
    _check(f"[{mode}] gmu", m.grad, r32[1], r64[1])
    _check(f"[{mode}] glogvar", l.grad, r32[2], r64[2])
    assert all(p.grad is None for p in critic.parameters())


# ------------------------------------------------------------------ 5. the critic network
def test_latent_critic_forward_and_backward_against_torch_modules():
    from disentangle_mlp_amd import model as M
    B, D = 65, 128
    g = torch.Generator().manual_seed(23)
    x, gy = torch.randn(B, D, generator=g), torch.randn(B, 2, generator=g)
    critic = M.LatentCritic(D, 96, 2, generator=torch.Generator().manual_seed(4)).cuda()
    ref = {}
    for dt in (torch.float64, torch.float32):
        net = R.torch_critic(critic, dt)
        xi = x.to(dt, copy=True).requires_grad_(True)
        y = net(xi)
        (y * gy.to(dt)).sum().backward()
        ref[dt] = dict(y=y.detach(), gx=xi.grad, **{k: p.grad for k, p in net.named_parameters()})
    xi = x.cuda().requires_grad_(True)
    y = critic(xi)
    assert y.shape == (B, 2)
    (y * gy.cuda()).sum().backward()
    got = dict(y=y.detach(), gx=xi.grad, **{k: p.grad for k, p in critic.named_parameters()})
    assert list(got) == list(ref[torch.float64])
    for k in got:
        _check(f"critic {k}", got[k], ref[torch.float32][k], ref[torch.float64][k])
