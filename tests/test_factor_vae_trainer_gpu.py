"""GPU: ``factor_vae`` through the trainers: one eager step against an autograd restatement built
from the package's own modules and plain torch losses, what each phase differentiates and moves, captured == eager bit for
bit under ONE capture with gamma annealed, the permutation's stream, gamma = 0, checkpoints and the non-finite guard.
Small throughout: a critic of width 64 and depth 2, B = 8, three to five iterations."""
import copy
import math

import pytest
import torch
import torch.nn.functional as tF

from conftest import BN_SHADOWED, GRADNORM_TOL, LOSS_TOL, gap
from test_grad_clip_trainer_gpu import _assert_same, _batch, _bits, _weights

pytestmark = pytest.mark.gpu

SMALL = dict(width=64, depth=2)
BETA, GAMMA, B = 4.0, 6.4, 8


def _uniforms(seed=21, b=B):
    return torch.rand(b, 128, generator=torch.Generator().manual_seed(seed)).cuda()


def _same_outputs_and_weights(ta, tb, oa, ob, what):
    assert oa.keys() == ob.keys()
    for k in oa:
        assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), (what, k)
    _assert_same(_weights(ta), _weights(tb))


def _norm(net, skip=()):
    return math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k not in skip))


# ------------------------------------------------------------------ 1. one eager step, restated with autograd
def test_vae_trainer_step_against_an_autograd_restatement():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    eps, u = lat[0], _uniforms()
    tr = T.VAETrainer(beta=BETA, graph=False, factor_vae=(GAMMA, SMALL))
    # the restatement: the same modules (copies, at the initial weights), the losses in plain torch
    m, c = copy.deepcopy(tr.model), copy.deepcopy(tr.critic)
    mu, logvar = m.encode(x)
    z = mu + eps * torch.exp(0.5 * logvar)
    recon = m.decode(z)
    kl = -0.5 * (1 + logvar - mu * mu - logvar.exp()).sum()
    for p in c.parameters():
        p.requires_grad_(False)
    logits = c(z)
    tc = (logits[:, 0] - logits[:, 1]).sum()
    kld, mse = BETA * kl + GAMMA * tc, ((recon - x) ** 2).sum()
    (mse + kld).backward()
    for p in c.parameters():
        p.requires_grad_(True)
    rows = torch.cat([z.detach(), z.detach().gather(0, torch.argsort(u, dim=0, stable=True))])
    labels = (torch.arange(2 * B, device="cuda") >= B).long()
    both = c(rows)
    critic_loss = tF.cross_entropy(both, labels, reduction="sum") / (2 * B)
    critic_loss.backward()
    acc = float((both.argmax(1) == labels).float().mean())
    ref = dict(mse=mse.item(), kld=kld.item(), kl=kl.item(), tc=tc.item(), critic_loss=critic_loss.item(), critic_acc=acc,
               VAE=_norm(m, BN_SHADOWED["eg"]), critic=_norm(c))
    seen = {}

    def hook(phase, net):
        seen[phase] = _norm(net, BN_SHADOWED["eg"] if phase == "VAE" else ())
        if phase == "VAE":                                            # the encoder phase forms no critic weight gradient
            seen["critic grads in the encoder phase"] = [p.grad for p in tr.critic.parameters()]

    out = tr.step(x, eps, grad_hook=hook, permute=u)
    assert list(out) == ["mse", "kld", "kl", "tc", "critic_loss", "critic_acc"]
    for k in out:
        tol = LOSS_TOL["mse" if k == "mse" else "kld"]
        print(f"{k}: {float(out[k]):.8g}  restatement {ref[k]:.8g}  tol {tol:.1e}")
        assert gap(float(out[k]), ref[k]) <= tol, (k, float(out[k]), ref[k])
    for phase in ("VAE", "critic"):                                   # both differentiate at the initial weights, as phase "D"
        print(f"gradient norm {phase}: {seen[phase]:.8g}  restatement {ref[phase]:.8g}  tol {GRADNORM_TOL['D']:.1e}")
        assert gap(seen[phase], ref[phase]) <= GRADNORM_TOL["D"]
    assert list(seen)[:2] == ["VAE", "critic grads in the encoder phase"] and list(seen)[-1] == "critic"
    assert all(g is None for g in seen["critic grads in the encoder phase"])
    # the weighted loss is what the parts say (fp32 roundings of the parts and of the loss, relative to the terms' magnitudes)
    terms = [BETA * float(out["kl"]), GAMMA * float(out["tc"])]
    assert abs(float(out["kld"]) - sum(terms)) <= 4 * 2.0 ** -24 * (sum(abs(t) for t in terms) + abs(float(out["kld"])))


# ------------------------------------------------------------------ 2. who differentiates, who moves
def test_each_phase_forms_and_moves_its_own():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    tr = T.VAETrainer(beta=BETA, graph=False, factor_vae=(GAMMA, SMALL))
    tr.step(x, lat[0])
    stale = [p.grad.clone() for p in tr.critic.parameters()]          # the critic phase's gradients of iteration 0
    start = {k: _weights(tr, only=k) for k in ("model", "critic")}
    seen = {}

    def hook(phase, net):
        if phase == "VAE":                                            # the encoder phase of iteration 1 added nothing to them
            seen["untouched"] = all(torch.equal(_bits(p.grad), _bits(g)) for p, g in zip(tr.critic.parameters(), stale))
            seen["frozen"] = [p.requires_grad for p in tr.critic.parameters()]
        else:                                                         # in front of the critic's step: only the VAE has moved
            seen["model"], seen["critic"] = _weights(tr, only="model"), _weights(tr, only="critic")

    tr.step(x, lat[0], grad_hook=hook)
    assert seen["untouched"] and all(seen["frozen"])                  # (frozen only while the forward builds its graph)
    _assert_same(seen["critic"], start["critic"])
    assert not any(torch.equal(seen["model"][k], start["model"][k]) for k in ("model.x_to_mu.3.weight", "model.deconv4.weight"))
    _assert_same(_weights(tr, only="model"), seen["model"])           # the critic's step moves the critic alone
    end = _weights(tr, only="critic")
    assert not any(torch.equal(end[k], start["critic"][k]) for k in ("critic.0.weight", "critic.4.bias"))


# ------------------------------------------------------------------ 3. captured == eager, gamma annealed under ONE capture
def _count_replays(T, count):
    real = T._CapturedIteration.replay

    def replay(self, *args, **kw):
        count["n"] += 1
        return real(self, *args, **kw)
    return real, replay


@pytest.mark.parametrize("name", ["VAETrainer", "BetaVAEGANTrainer"])
def test_captured_steps_equal_eager_steps_with_gamma_annealed(name):
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    args = (x, lat[0]) if name == "VAETrainer" else (x, *lat)
    schedule = lambda it: 1.5 * it                                    # noqa: E731
    kw = dict(beta=BETA, factor_vae=(schedule, SMALL))
    tg, te = getattr(T, name)(graph=True, **kw), getattr(T, name)(graph=False, **kw)
    assert tg.device_hyper and not te.device_hyper                    # gamma in a device word beside beta's / a float: the same bits
    count = {"n": 0}
    real, replay = _count_replays(T, count)
    T._CapturedIteration.replay = replay
    try:
        for it in range(5):                                           # (``permute`` is drawn: eager, and into the capture's static input)
            og = {k: v.clone() for k, v in tg.step(*args).items()}
            oe = {k: v.clone() for k, v in te.step(*args).items()}
            assert {"kld", "kl", "tc", "critic_loss", "critic_acc"} <= set(oe) and len(oe) == (6 if name == "VAETrainer" else 13)
            _same_outputs_and_weights(tg, te, og, oe, it)             # every parameter and moment of every net and the critic
            assert tg.gamma == te.gamma == 1.5 * it
    finally:
        T._CapturedIteration.replay = real
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert count["n"] == 3                                            # every iteration after the two warm-up ones
    assert [p.net for p in tg._parts][-1] == "critic" and "critic.0.weight" in _weights(tg)
    assert 0.0 <= float(og["critic_acc"]) <= 1.0 and float(og["critic_loss"]) > 0.0


# ------------------------------------------------------------------ 4. the permutation's stream
def test_supplied_permute_equals_a_drawn_one_and_the_latents_are_unchanged():
    from disentangle_mlp_amd import trainer as T
    x, _ = _batch(B)
    kw = dict(beta=BETA, seed=31, graph=False)
    plain, drawn, given = T.VAETrainer(**kw), T.VAETrainer(factor_vae=(GAMMA, SMALL), **kw), T.VAETrainer(factor_vae=(GAMMA, SMALL), **kw)
    stream = T._permute_generator("cuda", 31, 0)
    for it in range(3):
        eps = plain.draw_latents(B)                                   # the latent stream: what it is without the keyword
        od = {k: v.clone() for k, v in drawn.step(x).items()}
        u = torch.rand(B, 128, device="cuda", generator=stream)
        og = {k: v.clone() for k, v in given.step(x, eps, permute=u).items()}
        _same_outputs_and_weights(drawn, given, od, og, it)
    with pytest.raises(ValueError, match="permute must be a float32 tensor of shape"):
        given.step(x, permute=u[:4])
    with pytest.raises(TypeError, match="permute= belongs to factor_vae"):
        plain.step(x, permute=u)


# ------------------------------------------------------------------ 5. gamma = 0
def test_gamma_zero_leaves_the_other_networks_as_without_the_keyword():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    plain, keyed = T.BetaVAEGANTrainer(beta=BETA), T.BetaVAEGANTrainer(beta=BETA, factor_vae=(0.0, SMALL))
    init = _weights(keyed, only="critic")
    for it in range(3):                                               # (the third step of a shape is the captured one)
        plain.step(x, *lat)
        out = {k: v.clone() for k, v in keyed.step(x, *lat).items()}
    for net in ("netEG", "netD"):
        a, b = getattr(plain, net).state_dict(), getattr(keyed, net).state_dict()
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), net
    _assert_same(_weights(plain), {k: v for k, v in _weights(keyed).items() if not k.startswith("critic.")})
    end = _weights(keyed, only="critic")
    assert not any(torch.equal(end[k], init[k]) for k in ("critic.0.weight", "critic.4.bias"))      # the critic still trains
    assert float(out["kld"]) == float(torch.tensor(BETA, dtype=torch.float32) * out["kl"].cpu())
    assert len(plain._graphs) == len(keyed._graphs) == 1


# ------------------------------------------------------------------ 6. checkpoint
def test_checkpoint_load_and_step_equal_an_uninterrupted_run():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    kw = dict(beta=BETA, graph=False, factor_vae=(GAMMA, SMALL))
    a = T.BetaVAEGANTrainer(**kw)
    for it in range(2):
        a.step(x, *lat, permute=_uniforms(it))
    ck = copy.deepcopy(a.checkpoint(2))
    assert {"latent_critic", "latent_critic_optimizer"} <= set(ck)
    oa = {k: v.clone() for k, v in a.step(x, *lat, permute=_uniforms(2)).items()}
    b = T.BetaVAEGANTrainer(seed=1, **kw)                             # other weights, in every net and in the critic
    assert b.load(ck) == 2
    ob = {k: v.clone() for k, v in b.step(x, *lat, permute=_uniforms(2)).items()}
    _same_outputs_and_weights(a, b, oa, ob, "after load")
    # a checkpoint without the keys loads and leaves the critic alone
    before = _weights(b, only="critic")
    b.load({k: v for k, v in ck.items() if not k.startswith("latent_critic")})
    _assert_same(_weights(b, only="critic"), before)


# ------------------------------------------------------------------ 7. the guard
def test_nonfinite_guard_names_a_critic_parameter():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    tr = T.VAETrainer(beta=BETA, graph=False, nonfinite_guard=True, factor_vae=(GAMMA, SMALL))
    tr.step(x, lat[0])
    assert tr.check_finite() is None

    def hook(phase, net):
        if phase == "critic":
            net[2].weight.grad[1, 3] = float("nan")

    tr.step(x, lat[0], grad_hook=hook)
    with pytest.raises(T.NonFiniteError) as e:
        tr.check_finite()
    assert ("critic.2.weight", "grad+param") in e.value.found and all(n.startswith("critic.") for n, _ in e.value.found)
