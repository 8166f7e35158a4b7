"""GPU: ``gan_loss=`` through the trainers.  Default 64 x 64 options, B = 8.

1. One eager step of each trainer under each loss against an independent composition: copies of the trainer's networks
   at their initial weights, the package's feature path (`features_grouped`), then torch's own F.linear and torch's own
   loss forms under autograd, torch.optim.Adam between the phases.  Phase 1 at conftest's tight entries, the later
   phases at its looser ones (everything behind the first Adam step).
2. Captured == eager bit for bit with the labels flipped between iterations, under ONE capture.
3. A hooked head takes the unfused route and agrees within the kernels' bounds.
4. The point of the feature on the device: a saturated head still hands the generator its gradient.
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as tF

import _gan_loss_refs as R
from conftest import BN_SHADOWED, GRADNORM_TOL, LOSS_TOL, gap
from test_grad_clip_trainer_gpu import _assert_same, _batch, _bits, _weights
from test_losses_gpu import check

pytestmark = pytest.mark.gpu

B, LR, BETA = 8, 1e-3, 25.0
LOSSES = ("logistic", "hinge", "lsgan")
REAL, FAKE = 0.9, 0.1


def _norm(net, skip=()):
    return math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k not in skip))


def torch_gan_loss(name, role, s, label, div):
    """The loss of ``name`` in ``role`` on logits ``s`` in torch's own forms."""
    if name == "logistic":
        return tF.binary_cross_entropy_with_logits(s, torch.full_like(s, label), reduction="sum") / div
    if name == "lsgan":
        return 0.5 * tF.mse_loss(s, torch.full_like(s, label), reduction="sum") / div
    if role == "gen":
        return (-s).sum() / div
    return torch.relu(1 - s if role == "real" else 1 + s).sum() / div


def _logits(netD, feat):
    lin = netD.sigmoid_output[0]
    return tF.linear(feat, lin.weight, lin.bias).squeeze(-1)


def _freeze(net, frozen):
    for p in net.parameters():
        p.requires_grad_(not frozen)


def _compare(out, ref, seen, phases):
    for k, v in ref.items():
        if k in phases:
            continue
        tol = LOSS_TOL.get(k, LOSS_TOL["D_x"])          # (the sums of logits and of sigmoid: phase 1, the tight entry)
        print(f"{k}: {float(out[k]):.8g}  composition {v:.8g}  tol {tol:.1e}")
        assert gap(float(out[k]), v) <= tol, (k, float(out[k]), v)
    for ph, tol in phases.items():
        print(f"gradient norm {ph}: {seen[ph]:.8g}  composition {ref[ph]:.8g}  tol {tol:.1e}")
        assert gap(seen[ph], ref[ph]) <= tol, (ph, seen[ph], ref[ph])


# ------------------------------------------------------------------ 1. one eager step against an independent composition
@pytest.mark.parametrize("name", LOSSES)
def test_vaegan_step_against_an_independent_composition(name):
    from disentangle_mlp_amd import trainer as T
    x, (noise, eps2, eps3) = _batch(B)
    tr = T.BetaVAEGANTrainer(beta=BETA, lr=LR, graph=False, gan_loss=name)
    EG, D = copy.deepcopy(tr.netEG), copy.deepcopy(tr.netD)
    optEG, optD = torch.optim.Adam(EG.parameters(), lr=LR), torch.optim.Adam(D.parameters(), lr=LR)
    ref = {}
    # phase 1
    fake = EG.decode(noise)
    f_real, f_fake = D.features_grouped([x, fake.detach()])
    s_real, s_fake = _logits(D, f_real), _logits(D, f_fake)
    e_real, e_fake = torch_gan_loss(name, "real", s_real, REAL, B), torch_gan_loss(name, "fake", s_fake, FAKE, B)
    torch.autograd.backward([e_real, e_fake])
    ref.update(errD_real=e_real.item(), errD_fake=e_fake.item(), D_x_sum=torch.sigmoid(s_real.double()).sum().item(),
               D_logit_real_sum=s_real.double().sum().item(), D_logit_fake_sum=s_fake.double().sum().item(),
               D=_norm(D, BN_SHADOWED["d"]))
    optD.step()
    # phase 2
    _freeze(D, True)
    recon, mu, logvar = EG(x, eps2)
    f_data, f_fake, f_rec = D.features_grouped([x, fake, recon], no_grad=(True, False, False))
    s_fake, s_rec = _logits(D, f_fake), _logits(D, f_rec)
    g_fake, g_rec = torch_gan_loss(name, "gen", s_fake, REAL, B), torch_gan_loss(name, "gen", s_rec, REAL, B)
    sim, mse2 = 0.5 * ((f_rec - f_data.detach()) ** 2).sum(), ((recon - x) ** 2).sum()
    torch.autograd.backward([g_fake, g_rec, sim, mse2])
    _freeze(D, False)
    ref.update(errG_fake=g_fake.item(), errG_recon=g_rec.item(), sim=sim.item(), mse_dec=mse2.item(),
               EG2=_norm(EG, BN_SHADOWED["eg"]))
    optEG.step()
    # phase 3
    optEG.zero_grad(set_to_none=True)
    recon, mu, logvar = EG(x, eps3)
    kld, mse3 = BETA * (-0.5) * (1 + logvar - mu * mu - logvar.exp()).sum(), ((recon - x) ** 2).sum()
    torch.autograd.backward([kld, mse3])
    ref.update(kld=kld.item(), mse_enc=mse3.item(), EG3=_norm(EG, BN_SHADOWED["eg"]))

    seen = {}
    out = tr.step(x, noise, eps2, eps3, real_label=REAL, fake_label=FAKE,
                  grad_hook=lambda ph, net: seen.__setitem__(ph, _norm(net, BN_SHADOWED["d" if ph == "D" else "eg"])))
    assert list(out) == ["errD_real", "errD_fake", "D_x_sum", "D_logit_real_sum", "D_logit_fake_sum", "errG_fake", "errG_recon",
                         "sim", "mse_dec", "kld", "mse_enc"]
    _compare(out, ref, seen, GRADNORM_TOL)


@pytest.mark.parametrize("name", LOSSES)
def test_gan_step_against_an_independent_composition(name):
    from disentangle_mlp_amd import trainer as T
    x, (noise, _, _) = _batch(B)
    tr = T.GANTrainer(lr=LR, graph=False, gan_loss=name)
    G, D = copy.deepcopy(tr.netG), copy.deepcopy(tr.netD)
    optD = torch.optim.Adam(D.parameters(), lr=LR)
    fake = G(noise)
    f_real, f_fake = D.features_grouped([x, fake.detach()])
    s_real, s_fake = _logits(D, f_real), _logits(D, f_fake)
    e_real, e_fake = torch_gan_loss(name, "real", s_real, REAL, B), torch_gan_loss(name, "fake", s_fake, FAKE, B)
    torch.autograd.backward([e_real, e_fake])
    ref = dict(errD_real=e_real.item(), errD_fake=e_fake.item(), D_x_sum=torch.sigmoid(s_real.double()).sum().item(),
               D_logit_real_sum=s_real.double().sum().item(), D_logit_fake_sum=s_fake.double().sum().item(),
               D=_norm(D, BN_SHADOWED["d"]))
    optD.step()
    _freeze(D, True)
    s_gen = _logits(D, D.lth_features(D._features_of(fake)))
    e_g = torch_gan_loss(name, "gen", s_gen, REAL, B)
    e_g.backward()
    ref.update(errG=e_g.item(), G=_norm(G, BN_SHADOWED["g"]))
    seen = {}
    out = tr.step(x, noise, real_label=REAL, fake_label=FAKE,
                  grad_hook=lambda ph, net: seen.__setitem__(ph, _norm(net, BN_SHADOWED["d" if ph == "D" else "g"])))
    assert list(out) == ["errD_real", "errD_fake", "errG", "D_x_sum", "D_logit_real_sum", "D_logit_fake_sum"]
    _compare(out, ref, seen, {"D": GRADNORM_TOL["D"], "G": GRADNORM_TOL["EG2"]})      # (G: behind D's Adam step, as EG2)


# ------------------------------------------------------------------ 2. captured == eager, the labels flipped, ONE capture
@pytest.mark.parametrize("cls_name,name", [("BetaVAEGANTrainer", "logistic"), ("GANTrainer", "lsgan")])
def test_captured_steps_with_label_flips_equal_eager_steps(monkeypatch, cls_name, name):
    from disentangle_mlp_amd import trainer as T
    from test_diff_augment_trainer_gpu import _count_replays
    cls = getattr(T, cls_name)
    x, lat = _batch(B)
    args = (x, *lat) if cls is T.BetaVAEGANTrainer else (x, lat[0])
    count = _count_replays(monkeypatch)
    flips = ((0.9, 0.1), (0.1, 0.9), (0.9, 0.1), (0.1, 0.9))          # the reference flips the pair with probability 0.05
    tg, te = cls(graph=True, gan_loss=name), cls(graph=False, gan_loss=name)
    for it, (real, fake) in enumerate(flips):
        og = {k: v.clone() for k, v in tg.step(*args, real_label=real, fake_label=fake).items()}
        oe = {k: v.clone() for k, v in te.step(*args, real_label=real, fake_label=fake).items()}
        assert og.keys() == oe.keys() and {"D_logit_real_sum", "D_logit_fake_sum"} <= set(og)
        for k in og:
            assert torch.equal(_bits(og[k].float()), _bits(oe[k].float())), (name, it, k)
        _assert_same(_weights(tg), _weights(te))
        assert count["n"] == max(0, it - 1), (name, it, count)        # the third and the fourth are replays
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert tg._host_state_key()[-1] == ("gan_loss", name)             # part of the capture key (and only when set: the CPU test)


# ------------------------------------------------------------------ 3. a hooked head: the unfused route
def test_hooked_head_takes_the_unfused_route(monkeypatch):
    from disentangle_mlp_amd import functional as F, model as M, trainer as T
    D = M.Discriminator_celeba(T.ModelOpt()).cuda()
    x = R.head_inputs((B, 2048))
    lin = D.sigmoid_output[0]
    with torch.no_grad():
        lin.weight.copy_(x["w"]), lin.bias.copy_(x["bias"])
    calls = []
    real_fused, real_vec = F.dot_gan_loss, F.gan_loss
    monkeypatch.setattr(F, "dot_gan_loss", lambda *a, **k: calls.append("fused") or real_fused(*a, **k))
    monkeypatch.setattr(F, "gan_loss", lambda *a, **k: calls.append("vector") or real_vec(*a, **k))
    seen = []
    for name, role, label in (("logistic", "real", 0.9), ("hinge", "fake", 0.1), ("lsgan", "gen", 0.9)):
        kind = {v: k for k, v in R.KINDS.items()}[F.GAN_LOSSES[(name, role)]]
        r = R.dot_gan_loss(x["feat"], x["w"], x["bias"], kind, label, 2 * B)
        assert not bool(r["tie"].any())
        for route in ("fused", "hooked"):
            handle = lin.register_forward_hook(lambda m, i, o: seen.append(o.shape)) if route == "hooked" else None
            f = x["feat"].cuda().requires_grad_()
            calls.clear()
            p, logit, feats, loss = D.head_with_loss(f, name, role, label, 2 * B)
            assert calls == (["vector"] if route == "hooked" else ["fused"]), (route, calls)
            assert feats.data_ptr() == f.data_ptr() and not logit.requires_grad and not p.requires_grad
            lin.zero_grad()
            loss.backward()
            if handle is not None:
                handle.remove()
            what = f"head_with_loss {name}/{role} {route}"
            check(logit, r["logit"], r["logit_mag"], R.logit_k(2048), what + " logit")
            check(p, r["p"], r["p_mag"], R.k_for("p", 2048), what + " p")
            check(loss.reshape(1), r["loss"].reshape(1), r["loss_mag"].reshape(1), R.k_for("loss", 2048), what + " loss")
            check(f.grad, r["gfeat"], r["gfeat_mag"], R.k_for("gfeat", 2048), what + " gfeat")
            check(lin.weight.grad.reshape(-1), r["gw"], r["gw_mag"], R.k_for("gw", 2048, B), what + " gw")
            check(lin.bias.grad, r["gb"], r["gb_mag"], R.k_for("gb", 2048, B), what + " gb")
    assert len(seen) == 3 and all(s == (B, 1) for s in seen)
    # a hook on the Sigmoid does not change the route: that module is not on this path
    handle = D.sigmoid_output[1].register_forward_hook(lambda m, i, o: seen.append("sigmoid"))
    calls.clear()
    D.head_with_loss(x["feat"].cuda(), "logistic", "real", 0.9)
    handle.remove()
    assert calls == ["fused"] and "sigmoid" not in seen
    # the module tree and the state_dict are what they were: the Sigmoid stays, off the new path
    assert list(D.sigmoid_output.state_dict()) == ["0.weight", "0.bias"] and isinstance(D.sigmoid_output[1], M.HipSigmoid)
    with pytest.raises(ValueError, match="logistic.*hinge.*lsgan"):
        D.head_with_loss(x["feat"].cuda(), "wgan", "real", 0.9)


# ------------------------------------------------------------------ 4. the point of the feature, on the device
def test_saturated_head_still_hands_the_generator_its_gradient():
    from disentangle_mlp_amd import model as M, trainer as T
    D = M.Discriminator_celeba(T.ModelOpt()).cuda()
    lin = D.sigmoid_output[0]
    w = 1e-3 * R.randn(1, 2048, seed=2470)
    bias = torch.tensor([-40.0])
    with torch.no_grad():
        lin.weight.copy_(w), lin.bias.copy_(bias)
    feat = R.head_inputs((B, 2048))["feat"]
    t, div = 0.9, 2 * B
    r = R.dot_gan_loss(feat, w, bias, "logistic", t, div)
    assert float(r["logit"].max()) < -39 and float(r["logit"].min()) > -41
    f = feat.cuda().requires_grad_()
    p, logit, _, loss = D.head_with_loss(f, "logistic", "gen", t, div)
    loss.backward()
    # (sigmoid(s) - t) / divisor * w, per element
    check(f.grad, r["gfeat"], r["gfeat_mag"], R.k_for("gfeat", 2048), "saturated head, logistic: gfeat")
    expect = ((torch.sigmoid(r["logit"]) - R.f32(t)) / div)[:, None] * w.double()
    check(f.grad, expect, r["gfeat_mag"], R.k_for("gfeat", 2048), "saturated head, logistic: gfeat against the closed form")
    assert float((f.grad.cpu().double().abs() / w.double().abs()).min()) >= 0.89 / div
    f2 = feat.cuda().requires_grad_()
    _, _, bce = D.head_with_bce(f2, t, div)
    bce.backward()
    ratio = float((f2.grad.cpu().double().abs() / (w.double().abs() / div)).max())
    print(f"BCE route: max |gfeat| / (|w| / divisor) = {ratio:.3e}; logistic: {0.9:.1f}")
    assert bool((f2.grad.cpu().double().abs() <= 1e-5 * w.double().abs() / div).all()), ratio
