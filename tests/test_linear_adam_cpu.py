"""CPU: the host side of the fused weight-gradient + Adam route -- the eligibility decision as a pure function over its
switches, the two-part step's bookkeeping (`HipAdam.begin_fused_step` / `step`) and the backward's choice
(`functional._linear_weight_grad`) with the library calls stubbed.  No kernel runs here."""
import pytest
import torch


# ---------------------------------------------------------------- eligibility
OK = dict(dim=2, numel=2048 * 16384, in_features=16384)


def test_eligible_by_default():
    from disentangle_mlp_amd.optim import linear_adam_eligible
    assert linear_adam_eligible(**OK)


@pytest.mark.parametrize("off", [
    dict(switch=False), dict(grad_hook=True), dict(exchange=True), dict(update_ema=True), dict(clip=True),
    dict(weight_decay=1e-4), dict(device_hyper=True), dict(amsgrad=True), dict(maximize=True), dict(requires_grad=False),
    dict(native_tensor=False), dict(split_ok=False), dict(dim=4), dict(in_features=130, numel=128 * 130),
    dict(numel=0), dict(numel=1 << 31, in_features=1 << 16)], ids=lambda d: next(iter(d)))
def test_every_switch_turns_the_route_off(off):
    from disentangle_mlp_amd.optim import linear_adam_eligible
    assert not linear_adam_eligible(**{**OK, **off})


def test_single_use_weights_of_the_networks():
    """The encoder heads and -- only under the deferred weight gradient -- the discriminator's layer; never the decoder's
    128 -> 16384 layer, which the beta-VAE-GAN's second phase uses twice before one backward."""
    from disentangle_mlp_amd import model as M
    opt = M.ModelOpt() if hasattr(M, "ModelOpt") else __import__("disentangle_mlp_amd.trainer", fromlist=["ModelOpt"]).ModelOpt()
    vae, d = M.VAE(opt), M.Discriminator_celeba(opt)
    heads = M.single_use_linear_weights(vae)
    assert [id(w) for w in heads] == [id(vae.x_to_mu[0].weight), id(vae.x_to_logvar[0].weight)]
    assert [id(w) for w in M.single_use_linear_weights(d)] == [id(d.lth_features[0].weight)]
    assert M.single_use_linear_weights(d, deferred=False) == []
    assert M.single_use_linear_weights(M.Generator_celeba(opt)) == []


# ---------------------------------------------------------------- the two-part step
@pytest.fixture
def opt3(monkeypatch):
    """A HipAdam over two "big" weights and a bias, on the CPU: eligibility and the bound words are stubbed, `step` takes
    torch's path for what has a gradient -- the bookkeeping in front of it is what is under test."""
    from disentangle_mlp_amd import optim
    w1, w2, b = (torch.nn.Parameter(torch.randn(*shape)) for shape in ((8, 8), (8, 8), (8,)))
    opt = optim.HipAdam([w1, w2, b], lr=1e-3)
    opt._bounds, opt._bound_of = torch.zeros(2), {w1: 0, w2: 1}
    monkeypatch.setattr(optim, "linear_adam_eligible", lambda **kw: not kw["update_ema"] and not kw["grad_hook"])
    return opt, w1, w2, b


def test_reached_weight_is_counted_once_and_unreached_not_at_all(opt3):
    opt, w1, w2, b = opt3
    regs = opt.begin_fused_step()
    assert set(regs) == {id(w1), id(w2)} and all(r.open and not r.done and r.step == 1.0 for r in regs.values())
    assert float(opt.state[w1]["step"]) == 0.0           # the count moves in step(), and only for a weight that was reached
    assert regs[id(w1)].m is opt.state[w1]["exp_avg"] and regs[id(w1)].scalars is None
    assert regs[id(w1)].bc1 == pytest.approx(0.1) and regs[id(w1)].bc2_sqrt == pytest.approx(0.001 ** 0.5)
    regs[id(w1)].done = True                             # the backward updated w1; it never reached w2
    b.grad = torch.ones_like(b)
    before = w1.detach().clone()
    opt.step()
    assert float(opt.state[w1]["step"]) == 1.0 and float(opt.state[b]["step"]) == 1.0
    assert len(opt.state[w2]) == 0                       # not stepped, as with ``grad is None``
    assert [id(p) for p, st in opt.state.items() if len(st)] == [id(w1), id(b)]      # state_dict() keeps step()'s own order
    assert torch.equal(w1.detach(), before)              # step() did not touch the weight again
    assert not any(r.open for r in regs.values())
    opt.step()                                           # no registrations open: nothing is counted twice
    assert float(opt.state[w1]["step"]) == 1.0 and float(opt.state[b]["step"]) == 2.0
    regs = opt.begin_fused_step()
    assert regs == {} and len(opt.state[w2]) == 0        # w2 (would be step 1) and w1 (step 2) cannot share one prepare


def test_switches_reach_the_decision(opt3):
    opt = opt3[0]
    assert opt.begin_fused_step(grad_hook=True) == {}
    assert opt.begin_fused_step(only=[opt3[2]]).keys() == {id(opt3[2])}
    assert opt.begin_fused_step(only=[]) == {}


def test_a_gradient_on_an_updated_weight_is_an_error(opt3):
    opt, w1, _, _ = opt3
    regs = opt.begin_fused_step()
    regs[id(w1)].done = True
    w1.grad = torch.ones_like(w1)
    with pytest.raises(RuntimeError, match="also received a gradient"):
        opt.step()


def test_ema_on_this_call_is_not_eligible(monkeypatch):
    from disentangle_mlp_amd import optim
    w = torch.nn.Parameter(torch.randn(8, 8))
    opt = optim.HipAdam([w], ema_decay=0.9)
    opt._bounds, opt._bound_of = torch.zeros(1), {w: 0}
    seen = []
    monkeypatch.setattr(optim, "linear_adam_eligible", lambda **kw: seen.append(kw["update_ema"]) or False)
    opt.begin_fused_step(update_ema=True)
    opt.begin_fused_step(update_ema=False)
    assert seen == [True, False]


# ---------------------------------------------------------------- the backward's choice
def test_backward_takes_the_fused_launch_or_falls_back(monkeypatch):
    from disentangle_mlp_amd import functional as F, ops, optim
    w = torch.nn.Parameter(torch.zeros(4, 8))
    gy, x = torch.ones(32, 4), torch.ones(32, 8)
    calls = []
    monkeypatch.setattr(ops, "linear_split_ok", lambda reduction, n: True)
    monkeypatch.setattr(ops, "linear_wgrad", lambda g, a: calls.append("pair") or g.t() @ a)
    monkeypatch.setattr(F, "FUSE_LINEAR_ADAM", True)
    reg = optim.FusedLinearStep(p=w)
    F.open_fused_linear_steps({id(w): reg})
    try:
        monkeypatch.setattr(ops, "linear_wgrad_adam", lambda g, a, r: calls.append("refused") or False)
        assert F._linear_weight_grad(None, None, w, gy, x) is not None and not reg.done
        monkeypatch.setattr(ops, "linear_wgrad_adam", lambda g, a, r: calls.append("fused") or True)
        assert F._linear_weight_grad(None, None, w, gy, x) is None and reg.done
        assert calls == ["refused", "pair", "fused"]
        with pytest.raises(RuntimeError, match="second time"):
            F._linear_weight_grad(None, None, w, gy, x)
        reg.done, reg.open = False, False                # closed by the optimizer's step: the two launches again
        assert F._linear_weight_grad(None, None, w, gy, x) is not None and calls[-1] == "pair"
        reg.open = True
        monkeypatch.setattr(F, "FUSE_LINEAR_ADAM", False)
        assert F._linear_weight_grad(None, None, w, gy, x) is not None and calls[-1] == "pair"
    finally:
        reg.open = False
        F.open_fused_linear_steps(None)
        assert id(w) not in F._fused_steps
