"""Eval mode, the parts that need no GPU: the opt-in mark leaves state_dict keys and weights_init alone, an unmarked
module still refuses .eval() (and says how to opt in), tests/_eval_refs.py agrees with oracle.modules in .eval(), and the
new operations refuse CPU tensors."""
import pytest
import torch

import _eval_refs as E


@pytest.fixture(scope="module")
def M():
    from disentangle_mlp_amd import model
    return model


@pytest.fixture(scope="module")
def opt():
    from disentangle_mlp_amd.trainer import ModelOpt
    return ModelOpt()


@pytest.mark.parametrize("cls", ["VAE", "Encoder_celeba", "Generator_celeba", "Discriminator_celeba"])
def test_mark_is_not_state(M, opt, cls):
    def build(mark):
        torch.manual_seed(3)
        net = getattr(M, cls)(opt)
        if mark:
            assert M.enable_eval(net) is net
        net.apply(M.weights_init)
        return net
    a, b = build(False), build(True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    bns = [m for m in b.modules() if isinstance(m, M._HipBatchNormMixin)]
    assert bns and all(m.eval_enabled for m in bns)
    M.disable_eval(b)
    assert not any(m.eval_enabled for m in bns)


def test_unmarked_eval_raises_and_names_the_opt_in(M):
    bn = M.HipBatchNorm2d(4).eval()
    with pytest.raises(RuntimeError, match="enable_eval"):
        bn(torch.zeros(1, 4, 2, 2))
    assert bn._nbt_pending == 0


def test_eval_mode_restores_flags_and_marks(M, opt):
    net = M.Generator_celeba(opt)
    M.enable_eval(net.act1)                      # one BatchNorm marked before, the others not
    net.act2.eval()                              # one submodule already in eval
    before = [(m.training, m.__dict__.get("eval_enabled")) for m in net.modules()]
    with M.eval_mode(net) as n:
        assert n is net and not any(m.training for m in net.modules())
        assert all(m.eval_enabled for m in net.modules() if isinstance(m, M._HipBatchNormMixin))
    assert before == [(m.training, m.__dict__.get("eval_enabled")) for m in net.modules()]
    with pytest.raises(KeyError):
        with M.eval_mode(net):
            raise KeyError("inside")
    assert before == [(m.training, m.__dict__.get("eval_enabled")) for m in net.modules()]


def test_shadowed_bias_follows_the_batchnorm_behind_it(M, opt):
    from disentangle_mlp_amd import functional as F
    net = M.VAE(opt)
    layers = [net.features[0], net.x_to_mu[0], net.preprocess[0], net.deconv2]
    assert all(M._bias_mode(m) == F.BIAS_GRAD_ZERO for m in layers)
    n_shadowed = len(M.shadowed_bias_params(net))
    with M.eval_mode(net):
        assert all(M._bias_mode(m) == F.BIAS_GRAD_COMPUTE for m in layers)
        assert len(M.shadowed_bias_params(net)) == n_shadowed          # keeps its (train-mode) meaning
    assert all(M._bias_mode(m) == F.BIAS_GRAD_ZERO for m in layers)
    assert M._bias_mode(net.deconv4) == F.BIAS_GRAD_COMPUTE


def _randomise(mods, g):
    """Non-trivial parameters and running statistics for oracle layers, in place."""
    with torch.no_grad():
        for m in mods:
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.weight.copy_(1 + 0.2 * torch.randn(m.num_features, generator=g, dtype=torch.float64))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g, dtype=torch.float64))
            elif hasattr(m, "weight"):
                m.weight.copy_(0.05 * torch.randn(m.weight.shape, generator=g, dtype=torch.float64))
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g, dtype=torch.float64))


def _params_of(mods):
    """The layer table and parameter dicts `_eval_refs.chain_forward` takes, read off oracle modules."""
    import _chain_refs as R
    layers, params = [], []
    for m in mods:
        if isinstance(m, torch.nn.BatchNorm2d):
            layers.append(R.BN(m.num_features, "relu", m.eps, m.momentum))
            params.append(dict(gamma=m.weight.detach().clone().requires_grad_(), beta=m.bias.detach().clone().requires_grad_(),
                               rm=m.running_mean.clone(), rv=m.running_var.clone()))
        elif isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            tr = isinstance(m, torch.nn.ConvTranspose2d)
            layers.append(R.Conv(m.in_channels, m.out_channels, m.stride[0], tr))
            params.append(dict(w=m.weight.detach().clone().requires_grad_(), b=m.bias.detach().clone().requires_grad_()))
    return layers, params


def test_eval_refs_agree_with_oracle_modules():
    """`_eval_refs.chain_forward` against oracle.modules' own layers in .eval(): the encoder trunk the oracle builds
    (conv -> BatchNorm2d -> ReLU, three times) and the tail of its decoder (deconv3 -> act3 -> deconv4, with the
    literal output sizes), same parameters and running statistics, fp64: outputs and every gradient, the bias in front
    of a BatchNorm included; the oracle's buffers do not move."""
    from oracle import modules as O
    g = torch.Generator().manual_seed(12)
    trunk = O._enc_trunk(4, 4).double()
    gen = O.Generator_celeba(O.OracleOpt()).double()
    tail = [gen.deconv3, gen.act3[0], gen.deconv4]
    for name, mods, x in (("trunk", [m for m in trunk], torch.randn(2, 4, 16, 16, generator=g, dtype=torch.float64)),
                          ("decoder tail", tail, torch.randn(2, 128, 4, 4, generator=g, dtype=torch.float64))):
        _randomise(mods, g)
        for m in mods:
            m.eval()
        layers, params = _params_of(mods)
        before = [m.running_mean.clone() for m in mods if hasattr(m, "running_mean")]
        xo, xe = x.clone().requires_grad_(), x.clone().requires_grad_()
        if name == "trunk":
            yo = trunk(xo)
        else:
            h = gen.act3(gen.deconv3(xo, output_size=(2, 32, 8, 8)))
            yo = gen.deconv4(h, output_size=(2, 3, 8, 8))
        ye = E.chain_forward(layers, xe, params)
        gy = torch.randn(yo.shape, generator=g, dtype=torch.float64)
        (yo * gy).sum().backward()
        (ye * gy).sum().backward()
        assert E.rel_err(ye, yo)[0] < 1e-13, name
        assert E.rel_err(xe.grad, xo.grad)[0] < 1e-12, name
        own = [m for m in mods if hasattr(m, "weight")]
        for m, p in zip(own, params):
            for k, t in (("w", m.weight), ("b", m.bias)) if "w" in p else (("gamma", m.weight), ("beta", m.bias)):
                assert float(t.grad.abs().max()) > 0 and E.rel_err(p[k].grad, t.grad)[0] < 1e-12, (name, k)
        assert all(torch.equal(a, m.running_mean) for a, m in
                   zip(before, [m for m in mods if hasattr(m, "running_mean")])), name


def test_fid_eval_nets():
    """fid._eval_nets: the network behind ``fn`` for eval_mode=True -- a module, or a bound method of one; a plain
    function cannot say which network it decodes with."""
    from disentangle_mlp_amd import fid, model
    from disentangle_mlp_amd.trainer import ModelOpt
    net = model.Generator_celeba(ModelOpt())
    assert fid._eval_nets(net.forward, False) == () and fid._eval_nets(net, False) == ()
    assert fid._eval_nets(net.forward, True) == (net,) and fid._eval_nets(net, True) == (net,)
    with pytest.raises(ValueError, match="eval_mode"):
        fid._eval_nets(lambda z: net(z), True)


def test_new_ops_refuse_cpu_tensors():
    from disentangle_mlp_amd import ops
    c = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bn_eval_coeffs(c, c, c, c, 1e-5, 1)
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bn_eval_act_bwd(x, x, c, c, c, c, 1)
