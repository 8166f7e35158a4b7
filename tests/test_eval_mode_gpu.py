"""Eval mode of the module API (model.enable_eval / eval_mode) against oracle.modules in .eval(), fp64 on the host, same
state_dict.  The running statistics are made non-trivial by two train-mode oracle forwards.  Forward tolerance and metric:
those of test_step_gpu.py::test_kat0_forward (abs-sum within 2e-5 relative; elements within 1e-4 relative + 2e-6);
gradients: the step tests' ceiling, 3e-3 relative L2 per tensor."""
import pytest
import torch

import oracle
from oracle import modules as O

pytestmark = pytest.mark.gpu
REL, GRAD_TOL = 2e-5, 3e-3


@pytest.fixture(scope="module")
def M():
    from disentangle_mlp_amd import model
    return model


@pytest.fixture(scope="module")
def opt():
    from disentangle_mlp_amd.trainer import ModelOpt
    return ModelOpt()


def fwd_close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    a, b = float(got.abs().sum()), float(ref.abs().sum())
    worst = float(((got - ref).abs() - 1e-4 * torch.maximum(got.abs(), ref.abs())).max())
    print(f"{what}: abs-sum gap {abs(a - b) / max(a, b):.2e} (<= {REL:.0e}), worst element excess {worst:.2e} (<= 2e-6)")
    assert abs(a - b) <= REL * max(a, b), (what, a, b)
    assert worst <= 2e-6, (what, worst)


_pairs = {}


def pair(M, opt, cls):
    """(oracle module in .eval() with non-trivial running statistics, fp64; its state_dict)."""
    if cls not in _pairs:
        torch.manual_seed(17)
        ref = getattr(O, cls)(O.OracleOpt()).double()
        ref.apply(O.weights_init)
        g = torch.Generator().manual_seed(3)
        for _ in range(2):                          # two train-mode forwards
            if cls == "Generator_celeba":
                ref(torch.randn(6, 128, generator=g, dtype=torch.float64))
            else:
                x = torch.rand(6, 3, 64, 64, generator=g, dtype=torch.float64) * 2 - 1
                ref(x, torch.randn(6, 128, generator=g, dtype=torch.float64)) if cls != "Discriminator_celeba" else ref(x)
        ref.eval()
        _pairs[cls] = (ref, {k: v.clone() for k, v in ref.state_dict().items()})
    ref, sd = _pairs[cls]
    net = getattr(M, cls)(opt)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()})
    return ref, net.cuda()


def inputs(B=2):
    g = torch.Generator().manual_seed(1234)
    return (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g))


def unchanged(net, before):
    after = net.state_dict()
    return all(torch.equal(v, after[k]) for k, v in before.items())


@pytest.mark.parametrize("mode", ["fused", "unfused", "hooked"])
def test_forward_against_oracle_eval(M, opt, mode, monkeypatch):
    """FUSE_CONV_BN on and off, and once with a forward hook installed (fusion asked for: the chain falls back module by
    module)."""
    fuse, hook = mode != "unfused", mode == "hooked"
    monkeypatch.setattr(M, "FUSE_CONV_BN", fuse)
    x, eps, z = inputs()
    with torch.no_grad():
        ref, vae = pair(M, opt, "VAE")
        seen = []
        if hook:
            h = vae.act2[0].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
        before = {k: v.clone() for k, v in vae.state_dict().items()}
        with M.eval_mode(vae):
            mu, lv = vae.encode(x.cuda())
            dec = vae.decode(z.cuda())
            rec, mu2, _ = vae(x.cuda(), eps.cuda())
            one = vae.decode(z[:1].cuda())
        assert vae.training and unchanged(vae, before), "eval moved a buffer or num_batches_tracked"
        if hook:
            h.remove()
            assert len(seen) == 3
        rmu, rlv = ref.encode(x.double())
        fwd_close(mu, rmu, "VAE.encode mu"), fwd_close(lv, rlv, "VAE.encode logvar")
        fwd_close(dec, ref.decode(z.double()), "VAE.decode")
        fwd_close(rec, ref(x.double(), eps.double())[0], "VAE.forward")
        fwd_close(one, ref.decode(z[:1].double()), "VAE.decode B=1")
        if hook:
            return
        for cls in ("Encoder_celeba", "Generator_celeba", "Discriminator_celeba"):
            ref, net = pair(M, opt, cls)
            with M.eval_mode(net):
                if cls == "Encoder_celeba":
                    got, want = net(x.cuda(), eps.cuda())[0], ref(x.double(), eps.double())[0]
                elif cls == "Generator_celeba":
                    got, want = net(z.cuda()), ref(z.double())
                else:
                    (p, feat), (rp, rfeat) = net(x.cuda()), ref(x.double())
                    fwd_close(p, rp, cls + " p")
                    got, want = feat, rfeat
            fwd_close(got, want, cls)


def test_a_row_does_not_depend_on_its_batch(M, opt):
    _, vae = pair(M, opt, "VAE")
    g = torch.Generator().manual_seed(8)
    z = torch.randn(4, 128, generator=g).cuda()
    with torch.no_grad(), M.eval_mode(vae):
        four = vae.decode(z)
        for i in range(4):
            fwd_close(vae.decode(z[i:i + 1]), four[i:i + 1].cpu(), f"row {i} of B = 4 against its B = 1 decode")


def grad_close(got, ref, what):
    e = float((got.detach().cpu().double() - ref).norm() / ref.norm())
    print(f"{what}: rel L2 {e:.2e} (<= {GRAD_TOL:.0e})")
    assert e <= GRAD_TOL, (what, e)


def test_gradients_through_the_eval_discriminator(M, opt):
    """A scalar loss through D in eval to its input and its parameters -- the bn_shadowed convolution biases included,
    whose gradient is no longer zero."""
    ref, net = pair(M, opt, "Discriminator_celeba")
    x = inputs()[0]
    xr = x.double().requires_grad_()
    p, feat = ref(xr)
    (p.sum() + 0.01 * feat.pow(2).sum()).backward()
    xg = x.cuda().requires_grad_()
    with M.eval_mode(net):
        p, feat = net(xg)
        (p.sum() + 0.01 * feat.pow(2).sum()).backward()
    grad_close(xg.grad, xr.grad, "input")
    for (k, a), (_, b) in zip(net.named_parameters(), ref.named_parameters()):
        assert a.grad is not None, k
        grad_close(a.grad, b.grad, k)
    assert float(net.convs[3].bias.grad.abs().max()) > 0
    ref.zero_grad()


def test_mixed_modes(M, opt):
    """The discriminator enabled and in eval beside a VAE in training: one forward and backward; D's buffers stay, the
    VAE's move, the VAE's shadowed biases get no gradient, D's get one."""
    _, vae = pair(M, opt, "VAE")
    _, d = pair(M, opt, "Discriminator_celeba")
    x, eps, _ = inputs(4)
    d_before = {k: v.clone() for k, v in d.state_dict().items()}
    v_before = {k: v.clone() for k, v in vae.state_dict().items()}
    M.enable_eval(d).eval()
    rec, _, _ = vae(x.cuda(), eps.cuda())
    p, feat = d(rec)
    (p.sum() + feat.sum()).backward()
    d.train()
    M.disable_eval(d)
    assert unchanged(d, d_before) and not unchanged(vae, v_before)
    assert int(vae.state_dict()["features.1.num_batches_tracked"]) == int(v_before["features.1.num_batches_tracked"]) + 1
    assert vae.deconv1.bias.grad is None and vae.deconv1.weight.grad is not None
    assert d.convs[0].bias.grad is not None and bool(torch.isfinite(vae.features[0].weight.grad).all())


def test_eval_decode_captures_into_a_graph(M, opt):
    from disentangle_mlp_amd import ops
    _, vae = pair(M, opt, "VAE")
    z = inputs()[2].cuda()
    with torch.no_grad(), M.eval_mode(vae):
        eager = vae.decode(z).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            vae.decode(z)                                  # warm-up on the capture stream: workspaces, packs
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with ops.amax_capture_scope(), torch.cuda.graph(graph):
            out = vae.decode(z)
        keep = ops.buffers_in_use()
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        del keep


class _Recorder(torch.nn.Module):
    """``fn`` of fid.sample_statistics as a module around the network: records what it decoded and in which mode."""

    def __init__(self, vae):
        super().__init__()
        self.vae, self.seen, self.training_seen = vae, [], []

    def forward(self, z):
        x = self.vae.decode(z)
        self.seen.append(x.float().cpu())
        self.training_seen.append(self.vae.training)
        return x


def _extract(u8):
    return u8.reshape(u8.shape[0], -1)[:, :16].double()


def test_sample_statistics_in_eval_mode(M, opt):
    """sample_statistics(eval_mode=True, decode_batch=2): the recording ``fn`` sees float samples equal, within the
    forward tolerance, to the one-batch eval decode; the nets are back in training afterwards, marks gone."""
    from disentangle_mlp_amd import fid
    _, vae = pair(M, opt, "VAE")
    fn = _Recorder(vae)
    torch.manual_seed(4)
    fid.sample_statistics(fn, 4, 128, _extract, decode_batch=2, eval_mode=True)
    assert fn.training_seen == [False, False]
    assert vae.training and fn.training
    assert not any(m.eval_enabled for m in vae.modules() if isinstance(m, M._HipBatchNormMixin))
    assert [tuple(s.shape) for s in fn.seen] == [(2, 3, 64, 64)] * 2
    torch.manual_seed(4)
    z = torch.randn(4, 128)
    with torch.no_grad(), M.eval_mode(vae):
        whole = vae.decode(z.cuda())
    fwd_close(torch.cat(fn.seen), whole.cpu(), "decode_batch=2 against the one-batch eval decode")
    vae.eval()                                       # the opt-in is gone again: eval without it raises
    try:
        with pytest.raises(RuntimeError, match="enable_eval"):
            vae.decode(z.cuda())
    finally:
        vae.train()


def test_fid_of_generator_and_evaluate_in_eval_mode(M, opt, tmp_path):
    """get_fid_of_generator(netEG.decode, eval_mode=True) -- the bound-method form -- and
    BetaVAEGANTrainer.evaluate(eval_mode=True): the decoder runs in eval, the score is finite and the same by both
    routes (same seed, same latents, running statistics), the network is training again afterwards."""
    from disentangle_mlp_amd import fid
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
    tr = BetaVAEGANTrainer()
    g = torch.Generator().manual_seed(2)
    stats = tmp_path / "ref.npz"
    a = torch.randn(40, 16, generator=g, dtype=torch.float64) * 50 + 100
    fid.save_statistics(str(stats), a.mean(0), torch.cov(a.t()))
    modes = []
    h = tr.netEG.act1[0].register_forward_pre_hook(lambda m, i: modes.append(m.training))
    torch.manual_seed(6)
    one = fid.get_fid_of_generator(tr.netEG.decode, 6, 128, str(stats), feature_extractor=_extract, eval_mode=True)
    assert modes == [False] and tr.netEG.training
    torch.manual_seed(6)
    res = tr.evaluate([tr.checkpoint(1)], calc_fid=True, n_samples=6, fid_path_pretrained=str(stats), fid_on_device=True,
                      fid_feature_extractor=_extract, eval_mode=True)
    h.remove()
    assert modes == [False, False] and tr.netEG.training
    import math
    assert math.isfinite(one) and res[0]["FID"] == one
