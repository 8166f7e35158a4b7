"""CPU: clipping by global norm and skipping a non-finite step on HipAdam's inherited (torch) path, and the host side of
the trainers' switches.  CPU tensors take torch's step, which must carry the same semantics as the kernels:
``max_grad_norm`` is ``torch.nn.utils.clip_grad_norm_`` followed by ``torch.optim.Adam.step()`` bit for bit, a skipped
step touches nothing but the step counts, and the recorded norm is good to one fp32 rounding."""
import math

import pytest
import torch

SIZES = (1, 5, 257, 4099)
LR = 1e-2


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen)) for n in SIZES]


def _set_grads(ps, gen, scale):
    gs = [torch.randn(p.shape, generator=gen) * scale for p in ps]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    return gs


def _state_bits(opt, ps):
    out = []
    for p in ps:
        st = opt.state[p]
        out += [p.detach().clone().view(torch.int32), st["exp_avg"].clone().view(torch.int32),
                st["exp_avg_sq"].clone().view(torch.int32)]
    return out


@pytest.mark.parametrize("max_norm,scales", [(1.0, (5.0, 3.0, 7.0)), (1e4, (5.0, 3.0, 7.0)), (2.0, (5.0, 1e-3, 7.0))],
                         ids=["clipped", "unclipped", "mixed"])
def test_torch_path_is_clip_grad_norm_then_adam_bit_for_bit(max_norm, scales):
    from disentangle_mlp_amd.optim import HipAdam
    pa, pb = _params(), _params()
    oa = HipAdam(pa, lr=LR, max_grad_norm=max_norm)
    ob = torch.optim.Adam(pb, lr=LR)
    ga, gb = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    for k, scale in enumerate(scales):
        kept = _set_grads(pa, ga, scale)
        _set_grads(pb, gb, scale)
        norm64 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in kept))
        total = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        oa.step(), ob.step()
        for i, (x, y) in enumerate(zip(pa, pb)):
            assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)), (k, i)
            for name in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[x][name].view(torch.int32), ob.state[y][name].view(torch.int32)), (k, i, name)
            assert float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == k + 1
            assert torch.equal(x.grad, kept[i])                   # the gradients themselves are not written
        clipped = norm64 > max_norm
        coef = float(oa.clip_coef())
        assert (coef < 1.0) if clipped else (coef == 1.0), (k, coef)
        assert coef == float(torch.clamp(max_norm / (total + 1e-6), max=1.0))
        assert abs(float(oa.grad_norm()) - norm64) <= 2.0 ** -23 * norm64
    assert oa.skipped_steps() == 0
    assert sorted(oa.state_dict()["state"][0]) == sorted(ob.state_dict()["state"][0])      # torch.optim.Adam's state_dict


@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan")])
def test_skip_leaves_everything_but_the_step_count(poison):
    from disentangle_mlp_amd.optim import HipAdam
    pa, pb = _params(2), _params(2)
    oa = HipAdam(pa, lr=LR, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    ob = torch.optim.Adam(pb, lr=LR)
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    _set_grads(pa, ga, 4.0), _set_grads(pb, gb, 4.0)
    torch.nn.utils.clip_grad_norm_(pb, 1.0)
    oa.step(), ob.step()
    before = _state_bits(oa, pa) + [e.clone().view(torch.int32) for e in oa.ema_tensors()]
    _set_grads(pa, ga, 4.0), _set_grads(pb, gb, 4.0)
    pa[2].grad[100] = poison
    oa.step()                                                     # skipped; the torch twin does not step at all
    after = _state_bits(oa, pa) + [e.view(torch.int32) for e in oa.ema_tensors()]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert all(float(oa.state[p]["step"]) == 2.0 for p in pa)     # the count advances all the same
    assert oa.skipped_steps() == 1 and float(oa.clip_coef()) == 0.0
    assert not math.isfinite(float(oa.grad_norm()))
    # the next clean step is torch's step at that count
    for p in pb:
        ob.state[p]["step"] += 1
    _set_grads(pa, ga, 4.0), _set_grads(pb, gb, 4.0)
    torch.nn.utils.clip_grad_norm_(pb, 1.0)
    oa.step(), ob.step()
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)), i
        assert torch.equal(oa.state[x]["exp_avg_sq"].view(torch.int32), ob.state[y]["exp_avg_sq"].view(torch.int32)), i
        assert float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == 3.0
    assert oa.skipped_steps() == 1 and oa.reset_skipped() == 1 and oa.skipped_steps() == 0


def test_skip_on_the_very_first_step_and_skip_alone():
    """No state yet: the skipped step creates it (zero moments, step 1).  ``skip_nonfinite`` alone: coefficient 1."""
    from disentangle_mlp_amd.optim import HipAdam
    pa, pb = _params(4), _params(4)
    oa, ob = HipAdam(pa, lr=LR, skip_nonfinite=True), torch.optim.Adam(pb, lr=LR)
    p0 = [p.detach().clone() for p in pa]
    _set_grads(pa, torch.Generator().manual_seed(5), 1.0)
    pa[0].grad[0] = float("nan")
    oa.step()
    assert all(torch.equal(p.detach(), q) for p, q in zip(pa, p0)) and oa.skipped_steps() == 1
    assert all(float(oa.state[p]["step"]) == 1.0 and not oa.state[p]["exp_avg"].any() for p in pa)
    ga, gb = torch.Generator().manual_seed(6), torch.Generator().manual_seed(6)
    _set_grads(pa, ga, 50.0), _set_grads(pb, gb, 50.0)
    for p in pb:                                                  # torch's twin at the advanced count
        ob.state[p]["step"] = torch.tensor(1.0)
        ob.state[p]["exp_avg"], ob.state[p]["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
    oa.step(), ob.step()
    assert float(oa.clip_coef()) == 1.0                           # nothing clips
    assert all(torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)) for x, y in zip(pa, pb))


def test_without_skip_a_non_finite_gradient_poisons_as_torch_does():
    from disentangle_mlp_amd.optim import HipAdam
    pa = _params(7)
    oa = HipAdam(pa, lr=LR, max_grad_norm=1.0)
    _set_grads(pa, torch.Generator().manual_seed(8), 1.0)
    pa[1].grad[3] = float("nan")
    oa.step()
    assert all(bool(torch.isnan(p).all()) for p in pa)           # coef = NaN: clip_grad_norm_'s behaviour
    assert oa.skipped_steps() == 0


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_constructor_refuses_a_bad_max_grad_norm(bad):
    from disentangle_mlp_amd.optim import HipAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipAdam(_params(), max_grad_norm=bad)


def test_add_param_group_is_refused_and_accessors_need_the_feature():
    from disentangle_mlp_amd.optim import HipAdam
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        opt = HipAdam(_params(), **kw)
        with pytest.raises(RuntimeError, match="constructor"):
            opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})
    plain = HipAdam(_params())
    plain.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})
    for name in ("grad_norm", "clip_coef", "skipped_steps", "reset_skipped"):
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            getattr(plain, name)()


def test_one_norm_over_all_groups_and_none_grads_do_not_count():
    from disentangle_mlp_amd.optim import HipAdam
    ps = _params(9)
    opt = HipAdam([{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-3}], lr=LR, max_grad_norm=1.0)
    gs = _set_grads(ps, torch.Generator().manual_seed(10), 2.0)
    ps[3].grad = None
    opt.step()
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs[:3]))
    assert abs(float(opt.grad_norm()) - want) <= 2.0 ** -23 * want


def test_entry_points_are_bound_and_validate_on_the_host():
    import ctypes
    from disentangle_mlp_amd import _lib, build
    from disentangle_mlp_amd.optim import _AdamTensor
    build.build(verbose=False)
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 == lib.vg_version()              # entry points were only added
    lens = (ctypes.c_size_t * 5)(0, 1, 8192, 8193, 3 * 8192 + 7)
    assert lib.vg_grad_sumsq_partials(lens, 5) == 0 + 1 + 1 + 2 + 4
    assert lib.vg_grad_sumsq_partials(lens, 0) == 0
    ptrs = (ctypes.c_void_p * 5)()
    fake = ctypes.c_void_p(64)                                    # never dereferenced: every call below is refused
    assert lib.vg_grad_sumsq_multi(ptrs, lens, 5, None, 8, None) == -1          # no partials
    assert lib.vg_grad_sumsq_multi(ptrs, lens, 5, fake, 7, None) == -1          # capacity
    assert lib.vg_grad_sumsq_multi(ptrs, lens, 5, fake, 8, None) == -1          # a NULL gradient with elements
    assert lib.vg_grad_sumsq_multi(ptrs, lens, -1, fake, 8, None) == -1
    assert lib.vg_grad_clip_finalize(None, 0, 1.0, 0, fake, None) == -1
    assert lib.vg_grad_clip_finalize(fake, 0, 1.0, 0, None, None) == -1
    assert lib.vg_grad_clip_finalize(fake, 0, float("nan"), 0, fake, None) == -1
    arr = (_AdamTensor * 1)()
    ema = (ctypes.c_void_p * 1)()
    assert lib.vg_adam_step_clip(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, None, None, 0.0, None, None) == -1     # no record
    assert lib.vg_adam_step_dev_clip(arr, 1, 0.9, 0.999, 1e-8, fake, None, None, 0.0, None, None) == -1
    assert lib.vg_adam_step_dev_clip(arr, 1, 0.9, 0.999, 1e-8, None, None, None, 0.0, fake, None) == -1            # no scalars
    for decay in (0.0, 1.0, float("nan")):
        assert lib.vg_adam_step_clip(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, None, ema, decay, fake, None) == -1
        assert lib.vg_adam_step_dev_clip(arr, 1, 0.9, 0.999, 1e-8, fake, None, ema, decay, fake, None) == -1
    # only empty tensors: success, no launch -- with and without an average
    assert lib.vg_adam_step_clip(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, None, None, 0.0, fake, None) == 0
    assert lib.vg_adam_step_clip(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, None, ema, 0.9, fake, None) == 0


# ------------------------------------------------------------------ trainers
def _named(tr):
    return {f"{a}.{k}": p for a, net, _ in tr._guarded_optimizers() for k, p in net.named_parameters()}


def _stub_iteration(tr, seed):
    """The kernels need a GPU: one iteration here is random gradients on every parameter and every optimizer's step,
    in the trainer's own order."""
    gen = torch.Generator().manual_seed(seed)
    norms = {}
    for attr, net, opt in tr._guarded_optimizers():
        sq = 0.0
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=gen) * 0.01
            sq += float((p.grad.double() ** 2).sum())
        norms[attr] = math.sqrt(sq)
        opt.step()
    tr.iteration += 1
    return norms


def test_cpu_trainer_records_the_norm_of_its_gradients():
    from disentangle_mlp_amd.optim import HipAdam
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
    tr = BetaVAEGANTrainer(device="cpu", max_grad_norm=1.0)
    assert tr.max_grad_norm == 1.0 and tr.skip_nonfinite is False
    norms = _stub_iteration(tr, 11)
    for attr, _, opt in tr._guarded_optimizers():
        assert isinstance(opt, HipAdam) and opt.max_grad_norm == 1.0
        got, want = float(opt.grad_norm()), norms[attr]
        assert want > 1.0 and float(opt.clip_coef()) < 1.0
        assert abs(got - want) <= 2.0 ** -23 * want, (attr, got, want)
    assert tr.check_finite() is None and tr.skipped_steps() == {}


def test_trainer_switches_reach_the_optimizers_and_the_capture_key():
    from disentangle_mlp_amd import trainer as T
    from disentangle_mlp_amd.optim import HipAdam
    plain = T.VAETrainer(device="cpu")
    assert type(plain.optimizer) is torch.optim.Adam              # the defaults build what they built
    for make, attrs in ((T.VAETrainer, ("optimizer",)), (T.GANTrainer, ("optimizerG", "optimizerD"))):
        tr = make(device="cpu", max_grad_norm=0.5, skip_nonfinite=True)
        for a in attrs:
            opt = getattr(tr, a)
            assert isinstance(opt, HipAdam) and opt.max_grad_norm == 0.5 and opt.skip_nonfinite
    a, b = T.VAETrainer(device="cpu", max_grad_norm=1.0), T.VAETrainer(device="cpu", skip_nonfinite=True)
    assert len({plain._host_state_key(), a._host_state_key(), b._host_state_key()}) == 3
    assert a._host_state_key() == T.VAETrainer(device="cpu", max_grad_norm=1.0)._host_state_key()
    with pytest.raises(ValueError, match="max_grad_norm"):
        T.GANTrainer(device="cpu", max_grad_norm=float("nan"))


def test_check_finite_counts_a_skipped_step_instead_of_raising():
    from disentangle_mlp_amd.trainer import GANTrainer, NonFiniteError
    tr = GANTrainer(device="cpu", skip_nonfinite=True, nonfinite_guard=True)
    _stub_iteration(tr, 12)
    assert tr.skipped_steps() == {"netG": 0, "netD": 0}
    w0 = [p.detach().clone() for p in tr.netG.parameters()]
    d0 = [p.detach().clone() for p in tr.netD.parameters()]
    gen = torch.Generator().manual_seed(13)
    for net in (tr.netG, tr.netD):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=gen) * 0.01
    tr.netG.deconv1.weight.grad.view(-1)[7] = float("inf")
    tr.optimizerG.step(), tr.optimizerD.step()
    assert tr.check_finite() is None                              # only a GRAD bit: the step was skipped
    assert tr.skipped_steps() == {"netG": 1, "netD": 0}
    assert all(torch.equal(p.detach(), q) for p, q in zip(tr.netG.parameters(), w0))
    assert not any(torch.equal(p.detach(), q) for p, q in zip(tr.netD.parameters(), d0))      # the other optimizer stepped
    with torch.no_grad():
        tr.netD.convs[0].weight.view(-1)[0] = float("nan")        # a poisoned PARAMETER still raises
    with pytest.raises(NonFiniteError) as e:
        tr.check_finite()
    assert ("netD.convs.0.weight", "param") in e.value.found
    # without the opt-in the same gradient raises, as before
    tr2 = GANTrainer(device="cpu", nonfinite_guard=True)
    tr2.netG.deconv1.weight.grad = torch.full_like(tr2.netG.deconv1.weight, float("inf"))
    with pytest.raises(NonFiniteError):
        tr2.check_finite()
