"""CPU: the host side of learning-rate / beta / weight-decay schedules -- HipAdam's new arguments, the trainers' argument
validation, the inherited weight-decay path, the additional checkpoint keys.  No kernel runs here."""
import io

import pytest
import torch


def _lambda_lr(opt):
    return torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 0.9 ** i)


def test_device_hyper_needs_capturable_and_fixes_the_groups():
    from disentangle_mlp_amd.optim import HipAdam
    p = torch.nn.Parameter(torch.ones(4))
    with pytest.raises(ValueError, match="capturable"):
        HipAdam([p], device_hyper=True)
    opt = HipAdam([p], capturable=True, device_hyper=True)
    assert opt.device_hyper and opt._hyper[0].dtype == torch.float64 and opt._hyper[0].numel() == 2
    with pytest.raises(RuntimeError, match="device_hyper"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})
    words = opt._hyper[0]
    opt.param_groups[0]["lr"], opt.param_groups[0]["weight_decay"] = 0.25, 0.5
    opt.sync_hyper()
    assert opt._hyper[0] is words and words.tolist() == [0.25, 0.5]      # written in place, never replaced
    plain = HipAdam([torch.nn.Parameter(torch.ones(4))])
    plain.sync_hyper()                                                    # nothing to write: no words
    assert not plain.device_hyper and plain._hyper == {}
    plain.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_on_cpu_tensors_weight_decay_is_torchs(decoupled):
    from disentangle_mlp_amd.optim import HipAdam
    gen = torch.Generator().manual_seed(0)
    w = [torch.randn(7, 5, generator=gen), torch.randn(11, generator=gen)]
    pa, pb = ([torch.nn.Parameter(t.clone()) for t in w] for _ in range(2))
    kw = dict(lr=1e-2, weight_decay=0.1, decoupled_weight_decay=decoupled)
    oa, ob = HipAdam(pa, **kw), torch.optim.Adam(pb, **kw)
    assert oa.param_groups[0]["decoupled_weight_decay"] is decoupled
    for _ in range(3):
        for x, y in zip(pa, pb):
            x.grad = torch.randn(x.shape, generator=gen)
            y.grad = x.grad.clone()
        oa.step(), ob.step()
    for x, y, w0 in zip(pa, pb, w):
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))
        assert not torch.equal(x.detach(), w0)
    assert oa.state_dict()["param_groups"][0].keys() == ob.state_dict()["param_groups"][0].keys()


def test_replayed_counts_as_an_optimizer_step_for_torchs_schedulers():
    import warnings
    from disentangle_mlp_amd.optim import HipAdam
    opt = HipAdam([torch.nn.Parameter(torch.ones(4))], capturable=True)
    sched = _lambda_lr(opt)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        opt.replayed()
        sched.step()
    assert not [w for w in caught if "lr_scheduler.step()" in str(w.message)]
    assert opt.param_groups[0]["lr"] == 1e-3 * 0.9


def test_trainer_arguments_are_validated():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="beta_schedule"):
        T.GANTrainer(device="cpu", beta_schedule=lambda it: 1.0)
    with pytest.raises(TypeError, match="LRScheduler"):
        T.VAETrainer(device="cpu", lr_scheduler=lambda opt: 0.5)
    with pytest.raises(TypeError, match="callable"):
        T.VAETrainer(device="cpu", lr_scheduler=0.5)
    with pytest.raises(TypeError, match="callable"):
        T.VAETrainer(device="cpu", beta_schedule=2.0)
    with pytest.raises(ValueError, match="weight_decay"):
        T.VAETrainer(device="cpu", weight_decay=-1.0)
    with pytest.raises(ValueError, match="device_hyper"):
        T.VAETrainer(device="cpu", device_hyper=True)              # nothing to capture on the CPU
    tr = T.VAETrainer(device="cpu", lr_scheduler=_lambda_lr, beta_schedule=lambda it: 1.0 + it, weight_decay=1e-2,
                      decoupled_weight_decay=True)
    assert not tr.device_hyper and set(tr.lr_schedulers) == {"optimizer"}
    assert isinstance(tr.lr_schedulers["optimizer"], torch.optim.lr_scheduler.LRScheduler)
    g = tr.optimizer.param_groups[0]
    assert g["weight_decay"] == 1e-2 and g["decoupled_weight_decay"] is True
    assert tr._host_state_key() == T.VAETrainer(device="cpu")._host_state_key()      # device_hyper off: today's key
    # by hand
    tr.set_lr(0.125)
    assert g["lr"] == 0.125
    with pytest.raises(KeyError):
        tr.set_lr(0.1, which="optimizerD")
    tr.set_beta(3.0)
    assert tr.beta == 3.0
    with pytest.raises(TypeError):
        T.GANTrainer(device="cpu").set_beta(1.0)
    gan = T.GANTrainer(device="cpu", lr_scheduler=_lambda_lr)
    assert set(gan.lr_schedulers) == {"optimizerG", "optimizerD"}
    gan.set_lr(0.5, which="optimizerD")
    assert gan.optimizerD.param_groups[0]["lr"] == 0.5 and gan.optimizerG.param_groups[0]["lr"] == 3e-3


def test_schedules_step_with_the_trainer_and_checkpoint_keys_appear_only_with_a_schedule():
    from disentangle_mlp_amd import trainer as T
    plain = T.BetaVAEGANTrainer(device="cpu")
    ck0 = plain.checkpoint(1)
    assert set(ck0) == {"epoch", "encoder_decoder_model", "discriminator_model", "encoder_decoder_optimizer",
                        "discriminator_optimizer"}
    assert plain.lr_schedulers == {} and plain.beta_schedule is None and not plain.device_hyper
    tr = T.BetaVAEGANTrainer(device="cpu", lr_scheduler=_lambda_lr, beta_schedule=lambda it: 1.0 + 24.0 * min(it, 5) / 5)
    assert set(tr.lr_schedulers) == {"optimizerEG", "optimizerD"}
    # the host side of `step`, without the iteration itself (no kernels on the CPU)
    for it in range(3):
        tr._begin_step()
        assert tr.beta == 1.0 + 24.0 * it / 5
        tr.iteration += 1
        tr.optimizerEG._opt_called = tr.optimizerD._opt_called = True
        tr._end_step()
        assert tr.optimizerEG.param_groups[0]["lr"] == tr.optimizerD.param_groups[0]["lr"] == 1e-3 * 0.9 ** (it + 1)
    ck = tr.checkpoint(1)
    assert set(ck) == set(ck0) | {"lr_schedulers", "iteration"}
    assert ck["iteration"] == 3 and set(ck["lr_schedulers"]) == {"optimizerEG", "optimizerD"}
    only_beta = T.VAETrainer(device="cpu", beta_schedule=lambda it: 2.0)
    assert set(only_beta.checkpoint(0)) == {"epoch", "VAE_model", "optimizer", "iteration"}
    buf = io.BytesIO()
    torch.save(ck, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    fresh = T.BetaVAEGANTrainer(device="cpu", lr_scheduler=_lambda_lr, beta_schedule=lambda it: 1.0 + 24.0 * min(it, 5) / 5)
    assert fresh.load(ck) == 1
    assert fresh.iteration == 3 and fresh.beta == tr.beta
    assert fresh.optimizerEG.param_groups[0]["lr"] == 1e-3 * 0.9 ** 3
    assert fresh.lr_schedulers["optimizerD"].last_epoch == tr.lr_schedulers["optimizerD"].last_epoch == 3
    fresh._end_step()
    assert fresh.optimizerD.param_groups[0]["lr"] == 1e-3 * 0.9 ** 4
    # a checkpoint without the keys (the reference's) still loads, into a scheduled trainer too
    assert fresh.load(ck0) == 1 and fresh.iteration == 3
    assert plain.load(ck) == 1 and plain.iteration == 3          # (an unscheduled trainer takes the counter over too)
