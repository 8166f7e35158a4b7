"""GPU, B = 4: learning-rate, beta and weight-decay schedules inside the captured step.  Optimizer level: a captured
``HipAdam(capturable=True, device_hyper=True)`` step replayed under a changing lr (and weight decay) against eager steps of
a plain HipAdam.  Trainer level: a scheduled ``graph=True`` trainer against a ``graph=False`` trainer built WITHOUT the new
arguments whose lr and beta are set by hand -- bit for bit, under ONE capture; weight decay in the trainers; checkpoints."""
import io
import warnings

import pytest
import torch

import test_grad_clip_gpu as Z
from test_grad_clip_gpu import NT, SIZES
from test_grad_clip_trainer_gpu import _assert_same, _batch, _bits, _weights

pytestmark = pytest.mark.gpu

LR0 = 1e-3


def _lambda_lr(opt):
    return torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 0.9 ** i)


def _beta_warmup(it):
    return 1.0 + 24.0 * min(it, 5) / 5                           # linear 1 -> 25 over five iterations


def _no_order_warning(caught):
    assert not [str(w.message) for w in caught if "lr_scheduler.step()" in str(w.message)]


# ------------------------------------------------------------------ 7. the optimizer alone
@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (1e-2, False), (1e-2, True)], ids=["no-decay", "coupled", "decoupled"])
def test_captured_step_follows_lr_and_weight_decay_between_replays(wd, decoupled):
    from disentangle_mlp_amd.optim import HipAdam
    base = Z._state(20)
    gen = torch.Generator().manual_seed(21)
    plan = [[(torch.randn(n, generator=gen) * 0.1).cuda() for n in SIZES] for _ in range(5)]
    lrs = [5e-4, 2e-3, 1e-4, 3e-3]
    wds = [wd, wd, 3e-2, 3e-2] if decoupled else [wd] * 4         # decoupled: the weight decay changes once as well
    a, b = Z._clone(base), Z._clone(base)

    def make(st, **kw):
        ps = [torch.nn.Parameter(s["p"]) for s in st]
        for p, s in zip(ps, st):
            p.grad = s["g"]
        return ps, HipAdam(ps, lr=LR0, weight_decay=wd, decoupled_weight_decay=decoupled, **kw)

    pa, oa = make(a, capturable=True, device_hyper=True)
    pb, ob = make(b)                                              # plain: host scalars, host lr

    def load(st, gs):
        for s, g in zip(st, gs):
            s["g"].copy_(g)

    def same(what):
        torch.cuda.synchronize()
        Z._same(a, b, what, names=("pbuf",))
        for i, (x, y) in enumerate(zip(pa, pb)):
            for name in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(oa.state[x][name]), _bits(ob.state[y][name])), (what, i, name)

    load(a, plan[0]), load(b, plan[0])
    oa.step(), ob.step()                                          # one eager step each: the state exists
    same("eager")
    oa.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    load(a, plan[1])
    with torch.cuda.graph(graph):
        oa.step()
    words = oa._hyper[0]
    for it, (lr, w, gs) in enumerate(zip(lrs, wds, plan[1:])):
        for o in (oa, ob):
            o.param_groups[0]["lr"], o.param_groups[0]["weight_decay"] = lr, w
        oa.sync_hyper()
        load(a, gs), load(b, gs)
        graph.replay()
        if it:
            oa.replayed()
        ob.step()
        same(("replay", it))
        assert words.tolist() == [lr, w] and oa._hyper[0] is words
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert all(float(sa[i]["step"]) == float(sb[i]["step"]) == 5.0 for i in range(NT))
    assert not oa._torch_stepped and not ob._torch_stepped      # both on the kernel
    assert oa.state_dict()["param_groups"] == ob.state_dict()["param_groups"]      # serialisation: torch.optim.Adam's


# ------------------------------------------------------------------ 8. scheduled trainers
def _count_replays(monkeypatch, T):
    count = {"n": 0}
    real = T._CapturedIteration.replay

    def replay(self, *args, **kw):
        count["n"] += 1
        return real(self, *args, **kw)

    monkeypatch.setattr(T._CapturedIteration, "replay", replay)
    return count


def test_scheduled_vaegan_replays_one_graph_and_equals_the_schedule_applied_by_hand(monkeypatch):
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    replays = _count_replays(monkeypatch, T)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tg = T.BetaVAEGANTrainer(graph=True, lr_scheduler=_lambda_lr, beta_schedule=_beta_warmup)
        te = T.BetaVAEGANTrainer(graph=False)                     # the parent's own path: nothing new is passed
        assert tg.device_hyper and tg.optimizerEG.device_hyper and not te.device_hyper
        for it in range(6):
            for opt in (te.optimizerEG, te.optimizerD):
                opt.param_groups[0]["lr"] = LR0 * 0.9 ** it
            te.beta = _beta_warmup(it)
            og = {k: v.clone() for k, v in tg.step(x, *lat).items()}
            oe = {k: v.clone() for k, v in te.step(x, *lat).items()}
            assert len(oe) == 9
            for k in oe:
                assert torch.equal(_bits(og[k].float()), _bits(oe[k].float())), (it, k)
            _assert_same(_weights(tg), _weights(te))
            assert tg.beta == te.beta and tg.iteration == te.iteration == it + 1
            assert tg.optimizerEG.param_groups[0]["lr"] == tg.optimizerD.param_groups[0]["lr"] == LR0 * 0.9 ** (it + 1)
    _no_order_warning(caught)
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert replays["n"] >= 4
    assert set(tg.lr_schedulers) == {"optimizerEG", "optimizerD"}
    # the schedule took effect: an unscheduled trainer on the same batch ends elsewhere
    tu = T.BetaVAEGANTrainer(graph=True)
    for it in range(6):
        tu.step(x, *lat)
    wu, wg = _weights(tu), _weights(tg)
    assert any(not torch.equal(wu[k], wg[k]) for k in wu if k.endswith("weight"))


def test_scheduled_vae_and_gan_trainers(monkeypatch):
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    replays = _count_replays(monkeypatch, T)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        vg = T.VAETrainer(graph=True, lr_scheduler=_lambda_lr, beta_schedule=_beta_warmup)
        ve = T.VAETrainer(graph=False)
        gg = T.GANTrainer(graph=True, lr_scheduler=_lambda_lr)
        ge = T.GANTrainer(graph=False)
        for it in range(4):
            ve.optimizer.param_groups[0]["lr"] = 3e-3 * 0.9 ** it
            ve.beta = _beta_warmup(it)
            for opt in (ge.optimizerG, ge.optimizerD):
                opt.param_groups[0]["lr"] = 3e-3 * 0.9 ** it
            for a, b, args in ((vg, ve, (x, lat[0])), (gg, ge, (x, lat[0]))):
                oa = {k: v.clone() for k, v in a.step(*args).items()}
                ob = {k: v.clone() for k, v in b.step(*args).items()}
                for k in ob:
                    assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), (type(a).__name__, it, k)
                _assert_same(_weights(a), _weights(b))
    _no_order_warning(caught)
    assert len(vg._graphs) == 1 and len(gg._graphs) == 1 and vg.graph and gg.graph
    assert replays["n"] == 4                                      # two each: iterations 3 and 4


# ------------------------------------------------------------------ 9. weight decay in the trainer
def test_trainer_weight_decay_runs_on_the_kernel_and_captures():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    kw = dict(weight_decay=1e-2, decoupled_weight_decay=True)
    tg, te = T.BetaVAEGANTrainer(graph=True, **kw), T.BetaVAEGANTrainer(graph=False, **kw)
    for it in range(4):
        og = {k: v.clone() for k, v in tg.step(x, *lat).items()}
        oe = {k: v.clone() for k, v in te.step(x, *lat).items()}
        for k in oe:
            assert torch.equal(_bits(og[k].float()), _bits(oe[k].float())), (it, k)
    _assert_same(_weights(tg), _weights(te))
    assert len(tg._graphs) == 1 and tg.graph
    for tr in (tg, te):
        for opt in (tr.optimizerEG, tr.optimizerD):
            assert not opt._torch_stepped and opt.param_groups[0]["decoupled_weight_decay"] is True
    plain = T.BetaVAEGANTrainer(graph=False)
    for it in range(4):
        plain.step(x, *lat)
    wp, wg = _weights(plain), _weights(tg)
    assert any(not torch.equal(wp[k], wg[k]) for k in wp if k.endswith("weight"))


# ------------------------------------------------------------------ 10. checkpoint
def test_checkpoint_resumes_the_schedules(monkeypatch):
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    kw = dict(graph=True, lr_scheduler=_lambda_lr, beta_schedule=_beta_warmup)
    tu = T.BetaVAEGANTrainer(**kw)
    for it in range(3):
        tu.step(x, *lat)
    buf = io.BytesIO()
    torch.save(tu.checkpoint(1), buf)
    tu.step(x, *lat)
    want = _weights(tu)
    want_hyper = (tu.optimizerEG.param_groups[0]["lr"], tu.optimizerD.param_groups[0]["lr"], tu.beta, tu.iteration)
    assert want_hyper == (LR0 * 0.9 ** 4, LR0 * 0.9 ** 4, _beta_warmup(3), 4)

    def hyper(tr):
        return (tr.optimizerEG.param_groups[0]["lr"], tr.optimizerD.param_groups[0]["lr"], tr.beta, tr.iteration)

    def read():                                                   # (a loaded optimizer shares the dict's moment tensors: one read per use)
        buf.seek(0)
        return torch.load(buf, weights_only=False, map_location="cuda")

    ck = read()
    assert {"lr_schedulers", "iteration"} <= set(ck)
    fresh = T.BetaVAEGANTrainer(**kw)
    assert fresh.load(ck) == 1
    assert hyper(fresh)[:2] == (LR0 * 0.9 ** 3,) * 2 and fresh.iteration == 3
    fresh.step(x, *lat)
    assert hyper(fresh) == want_hyper
    _assert_same(_weights(fresh), want)
    # in place, under the capture the uninterrupted trainer already has: the same iteration again, no new capture
    caps = list(tu._graphs.values())
    replays = _count_replays(monkeypatch, T)
    assert tu.load_in_place(read()) == 1
    assert hyper(tu)[:2] == (LR0 * 0.9 ** 3,) * 2 and tu.iteration == 3
    tu.step(x, *lat)
    assert hyper(tu) == want_hyper
    _assert_same(_weights(tu), want)
    assert list(tu._graphs.values()) == caps and len(caps) == 1 and replays["n"] == 1
