"""GPU, B = 4: the weight EMA driven by the trainers.

Kernel level (through ``optim.HipAdam``): ``vg_adam_step_dev_ema_dev`` -- the averaging step that reads ``(float)(1 - decay)``
from a device word -- bit for bit against the entry points a constant decay selects, on tensors of sizes around the
4-element vector and the 8192-element chunk, one of them with its average one float off 16-byte alignment (the scalar
loop) and one large enough to carry a bound word; decay 0; a decay that changes between the replays of one capture; a
skipped step; ``update_ema=False``.

Trainer level: the live state is what it is without the average; `ema_model` follows the fp64 recurrence; one captured
graph serves a decay that changes every iteration; sampling and FID through the shadow; standing BatchNorm statistics
against oracle.modules with ``momentum=None``; checkpoints.

Tolerance of the average (derived, not measured): one step ``fl(e + fl(w * fl(p - e)))`` rounds three times, the weight
``w = (float)(1 - d)`` once more; each rounding is at most 2^-24 relative to a quantity no larger than max(|p|, |e|)
here (p and e have one sign pattern and lie close: |p - e| <= max(|p|, |e|)), and errors carried from earlier steps shrink
by d < 1.  After N averaged steps: 4 * N * 2^-24 * max(|p|, |e|) per tensor, the maximum taken over the tensor and the
averaged steps.  Iterations before ``start_iteration`` (decay 0) copy bits and add nothing."""
import math

import pytest
import torch

import oracle  # noqa: F401
from oracle import modules as O

from test_eval_mode_gpu import _extract, fwd_close
from test_grad_clip_trainer_gpu import _assert_same, _batch, _bits, _weights
from test_schedules_gpu import _count_replays

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 8192, 8193, 2 * 8192 + 7]
OFFSET_N = 8197                     # the tensor whose average is one float off 16-byte alignment: body, tail, two chunks
BIG = (1024, 1024)                  # a Linear weight large enough for a bound word (ops.LINEAR_SPLIT_MIN_WEIGHTS)
DECAY = 0.999
LOSSES = 9


# ------------------------------------------------------------------ kernel level
def _zoo(seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(n,) for n in SIZES] + [(OFFSET_N,), BIG]
    return [dict(p=torch.randn(*s, generator=g), e=torch.randn(*s, generator=g)) for s in shapes]


def _make(zoo, **kw):
    """(parameters, their averages, the optimizer) on clones of ``zoo``; the average of the OFFSET_N tensor starts 4
    bytes into its allocation."""
    from disentangle_mlp_amd.optim import HipAdam
    ps = [torch.nn.Parameter(z["p"].clone().cuda()) for z in zoo]
    es = []
    for z in zoo:
        if z["e"].numel() == OFFSET_N:
            e = torch.zeros(OFFSET_N + 1, device="cuda")[1:]
            e.copy_(z["e"])
            assert e.data_ptr() % 16 == 4 and e.is_contiguous()
        else:
            e = z["e"].clone().cuda()
        es.append(e)
    return ps, es, HipAdam(ps, lr=1e-3, capturable=True, ema_targets=es, **kw)


def _grads(zoo, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(z["p"].shape, generator=g) * scale).cuda() for z in zoo]


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _same_state(a, b, what):
    (pa, ea, oa), (pb, eb, ob) = a, b
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(_bits(x.detach()), _bits(y.detach())), (what, "p", i)
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(oa.state[x][name]), _bits(ob.state[y][name])), (what, name, i)
    for i, (x, y) in enumerate(zip(ea, eb)):
        assert torch.equal(_bits(x), _bits(y)), (what, "e", i)
    assert (oa._bounds is None) == (ob._bounds is None)
    if oa._bounds is not None:
        assert oa._bounds.numel() == 1 and int(_bits(oa._bounds)[0]) != 0      # (emitted: max |p| of the BIG weight)
        assert torch.equal(_bits(oa._bounds), _bits(ob._bounds)), (what, "bound words")
    if oa.nonfinite_guard:
        assert torch.equal(oa.nonfinite_words(), ob.nonfinite_words()), (what, "flag words")
    if oa._clip_rec is not None:
        assert torch.equal(oa.clip_record(), ob.clip_record()), (what, "clip record")


@pytest.mark.parametrize("wd", [dict(), dict(weight_decay=1e-2), dict(weight_decay=1e-2, decoupled_weight_decay=True)],
                         ids=["no-decay", "coupled", "decoupled"])
@pytest.mark.parametrize("clip", [None, 1.0], ids=["no-clip", "clip"])
@pytest.mark.parametrize("guard", [False, True], ids=["no-guard", "guard"])
def test_device_decay_word_gives_the_bits_of_the_constant_decay(guard, clip, wd):
    """Three steps: the decay in a device word against the constant decay of today's entry points (vg_adam_step_dev_ema,
    _dev_clip or _dev_decay, as the configuration selects)."""
    zoo = _zoo()
    cfg = dict(nonfinite_guard=guard, max_grad_norm=clip, **wd)
    new = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True, **cfg)
    old = _make(zoo, ema_decay=DECAY, **cfg)
    assert new[2]._ema_omd is not None and old[2]._ema_omd is None
    for k in range(3):
        grads = _grads(zoo, 40 + k)
        if guard and k == 2:
            grads[4][7] = float("nan")                            # the flag words have something to say (data, not a fault)
        _set_grads(new[0], grads), _set_grads(old[0], grads)
        e_before = [e.clone() for e in new[1]]
        new[2].step(), old[2].step()
        _same_state(new, old, ("step", k))
        assert all(not torch.equal(e, b) for e, b in zip(new[1], e_before))      # the averages moved
        if clip is not None and k == 0:
            assert 0.0 < float(new[2].clip_coef()) < 1.0          # the clip is active
    if guard:
        assert int(new[2].nonfinite_words()[4]) != 0
    word = new[2]._ema_omd
    assert word.dtype == torch.float32 and word.numel() == 1
    assert float(word[0]) == float(torch.tensor(1.0 - DECAY, dtype=torch.float64).float())


def test_decay_zero_stores_the_bits_of_p():
    zoo = _zoo()
    ps, es, opt = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True)
    word = opt._ema_omd
    _set_grads(ps, _grads(zoo, 50))
    opt.set_ema_decay(0.0)
    opt.step()
    torch.cuda.synchronize()
    assert float(word[0]) == 1.0 and opt._ema_omd is word
    for i, (p, e) in enumerate(zip(ps, es)):
        assert torch.equal(_bits(p.detach()), _bits(e)), i
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            opt.set_ema_decay(bad)
    assert opt.ema_decay == 0.0


def test_the_decay_changes_between_the_replays_of_one_capture():
    zoo = _zoo()
    a = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True, nonfinite_guard=True)
    b = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True, nonfinite_guard=True)      # the eager twin
    plan = [_grads(zoo, 60 + k) for k in range(5)]
    _set_grads(a[0], plan[0]), _set_grads(b[0], plan[0])
    a[2].step(), b[2].step()                                      # one eager step each: the state exists
    _same_state(a, b, "eager")
    a[2].prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a[2].step()
    word = a[2]._ema_omd
    for it, (d, gs) in enumerate(zip([0.0, 0.5, 0.999, 0.1], plan[1:])):
        for _, _, o in (a, b):
            o.set_ema_decay(d)
        a[2].sync_hyper()
        _set_grads(a[0], gs), _set_grads(b[0], gs)
        graph.replay()
        if it:
            a[2].replayed()
        b[2].step()
        _same_state(a, b, ("replay", it, d))
        assert a[2]._ema_omd is word and float(word[0]) == float(torch.tensor(1.0 - d, dtype=torch.float64).float())
        if d == 0.0:
            assert all(torch.equal(_bits(p.detach()), _bits(e)) for p, e in zip(a[0], a[1]))
    sa, sb = a[2].state_dict()["state"], b[2].state_dict()["state"]
    assert all(float(sa[i]["step"]) == float(sb[i]["step"]) == 5.0 for i in range(len(zoo)))


def test_a_skipped_step_keeps_the_average():
    zoo = _zoo()
    ps, es, opt = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True, skip_nonfinite=True)
    grads = _grads(zoo, 70)
    _set_grads(ps, grads)
    opt.step()                                                    # a clean step: the state exists, the averages moved
    grads[6][11] = float("inf")
    _set_grads(ps, grads)
    e_before, p_before = [e.clone() for e in es], [p.detach().clone() for p in ps]
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1
    for i, (e, b) in enumerate(zip(es, e_before)):
        assert torch.equal(_bits(e), _bits(b)), i
    for i, (p, b) in enumerate(zip(ps, p_before)):
        assert torch.equal(_bits(p.detach()), _bits(b)), i


def test_update_ema_false_leaves_the_average_and_steps_alike():
    zoo = _zoo()
    a = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True)
    b = _make(zoo, ema_decay=DECAY, ema_decay_on_device=True)
    grads = _grads(zoo, 80)
    _set_grads(a[0], grads), _set_grads(b[0], grads)
    e_before = [e.clone() for e in a[1]]
    a[2].step(update_ema=False), b[2].step()
    torch.cuda.synchronize()
    for i, (e, before, moved) in enumerate(zip(a[1], e_before, b[1])):
        assert torch.equal(_bits(e), _bits(before)) and not torch.equal(e, moved), i
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(x.detach()), _bits(y.detach())), i


# ------------------------------------------------------------------ trainer level
START = 2


def _T():
    from disentangle_mlp_amd import trainer as T
    return T


def _live_params(tr):
    net = getattr(tr, tr._ema_names[0])
    return [p.detach() for p in net.parameters()]


class _Recurrence:
    """``e_k = e_{k-1} + (1 - d_k)(p_k - e_{k-1})`` in fp64 from ``e_0 = p_0``, with the running per-tensor maximum of
    |p| and |e| over the averaged steps."""

    def __init__(self, tr):
        self.e = [p.double().clone() for p in _live_params(tr)]
        self.peak = [torch.zeros((), dtype=torch.float64, device=p.device) for p in self.e]
        self.n = 0

    def update(self, tr, d):
        for i, p in enumerate(_live_params(tr)):
            if d == 0.0:
                self.e[i] = p.double().clone()                    # (1 - d = 1: e_k = p_k, without fp64's own rounding)
            else:
                self.e[i] += (1.0 - d) * (p.double() - self.e[i])
        if d > 0.0:
            self.n += 1
            shadow = list(tr.ema_model.parameters())
            for i, p in enumerate(_live_params(tr)):
                self.peak[i] = torch.maximum(self.peak[i], torch.maximum(p.abs().max(), shadow[i].abs().max()).double())

    def check(self, tr, what):
        names = [k for k, _ in tr.ema_model.named_parameters()]
        worst = 0.0
        for i, e in enumerate(tr.ema_model.parameters()):
            err = float((e.double() - self.e[i]).abs().max())
            bound = 4 * self.n * 2.0 ** -24 * float(self.peak[i])
            worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else math.inf))
            assert err <= bound, (what, names[i], err, bound)
        print(f"{what}: worst error / bound over {len(names)} tensors after {self.n} averaged steps: {worst:.3f}")


def _shadow_has_the_bits_of_the_live(tr):
    return all(torch.equal(_bits(e), _bits(p)) for e, p in zip(tr.ema_model.parameters(), _live_params(tr)))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_vaegan_live_state_is_unchanged_and_the_shadow_follows_the_recurrence(graph, monkeypatch):
    T = _T()
    x, lat = _batch()
    replays = _count_replays(monkeypatch, T)
    sched = T.ema_warmup(DECAY, START)
    tr = T.BetaVAEGANTrainer(graph=graph, ema_decay=sched)
    tw = T.BetaVAEGANTrainer(graph=graph, ema_decay=None)         # the control: today's trainer
    assert tw.ema_model is None and tr.ema_model is not tr.netEG
    shadow, shadow_params = tr.ema_model, list(tr.ema_model.parameters())
    assert all(not p.requires_grad and p.is_cuda for p in shadow_params)
    assert all(a is b for a, b in zip(tr.optimizerEG.ema_tensors(), shadow_params))
    assert tr.optimizerEG.device_scalars and tr.optimizerEG._ema_omd is not None
    assert getattr(tr.optimizerD, "_ema", None) is None          # never the discriminator
    live_ptrs = {p.data_ptr() for p in tr.netEG.parameters()} | {b.data_ptr() for b in tr.netEG.buffers()}
    assert not live_ptrs & ({p.data_ptr() for p in shadow_params} | {b.data_ptr() for b in shadow.buffers()})
    ref = _Recurrence(tr)
    n_tr = 0
    for it in range(6):
        before = replays["n"]
        out = {k: v.clone() for k, v in tr.step(x, *lat).items()}
        n_tr += replays["n"] - before
        ctl = {k: v.clone() for k, v in tw.step(x, *lat).items()}
        assert len(out) == len(ctl) == LOSSES
        for k in ctl:
            assert torch.equal(_bits(out[k].float()), _bits(ctl[k].float())), (it, k)
        _assert_same(_weights(tr), _weights(tw))
        d = sched(it)
        assert tr.optimizerEG.ema_decay == d
        ref.update(tr, d)
        if it < START:
            assert d == 0.0 and _shadow_has_the_bits_of_the_live(tr), it
        else:
            assert not _shadow_has_the_bits_of_the_live(tr), it
    ref.check(tr, f"BetaVAEGANTrainer graph={graph}")
    assert ref.n == 6 - START
    assert tr.ema_model is shadow and all(a is b for a, b in zip(tr.ema_model.parameters(), shadow_params))
    if graph:
        assert tr.graph and len(tr._graphs) == 1                  # one capture serves every decay
        assert n_tr >= 3
    else:
        assert not tr._graphs and n_tr == 0


@pytest.mark.parametrize("cls", ["VAETrainer", "GANTrainer"])
def test_vae_and_gan_trainers_average_their_generating_network(cls, monkeypatch):
    T = _T()
    x, lat = _batch()
    replays = _count_replays(monkeypatch, T)
    sched = T.ema_warmup(DECAY, START)
    tr = getattr(T, cls)(ema_decay=sched)
    tw = getattr(T, cls)()
    live = tr.model if cls == "VAETrainer" else tr.netG
    assert type(tr.ema_model) is type(live) and tr.ema_model is not live
    assert all(a is b for a, b in zip(getattr(tr, tr._ema_names[1]).ema_tensors(), tr.ema_model.parameters()))
    if cls == "GANTrainer":
        assert tr.optimizerD._ema is None
    ref = _Recurrence(tr)
    n_tr = 0
    for it in range(4):
        before = replays["n"]
        out = {k: v.clone() for k, v in tr.step(x, lat[0]).items()}
        n_tr += replays["n"] - before
        ctl = {k: v.clone() for k, v in tw.step(x, lat[0]).items()}
        for k in ctl:
            assert torch.equal(_bits(out[k].float()), _bits(ctl[k].float())), (it, k)
        _assert_same(_weights(tr), _weights(tw))
        ref.update(tr, sched(it))
        assert _shadow_has_the_bits_of_the_live(tr) == (it < START), it
    ref.check(tr, cls)
    assert tr.graph and len(tr._graphs) == 1 and n_tr == 2        # iterations 3 and 4, under one capture
    key = {"VAETrainer": "VAE_model_ema", "GANTrainer": "netG_ema"}[cls]
    ck = tr.checkpoint(1)
    assert set(ck) - set(tw.checkpoint(1)) == {key, "iteration"}
    assert ck[key].keys() == live.state_dict().keys()


@pytest.fixture(scope="module")
def trained():
    """A BetaVAEGANTrainer after three iterations, the last one averaged (shared; the tests below leave its weights
    alone)."""
    T = _T()
    x, lat = _batch()
    tr = T.BetaVAEGANTrainer(ema_decay=T.ema_warmup(DECAY, START))
    for _ in range(3):
        tr.step(x, *lat)
    assert not _shadow_has_the_bits_of_the_live(tr)
    return tr


def _stats_file(tmp_path):
    from disentangle_mlp_amd import fid
    g = torch.Generator().manual_seed(2)
    a = torch.randn(40, 16, generator=g, dtype=torch.float64) * 50 + 100
    path = tmp_path / "ref.npz"
    fid.save_statistics(str(path), a.mean(0), torch.cov(a.t()))
    return str(path)


def test_sampling_and_fid_go_through_the_shadow(trained, tmp_path):
    from disentangle_mlp_amd import fid, model
    from disentangle_mlp_amd.trainer import ModelOpt
    tr = trained
    z = torch.randn(4, 128, generator=torch.Generator().manual_seed(9)).cuda()
    fresh = model.VAE(ModelOpt())
    fresh.load_state_dict({k: v.clone() for k, v in tr.ema_model.state_dict().items()})
    fresh = fresh.cuda()
    with torch.no_grad():
        want, got = fresh.decode(z), tr.ema_model.decode(z)
        live = tr.netEG.decode(z)
    assert torch.equal(_bits(got), _bits(want)) and not torch.equal(got, live)
    stats = _stats_file(tmp_path)
    kw = dict(feature_extractor=_extract)
    ck = tr.checkpoint(1)
    torch.manual_seed(6)
    direct = fid.get_fid_of_generator(tr.ema_model.decode, 6, 128, stats, **kw)
    torch.manual_seed(6)
    res = tr.evaluate([ck], calc_fid=True, n_samples=6, fid_path_pretrained=stats, fid_on_device=True,
                      fid_feature_extractor=_extract, use_ema=True)
    torch.manual_seed(6)
    of_live = fid.get_fid_of_generator(tr.netEG.decode, 6, 128, stats, **kw)
    torch.manual_seed(6)
    res_live = tr.evaluate([ck], calc_fid=True, n_samples=6, fid_path_pretrained=stats, fid_on_device=True,
                           fid_feature_extractor=_extract)
    print(f"FID through the shadow {direct!r}, through the live decoder {of_live!r}")
    assert math.isfinite(direct) and res[0]["FID"] == direct
    assert res_live[0]["FID"] == of_live and of_live != direct


def test_standing_statistics_against_the_oracle(trained):
    from disentangle_mlp_amd import model
    tr = trained
    g = torch.Generator().manual_seed(31)
    batches = [torch.rand(4, 3, 64, 64, generator=g) * 2 - 1 for _ in range(3)]
    eps_gen = torch.Generator(device="cuda")
    eps_gen.manual_seed(5)
    eps = [torch.randn(4, 128, device="cuda", generator=eps_gen).cpu() for _ in range(3)]
    eps_gen.manual_seed(5)
    live_before = {k: v.clone() for k, v in tr.netEG.state_dict().items()}
    weights_before = [p.clone() for p in tr.ema_model.parameters()]
    bns = [m for net in (tr.netEG, tr.ema_model) for m in net.modules() if isinstance(m, model._HipBatchNormMixin)]
    assert bns and all(m.momentum == 0.1 for m in bns)
    # the oracle: the shadow's weights, cumulative averaging, statistics reset
    ref = O.VAE(O.OracleOpt()).double()
    ref.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu()
                         for k, v in tr.ema_model.state_dict().items()}, strict=True)
    for m in ref.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.momentum = None
            m.reset_running_stats()
    ref.train()
    with torch.no_grad():
        for x, e in zip(batches, eps):
            ref(x.double(), e.double())
    used = tr.recalibrate_ema_bn([(x, None) for x in batches] + [None], max_batches=3, eps_generator=eps_gen)
    assert used == 3
    got, want = tr.ema_model.state_dict(), ref.state_dict()
    checked = 0
    for k in want:
        if k.endswith("running_mean") or k.endswith("running_var"):
            fwd_close(got[k], want[k], k)
            checked += 1
    assert checked == len(bns)                                    # a mean and a variance per BatchNorm of the shadow
    assert all(m.momentum == 0.1 for m in bns)
    after = tr.netEG.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in live_before.items())
    assert all(torch.equal(a, b) for a, b in zip(weights_before, tr.ema_model.parameters())) and tr.ema_model.training

    def failing():
        yield batches[0]
        raise RuntimeError("loader died")
    with pytest.raises(RuntimeError, match="loader died"):
        tr.recalibrate_ema_bn(failing())
    assert all(m.momentum == 0.1 for m in bns) and tr.ema_model.training
    with torch.no_grad(), model.eval_mode(tr.ema_model):
        one = tr.ema_model.decode(torch.randn(1, 128, generator=g).cuda())
    assert one.shape == (1, 3, 64, 64) and bool(torch.isfinite(one).all()) and tr.ema_model.training


TODAYS_KEYS = {"epoch", "encoder_decoder_model", "discriminator_model", "encoder_decoder_optimizer",
               "discriminator_optimizer"}


def _clone_checkpoint(ck):
    import copy
    return copy.deepcopy(ck)


def test_checkpoint_round_trip_continues_identically(tmp_path):
    T = _T()
    x, lat = _batch()
    sched = T.ema_warmup(DECAY, START)
    ta = T.BetaVAEGANTrainer(ema_decay=sched)
    for _ in range(4):
        ta.step(x, *lat)
    path = str(tmp_path / "model_1.tar")
    ta.save(path, 1)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == TODAYS_KEYS | {"encoder_decoder_ema", "iteration"} and ck["iteration"] == 4
    assert ck["encoder_decoder_ema"].keys() == ck["encoder_decoder_model"].keys()
    O.VAE(O.OracleOpt()).load_state_dict(ck["encoder_decoder_ema"], strict=True)      # a plain VAE state dict
    tb = T.BetaVAEGANTrainer(ema_decay=sched)
    shadow = tb.ema_model
    assert tb.load(path) == 1 and tb.ema_model is shadow and tb.iteration == 4
    _assert_same(dict(ta.ema_model.state_dict()), dict(tb.ema_model.state_dict()))
    assert not _shadow_has_the_bits_of_the_live(tb)
    for it in range(2):
        oa = {k: v.clone() for k, v in ta.step(x, *lat).items()}
        ob = {k: v.clone() for k, v in tb.step(x, *lat).items()}
        for k in oa:
            assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), (it, k)
        _assert_same(_weights(ta), _weights(tb))
        _assert_same(dict(ta.ema_model.state_dict()), dict(tb.ema_model.state_dict()))
    assert ta.optimizerEG.ema_decay == tb.optimizerEG.ema_decay == sched(5)


def test_checkpoint_without_the_average_and_load_in_place(monkeypatch):
    T = _T()
    x, lat = _batch()
    replays = _count_replays(monkeypatch, T)
    plain = T.BetaVAEGANTrainer(ema_decay=None)
    plain.step(x, *lat)
    ck_plain = _clone_checkpoint(plain.checkpoint(3))
    assert set(ck_plain) == TODAYS_KEYS                           # exactly today's keys
    tr = T.BetaVAEGANTrainer(ema_decay=T.ema_warmup(DECAY, 0))
    for _ in range(3):
        tr.step(x, *lat)
    assert len(tr._graphs) == 1
    cap = next(iter(tr._graphs.values()))
    ck3 = _clone_checkpoint(tr.checkpoint(1))
    tr.step(x, *lat)                                              # iteration 4, from the state of ck3
    want = (_weights(tr), {k: v.clone() for k, v in tr.ema_model.state_dict().items()})
    tr.step(x, *lat)
    n = replays["n"]
    assert tr.load_in_place(ck3) == 1 and tr.iteration == 3
    _assert_same(dict(tr.ema_model.state_dict()), ck3["encoder_decoder_ema"])
    tr.step(x, *lat)                                              # iteration 4 again: a replay of the same capture
    assert replays["n"] == n + 1 and list(tr._graphs.values()) == [cap]
    _assert_same(_weights(tr), want[0])
    _assert_same(dict(tr.ema_model.state_dict()), want[1])
    # a checkpoint without the key: the shadow takes the loaded live weights and buffers, nothing raises
    shadow = tr.ema_model
    assert not _shadow_has_the_bits_of_the_live(tr)
    assert tr.load(ck_plain) == 3 and tr.ema_model is shadow
    _assert_same(dict(tr.ema_model.state_dict()), dict(tr.netEG.state_dict()))
    _assert_same(dict(tr.netEG.state_dict()), ck_plain["encoder_decoder_model"])


class _OneBatch(list):
    """A loader of one batch, as `fit` / `train_epoch` read one: ``for data, _ in loader`` and ``len(loader.dataset)``."""

    def __init__(self, x):
        super().__init__([(x, None)])
        self.dataset = range(x.size(0))


def test_fit_scores_the_shadow_and_evaluate_takes_it_in_eval_mode(tmp_path):
    from disentangle_mlp_amd import fid
    T = _T()
    x, _ = _batch()
    stats = _stats_file(tmp_path)
    tr = T.BetaVAEGANTrainer(ema_decay=0.5)                       # a constant decay: no schedule, no "iteration" key
    assert tr.ema_schedule is None and set(tr.checkpoint(1)) == TODAYS_KEYS | {"encoder_decoder_ema"}
    kw = dict(epochs=1, calc_fid=True, n_samples=6, fid_path_pretrained=stats, fid_on_device=True,
              fid_feature_extractor=_extract, verbose=False)
    torch.manual_seed(6)
    row = tr.fit(_OneBatch(x), use_ema=True, **kw)[0]             # one iteration, then the epoch's FID
    assert tr.iteration == 1 and not _shadow_has_the_bits_of_the_live(tr)
    torch.manual_seed(6)
    direct = fid.get_fid_of_generator(tr.ema_model.decode, 6, 128, stats, feature_extractor=_extract)
    torch.manual_seed(6)
    of_live = fid.get_fid_of_generator(tr.netEG.decode, 6, 128, stats, feature_extractor=_extract)
    assert math.isfinite(direct) and row["FID"] == direct and direct != of_live
    # eval mode applies to the shadow: running statistics of its own first
    assert tr.recalibrate_ema_bn([x, x], max_batches=1) == 1
    modes = []
    h = tr.ema_model.act1[0].register_forward_pre_hook(lambda m, i: modes.append(m.training))
    hl = tr.netEG.act1[0].register_forward_pre_hook(lambda m, i: modes.append("live"))
    torch.manual_seed(6)
    res = tr.evaluate([tr.checkpoint(1)], calc_fid=True, n_samples=6, fid_path_pretrained=stats, fid_on_device=True,
                      fid_feature_extractor=_extract, eval_mode=True, use_ema=True)
    h.remove(), hl.remove()
    assert modes == [False] and tr.ema_model.training and tr.netEG.training
    assert math.isfinite(res[0]["FID"]) and res[0]["FID"] != direct
