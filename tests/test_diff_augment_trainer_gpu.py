"""GPU: ``diff_augment=`` through the trainers -- exact throughout, no tolerance.  B = 4, the
shapes of the step goldens."""
import pytest
import torch

import _augment_refs as R
from test_grad_clip_trainer_gpu import _assert_same, _batch, _bits, _weights

pytestmark = pytest.mark.gpu

B = 4
FULL = "color,translation,cutout"


def _same(ta, tb, oa, ob, what):
    assert oa.keys() == ob.keys()
    for k in oa:
        assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), (what, k)
    _assert_same(_weights(ta), _weights(tb))


def _cases():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    return ((T.BetaVAEGANTrainer, (x, *lat)), (T.GANTrainer, (x, lat[0])))


def _count_replays(monkeypatch):
    from disentangle_mlp_amd import trainer as T
    count = {"n": 0}
    real = T._CapturedIteration.replay

    def replay(self, *args, **kw):
        count["n"] += 1
        return real(self, *args, **kw)

    monkeypatch.setattr(T._CapturedIteration, "replay", replay)
    return count


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_p_zero_is_the_trainer_without_the_keyword(graph):
    """Every call is a copy: losses and every weight after three steps, bit for bit (the third one is captured)."""
    for cls, args in _cases():
        plain, keyed = cls(graph=graph), cls(graph=graph, diff_augment=(FULL, 0.0))
        for it in range(3):
            oa = {k: v.clone() for k, v in plain.step(*args).items()}
            ob = {k: v.clone() for k, v in keyed.step(*args).items()}
            _same(plain, keyed, oa, ob, (cls.__name__, graph, it))
        assert len(plain._graphs) == len(keyed._graphs) == (1 if graph else 0)
        assert set(plain.checkpoint(0)) == set(keyed.checkpoint(0))


def test_captured_steps_equal_eager_steps_and_replay_one_graph(monkeypatch):
    """p = 1, the uniforms drawn anew by each trainer from its own stream every iteration: the iterations past the warm-up
    are replays of ONE capture."""
    count = _count_replays(monkeypatch)
    for cls, args in _cases():
        count["n"] = 0
        tg, te = cls(graph=True, diff_augment=FULL), cls(graph=False, diff_augment=FULL)
        drawn = []
        for it in range(6):
            og = {k: v.clone() for k, v in tg.step(*args).items()}
            oe = {k: v.clone() for k, v in te.step(*args).items()}
            _same(tg, te, og, oe, (cls.__name__, it))
            if it >= 2:                                           # the capture's static input holds this iteration's draw
                drawn.append(next(iter(tg._graphs.values())).inputs["augment"].clone())
        assert len(tg._graphs) == 1 and tg.graph and not te._graphs
        assert count["n"] == 4                                    # every iteration after the two warm-up ones
        assert all(not torch.equal(a, b) for a, b in zip(drawn, drawn[1:]))      # u changed under the one capture
        assert drawn[0].shape == (cls._augment_sets, B, 8)
        # the eager trainer's stream is where the captured one's is: the same number of draws
        assert torch.equal(tg.draw_augment(B), te.draw_augment(B))


def test_given_uniforms_equal_drawn_ones():
    """`step(augment=...)` with what the trainer would have drawn: the same bits."""
    from disentangle_mlp_amd import trainer as T
    for cls, args in _cases():
        a, b, src = (cls(graph=False, diff_augment=FULL) for _ in range(3))
        for it in range(2):
            oa = {k: v.clone() for k, v in a.step(*args).items()}
            ob = {k: v.clone() for k, v in b.step(*args, augment=src.draw_augment(B)).items()}
            _same(a, b, oa, ob, (cls.__name__, it))
    with pytest.raises(TypeError, match="augment= belongs to diff_augment"):
        T.GANTrainer(graph=False).step(*_cases()[1][1], augment=torch.zeros(3, B, 8).cuda())
    with pytest.raises(ValueError, match="augment must be a float32 tensor of shape"):
        T.GANTrainer(graph=False, diff_augment=FULL).step(*_cases()[1][1], augment=torch.zeros(4, B, 8).cuda())


def test_wiring(monkeypatch):
    """Which tensor goes through which parameter set, in which order; `recon` and phase 2's `data` get the same set."""
    from disentangle_mlp_amd import functional as F, trainer as T
    calls = []
    real = F.diff_augment

    def recording(x, u, policy, p):
        calls.append((x, u, policy, p))
        return real(x, u, policy, p)

    monkeypatch.setattr(F, "diff_augment", recording)
    x, lat = _batch(B)
    g = torch.Generator().manual_seed(3)
    for cls, args, sets in ((T.BetaVAEGANTrainer, (x, *lat), [0, 1, 2, 3, 2]), (T.GANTrainer, (x, lat[0]), [0, 1, 2])):
        aug = torch.rand(cls._augment_sets, B, 8, generator=g).cuda()
        tr = cls(graph=False, diff_augment=("cutout,translation", 0.75))
        calls.clear()
        tr.step(*args, augment=aug)
        assert [(pol, p) for _, _, pol, p in calls] == [(6, 0.75)] * len(sets)
        rows = [next(k for k in range(cls._augment_sets) if u.data_ptr() == aug[k].data_ptr()) for _, u, _, _ in calls]
        assert rows == sets, (cls.__name__, rows)
        for (_, u, _, _), k in zip(calls, rows):
            assert torch.equal(u, aug[k])
        xs = [c[0] for c in calls]
        assert xs[0].data_ptr() == x.data_ptr() and not xs[0].requires_grad               # data
        assert not xs[1].requires_grad and xs[1].shape == x.shape                            # fake.detach()
        if cls is T.BetaVAEGANTrainer:
            assert xs[2].data_ptr() == x.data_ptr()                                          # data again: the no-grad pass
            assert xs[3].requires_grad and xs[3].data_ptr() == xs[1].data_ptr()                # fake, attached
            assert xs[4].requires_grad and xs[4].data_ptr() not in (x.data_ptr(), xs[3].data_ptr())      # recon
        else:
            assert xs[2].requires_grad and xs[2].data_ptr() == xs[1].data_ptr()                # fake, attached


def test_latents_do_not_depend_on_the_option():
    """The streams are separate: the latents a trainer draws are the same with the option on or off, eager and captured."""
    from disentangle_mlp_amd import trainer as T
    x, _ = _batch(B)
    seen = {}
    for name, kw in (("off", {}), ("on", dict(diff_augment=FULL))):
        tr = T.GANTrainer(graph=True, **kw)
        taken = []
        for it in range(4):
            tr.step(x)
            if tr._graphs:
                taken.append(next(iter(tr._graphs.values())).inputs["noise"].clone())
        taken.append(tr.draw_latents(B))
        seen[name] = taken
    assert len(seen["on"]) == len(seen["off"]) == 3
    for a, b in zip(seen["on"], seen["off"]):
        assert torch.equal(a, b)


def test_gradient_at_fake_is_zero_where_the_transpose_drops_it():
    """Policy "translation,cutout" and given uniforms: the gradient arriving at `fake` (phase 2, parameter set 3) is exactly
    0 at every source pixel shifted out of the frame or under the cut, and not all zero elsewhere."""
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    g = torch.Generator().manual_seed(8)
    aug = torch.rand(4, B, 8, generator=g)
    aug[3, 0, 3:7] = torch.tensor([0.0, R.ALMOST_ONE, 0.0, R.ALMOST_ONE])      # image 0: the largest shift, cuts at the corners
    tr = T.BetaVAEGANTrainer(graph=False, diff_augment="translation,cutout")
    got = []
    tr.probe = lambda name, t: got.append(t.detach().clone()) if name == "grad_wrt_fake" else None
    tr.step(x, *lat, augment=aug.cuda())
    assert len(got) == 1 and got[0].shape == x.shape
    grad = got[0].cpu()
    for b in range(B):
        dropped = R.dropped_sources(aug[3, b], 64, 64, 6)
        assert int(dropped.sum()) > 0 and int((~dropped).sum()) > 0
        assert bool((grad[b][:, dropped] == 0).all()), b
        assert bool((grad[b][:, ~dropped] != 0).any()), b


def test_the_option_adds_no_bound_pass(monkeypatch):
    """The 3-channel convolutions that consume the augmented images ask for no bound of their input, so the apply pass
    emits none -- and the option must add no vg_absmax* launch: counted on a recording proxy of the library."""
    from disentangle_mlp_amd import _lib, trainer as T
    from test_optim_launches_gpu import _Recorder
    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", rec)
    for cls, args in _cases():
        counts = {}
        for name, kw in (("off", {}), ("on", dict(diff_augment=FULL))):
            tr = cls(graph=False, **kw)
            tr.step(*args)                                        # (the first iteration packs filter by filter)
            rec.names.clear()
            tr.step(*args)
            torch.cuda.synchronize()
            counts[name] = rec.names.count("vg_absmax") + rec.names.count("vg_absmax_affine") + rec.names.count("vg_absmax_multi")
            augs = (rec.names.count("vg_diff_augment_fwd"), rec.names.count("vg_diff_augment_bwd"))
            # forward: one call per use; backward: one per use that carries a gradient (fake and recon; fake)
            assert augs == ((0, 0) if name == "off" else ((5, 2) if cls is T.BetaVAEGANTrainer else (3, 1))), (cls.__name__, augs)
        assert counts["on"] == counts["off"], (cls.__name__, counts)


def test_vae_trainer_refuses_the_keyword():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="VAETrainer has no discriminator: diff_augment does not apply"):
        T.VAETrainer(diff_augment=FULL)
