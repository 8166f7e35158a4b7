"""GPU: ``ada=`` through the trainers -- exact throughout, no tolerance.  B = 8; interval 2 and
rate 1/64 (``kimg=0.064``), so an adjustment moves p by 16/64 = 0.25, from p0 = 0.5."""
import copy

import numpy as np
import pytest
import torch

import _ada_refs as A
from test_diff_augment_trainer_gpu import _count_replays, _same
from test_grad_clip_trainer_gpu import _assert_same, _batch, _bits, _weights

pytestmark = pytest.mark.gpu

B = 8
FULL = "color,translation,cutout"
ADA = dict(interval=2, kimg=0.064)
CASES = [(name, loss) for name in ("BetaVAEGANTrainer", "GANTrainer") for loss in (None, "logistic")]
IDS = [f"{name}-{loss or 'bce'}" for name, loss in CASES]


def _case(name):
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch(B)
    return getattr(T, name), ((x, *lat) if name == "BetaVAEGANTrainer" else (x, lat[0]))


def _kw(loss, **more):
    return dict(diff_augment=(FULL, 0.5), ada=ADA, **({} if loss is None else dict(gan_loss=loss)), **more)


def _planted(sets, seed):
    """Uniforms with the gates spread over [0, 1): every p of the 0.25 grid opens another set of images."""
    u = torch.rand(sets, B, 8, generator=torch.Generator().manual_seed(seed))
    u[:, :, 7] = (torch.arange(B) + 0.5) / B
    return u.cuda()


def _load(tr, ck):
    return tr.load(copy.deepcopy(ck))                                  # (an optimizer may adopt the tensors it is given)


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("name,loss", CASES, ids=IDS)
def test_capture_equals_eager_and_r_t_comes_from_the_real_head(name, loss, monkeypatch):
    """Six iterations, 3..6 replays of ONE capture, against an eager twin: weights, dict and the eight words bit for bit.
    In the eager twin the controller's input is recorded: its sum is the dict's sum of the phase-1 real head, and the
    restatement fed with the recorded vectors gives the trajectory of ``augment_p`` / ``ada_rt``."""
    from disentangle_mlp_amd import ops
    cls, args = _case(name)
    count = _count_replays(monkeypatch)
    tg, te = cls(graph=True, **_kw(loss)), cls(graph=False, **_kw(loss))
    recorded, real = [], ops.ada_update

    def recording(d, state, *a, **k):
        if state is te._ada_state:                                    # (the eager twin only: no clone inside the capture)
            recorded.append((d.clone(), a, k))
        return real(d, state, *a, **k)

    monkeypatch.setattr(ops, "ada_update", recording)
    key, threshold = ("D_x_sum", 0.5) if loss is None else ("D_logit_real_sum", 0.0)
    st, ps = A.state(0.5), []
    for it in range(6):
        og, oe = _clone(tg.step(*args)), _clone(te.step(*args))
        _same(tg, te, og, oe, (name, loss, it))
        assert {"augment_p", "ada_rt"} <= og.keys()
        assert torch.equal(tg._ada_state, te._ada_state), it
        assert len(recorded) == it + 1
        d, a, k = recorded[-1]
        assert (a, k) == ((threshold, 0.6, 1 / 64, 2), {}) and d.shape == (B,)
        assert torch.equal(_bits(d.sum()), _bits(oe[key])), (it, key)      # the phase-1 REAL head's output of this iteration
        st = A.update(st, d.cpu().numpy(), threshold, 0.6, 1 / 64, 2)
        assert np.array_equal(te._ada_state.cpu().numpy(), A.words(st)), it
        assert float(oe["augment_p"]) == float(st["p"]) == float(tg.augment_p) and float(oe["ada_rt"]) == float(st["rt"])
        ps.append(float(st["p"]))
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs and count["n"] == 4
    assert st["adjustments"] == 3 and ps[0] == 0.5 and ps[1] == ps[2] != 0.5 and ps[3] != ps[1]      # p moved under the one capture
    assert tg.ada_report() == {w: (float(st[w]) if w in ("p", "rt") else st[w]) for w in A.WORDS}


@pytest.mark.parametrize("name,loss", CASES, ids=IDS)
def test_an_iteration_uses_the_p_the_previous_one_left(name, loss):
    """In front of iteration 3, right after the adjustment of iteration 2: the step of the ADA trainer equals the step of
    a trainer WITHOUT the keyword, built at that fixed p and loaded from the checkpoint, on the same inputs."""
    cls, args = _case(name)
    ta = cls(graph=False, **_kw(loss))
    for _ in range(2):
        ta.step(*args)
    rep = ta.ada_report()
    p_t = rep["p"]
    assert rep["adjustments"] == 1 and p_t in (0.25, 0.75)
    ck = copy.deepcopy(ta.checkpoint(0))
    tb = cls(graph=False, diff_augment=(FULL, p_t), **({} if loss is None else dict(gan_loss=loss)))
    _load(tb, ck)
    assert tb._ada_state is None
    aug = _planted(cls._augment_sets, seed=5)
    gates = aug[0, :, 7].cpu()
    assert int((gates < p_t).sum()) != int((gates < 0.5).sum())       # the inputs tell p_t from p0
    oa, ob = _clone(ta.step(*args, augment=aug)), _clone(tb.step(*args, augment=aug))
    assert oa.keys() - ob.keys() == {"augment_p", "ada_rt"} and ob.keys() <= oa.keys()
    for k in ob:
        assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), k
    _assert_same(_weights(ta), _weights(tb))
    assert float(oa["augment_p"]) == p_t                              # (iteration 3 is mid-interval: the word stayed)


@pytest.mark.parametrize("name,loss", CASES, ids=IDS)
def test_checkpoint_round_trip_continues_the_trajectory(name, loss):
    """Checkpoint mid-interval (calls = 1) -> a new trainer -> load: the next three iterations bit for bit, the words
    included; BetaVAEGANTrainer: `load_in_place` does the same under the live capture (GANTrainer has none)."""
    cls, args = _case(name)
    augs = [_planted(cls._augment_sets, seed=s) for s in range(6)]
    ta = cls(graph=True, **_kw(loss))
    for it in range(3):
        ta.step(*args, augment=augs[it])
    ck = copy.deepcopy(ta.checkpoint(0))
    assert ck["ada_state"].device.type == "cpu" and int(ck["ada_state"][3]) == 1 and int(ck["ada_state"][5]) == 1

    def three_more(tr):
        outs = []
        for it in range(3, 6):
            outs.append((_clone(tr.step(*args, augment=augs[it])), tr._ada_state.clone()))
        return outs, _weights(tr)

    first, w_first = three_more(ta)
    assert int(first[-1][1][5]) == 3                                  # two more adjustments on the way
    tb = cls(graph=True, diff_augment=(FULL, 0.0), ada=ADA, **({} if loss is None else dict(gan_loss=loss)))      # (another p0)
    buffer = tb._ada_state
    _load(tb, ck)
    assert tb._ada_state is buffer and torch.equal(buffer.cpu(), ck["ada_state"])
    second, w_second = three_more(tb)
    for (oa, sa), (ob, sb) in zip(first, second):
        assert oa.keys() == ob.keys() and torch.equal(sa, sb)
        for k in oa:
            assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), k
    _assert_same(w_first, w_second)
    # a checkpoint without the key loads and keeps the current state
    before = tb._ada_state.clone()
    _load(tb, {k: v for k, v in ck.items() if k != "ada_state"})
    assert torch.equal(tb._ada_state, before)
    if hasattr(ta, "load_in_place"):
        graphs = dict(ta._graphs)
        assert len(graphs) == 1
        ta.load_in_place(ck)
        assert torch.equal(ta._ada_state.cpu(), ck["ada_state"])
        third, w_third = three_more(ta)
        assert ta._graphs == graphs                                   # the same capture, replayed from the loaded state
        for (oa, sa), (oc, sc) in zip(first, third):
            assert torch.equal(sa, sc)
            for k in oa:
                assert torch.equal(_bits(oa[k].float()), _bits(oc[k].float())), k
        _assert_same(w_first, w_third)


@pytest.mark.parametrize("name", ["BetaVAEGANTrainer", "GANTrainer"])
def test_keyword_off_changes_nothing(name, monkeypatch):
    """Without the keyword the step's dict has no new key, no `_dev` launch and no controller is launched and the capture
    key is the fixed-p form; with it the key carries the policy and the controller's arguments in place of p."""
    from disentangle_mlp_amd import _lib
    from test_optim_launches_gpu import _Recorder
    cls, args = _case(name)
    fwd, bwd = (5, 2) if name == "BetaVAEGANTrainer" else (3, 1)      # one call per use; backward: per use that carries a gradient
    off, on = cls(graph=False, diff_augment=(FULL, 0.5)), cls(graph=False, **_kw(None))
    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", rec)
    names = {}
    for label, tr in (("off", off), ("on", on)):
        rec.names.clear()
        out = tr.step(*args)
        torch.cuda.synchronize()
        names[label] = (list(rec.names), set(out))
    assert names["on"][1] - names["off"][1] == {"augment_p", "ada_rt"} and names["off"][1] <= names["on"][1]
    calls_off, calls_on = names["off"][0], names["on"][0]
    assert not any(n.endswith("_dev") and "augment" in n for n in calls_off) and "vg_ada_update" not in calls_off
    assert calls_off.count("vg_diff_augment_fwd") == fwd and calls_off.count("vg_diff_augment_bwd") == bwd
    assert calls_on.count("vg_diff_augment_fwd_dev") == fwd and calls_on.count("vg_diff_augment_bwd_dev") == bwd
    assert "vg_diff_augment_fwd" not in calls_on and "vg_diff_augment_bwd" not in calls_on
    assert calls_on.count("vg_ada_update") == 1 and calls_on[-1] == "vg_ada_update"      # the iteration's last launch
    assert (FULL, 7, 0.5) in off._host_state_key() and not any(isinstance(k, tuple) and k and k[0] == "ada" for k in off._host_state_key())
    assert (FULL, 7) in on._host_state_key() and ("ada", 0.6, 1 / 64, 2) in on._host_state_key()
    assert (FULL, 7, 0.5) not in on._host_state_key()
