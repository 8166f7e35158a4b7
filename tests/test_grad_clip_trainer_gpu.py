"""GPU, B = 4: the trainers with ``max_grad_norm`` / ``skip_nonfinite``.  The captured iteration -- norm pass, finalize
and clip step inside the graph -- is the eager iteration bit for bit and clips in every optimizer step; an inf planted in
ONE gradient of ONE optimizer step (a tensor hook on a parameter: data, nothing faults the device) is skipped, counted
and leaves the other optimizer steps of the iteration those of an undisturbed trainer; without the opt-in the same inf
raises `NonFiniteError` as before.

Global gradient norms seen at B = 4 (seed 999, this batch, max_grad_norm = 1), iterations 1 - 4: discriminator step
11.9, 4.79, 56.5, 47.9; EG phase 2 2.79e5, 1.71e5, 2.55e5, 4.04e5; EG phase 3 9.31e4, 8.02e4, 7.91e4, 4.20e4 -- every
one above the max_grad_norm of 1.0 used here, so every step is clipped (the test asserts it).

The first test also pins what keeps a captured iteration's buffers alive (`_CapturedIteration._buffers`): see
`_plant_stale_capture_workspace`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 4
MAX_NORM = 1.0
HOOKED = "x_to_mu.3.weight"                  # an encoder Linear weight: one gradient in phase 2, one in phase 3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch(b=B, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(b, 3, 64, 64, generator=g) * 2 - 1).cuda()
    lat = [torch.randn(b, 128, generator=g).cuda() for _ in range(3)]
    return x, lat


def _weights(tr, only=None):
    sd = {}
    for a, net, opt in tr._guarded_optimizers():
        if only is not None and a != only:
            continue
        sd.update({f"{a}.{k}": v.detach().clone() for k, v in net.state_dict().items()})
        for i, st in opt.state_dict()["state"].items():      # (state_dict: the host's step counts follow the replays)
            sd.update({f"{a}.opt{i}.{k}": v.detach().clone() for k, v in st.items()})
    return sd


def _assert_same(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if any(s in k for s in skip):
            continue
        x, y = a[k], b[k]
        assert torch.equal(x, y) if not x.is_floating_point() else torch.equal(_bits(x.float()), _bits(y.float())), k


def _plant_stale_capture_workspace():
    """What an earlier, since destroyed capture leaves behind: a workspace under the capture stream's key that the next
    capture finds too small.  One byte, so the first request of the capture replaces it before any kernel could use it."""
    from disentangle_mlp_amd import ops
    if torch.cuda.graph.default_capture_stream is None:          # (what torch.cuda.graph does on first use)
        torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
    key = ("cuda", torch.cuda.current_device(), torch.cuda.graph.default_capture_stream.cuda_stream)
    stale = ops._workspaces[key] = torch.empty(1, dtype=torch.uint8, device="cuda")
    return stale


def test_graphed_iteration_with_clipping_is_the_eager_one_and_clips_every_step():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    tg = T.BetaVAEGANTrainer(beta=25.0, graph=True, max_grad_norm=MAX_NORM)
    te = T.BetaVAEGANTrainer(beta=25.0, graph=False, max_grad_norm=MAX_NORM)
    seen = []                                                    # (iteration, step, norm, coef) of the eager trainer

    def look(phase, net):                                        # in front of the phase-3 step: phase 2's record
        if phase == "EG3":
            seen.append((te.iteration, "EG2", te.optimizerEG.grad_norm().clone(), te.optimizerEG.clip_coef().clone()))

    for it in range(4):                                          # two eager warm-up iterations, the capture, one more replay
        if it == 2:
            stale = _plant_stale_capture_workspace()
        og = {k: v.clone() for k, v in tg.step(x, *lat).items()}
        oe = {k: v.clone() for k, v in te.step(x, *lat, grad_hook=look).items()}
        for k in oe:
            assert torch.equal(_bits(og[k].float()), _bits(oe[k].float())), (it, k)
        for name, a, b in (("D", tg.optimizerD, te.optimizerD), ("EG3", tg.optimizerEG, te.optimizerEG)):
            assert torch.equal(a.clip_record(), b.clip_record()), (it, name)      # norm, coefficient, skip, count
            seen.append((it, name, b.grad_norm().clone(), b.clip_coef().clone()))
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs                   # replaying, no fallback
    # a workspace that existed when the capture began is kept for as long as the graph: nodes captured before a regrow
    # in the middle of the capture point into it (here nothing does: the planted one is too small for any kernel)
    assert any(b is stale for b in next(iter(tg._graphs.values()))._buffers)
    _assert_same(_weights(tg), _weights(te))
    assert tg.check_finite() is None and te.check_finite() is None
    assert tg.skipped_steps() == {} == te.skipped_steps()                          # skip_nonfinite is off
    assert len(seen) == 12
    for it, name, norm, coef in seen:
        print(f"iteration {it} {name}: norm {float(norm):.6g} coef {float(coef):.6g}")
        assert float(norm) > MAX_NORM and 0.0 < float(coef) < 1.0, (it, name, float(norm), float(coef))
        assert abs(float(coef) - MAX_NORM / (float(norm) + 1e-6)) <= 2.0 ** -22 * float(coef)      # (norm itself is rounded)


def _run_with_one_poisoned_gradient(tr, x, lat, at_iteration):
    """``tr.step`` with an inf planted into ``HOOKED``'s gradient of the phase-3 backward of iteration ``at_iteration``."""
    state = {"armed": False, "fired": 0}
    p = dict(tr.netEG.named_parameters())[HOOKED]

    def poison(g):
        if not state["armed"]:
            return None
        state["armed"], state["fired"] = False, state["fired"] + 1
        g = g.clone()
        g.view(-1)[5] = float("inf")
        return g

    def arm(phase, net):                                         # in front of the phase-2 step: the next backward is phase 3's
        if phase == "EG2" and tr.iteration == at_iteration:
            state["armed"] = True

    handle = p.register_hook(poison)
    try:
        for _ in range(at_iteration + 1):
            tr.step(x, *lat, grad_hook=arm)
    finally:
        handle.remove()
    assert state["fired"] == 1
    return p


def test_a_poisoned_step_is_skipped_counted_and_leaves_the_other_steps_alone():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    tr = T.BetaVAEGANTrainer(beta=25.0, graph=False, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    un = T.BetaVAEGANTrainer(beta=25.0, graph=False, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    snap = {}

    def before_phase3(phase, net):
        if phase == "EG3" and un.iteration == 1:
            snap.update(_weights(un, only="netEG"))

    for _ in range(2):
        un.step(x, *lat, grad_hook=before_phase3)
    p = _run_with_one_poisoned_gradient(tr, x, lat, at_iteration=1)
    assert bool(torch.isinf(p.grad.view(-1)[5]))                 # the planted gradient is what the step read
    assert tr.check_finite() is None                             # skipped: the weights are clean
    assert tr.skipped_steps() == {"netEG": 1, "netD": 0}
    assert tr.optimizerEG.nonfinite() == {}                      # the skipped step's GRAD bit was cleared
    assert float(tr.optimizerEG.clip_coef()) == 0.0
    # the discriminator's step of that iteration: the undisturbed trainer's
    _assert_same(_weights(tr, only="netD"), _weights(un, only="netD"))
    # netEG: phase 2's step was made, phase 3's was not -- weights and moments are the undisturbed trainer's in front of
    # its phase-3 step; BatchNorm's running statistics saw phase 3's forward pass, the step count advanced
    _assert_same(_weights(tr, only="netEG"), snap, skip=("running_", "num_batches_tracked", ".step"))
    steps = {float(st["step"]) for st in tr.optimizerEG.state_dict()["state"].values()}
    assert steps == {4.0}
    assert all(bool(torch.isfinite(q).all()) for q in tr.netEG.parameters())
    # the run goes on
    tr.step(x, *lat)
    assert tr.check_finite() is None and tr.skipped_steps() == {"netEG": 1, "netD": 0}


def test_without_the_opt_in_the_same_gradient_raises():
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    tr = T.BetaVAEGANTrainer(beta=25.0, graph=False, max_grad_norm=MAX_NORM)
    _run_with_one_poisoned_gradient(tr, x, lat, at_iteration=1)
    with pytest.raises(T.NonFiniteError) as e:
        tr.check_finite()
    assert {n.split(".")[0] for n, _ in e.value.found} == {"netEG"}
    assert (f"netEG.{HOOKED}", "grad+param") in e.value.found
