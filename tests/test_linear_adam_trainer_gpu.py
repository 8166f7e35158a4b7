"""GPU: the fused weight-gradient + Adam launch of the big Linear layers through the trainers.

Route on (functional.FUSE_LINEAR_ADAM) against route off, in one process, on the same data: every loss of every
iteration and every entry of ``checkpoint(0)`` -- weights, BatchNorm statistics, Adam moments and step counts -- must be
``torch.equal``; there is no tolerance, the fused launch forms the pair's bits.  B = 32 is the smallest batch
`ops.linear_split_ok` admits for the weight gradient (its reduction).

Which launches ran is counted through a wrapper on the library's two fused entry points, not through timing.  Per
beta-VAE-GAN iteration the route takes five: D's ``lth_features.0`` in phase 1, the two encoder heads in phases 2 and 3.
``max_grad_norm`` and a ``grad_hook`` leave none.  ``ema_decay`` leaves three: the averaging step (phase 3, the two
heads) takes the unfused launches; D's optimizer has no average and phase 2 is stepped with ``update_ema=False``, and
"no EMA on this call" is the rule."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, SEED = 32, 4321
LABELS = ((0.9, 0.1), (0.1, 0.9))


def _differences(a, b, where="checkpoint"):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        same = (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a, b))
        return [] if same else [where]
    if isinstance(a, dict) and isinstance(b, dict):
        if list(a) != list(b):
            return [f"{where}: keys {list(a)} != {list(b)}"]
        return [d for k in a for d in _differences(a[k], b[k], f"{where}[{k!r}]")]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [f"{where}: lengths {len(a)} != {len(b)}"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _differences(x, y, f"{where}[{i}]")]
    return [] if type(a) is type(b) and a == b else [where]


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(SEED)
    return [(torch.rand(BATCH, 3, 64, 64, generator=g) * 2 - 1).cuda() for _ in range(6)]


@pytest.fixture
def fused_calls(monkeypatch):
    """[n]: calls of the two fused entry points that launched (returned 0) since the fixture was made."""
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    n = [0]

    def counting(fn):
        def call(*a):
            rc = fn(*a)
            n[0] += rc == 0
            return rc
        return call
    for name in ("vg_linear_wgrad_adam", "vg_linear_wgrad_adam_dev"):
        monkeypatch.setattr(lib, name, counting(getattr(lib, name)), raising=False)
    return n


def _run(name, route, data, iterations, monkeypatch, step_kw=None, **kw):
    from disentangle_mlp_amd import functional as F, trainer as T
    monkeypatch.setattr(F, "FUSE_LINEAR_ADAM", route)
    tr = getattr(T, name)(seed=SEED, **kw)
    losses = []
    for i in range(iterations):
        labels = {} if name == "VAETrainer" else dict(real_label=LABELS[i % 2][0], fake_label=LABELS[i % 2][1])
        losses.append({k: v.clone() for k, v in tr.step(data[i], **labels, **(step_kw or {})).items()})
    torch.cuda.synchronize()
    return tr, losses, tr.checkpoint(0)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_betavaegan_route_on_is_route_off(graph, data, fused_calls, monkeypatch):
    tr0, l0, c0 = _run("BetaVAEGANTrainer", False, data, 6, monkeypatch, graph=graph)
    assert fused_calls[0] == 0
    tr1, l1, c1 = _run("BetaVAEGANTrainer", True, data, 6, monkeypatch, graph=graph)
    if graph:
        assert tr1.graph and len(tr1._graphs) == 1 and fused_calls[0] >= 5      # (the eager warm-up iterations and the capture)
    else:
        assert fused_calls[0] == 5 * 6
    assert (len(tr0._graphs), tr0.graph, tr0.iteration) == (len(tr1._graphs), tr1.graph, tr1.iteration)
    assert _differences(l0, l1, "losses") + _differences(c0, c1) == []
    heads = [tr1.netEG.x_to_mu[0].weight, tr1.netEG.x_to_logvar[0].weight]
    assert all(w.grad is None for w in heads)            # updated inside the backward: no gradient was ever written
    assert [float(tr1.optimizerEG.state[w]["step"]) for w in heads] == [12.0, 12.0]      # two steps per iteration, counted once each


@pytest.mark.parametrize("case", ["ema_decay", "max_grad_norm", "grad_hook"])
def test_options_take_the_unfused_launches(case, data, fused_calls, monkeypatch):
    kw = dict(ema_decay=dict(ema_decay=0.9), max_grad_norm=dict(max_grad_norm=50.0), grad_hook={})[case]
    step_kw = dict(grad_hook=lambda ph, net: None) if case == "grad_hook" else None
    _, l1, c1 = _run("BetaVAEGANTrainer", True, data, 2, monkeypatch, step_kw=step_kw, graph=False, **kw)
    assert fused_calls[0] == (3 * 2 if case == "ema_decay" else 0)
    _, l0, c0 = _run("BetaVAEGANTrainer", False, data, 2, monkeypatch, step_kw=step_kw, graph=False, **kw)
    assert _differences(l0, l1, "losses") + _differences(c0, c1) == []


@pytest.mark.parametrize("name,per_iteration", [("VAETrainer", 2), ("GANTrainer", 1)])
def test_vae_and_gan_trainers(name, per_iteration, data, fused_calls, monkeypatch):
    _, l0, c0 = _run(name, False, data, 1, monkeypatch, graph=False)
    assert fused_calls[0] == 0
    _, l1, c1 = _run(name, True, data, 1, monkeypatch, graph=False)
    assert fused_calls[0] == per_iteration
    assert _differences(l0, l1, "losses") + _differences(c0, c1) == []
