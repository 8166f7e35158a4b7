"""GPU: which library entry points one ``HipAdam.step()`` calls, and in which order, per configuration.

Which entry point a step takes decides which kernel runs (plain or feature) and how it contracts, so the choice is pinned
here as literal lists.  A recording proxy stands in ``disentangle_mlp_amd._lib._lib`` -- the slot `use_tuning` switches --
forwards every call to the real library and logs its name; the names ``vg_adam_*``, ``vg_grad_*`` and ``vg_absmax*`` are
compared.  Only public API and that slot are touched: the file passes unchanged on either side of a refactor of optim.py.

Tensors: fp32 of 0, 5 and 8192 + 7 elements -- an empty tensor, a pure scalar tail, and a full 8192-element chunk followed
by both a 16-byte body and a tail."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (0, 5, 8192 + 7)
NORM = ["vg_grad_sumsq_partials", "vg_grad_sumsq_multi", "vg_grad_clip_finalize"]
PREFIXES = ("vg_adam_", "vg_grad_", "vg_absmax")


class _Recorder:
    """Forwards every attribute of the real library; calls are logged by name."""

    def __init__(self, lib):
        self._real, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call

    def taken(self):
        return [n for n in self.names if n.startswith(PREFIXES)]


@pytest.fixture
def recorder(monkeypatch):
    from disentangle_mlp_amd import _lib
    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=gen).cuda().requires_grad_() for n in SIZES]
    for p in ps:
        p.grad = torch.randn(p.numel(), generator=gen).cuda()
    return ps


def _step(recorder, groups, **kw):
    from disentangle_mlp_amd.optim import HipAdam
    opt = HipAdam(groups, lr=1e-3, **kw)
    recorder.names.clear()
    opt.step()
    torch.cuda.synchronize()
    return recorder.taken()


# configuration -> (host-scalar launches, capturable launches)
ONE_GROUP = {
    "plain": (dict(), ["vg_adam_step"], ["vg_adam_prepare", "vg_adam_step_dev"]),
    "guard": (dict(nonfinite_guard=True), ["vg_adam_step_checked"], ["vg_adam_prepare", "vg_adam_step_dev_checked"]),
    "ema": (dict(ema_decay=0.9), ["vg_adam_step_ema"], ["vg_adam_prepare", "vg_adam_step_dev_ema"]),
    "clip": (dict(max_grad_norm=1.0), NORM + ["vg_adam_step_clip"], NORM + ["vg_adam_prepare", "vg_adam_step_dev_clip"]),
    "clip-skip": (dict(max_grad_norm=1.0, skip_nonfinite=True), NORM + ["vg_adam_step_clip"],
                  NORM + ["vg_adam_prepare", "vg_adam_step_dev_clip"]),
    "decay-coupled": (dict(weight_decay=0.01), ["vg_adam_step_decay"], ["vg_adam_prepare_dev", "vg_adam_step_dev_decay"]),
    "decay-decoupled": (dict(weight_decay=0.01, decoupled_weight_decay=True), ["vg_adam_step_decay"],
                        ["vg_adam_prepare_dev", "vg_adam_step_dev_decay"]),
}


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@pytest.mark.parametrize("config", list(ONE_GROUP))
def test_one_group_launches(recorder, config, capturable):
    kw, host, dev = ONE_GROUP[config]
    ps = _params()
    before = ps[2].detach().clone()
    assert _step(recorder, ps, capturable=capturable, **kw) == (dev if capturable else host)
    assert not torch.equal(ps[2].detach(), before), "the step must have written the weights"


def test_device_hyper_launches(recorder):
    assert _step(recorder, _params(), capturable=True, device_hyper=True) == ["vg_adam_prepare_dev", "vg_adam_step_dev"]


def test_ema_decay_on_device_launches(recorder):
    got = _step(recorder, _params(), capturable=True, ema_decay=0.9, ema_decay_on_device=True)
    assert got == ["vg_adam_prepare_dev", "vg_adam_step_dev_ema_dev"]


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
def test_decay_in_one_group_only(recorder, capturable):
    """Groups without decay make the launches they always made."""
    ps = _params()
    groups = [dict(params=ps[:2]), dict(params=ps[2:], weight_decay=0.01)]
    want = (["vg_adam_prepare", "vg_adam_step_dev", "vg_adam_prepare_dev", "vg_adam_step_dev_decay"] if capturable
            else ["vg_adam_step", "vg_adam_step_decay"])
    assert _step(recorder, groups, capturable=capturable) == want


def test_two_part_step_of_a_big_linear_weight(recorder):
    """A 1024 x 1024 weight -- the smallest `ops.LINEAR_SPLIT_MIN_WEIGHTS` admits -- stepped inside its weight gradient:
    `begin_fused_step` runs the one prepare of the step, `step()` launches nothing more for that weight."""
    from disentangle_mlp_amd import ops
    from disentangle_mlp_amd.optim import HipAdam
    N = K = 1024
    assert N * K == ops.LINEAR_SPLIT_MIN_WEIGHTS
    gen = torch.Generator().manual_seed(1)
    w = (torch.randn(N, K, generator=gen) * 0.02).cuda().requires_grad_()
    gy, x = torch.randn(32, N, generator=gen).cuda(), torch.randn(32, K, generator=gen).cuda()
    opt = HipAdam([w], lr=1e-3, capturable=True)
    before = w.detach().clone()
    recorder.names.clear()
    regs = opt.begin_fused_step()
    reg = regs[id(w)]
    assert ops.linear_wgrad_adam(gy, x, reg), "the entry point must take this shape"
    reg.done = True                                      # (what functional's backward records)
    opt.step()
    torch.cuda.synchronize()
    taken = recorder.taken()
    assert taken.count("vg_adam_prepare") == 1 and "vg_adam_prepare_dev" not in taken
    assert not [n for n in taken if n.startswith("vg_adam_step")]
    assert [n for n in taken if not n.startswith("vg_absmax")] == ["vg_adam_prepare"]      # (the operands' bounds aside)
    assert "vg_linear_wgrad_adam_dev" in recorder.names
    assert float(opt.state[w]["step"]) == 1.0 and not torch.equal(w.detach(), before)
