"""CPU: the host side of the weight EMA -- the two ``_ema`` Adam entry points of the C ABI (exported, bound, validating
before any launch), optim.HipAdam(ema_decay=...) on the torch fallback path (CPU parameters) against an fp64 recurrence,
its constructor's checks and its state access.

The tolerance is derived, not measured.  One lerp ``fl(e + fl(w * fl(p - e)))`` rounds at most three times, each by at
most 2^-24 relative to a quantity no larger than 2 max(|e|, |p|): per step |e - e_fp64| <= 8 * 2^-24 * max(|e|, |p|).
Errors carried from earlier steps shrink by decay < 1, so after k averaging steps the bound is k * 8 * 2^-24 * M with M
the largest |p|, |e| seen for the element's tensor.  Every element is compared."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_ema_entry_points_are_exported_bound_and_validate_on_the_host(lib):
    from disentangle_mlp_amd import _lib
    from disentangle_mlp_amd.optim import _AdamTensor
    assert _lib.ABI_VERSION == 7 == lib.vg_version()            # entry points were only added: the version stays
    for name in ("vg_adam_step_ema", "vg_adam_step_dev_ema"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the checked signatures plus the host array of device pointers and the decay, in front of the stream
    for ema, checked in (("vg_adam_step_ema", "vg_adam_step_checked"), ("vg_adam_step_dev_ema", "vg_adam_step_dev_checked")):
        assert _lib.SIGNATURES[ema][1] == _lib.SIGNATURES[checked][1][:-1] + [ctypes.c_void_p, ctypes.c_double,
                                                                             ctypes.c_void_p]
    arr = (_AdamTensor * 1)()
    arr[0] = _AdamTensor(None, None, None, None, 0, None)       # an empty tensor: skipped, nothing is launched
    ema = (ctypes.c_void_p * 1)()
    scal = ctypes.c_void_p(64)                                  # never dereferenced on the host: every call below returns first

    def host(tensors, count, ema, decay, flags=None):
        return lib.vg_adam_step_ema(tensors, count, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, flags, ema, decay, None)

    def dev(tensors, count, ema, decay, flags=None):
        return lib.vg_adam_step_dev_ema(tensors, count, 0.9, 0.999, 1e-8, scal, flags, ema, decay, None)

    flags = (ctypes.c_void_p * 1)()
    for call in (host, dev):
        for fl in (None, flags):
            assert call(None, 1, ema, 0.9, fl) == -1            # NULL tensors with count > 0
            assert call(arr, -1, ema, 0.9, fl) == -1
            assert call(arr, 1, None, 0.9, fl) == -1            # ema == NULL: what the existing entry points are for
            assert call(None, 0, None, 0.9, fl) == -1
            for decay in (0.0, 1.0, -0.1, float("nan"), 1.5, float("inf")):
                assert call(arr, 1, ema, decay, fl) == -1, decay
            # nothing to do -- no tensors, or only empty ones: success, no launch
            assert call(None, 0, ema, 0.9, fl) == 0
            assert call(arr, 1, ema, 0.9, fl) == 0
    # the checks the EMA entries share with the checked ones
    assert lib.vg_adam_step_ema(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.03, None, ema, 0.9, None) == -1     # bias_correction1
    assert lib.vg_adam_step_dev_ema(arr, 1, 0.9, 0.999, 1e-8, None, None, ema, 0.9, None) == -1           # no scalars
    arr[0] = _AdamTensor(None, None, None, None, 16, None)      # elements but NULL pointers
    assert host(arr, 1, ema, 0.9) == -1 and dev(arr, 1, ema, 0.9) == -1


def _bound(k, *tensors):
    return k * 8 * 2.0 ** -24 * max(float(t.abs().max()) for t in tensors)


def test_hip_adam_torch_path_follows_the_fp64_recurrence_and_skips_when_told():
    """CPU parameters take torch's step; the EMA is then formed by torch._foreach_lerp_ after it."""
    from disentangle_mlp_amd.optim import HipAdam
    decay = 0.9
    g = torch.Generator().manual_seed(5)
    shapes = [(7,), (3, 5), (1,), (4, 2, 5, 5), (8193,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    opt = HipAdam(ps, lr=1e-2, ema_decay=decay)
    ema = opt.ema_tensors()
    assert len(ema) == len(ps)
    for e, p in zip(ema, ps):                                   # fp32 clones of the parameters
        assert e.dtype == torch.float32 and e.shape == p.shape and e.data_ptr() != p.data_ptr() and not e.requires_grad
        assert torch.equal(e, p.detach())
    ref = [p.detach().double().clone() for p in ps]
    seen = [[p.detach().abs().max()] for p in ps]
    k = 0
    for it, update in enumerate((True, False, True, True)):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        if it == 3:
            ps[2].grad = None                                   # a parameter the step skips keeps its EMA that step
        before = [e.clone() for e in ema]
        p_before = [p.detach().clone() for p in ps]
        opt.step(update_ema=update) if not update else opt.step()
        assert all(not torch.equal(p.detach(), q) for i, (p, q) in enumerate(zip(ps, p_before)) if p.grad is not None)
        if not update:
            assert all(torch.equal(e, b) for e, b in zip(ema, before))
            continue
        k += 1
        for i, (p, e) in enumerate(zip(ps, ema)):
            if p.grad is None:
                assert torch.equal(e, before[i]) and torch.equal(p.detach(), p_before[i])
                continue
            ref[i] = ref[i] + (1.0 - decay) * (p.detach().double() - ref[i])
            seen[i] += [p.detach().abs().max(), e.abs().max()]
            err = float((e.double() - ref[i]).abs().max())
            assert err <= _bound(k, *seen[i]), (it, i, err, _bound(k, *seen[i]))
            assert not torch.equal(e, before[i])                # (it moved)
    assert opt.ema_tensors()[0] is ema[0]                       # fixed at construction, never replaced
    # state_dict stays torch.optim.Adam's
    assert set(opt.state_dict()) == set(torch.optim.Adam([torch.nn.Parameter(torch.ones(1))]).state_dict())
    # the closure path is the torch path too
    ps[0].grad = torch.ones_like(ps[0])
    e0 = ema[0].clone()
    opt.step(lambda: None)
    assert not torch.equal(ema[0], e0)


def test_constructor_validation():
    from disentangle_mlp_amd.optim import HipAdam

    def params():
        return [torch.nn.Parameter(torch.ones(4, 3)), torch.nn.Parameter(torch.ones(5))]
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            HipAdam(params(), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_targets"):
        HipAdam(params(), ema_targets=[torch.ones(4, 3), torch.ones(5)])                 # targets without a decay
    for targets in ([torch.ones(4, 3)],                                                  # too few
                    [torch.ones(3, 4), torch.ones(5)],                                   # mis-shaped
                    [torch.ones(4, 3), torch.ones(5, dtype=torch.float64)],              # another dtype
                    [torch.ones(3, 4).t(), torch.ones(5)]):                              # not contiguous
        with pytest.raises(ValueError, match="ema_targets"):
            HipAdam(params(), ema_decay=0.5, ema_targets=targets)
    ps = params()
    with pytest.raises(ValueError, match="own storage"):
        HipAdam(ps, ema_decay=0.5, ema_targets=[p.detach() for p in ps])
    # the caller's tensors ARE the EMA tensors (a trainer's shadow module), whatever they held
    targets = [torch.full((4, 3), 7.0), torch.full((5,), -2.0)]
    opt = HipAdam(ps, ema_decay=0.5, ema_targets=iter(targets))
    assert all(a is b for a, b in zip(opt.ema_tensors(), targets)) and float(targets[0][0, 0]) == 7.0
    with pytest.raises(RuntimeError, match="constructor"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})
    off = HipAdam(params())
    assert off.ema_decay is None
    for call in (off.ema_tensors, off.reset_ema, off.ema_state, lambda: off.load_ema_state([])):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()
    off.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})               # (still allowed without EMA / guard)


def test_ema_state_round_trip_keeps_the_tensors():
    from disentangle_mlp_amd.optim import HipAdam
    ps = [torch.nn.Parameter(torch.arange(6.0).reshape(2, 3)), torch.nn.Parameter(torch.ones(5))]
    opt = HipAdam(ps, lr=0.1, ema_decay=0.75)
    ptrs = [e.data_ptr() for e in opt.ema_tensors()]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    saved = opt.ema_state()
    assert all(s.data_ptr() != q for s, q in zip(saved, ptrs))                           # copies
    opt.step()
    assert not torch.equal(opt.ema_tensors()[0], saved[0])
    opt.load_ema_state(saved)
    assert all(torch.equal(e, s) for e, s in zip(opt.ema_tensors(), saved))
    assert [e.data_ptr() for e in opt.ema_tensors()] == ptrs
    opt.reset_ema()
    assert all(torch.equal(e, p.detach()) for e, p in zip(opt.ema_tensors(), ps))
    assert [e.data_ptr() for e in opt.ema_tensors()] == ptrs
    opt.load_state_dict(opt.state_dict())
    assert [e.data_ptr() for e in opt.ema_tensors()] == ptrs                             # not by load_state_dict either
    with pytest.raises(ValueError):
        opt.load_ema_state(saved[:1])
    with pytest.raises(ValueError):
        opt.load_ema_state([saved[1], saved[0]])
