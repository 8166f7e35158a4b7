"""GPU: weight decay inside the fused Adam step and the step's hyper-parameters on the device.  Kernel level, through
the ctypes binding, on the tensor zoo of tests/test_grad_clip_gpu.py (26 tensors = two launches, sizes around the
8192-element chunk, two tensors and one EMA tensor one float off 16-byte alignment, some tensors without an average,
sentinels around every written buffer).

Bit identity: the decay step against ``vg_adam_step_clip`` / ``vg_adam_step_dev_clip`` (the entry points that existed
before) run on inputs torch prepared on the device with the same roundings -- decoupled ``p.mul_(s2)``; coupled ``coef * g``
(one op), ``wd32 * p`` (one op), their sum (one op) -- under a record whose coefficient is exactly 1.

Meaning: three steps against ``torch.optim.Adam(weight_decay=..., decoupled_weight_decay=...)`` in fp64 on the CPU.  With E0
the error of the step without decay (``vg_adam_step_clip``, wd = 0) against fp64 Adam, measured in the same test, the decay
step must stay within ``2 E0 + 3 * 2^-23 * max|p|``: the factor 2 for the update's sensitivity to the perturbed gradient,
the second term for the decay's own roundings (at most two per step, three steps).  Measured on an MI355X (lr 1e-3, wd 1e-2,
max|p| 4.605): E0 = 3.452e-07, bound 2.337e-06; coupled 3.313e-07, decoupled 7.423e-07 (host and device scalars alike).

inf / NaN are planted as DATA; nothing here faults the device."""
import ctypes

import numpy as np
import pytest
import torch

import test_grad_clip_gpu as Z
from test_grad_clip_gpu import B1, B2, CHUNK, DECAY, EPS, GRAD, LR, NT, NULL_EMA, PARAM, SENTINEL, SIZES

pytestmark = pytest.mark.gpu

WD = 1e-2
MODES = [("coupled", 0), ("decoupled", 1)]


def _unit_record():
    """A record as vg_grad_clip_finalize leaves it when nothing is clipped: coefficient exactly 1, skip down."""
    rec = torch.zeros(4, device="cuda")
    rec[1] = 1.0
    return rec


def _arrays(st, words, amax, ema_on, grads=None):
    from disentangle_mlp_amd.optim import _AdamTensor
    n = len(st)
    arr = (_AdamTensor * n)()
    for i, s in enumerate(st):
        g = s["g"] if grads is None else grads[i]
        arr[i] = _AdamTensor(s["p"].data_ptr(), g.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["p"].numel(),
                             amax[i:i + 1].data_ptr())
    flags = (ctypes.c_void_p * n)(*[words.data_ptr() + 4 * i for i in range(n)])
    ema = None
    if ema_on:
        ema = (ctypes.c_void_p * n)(*[None if i in NULL_EMA else s["e"].data_ptr() for i, s in enumerate(st)])
    return arr, flags, ema


def _decay_step(st, dev, step, words, amax, rec, ema_on, wd, decoupled, lr=LR):
    """One step through vg_adam_step_decay (``dev`` False) or vg_adam_prepare_dev + vg_adam_step_dev_decay (True);
    ``rec``: the four-word record or None."""
    from disentangle_mlp_amd._lib import check
    lib, stream, n = Z._lib(), Z._stream(), len(st)
    arr, flags, ema = _arrays(st, words, amax, ema_on)
    r = None if rec is None else rec.data_ptr()
    if dev:
        hyper = torch.tensor([lr, wd], dtype=torch.float64, device="cuda")
        scal = torch.zeros(4, device="cuda")
        check(lib.vg_adam_prepare_dev(float(step), None, 0, hyper.data_ptr(), decoupled, B1, B2, scal.data_ptr(), stream),
              "vg_adam_prepare_dev")
        check(lib.vg_adam_step_dev_decay(arr, n, B1, B2, EPS, scal.data_ptr(), flags, ema, DECAY, r, stream),
              "vg_adam_step_dev_decay")
    else:
        bc1, bc2s = 1.0 - B1 ** step, (1.0 - B2 ** step) ** 0.5
        check(lib.vg_adam_step_decay(arr, n, lr, B1, B2, EPS, bc1, bc2s, flags, ema, DECAY, r, wd, decoupled, stream),
              "vg_adam_step_decay")
    torch.cuda.synchronize()


def _torch_prepared(st, coef, wd, decoupled, lr=LR):
    """What the decay step forms in registers, formed by torch on the device: returns the gradients to step on and, for
    the decoupled form, decays ``p`` in place."""
    if decoupled:
        s2 = torch.tensor(np.float32(1.0 - lr * wd), device="cuda")
        for s in st:
            s["p"].mul_(s2)
        return [s["g"] * coef for s in st] if coef is not None else [s["g"] for s in st]
    wd32 = torch.tensor(np.float32(wd), device="cuda")
    out = []
    for s in st:
        gs = s["g"] * coef if coef is not None else s["g"]      # one op
        wp = wd32 * s["p"]                                       # a product of its own ...
        out.append(gs + wp)                                      # ... and a sum of its own
    return out


# ------------------------------------------------------------------ 1. prepare
def test_prepare_dev_forms_the_scalars_of_prepare_and_the_two_decay_words():
    from disentangle_mlp_amd._lib import check
    lib, stream = Z._lib(), Z._stream()
    cases = [(lr, step, adv, wd, dec) for lr in (1e-3, 3e-4, 0.0, 1.0) for step in (1.0, 2.0, 10.0, 1000.0)
             for adv in (0, 1) for wd in (0.0, 1e-2, 0.5) for dec in (0, 1)]
    n = len(cases)
    got = torch.full((n, 8), SENTINEL, device="cuda")            # the four scalars at [i, 2:6], sentinels around
    ref = torch.full((n, 8), SENTINEL, device="cuda")            # vg_adam_prepare's two at [i, 2:4]
    hyper = torch.tensor([[c[0], c[3]] for c in cases], dtype=torch.float64, device="cuda")
    counters = torch.tensor([[c[1] - 1.0, c[1] - 1.0] if c[2] else [-5.0, -5.0] for c in cases], dtype=torch.float64,
                            device="cuda")                        # [:, 0] for the code under test, [:, 1] for the yardstick
    for i, (lr, step, adv, wd, dec) in enumerate(cases):
        check(lib.vg_adam_prepare_dev(0.0 if adv else step, counters[i, 0:1].data_ptr(), adv, hyper[i].data_ptr(), dec,
                                      B1, B2, got[i, 2:].data_ptr(), stream), "vg_adam_prepare_dev")
        check(lib.vg_adam_prepare(0.0 if adv else step, counters[i, 1:2].data_ptr(), adv, lr, B1, B2,
                                  ref[i, 2:].data_ptr(), stream), "vg_adam_prepare")
    torch.cuda.synchronize()
    assert bool((got[:, :2] == SENTINEL).all()) and bool((got[:, 6:] == SENTINEL).all())
    assert torch.equal(Z._bits(got[:, 2:4]), Z._bits(ref[:, 2:4]))
    assert counters[:, 0].tolist() == counters[:, 1].tolist() == [c[1] for c in cases]      # advanced, or stored
    want2 = [np.float32(1.0 - lr * wd) if dec and wd != 0.0 else np.float32(1.0) for lr, _, _, wd, dec in cases]
    want3 = [np.float32(0.0) if dec else np.float32(wd) for _, _, _, wd, dec in cases]
    assert got[:, 4].cpu().numpy().view(np.int32).tolist() == np.array(want2, dtype=np.float32).view(np.int32).tolist()
    assert got[:, 5].cpu().numpy().view(np.int32).tolist() == np.array(want3, dtype=np.float32).view(np.int32).tolist()
    # without a counter (an eager step of an optimizer that was never captured)
    solo = torch.full((8,), SENTINEL, device="cuda")
    check(lib.vg_adam_prepare_dev(3.0, None, 0, hyper[0].data_ptr(), 1, B1, B2, solo[2:].data_ptr(), stream), "solo")
    check(lib.vg_adam_prepare(3.0, None, 0, cases[0][0], B1, B2, ref[0, 2:].data_ptr(), stream), "solo yardstick")
    torch.cuda.synchronize()
    assert torch.equal(Z._bits(solo[2:4]), Z._bits(ref[0, 2:4])) and float(solo[4]) == 1.0 and float(solo[5]) == 0.0
    assert bool((solo[:2] == SENTINEL).all()) and bool((solo[6:] == SENTINEL).all())


# ------------------------------------------------------------------ 2. bit identity
@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-scalars"])
@pytest.mark.parametrize("ema_on", [True, False], ids=["ema", "no-ema"])
@pytest.mark.parametrize("record", ["clipped", "coef-1", "null"])
@pytest.mark.parametrize("name,decoupled", MODES, ids=[m[0] for m in MODES])
def test_decay_step_is_the_clip_step_on_inputs_torch_decayed(dev, ema_on, record, name, decoupled):
    base = Z._state()
    a, b = Z._clone(base), Z._clone(base)
    wa, wb = (torch.full((NT,), 0x10, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    gen = torch.Generator().manual_seed(1)
    unit = _unit_record()
    for k in (1, 2):
        Z._fresh_grads((a, b), gen, 0.1)
        rec = coef = None
        if record != "null":
            _, rec = Z._record_for(a, 1.0 if record == "clipped" else 1e6, 1)
            coef = rec[1:2].clone()
            assert (float(coef) < 1.0) if record == "clipped" else (float(coef) == 1.0)
        prepared = _torch_prepared(b, coef if record == "clipped" else None, WD, decoupled)
        ama.zero_(), amb.zero_()
        _decay_step(a, dev, float(k), wa, ama, rec, ema_on, WD, decoupled)
        Z._step(b, "dev_clip" if dev else "clip", float(k), wb, amb, rec=unit, ema_on=ema_on, grads=prepared)
        Z._same(a, b, (k, name))                                  # p, m, v, the EMA -- sentinels included
        assert torch.equal(Z._bits(ama), Z._bits(amb)) and torch.equal(wa, wb) and wa.tolist() == [0x10] * NT
        assert all(float(ama[i]) == float(a[i]["p"].abs().max()) for i in range(NT))
        Z._same(a, b, k, names=("gbuf",))                         # the gradients are only read
        Z._sentinels_intact(a)
    moved = [i for i in range(NT) if not torch.equal(a[i]["e"], base[i]["e"])]
    assert moved == ([i for i in range(NT) if i not in NULL_EMA] if ema_on else [])


@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-scalars"])
@pytest.mark.parametrize("name,decoupled", MODES, ids=[m[0] for m in MODES])
def test_zero_decay_is_the_clip_step_even_on_an_inf_weight(dev, name, decoupled):
    base = Z._state(2)
    t, el = 7, CHUNK + 3
    base[t]["p"][el] = float("inf")                               # data: 0 * inf would be a NaN the clip step does not have
    a, b = Z._clone(base), Z._clone(base)
    wa, wb = (torch.zeros(NT, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    gen = torch.Generator().manual_seed(3)
    for k in (1, 2):
        Z._fresh_grads((a, b), gen, 0.1)
        _, rec = Z._record_for(a, 1.0, 0)
        ama.zero_(), amb.zero_()
        _decay_step(a, dev, float(k), wa, ama, rec, True, 0.0, decoupled)
        Z._step(b, "dev_clip" if dev else "clip", float(k), wb, amb, rec=rec, ema_on=True)
        Z._same(a, b, (k, name))
        assert torch.equal(Z._bits(ama), Z._bits(amb)) and torch.equal(wa, wb)
        assert wa.tolist() == [PARAM if i == t else 0 for i in range(NT)]
        assert bool(torch.isinf(a[t]["p"][el])) and int((~torch.isfinite(a[t]["p"])).sum()) == 1
    Z._sentinels_intact(a)


# ------------------------------------------------------------------ 3. meaning
def test_decay_step_against_fp64_adam():
    base = Z._state(14)
    gen = torch.Generator().manual_seed(15)
    plan = [[(torch.randn(n, generator=gen)).cuda() for n in SIZES] for _ in range(3)]
    unit = _unit_record()

    def fp64(wd, decoupled):
        ps = [torch.nn.Parameter(s["p"].double().cpu()) for s in base]
        opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, decoupled_weight_decay=bool(decoupled))
        for i, (p, s) in enumerate(zip(ps, base)):               # the zoo's moments, at step 0 (as the kernel is told)
            opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=s["m"].double().cpu(), exp_avg_sq=s["v"].double().cpu())
        for gs in plan:
            for p, g in zip(ps, gs):
                p.grad = g.double().cpu()
            opt.step()
        return [p.detach() for p in ps]

    def err(st, ref):
        return max(float((s["p"].double().cpu() - r).abs().max()) for s, r in zip(st, ref))

    words, amax = torch.zeros(NT, dtype=torch.int32, device="cuda"), torch.zeros(NT, device="cuda")
    a = Z._clone(base)
    for k, gs in enumerate(plan, 1):
        Z._step(a, "clip", float(k), words, amax, rec=unit, ema_on=False, grads=gs)
    e0 = err(a, fp64(0.0, 0))
    pmax = max(float(s["p"].abs().max()) for s in base)
    bound = 2.0 * e0 + 3.0 * 2.0 ** -23 * pmax
    print(f"E0 (no decay, vg_adam_step_clip vs fp64 Adam) {e0:.3e}  max|p| {pmax:.3f}  bound {bound:.3e}")
    assert 0.0 < e0 < 1e-5
    for name, decoupled in MODES:
        for dev in (False, True):
            a = Z._clone(base)
            for k, gs in enumerate(plan, 1):
                for s, g in zip(a, gs):
                    s["g"].copy_(g)
                _decay_step(a, dev, float(k), words, amax, None, False, WD, decoupled)
            e = err(a, fp64(WD, decoupled))
            moved = err(a, fp64(0.0, 0))
            print(f"{name} {'dev' if dev else 'host'}: error {e:.3e}  (distance to the undecayed fp64 run {moved:.3e})")
            assert e <= bound, (name, dev, e, bound)
            assert moved > 2.0 * bound                            # the decay is above what the bound would hide
    assert words.tolist() == [0] * NT


# ------------------------------------------------------------------ 4. skip
@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-scalars"])
@pytest.mark.parametrize("name,decoupled", MODES, ids=[m[0] for m in MODES])
def test_skip_stores_nothing_decays_nothing_and_the_next_step_is_the_plain_decay_step(dev, name, decoupled):
    base = Z._state(4)
    gen = torch.Generator().manual_seed(5)
    a, b = Z._clone(base), Z._clone(base)
    wa, wb = (torch.zeros(NT, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    Z._fresh_grads((a, b), gen, 0.1)
    t, el = 7, 2 * CHUNK + 5
    a[t]["g"][el] = float("inf")
    full, rec = Z._record_for(a, 1.0, 1)
    assert rec.view(torch.int32)[2:].tolist() == [1, 1]
    _decay_step(a, dev, 1.0, wa, ama, rec, True, WD, decoupled)
    Z._same(a, base, "skipped")                                   # p, m, v, e of every tensor, sentinels included
    assert all(float(ama[i]) == float(base[i]["p"].abs().max()) for i in range(NT))
    assert wa.tolist() == [GRAD if i == t else 0 for i in range(NT)]
    # the following clean step: the plain decay step at the advanced count
    wa.zero_()
    Z._fresh_grads((a, b), gen, 0.1)
    full, rec = Z._record_for(a, 1.0, 1, rec=full)
    assert rec.view(torch.int32)[2:].tolist() == [0, 1]
    ama.zero_(), amb.zero_()
    _decay_step(a, dev, 2.0, wa, ama, rec, True, WD, decoupled)
    _decay_step(b, dev, 2.0, wb, amb, rec, True, WD, decoupled)
    Z._same(a, b, "after")
    assert torch.equal(Z._bits(ama), Z._bits(amb)) and wa.tolist() == wb.tolist() == [0] * NT
    assert all(not torch.equal(a[i]["p"], base[i]["p"]) for i in range(NT))
    Z._sentinels_intact(a)


# ------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_launch_nothing():
    lib, stream = Z._lib(), Z._stream()
    base = Z._state(8)
    a = Z._clone(base)
    Z._fresh_grads((a,), torch.Generator().manual_seed(9), 0.1)
    words, amax = torch.zeros(NT, dtype=torch.int32, device="cuda"), torch.zeros(NT, device="cuda")
    arr, flags, ema = _arrays(a, words, amax, True)
    bc1, bc2s = 1.0 - B1, (1.0 - B2) ** 0.5
    scal = torch.full((12,), SENTINEL, device="cuda")
    hyper = torch.tensor([LR, WD], dtype=torch.float64, device="cuda")
    counter = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    rec = _unit_record()
    for wd in (-1e-2, float("nan"), -float("inf")):
        for dec in (0, 1):
            assert lib.vg_adam_step_decay(arr, NT, LR, B1, B2, EPS, bc1, bc2s, flags, ema, DECAY, rec.data_ptr(), wd, dec,
                                          stream) == -1
    for decay in (0.0, 1.0, float("nan")):                        # the clip step's own rejections
        assert lib.vg_adam_step_decay(arr, NT, LR, B1, B2, EPS, bc1, bc2s, flags, ema, decay, None, WD, 0, stream) == -1
        assert lib.vg_adam_step_dev_decay(arr, NT, B1, B2, EPS, scal[4:].data_ptr(), flags, ema, decay, None, stream) == -1
    assert lib.vg_adam_step_decay(arr, NT, LR, B1, B2, EPS, 0.0, bc2s, flags, ema, DECAY, None, WD, 0, stream) == -1
    assert lib.vg_adam_step_dev_decay(arr, NT, B1, B2, EPS, None, flags, ema, DECAY, None, stream) == -1      # no scalars
    assert lib.vg_adam_prepare_dev(1.0, counter.data_ptr(), 0, None, 0, B1, B2, scal[4:].data_ptr(), stream) == -1
    assert lib.vg_adam_prepare_dev(1.0, counter.data_ptr(), 0, hyper.data_ptr(), 0, B1, B2, None, stream) == -1
    assert lib.vg_adam_prepare_dev(1.0, None, 1, hyper.data_ptr(), 0, B1, B2, scal[4:].data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert bool((scal == SENTINEL).all()) and float(counter) == 7.0 and words.tolist() == [0] * NT
    assert float(amax.abs().max()) == 0.0
    Z._same(a, base, "refused")
