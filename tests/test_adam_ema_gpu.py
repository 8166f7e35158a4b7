"""GPU: the weight EMA inside the fused Adam step.  Kernel level -- vg_adam_step_ema / vg_adam_step_dev_ema through the
ctypes binding: p, m, v, the amax words and the flag words are the checked step's bits, every EMA element follows an
fp64 lerp of the device's own p, sentinels and un-averaged tensors stay untouched, a NaN goes through.  Optimizer level --
optim.HipAdam(ema_decay=...) with host and device scalars: the caller's ``ema_targets`` are written in place,
``update_ema=False`` makes the plain step, and the step itself is the bits of an optimizer without EMA.

The tolerance is derived, not measured.  One lerp ``fl(e + fl(w * fl(p - e)))`` rounds at most three times, each by at
most 2^-24 relative to a quantity no larger than 2 max(|e|, |p|): per step |e_dev - e_fp64| <= 8 * 2^-24 * max(|e|, |p|).
Errors carried from earlier steps shrink by decay < 1, so after k steps the bound is k * 8 * 2^-24 * M with M the largest
|p|, |e| seen for the element's tensor.  Every element is compared.

NaNs are planted as DATA (a NaN written into a gradient); nothing here faults the device."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD, PARAM = 1, 2
CHUNK = 8192
CYCLE = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
NT = 26                                      # two launches: 24 + 2
SIZES = [CYCLE[i % len(CYCLE)] for i in range(NT)]
UNALIGNED = (6, 13)                          # p, g, m, v (and e) start one float into their allocation: the scalar path
EMA_OFFSET = 15                              # p, g, m, v aligned, the EMA tensor one float off: the scalar path as well
NULL_EMA = (2, 9, 12, 21, 25)                # stepped, not averaged (one of them in the second launch)
PAD = 64                                     # sentinel floats on each side of every EMA buffer
SENTINEL = -12345.678
DECAY = 0.9
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _bits(t):
    return t.contiguous().view(torch.int32)


def _off(t, i):
    """A tensor with ``t``'s values that starts one float into its allocation for the unaligned tensors."""
    if i in UNALIGNED:
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:].copy_(t)
        return buf[1:]
    return t.clone()


def _state(seed=0):
    gen = torch.Generator().manual_seed(seed)
    st = []
    for i, n in enumerate(SIZES):
        p = _off(torch.randn(n, generator=gen).cuda(), i)
        g = _off(torch.zeros(n).cuda(), i)
        m = _off((torch.randn(n, generator=gen) * 0.01).cuda(), i)
        v = _off((torch.rand(n, generator=gen) * 1e-3).cuda(), i)
        shift = 1 if i in UNALIGNED or i == EMA_OFFSET else 0
        ebuf = torch.full((n + 2 * PAD + 1,), SENTINEL, device="cuda")
        e = ebuf[PAD + shift:PAD + shift + n]
        e.copy_(torch.randn(n, generator=gen))               # (not the parameters: the average has a history)
        st.append(dict(p=p, g=g, m=m, v=v, ebuf=ebuf, e=e, shift=shift))
    for i in UNALIGNED:
        assert all(st[i][k].data_ptr() % 16 == 4 for k in "pgmve")
    assert all(st[EMA_OFFSET][k].data_ptr() % 16 == 0 for k in "pgmv") and st[EMA_OFFSET]["e"].data_ptr() % 16 == 4
    assert all(st[i][k].data_ptr() % 16 == 0 for i in range(NT) if i not in UNALIGNED + (EMA_OFFSET,) for k in "pgmve")
    return st


def _clone(st):
    out = []
    for i, s in enumerate(st):
        ebuf = s["ebuf"].clone()
        out.append(dict(p=_off(s["p"], i), g=_off(s["g"], i), m=_off(s["m"], i), v=_off(s["v"], i), ebuf=ebuf,
                        e=ebuf[PAD + s["shift"]:PAD + s["shift"] + s["p"].numel()], shift=s["shift"]))
    return out


def _fresh_grads(sts, gen, scale=0.1):
    for i, n in enumerate(SIZES):
        g = (torch.randn(n, generator=gen) * scale).cuda()
        for st in sts:
            st[i]["g"].copy_(g)


def _two_scalars():
    """The two device scalars ``vg_adam_prepare`` writes, as the front of a four-float buffer whose words [2:4] hold NaN.
    The entry points paired with ``vg_adam_prepare`` own two words: had one of them read scalars[2..3] (the decay words
    of ``vg_adam_prepare_dev``), every weight would decay by NaN and no bit comparison below would hold."""
    buf = torch.full((4,), float("nan"), device="cuda")
    return buf, buf[:2]


def _step(st, mode, step, words=None, amax=None, decay=DECAY, null_ema=NULL_EMA, omd_word=None):
    """One step through the C ABI.  ``mode``: "checked" | "ema" | "dev_ema" | "dev_ema_dev" (the decay read from the
    device word ``omd_word``; no weight decay, no record)."""
    from disentangle_mlp_amd import _lib
    from disentangle_mlp_amd._lib import check
    from disentangle_mlp_amd.optim import _AdamTensor
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n = len(st)
    arr = (_AdamTensor * n)()
    for i, s in enumerate(st):
        arr[i] = _AdamTensor(s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["p"].numel(),
                             None if amax is None else amax[i:i + 1].data_ptr())
    flags = None if words is None else (ctypes.c_void_p * n)(*[words.data_ptr() + 4 * i for i in range(n)])
    ema = (ctypes.c_void_p * n)(*[None if i in null_ema else s["e"].data_ptr() for i, s in enumerate(st)])
    bc1, bc2s = 1.0 - B1 ** step, (1.0 - B2 ** step) ** 0.5
    if mode == "checked":
        check(lib.vg_adam_step_checked(arr, n, LR, B1, B2, EPS, bc1, bc2s, flags, stream), "checked")
    elif mode == "ema":
        check(lib.vg_adam_step_ema(arr, n, LR, B1, B2, EPS, bc1, bc2s, flags, ema, decay, stream), "ema")
    elif mode == "dev_ema":
        buf, scal = _two_scalars()
        check(lib.vg_adam_prepare(float(step), None, 0, LR, B1, B2, scal.data_ptr(), stream), "vg_adam_prepare")
        check(lib.vg_adam_step_dev_ema(arr, n, B1, B2, EPS, scal.data_ptr(), flags, ema, decay, stream), "dev_ema")
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[2:]).all()) and bool(torch.isfinite(scal).all())
    elif mode == "dev_ema_dev":
        hyper = torch.tensor([LR, 0.0], dtype=torch.float64, device="cuda")
        scal = torch.zeros(4, device="cuda")
        check(lib.vg_adam_prepare_dev(float(step), None, 0, hyper.data_ptr(), 0, B1, B2, scal.data_ptr(), stream),
              "vg_adam_prepare_dev")
        check(lib.vg_adam_step_dev_ema_dev(arr, n, B1, B2, EPS, scal.data_ptr(), flags, ema, omd_word.data_ptr(), None,
                                           stream), "dev_ema_dev")
    else:
        raise ValueError(mode)
    torch.cuda.synchronize()


def _bound(k, seen):
    return k * 8 * 2.0 ** -24 * max(float(t) for t in seen)


def _lerp64(ref, p, decay):
    return ref + (1.0 - decay) * (p.double() - ref)


def _assert_follows(e, ref, k, seen, what):
    """EVERY element of ``e`` within the derived bound of the fp64 recurrence ``ref``."""
    err = float((e.double() - ref).abs().max())
    assert err <= _bound(k, seen), (what, err, _bound(k, seen))


def test_kernel_parity_per_element():
    assert len(set(SIZES)) == len(CYCLE) and NT > 24
    base = _state()
    a, b = _clone(base), _clone(base)
    wa, wb = (torch.full((NT,), 0x10, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    ref = [s["e"].double().clone() for s in base]
    seen = [[s["e"].abs().max(), s["p"].abs().max()] for s in base]
    gen = torch.Generator().manual_seed(1)
    for k in (1, 2, 3):
        _fresh_grads((a, b), gen)
        ama.zero_(), amb.zero_()
        _step(a, "ema", float(k), words=wa, amax=ama)
        _step(b, "checked", float(k), words=wb, amax=amb)
        # (a) the step itself is the checked step, bit for bit -- also where the EMA pointer alone forces the scalar loop
        for i, (x, y) in enumerate(zip(a, b)):
            for name in "pmv":
                assert torch.equal(_bits(x[name]), _bits(y[name])), (k, i, name)
        assert torch.equal(_bits(ama), _bits(amb)) and torch.equal(wa, wb) and wa.tolist() == [0x10] * NT
        assert all(float(ama[i]) == float(a[i]["p"].abs().max()) for i in range(NT))
        # (b) every EMA element against the fp64 lerp of the device's own fp32 p
        for i, s in enumerate(a):
            if i in NULL_EMA:
                continue
            ref[i] = _lerp64(ref[i], s["p"], DECAY)
            seen[i] += [s["p"].abs().max(), s["e"].abs().max()]
            _assert_follows(s["e"], ref[i], k, seen[i], (k, i))
        # (c) sentinels, and the buffers of tensors that are not averaged, bit-unchanged
        for i, (s, s0) in enumerate(zip(a, base)):
            n, lo = SIZES[i], PAD + s["shift"]
            if i in NULL_EMA:
                assert torch.equal(_bits(s["ebuf"]), _bits(s0["ebuf"])), (k, i)
            else:
                assert torch.equal(_bits(s["ebuf"][:lo]), _bits(s0["ebuf"][:lo])), (k, i)
                assert torch.equal(_bits(s["ebuf"][lo + n:]), _bits(s0["ebuf"][lo + n:])), (k, i)
                assert bool((s["ebuf"][:lo] == SENTINEL).all()) and bool((s["ebuf"][lo + n:] == SENTINEL).all())
    assert all(not torch.equal(a[i]["e"], base[i]["e"]) for i in range(NT) if i not in NULL_EMA)      # (it did average)
    # the checked step never touched an EMA buffer
    assert all(torch.equal(_bits(x["ebuf"]), _bits(y["ebuf"])) for x, y in zip(b, base))


def test_device_scalar_variant_gives_the_host_variants_bits():
    base = _state(2)
    a, b = _clone(base), _clone(base)
    wa, wb = (torch.zeros(NT, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    gen = torch.Generator().manual_seed(3)
    for k in (1, 2):
        _fresh_grads((a, b), gen)
        ama.zero_(), amb.zero_()
        _step(a, "ema", float(k), words=wa, amax=ama)
        _step(b, "dev_ema", float(k), words=wb, amax=amb)
        for i, (x, y) in enumerate(zip(a, b)):
            for name in ("p", "m", "v", "ebuf"):
                assert torch.equal(_bits(x[name]), _bits(y[name])), (k, i, name)
        assert torch.equal(_bits(ama), _bits(amb)) and torch.equal(wa, wb)
    # without flag words: the same bits
    c = _clone(base)
    gen = torch.Generator().manual_seed(3)
    for k in (1, 2):
        _fresh_grads((c,), gen)
        _step(c, "dev_ema", float(k))
    for i, (x, y) in enumerate(zip(a, c)):
        for name in ("p", "m", "v", "ebuf"):
            assert torch.equal(_bits(x[name]), _bits(y[name])), (i, name)


def test_nan_propagates_into_its_own_ema_alone():
    base = _state(4)
    gen = torch.Generator().manual_seed(5)
    _fresh_grads((base,), gen)
    t, el = 7, 2 * CHUNK + 5                                 # the scalar tail of the last chunk of a three-chunk tensor
    assert t not in NULL_EMA and el < SIZES[t]
    base[t]["g"][el] = float("nan")
    a, b = _clone(base), _clone(base)
    wa, wb = (torch.zeros(NT, dtype=torch.int32, device="cuda") for _ in range(2))
    _step(a, "ema", 1.0, words=wa)
    _step(b, "checked", 1.0, words=wb)
    want = [0] * NT
    want[t] = GRAD | PARAM
    assert wa.tolist() == want == wb.tolist()
    for i, s in enumerate(a):
        nan = torch.isnan(s["e"])
        if i == t:
            assert nan.nonzero().flatten().tolist() == [el] and bool(torch.isnan(s["p"][el]))
        else:
            assert not bool(nan.any()) and bool(torch.isfinite(s["e"]).all()), i
        for name in "pmv":
            assert torch.equal(_bits(s[name]), _bits(b[i][name])), (i, name)


def test_host_decay_that_rounds_to_one_still_lerps_and_only_the_device_word_follows():
    """Following the weights (e <- the bits of p) belongs to the DEVICE word 1.0f alone.  A host decay whose
    ``(float)(1 - decay)`` rounds to 1.0f keeps the lerp: e <- e + 1 * (p_new - e), which is fl(e + fl(p_new - e)) however
    the product and the sum are contracted -- and that is not p_new wherever p_new - e rounds."""
    decay = 1e-9
    assert 0.0 < decay < 1.0 and float(torch.tensor(1.0 - decay, dtype=torch.float64).float()) == 1.0
    base = _state(8)
    a, b, c = _clone(base), _clone(base), _clone(base)
    _fresh_grads((a, b, c), torch.Generator().manual_seed(9))
    _step(a, "ema", 1.0, decay=decay)
    _step(b, "checked", 1.0)
    differ = 0
    for i, (x, y, s0) in enumerate(zip(a, b, base)):
        for name in "pmv":
            assert torch.equal(_bits(x[name]), _bits(y[name])), (i, name)
        if i in NULL_EMA:
            assert torch.equal(_bits(x["ebuf"]), _bits(s0["ebuf"])), i
            continue
        want = s0["e"] + (x["p"] - s0["e"])                        # torch on the device: two fp32 roundings
        assert torch.equal(_bits(x["e"]), _bits(want)), i
        differ += int((_bits(want) != _bits(x["p"])).sum())
    assert differ > 0                                              # (the lerp and the copy are told apart)
    # the same inputs, the decay word 1.0f on the device: the average IS the new weights
    _step(c, "dev_ema_dev", 1.0, omd_word=torch.ones(1, device="cuda"))
    for i, (x, y, s0) in enumerate(zip(c, b, base)):
        for name in "pmv":
            assert torch.equal(_bits(x[name]), _bits(y[name])), (i, name)
        if i in NULL_EMA:
            assert torch.equal(_bits(x["ebuf"]), _bits(s0["ebuf"])), i
        else:
            assert torch.equal(_bits(x["e"]), _bits(x["p"])), i


@pytest.mark.parametrize("capturable", [False, True], ids=["host-scalars", "device-scalars"])
def test_hip_adam_ema(capturable):
    from disentangle_mlp_amd.optim import HipAdam
    base = _state(6)

    def make(st, **kw):
        ps = [torch.nn.Parameter(s["p"]) for s in st]
        for p, s in zip(ps, st):
            p.grad = s["g"]
        return ps, HipAdam(ps, lr=LR, capturable=capturable, nonfinite_guard=True, **kw)

    a, b = _clone(base), _clone(base)
    pa, oa = make(a, ema_decay=DECAY, ema_targets=[s["e"] for s in a])      # the caller's tensors, sentinels around them
    pb, ob = make(b)
    assert all(x.data_ptr() == s["e"].data_ptr() for x, s in zip(oa.ema_tensors(), a))
    ref = [s["e"].double().clone() for s in base]
    seen = [[s["e"].abs().max(), s["p"].abs().max()] for s in base]
    gen = torch.Generator().manual_seed(7)
    k = 0
    for it, update in enumerate((True, False, True, True)):
        _fresh_grads((a, b), gen)
        before = [s["ebuf"].clone() for s in a]
        oa.step(update_ema=update), ob.step()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(pa, pb)):                 # EMA on or off: the same training, bit for bit
            assert torch.equal(_bits(x.data), _bits(y.data)), (it, i)
            for name in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(oa.state[x][name]), _bits(ob.state[y][name])), (it, i, name)
        if not update:
            assert all(torch.equal(_bits(s["ebuf"]), _bits(q)) for s, q in zip(a, before))
            continue
        k += 1
        for i, s in enumerate(a):
            ref[i] = _lerp64(ref[i], pa[i].data, DECAY)
            seen[i] += [pa[i].data.abs().max(), s["e"].abs().max()]
            _assert_follows(s["e"], ref[i], k, seen[i], (it, i))
            n, lo = SIZES[i], PAD + s["shift"]
            assert bool((s["ebuf"][:lo] == SENTINEL).all()) and bool((s["ebuf"][lo + n:] == SENTINEL).all())
    assert oa.nonfinite() == {} and torch.equal(oa.nonfinite_words(), ob.nonfinite_words())
    # a parameter the step skips keeps its average; state access copies in place
    pa[3].grad = None
    e3, e4 = a[3]["e"].clone(), a[4]["e"].clone()
    oa.step()
    assert torch.equal(a[3]["e"], e3) and not torch.equal(a[4]["e"], e4)
    saved, ptrs = oa.ema_state(), [e.data_ptr() for e in oa.ema_tensors()]
    oa.reset_ema()
    assert all(torch.equal(e, p.data) for e, p in zip(oa.ema_tensors(), pa))
    oa.load_ema_state(saved)
    assert all(torch.equal(e, q) for e, q in zip(oa.ema_tensors(), saved))
    assert [e.data_ptr() for e in oa.ema_tensors()] == ptrs
    # without targets: fp32 clones of the parameters
    pc, oc = make(_clone(base), ema_decay=DECAY)
    assert all(torch.equal(e, p.data) and e.data_ptr() != p.data_ptr() for e, p in zip(oc.ema_tensors(), pc))
