"""GPU: clipping by global norm and skipping a non-finite step in front of / inside the fused Adam step.  Kernel level,
through the ctypes binding: the norm pass against an fp64 sum of squares, the coefficient, the clip step against the
kernels of the entry points that existed before (bit identity on ``g * coef`` formed by torch with the device's own
coefficient), the skip, the rejected arguments.  Optimizer level: a captured HipAdam step against the same eager steps.

Tolerance of the norm, derived, not measured: the squares are exact in fp64, a sum of n of them errs by at most
n * 2^-53 relative (n < 2^20 here: below 2^-33), the square root adds 2^-53, and the single rounding to fp32 at most
2^-24; the fp64 reference errs as little.  Together well inside 2^-23 relative.

inf / NaN are planted as DATA (written into a gradient); nothing here faults the device."""
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
PAD = 64                                     # sentinel floats on each side of every p, m, v and EMA buffer
SENTINEL = -12345.678
DECAY = 0.9
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
TOL = 2.0 ** -23


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lib():
    from disentangle_mlp_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ the norm pass
def _norm_pass(grads, max_norm, skip, rec=None, pad=8):
    """vg_grad_sumsq_multi + vg_grad_clip_finalize.  Returns (record buffer with sentinels, partials buffer with
    sentinels, slots); the record is buf[pad:pad + 4]."""
    from disentangle_mlp_amd._lib import check
    lib = _lib()
    n = len(grads)
    ptrs = (ctypes.c_void_p * n)(*[g.data_ptr() if g.numel() else None for g in grads])
    lens = (ctypes.c_size_t * n)(*[g.numel() for g in grads])
    slots = lib.vg_grad_sumsq_partials(lens, n)
    assert slots == sum((g.numel() + CHUNK - 1) // CHUNK for g in grads)
    part = torch.full((slots + 2 * pad,), -7.0, dtype=torch.float64, device="cuda")
    if rec is None:
        rec = torch.full((4 + 2 * pad,), SENTINEL, device="cuda")
        rec[pad:pad + 4] = 0.0
    check(lib.vg_grad_sumsq_multi(ptrs, lens, n, part[pad:].data_ptr(), slots, _stream()), "vg_grad_sumsq_multi")
    check(lib.vg_grad_clip_finalize(part[pad:].data_ptr(), slots, float(max_norm), int(skip), rec[pad:].data_ptr(),
                                    _stream()), "vg_grad_clip_finalize")
    torch.cuda.synchronize()
    assert bool((part[:pad] == -7.0).all()) and bool((part[pad + slots:] == -7.0).all())
    assert bool((rec[:pad] == SENTINEL).all()) and bool((rec[pad + 4:] == SENTINEL).all())
    return rec, part, slots


def _rec_fields(rec, pad=8):
    r = rec[pad:pad + 4]
    w = r.view(torch.int32).tolist()
    return float(r[0]), float(r[1]), w[2], w[3]


def _off_by_one(t):
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:].copy_(t)
    return buf[1:]


def _norm_zoo():
    gen = torch.Generator().manual_seed(20)
    lens = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 0]
    lens = lens + [CYCLE[i % len(CYCLE)] for i in range(26 - len(lens))]
    gs = []
    for i, n in enumerate(lens):
        g = torch.randn(n, generator=gen).cuda()
        gs.append(_off_by_one(g) if i in (4, 7) else g)          # two tensors one float off 16-byte alignment
    assert len(gs) == 26 and gs[4].data_ptr() % 16 == 4 and gs[7].data_ptr() % 16 == 4 and gs[8].numel() == 0
    return gs


def _norm64(gs):
    return float(torch.stack([(g.double() ** 2).sum() for g in gs]).sum().sqrt())


def test_norm_against_fp64_and_reproducible():
    gs = _norm_zoo()
    rec, part, slots = _norm_pass(gs, 0.0, 0)
    norm, coef, skip, skipped = _rec_fields(rec)
    want = _norm64(gs)
    print("norm", norm, "fp64", want, "rel", abs(norm - want) / want)
    assert abs(norm - want) <= TOL * want
    assert (coef, skip, skipped) == (1.0, 0, 0)                   # no max_norm: coefficient 1
    # every partial is its own chunk's sum of squares (the same derivation, per chunk)
    flat = torch.cat([torch.nn.functional.pad(g.double() ** 2, (0, -g.numel() % CHUNK)).view(-1, CHUNK).sum(1)
                      for g in gs if g.numel()])
    assert flat.numel() == slots
    assert bool(((part[8:8 + slots] - flat).abs() <= 2.0 ** -39 * flat).all())      # 8192 * 2^-53 on either side
    rec2, part2, _ = _norm_pass(gs, 0.0, 0)
    assert torch.equal(_bits(rec), _bits(rec2)) and torch.equal(part.view(torch.int64), part2.view(torch.int64))


def test_norm_over_forty_decades_neither_overflows_nor_vanishes():
    gen = torch.Generator().manual_seed(21)
    mags = [1e-20, 1e-12, 1e-3, 1.0, 1e6, 1e12, 1e19]
    gs = [(torch.randn(n, generator=gen) * s).cuda() for s, n in zip(mags, [5, CHUNK + 1, 3, 4, 2 * CHUNK + 7, 1, CHUNK - 1])]
    assert float(gs[-1].abs().max()) > 1.9e19                     # its fp32 square would be inf
    norm, coef, skip, _ = _rec_fields(_norm_pass(gs, 0.0, 1)[0])
    want = _norm64(gs)
    print("norm", norm, "fp64", want, "rel", abs(norm - want) / want)
    assert abs(norm - want) <= TOL * want and (coef, skip) == (1.0, 0)
    # the small end alone: far below fp32's smallest square
    norm, _, _, _ = _rec_fields(_norm_pass(gs[:1], 0.0, 1)[0])
    want = _norm64(gs[:1])
    assert want < 1e-19 and abs(norm - want) <= TOL * want
    # nothing at all: norm 0, coefficient 1
    assert _rec_fields(_norm_pass([torch.empty(0, device="cuda")], 1.0, 1)[0]) == (0.0, 1.0, 0, 0)


def test_coefficient():
    gs = _norm_zoo()
    want = _norm64(gs)
    norm, coef, skip, _ = _rec_fields(_norm_pass(gs, 2.0 * want, 0)[0])
    assert coef == 1.0 and skip == 0                              # below max_norm: exactly 1
    for max_norm in (1.0, 0.37 * want, 1e-3):
        norm, coef, skip, _ = _rec_fields(_norm_pass(gs, max_norm, 1)[0])
        ref = max_norm / (want + 1e-6)
        print("coef", coef, "fp64", ref, "rel", abs(coef - ref) / ref)
        assert coef < 1.0 and abs(coef - ref) <= TOL * ref and skip == 0
    # a non-finite norm: skip_nonfinite decides; without it the formula stands (torch: inf -> 0, NaN -> NaN)
    for poison, formula in ((float("inf"), 0.0), (float("nan"), float("nan"))):
        hs = [g.clone() for g in gs]
        hs[7][CHUNK + 3] = poison
        rec = _norm_pass(hs, 1.0, 1)[0]
        norm, coef, skip, skipped = _rec_fields(rec)
        assert norm != norm or norm == float("inf")
        assert (coef, skip, skipped) == (0.0, 1, 1)
        assert _rec_fields(_norm_pass(hs, 1.0, 1, rec=rec)[0])[2:] == (1, 2)      # the count only goes up ...
        assert _rec_fields(_norm_pass(gs, 1.0, 1, rec=rec)[0])[2:] == (0, 2)      # ... and stays in a clean pass
        norm, coef, skip, skipped = _rec_fields(_norm_pass(hs, 1.0, 0)[0])
        assert (skip, skipped) == (0, 0) and (coef == formula or (coef != coef and formula != formula))


# ------------------------------------------------------------------ the clip step
def _padded(vals, shift):
    n = vals.numel()
    buf = torch.full((n + 2 * PAD + 1,), SENTINEL, device="cuda")
    view = buf[PAD + shift:PAD + shift + n]
    view.copy_(vals)
    return buf, view


def _state(seed=0):
    """The tensor zoo of tests/test_adam_ema_gpu.py, with sentinels around p, m, v and the EMA."""
    gen = torch.Generator().manual_seed(seed)
    st = []
    for i, n in enumerate(SIZES):
        s1 = 1 if i in UNALIGNED else 0
        se = 1 if i in UNALIGNED or i == EMA_OFFSET else 0
        d = dict(shift=s1, eshift=se)
        d["pbuf"], d["p"] = _padded(torch.randn(n, generator=gen), s1)
        d["gbuf"], d["g"] = _padded(torch.zeros(n), s1)
        d["mbuf"], d["m"] = _padded(torch.randn(n, generator=gen) * 0.01, s1)
        d["vbuf"], d["v"] = _padded(torch.rand(n, generator=gen) * 1e-3, s1)
        d["ebuf"], d["e"] = _padded(torch.randn(n, generator=gen), se)
        st.append(d)
    for i in UNALIGNED:
        assert all(st[i][k].data_ptr() % 16 == 4 for k in "pgmve")
    assert all(st[EMA_OFFSET][k].data_ptr() % 16 == 0 for k in "pgmv") and st[EMA_OFFSET]["e"].data_ptr() % 16 == 4
    assert all(st[i][k].data_ptr() % 16 == 0 for i in range(NT) if i not in UNALIGNED + (EMA_OFFSET,) for k in "pgmve")
    return st


def _clone(st):
    out = []
    for s in st:
        d = dict(shift=s["shift"], eshift=s["eshift"])
        n = s["p"].numel()
        for k in "pgmve":
            sh = s["eshift"] if k == "e" else s["shift"]
            d[k + "buf"] = s[k + "buf"].clone()
            d[k] = d[k + "buf"][PAD + sh:PAD + sh + n]
        out.append(d)
    return out


def _fresh_grads(sts, gen, scale):
    for i, n in enumerate(SIZES):
        g = (torch.randn(n, generator=gen) * scale).cuda()
        for st in sts:
            st[i]["g"].copy_(g)


def _same(a, b, what, names=("pbuf", "mbuf", "vbuf", "ebuf")):
    for i, (x, y) in enumerate(zip(a, b)):
        for name in names:
            assert torch.equal(_bits(x[name]), _bits(y[name])), (what, i, name)


def _sentinels_intact(st):
    for i, s in enumerate(st):
        n = SIZES[i]
        for k in "pmve":
            lo = PAD + (s["eshift"] if k == "e" else s["shift"])
            buf = s[k + "buf"]
            assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all()), (i, k)


def _step(st, mode, step, words, amax, rec=None, ema_on=True, grads=None):
    """One step through the C ABI.  ``mode``: "clip" | "dev_clip" (the code under test, reading the record ``rec``) or
    "checked" | "dev_checked" | "ema" | "dev_ema" (the yardstick: the entry points that existed before)."""
    from disentangle_mlp_amd._lib import check
    from disentangle_mlp_amd.optim import _AdamTensor
    lib, stream, n = _lib(), _stream(), len(st)
    arr = (_AdamTensor * n)()
    for i, s in enumerate(st):
        g = s["g"] if grads is None else grads[i]
        arr[i] = _AdamTensor(s["p"].data_ptr(), g.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["p"].numel(),
                             amax[i:i + 1].data_ptr())
    flags = (ctypes.c_void_p * n)(*[words.data_ptr() + 4 * i for i in range(n)])
    ema = None
    if ema_on:
        ema = (ctypes.c_void_p * n)(*[None if i in NULL_EMA else s["e"].data_ptr() for i, s in enumerate(st)])
    bc1, bc2s = 1.0 - B1 ** step, (1.0 - B2 ** step) ** 0.5
    # two scalars in front of two NaN words: the entry points paired with vg_adam_prepare own scalars[0..1] alone -- had
    # one read scalars[2..3] (the decay words of vg_adam_prepare_dev), no bit comparison against the host-scalar variants
    # would hold
    scal = torch.full((4,), float("nan"), device="cuda")[:2]
    if mode.startswith("dev"):
        check(lib.vg_adam_prepare(float(step), None, 0, LR, B1, B2, scal.data_ptr(), stream), "vg_adam_prepare")
    if mode == "clip":
        check(lib.vg_adam_step_clip(arr, n, LR, B1, B2, EPS, bc1, bc2s, flags, ema, DECAY, rec.data_ptr(), stream), mode)
    elif mode == "dev_clip":
        check(lib.vg_adam_step_dev_clip(arr, n, B1, B2, EPS, scal.data_ptr(), flags, ema, DECAY, rec.data_ptr(), stream), mode)
    elif mode == "checked":
        check(lib.vg_adam_step_checked(arr, n, LR, B1, B2, EPS, bc1, bc2s, flags, stream), mode)
    elif mode == "dev_checked":
        check(lib.vg_adam_step_dev_checked(arr, n, B1, B2, EPS, scal.data_ptr(), flags, stream), mode)
    elif mode == "ema":
        check(lib.vg_adam_step_ema(arr, n, LR, B1, B2, EPS, bc1, bc2s, flags, ema, DECAY, stream), mode)
    elif mode == "dev_ema":
        check(lib.vg_adam_step_dev_ema(arr, n, B1, B2, EPS, scal.data_ptr(), flags, ema, DECAY, stream), mode)
    else:
        raise ValueError(mode)
    torch.cuda.synchronize()


def _record_for(st, max_norm, skip, rec=None):
    rec = _norm_pass([s["g"] for s in st], max_norm, skip, rec=rec)[0]
    return rec, rec[8:12]


@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-scalars"])
@pytest.mark.parametrize("ema_on", [True, False], ids=["ema", "no-ema"])
@pytest.mark.parametrize("active", [True, False], ids=["clipped", "coef-1"])
def test_clip_step_is_the_parents_step_on_the_scaled_gradient(dev, ema_on, active):
    assert len(set(SIZES)) == len(CYCLE) and NT > 24
    base = _state()
    a, b = _clone(base), _clone(base)
    wa, wb = (torch.full((NT,), 0x10, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    gen = torch.Generator().manual_seed(1)
    yard = ("dev_" if dev else "") + ("ema" if ema_on else "checked")
    for k in (1, 2, 3):
        _fresh_grads((a, b), gen, 0.1)
        _, rec = _record_for(a, 1.0 if active else 1e6, 1)
        coef = rec[1:2].clone()                                  # the device's own word
        assert (float(coef) < 1.0) if active else (float(coef) == 1.0)
        # the yardstick: torch scales (unclipped: the untouched gradients), the parent's kernel steps
        scaled = [s["g"] * coef for s in b] if active else None
        ama.zero_(), amb.zero_()
        _step(a, "dev_clip" if dev else "clip", float(k), wa, ama, rec=rec, ema_on=ema_on)
        _step(b, yard, float(k), wb, amb, grads=scaled)
        _same(a, b, (k, yard))
        assert torch.equal(_bits(ama), _bits(amb)) and torch.equal(wa, wb) and wa.tolist() == [0x10] * NT
        assert all(float(ama[i]) == float(a[i]["p"].abs().max()) for i in range(NT))
        _same(a, b, k, names=("gbuf",))                           # the gradients are only read
        _sentinels_intact(a)
    moved = [i for i in range(NT) if not torch.equal(a[i]["e"], base[i]["e"])]
    assert moved == ([i for i in range(NT) if i not in NULL_EMA] if ema_on else [])
    assert all(not torch.equal(a[i]["p"], base[i]["p"]) for i in range(NT))


SKIP_SPOTS = [(7, 0, "first"), (4, CHUNK - 2, "last"), (7, 2 * CHUNK + 5, "tail"), (6, 3, "unaligned")]


@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("t,el,where", SKIP_SPOTS, ids=[s[2] for s in SKIP_SPOTS])
def test_skip_stores_nothing_and_the_next_step_is_the_plain_step(poison, t, el, where):
    assert el < SIZES[t] and (where != "last" or el == SIZES[t] - 1) and (where != "tail" or el >= (SIZES[t] & ~3))
    base = _state(4)
    gen = torch.Generator().manual_seed(5)
    a, b = _clone(base), _clone(base)
    wa, wb = (torch.zeros(NT, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    _fresh_grads((a, b), gen, 0.1)
    a[t]["g"][el] = poison
    full, rec = _record_for(a, 1.0, 1)
    assert rec.view(torch.int32)[2:].tolist() == [1, 1]
    _step(a, "clip", 1.0, wa, ama, rec=rec)
    _same(a, base, "skipped")                                     # p, m, v, e of every tensor, sentinels included
    _sentinels_intact(a)
    assert all(float(ama[i]) == float(base[i]["p"].abs().max()) for i in range(NT))
    assert wa.tolist() == [GRAD if i == t else 0 for i in range(NT)]
    # the device-scalar variant skips alike
    c = _clone(base)
    c[t]["g"].copy_(a[t]["g"])
    wc, amc = torch.zeros(NT, dtype=torch.int32, device="cuda"), torch.zeros(NT, device="cuda")
    _step(c, "dev_clip", 1.0, wc, amc, rec=rec)
    _same(c, base, "skipped-dev")
    assert torch.equal(wc, wa) and torch.equal(_bits(amc), _bits(ama))
    # the following clean step: the plain (EMA) step at the advanced count, on the scaled gradient
    wa.zero_()
    _fresh_grads((a, b), gen, 0.1)
    full, rec = _record_for(a, 1.0, 1, rec=full)
    assert rec.view(torch.int32)[2:].tolist() == [0, 1]           # the count stays
    coef = rec[1:2].clone()
    ama.zero_(), amb.zero_()
    _step(a, "clip", 2.0, wa, ama, rec=rec)
    _step(b, "ema", 2.0, wb, amb, grads=[s["g"] * coef for s in b])
    _same(a, b, "after")
    assert torch.equal(_bits(ama), _bits(amb)) and wa.tolist() == wb.tolist() == [0] * NT


def test_without_skip_the_poison_goes_through_as_in_torch():
    base = _state(6)
    gen = torch.Generator().manual_seed(7)
    a, b = _clone(base), _clone(base)
    _fresh_grads((a, b), gen, 0.1)
    t, el = 7, 2 * CHUNK + 5
    a[t]["g"][el] = b[t]["g"][el] = float("inf")
    wa, wb = (torch.zeros(NT, dtype=torch.int32, device="cuda") for _ in range(2))
    ama, amb = torch.zeros(NT, device="cuda"), torch.zeros(NT, device="cuda")
    _, rec = _record_for(a, 1.0, 0)
    coef = rec[1:2].clone()
    assert float(coef) == 0.0 and rec.view(torch.int32)[2:].tolist() == [0, 0]      # max_norm / inf; nothing skipped
    _step(a, "clip", 1.0, wa, ama, rec=rec)
    _step(b, "ema", 1.0, wb, amb, grads=[s["g"] * coef for s in b])                 # torch: 0 * inf = NaN
    _same(a, b, "poisoned")
    assert wa.tolist() == wb.tolist() == [GRAD | PARAM if i == t else 0 for i in range(NT)]
    assert bool(torch.isnan(a[t]["p"][el])) and int(torch.isnan(a[t]["p"]).sum()) == 1


def test_bad_arguments_launch_nothing():
    from disentangle_mlp_amd.optim import _AdamTensor
    lib, stream = _lib(), _stream()
    base = _state(8)
    a = _clone(base)
    _fresh_grads((a,), torch.Generator().manual_seed(9), 0.1)
    n = NT
    ptrs = (ctypes.c_void_p * n)(*[s["g"].data_ptr() for s in a])
    lens = (ctypes.c_size_t * n)(*[s["g"].numel() for s in a])
    slots = lib.vg_grad_sumsq_partials(lens, n)
    part = torch.full((slots + 16,), -7.0, dtype=torch.float64, device="cuda")
    rec = torch.full((20,), SENTINEL, device="cuda")
    assert lib.vg_grad_sumsq_multi(ptrs, lens, n, None, slots, stream) == -1
    assert lib.vg_grad_sumsq_multi(ptrs, lens, n, part[8:].data_ptr(), slots - 1, stream) == -1
    assert lib.vg_grad_clip_finalize(None, slots, 1.0, 1, rec[8:].data_ptr(), stream) == -1
    assert lib.vg_grad_clip_finalize(part[8:].data_ptr(), slots, 1.0, 1, None, stream) == -1
    assert lib.vg_grad_clip_finalize(part[8:].data_ptr(), slots, float("nan"), 1, rec[8:].data_ptr(), stream) == -1
    arr = (_AdamTensor * n)()
    for i, s in enumerate(a):
        arr[i] = _AdamTensor(s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["p"].numel(), None)
    ema = (ctypes.c_void_p * n)(*[s["e"].data_ptr() for s in a])
    scal = torch.ones(2, device="cuda")
    bc1, bc2s = 1.0 - B1, (1.0 - B2) ** 0.5
    r = rec[8:].data_ptr()
    assert lib.vg_adam_step_clip(arr, n, LR, B1, B2, EPS, bc1, bc2s, None, ema, DECAY, None, stream) == -1
    assert lib.vg_adam_step_dev_clip(arr, n, B1, B2, EPS, scal.data_ptr(), None, ema, DECAY, None, stream) == -1
    for decay in (0.0, 1.0, -0.5, float("nan")):
        assert lib.vg_adam_step_clip(arr, n, LR, B1, B2, EPS, bc1, bc2s, None, ema, decay, r, stream) == -1
        assert lib.vg_adam_step_dev_clip(arr, n, B1, B2, EPS, scal.data_ptr(), None, ema, decay, r, stream) == -1
    torch.cuda.synchronize()
    assert bool((part == -7.0).all()) and bool((rec == SENTINEL).all())      # no kernel ran
    _same(a, base, "refused")


# ------------------------------------------------------------------ optimizer level
def _make_opt(st, **kw):
    from disentangle_mlp_amd.optim import HipAdam
    ps = [torch.nn.Parameter(s["p"]) for s in st]
    for p, s in zip(ps, st):
        p.grad = s["g"]
    return ps, HipAdam(ps, lr=LR, nonfinite_guard=True, ema_decay=DECAY, ema_targets=[s["e"] for s in st], **kw)


def _same_opt(a, pa, oa, b, pb, ob, what):
    """p and the EMA with their sentinels; the optimizers' own moment tensors."""
    _same(a, b, what, names=("pbuf", "ebuf"))
    for i, (x, y) in enumerate(zip(pa, pb)):
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(oa.state[x][name]), _bits(ob.state[y][name])), (what, i, name)


def test_captured_step_is_the_eager_step():
    base = _state(10)
    gen = torch.Generator().manual_seed(11)
    plan = []                                                    # clipped, unclipped, one with an inf
    for scale, poison in ((0.1, False), (1e-5, False), (0.1, True), (0.1, False)):
        gs = [(torch.randn(n, generator=gen) * scale).cuda() for n in SIZES]
        if poison:
            gs[4][CHUNK - 2] = float("inf")
        plan.append(gs)
    a, b = _clone(base), _clone(base)
    pa, oa = _make_opt(a, capturable=True, max_grad_norm=1.0, skip_nonfinite=True)
    pb, ob = _make_opt(b, capturable=True, max_grad_norm=1.0, skip_nonfinite=True)

    def load(st, gs):
        for s, g in zip(st, gs):
            s["g"].copy_(g)

    load(a, plan[0]), load(b, plan[0])
    oa.step(), ob.step()                                         # one eager step each: the state exists
    oa.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    load(a, plan[1])
    with torch.cuda.graph(graph):
        oa.step()
    coefs = []
    for it, gs in enumerate(plan[1:]):
        load(a, gs), load(b, gs)
        graph.replay()
        if it:
            oa.replayed()
        ob.step()
        torch.cuda.synchronize()
        _same_opt(a, pa, oa, b, pb, ob, ("replay", it))
        assert torch.equal(oa.clip_record(), ob.clip_record()), it
        coefs.append(float(oa.clip_coef()))
    assert coefs[0] == 1.0 and coefs[1] == 0.0 and 0.0 < coefs[2] < 1.0
    assert oa.skipped_steps() == ob.skipped_steps() == 1
    _sentinels_intact(a)
    assert torch.equal(oa.nonfinite_words(), ob.nonfinite_words())
    assert {p: v for p, v in oa.nonfinite().items()} == {pa[4]: GRAD}
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert all(float(sa[i]["step"]) == float(sb[i]["step"]) == 4.0 for i in range(NT))      # the skipped step counted


def test_hip_adam_clip_is_hip_adam_on_scaled_gradients_and_composes_with_update_ema():
    base = _state(12)
    gen = torch.Generator().manual_seed(13)
    a, b = _clone(base), _clone(base)
    pa, oa = _make_opt(a, max_grad_norm=1.0)
    pb, ob = _make_opt(b)
    for it, update in enumerate((True, False, True)):
        _fresh_grads((a, b), gen, 0.1)
        oa.step(update_ema=update)
        coef = oa.clip_coef().clone().reshape(1)
        assert 0.0 < float(coef) < 1.0
        want = _norm64([s["g"] for s in a])
        assert abs(float(oa.grad_norm()) - want) <= TOL * want
        for p, s in zip(pb, b):
            p.grad = s["g"] * coef
        ob.step(update_ema=update)
        torch.cuda.synchronize()
        _same_opt(a, pa, oa, b, pb, ob, it)
    # a parameter without a gradient does not count
    pa[3].grad = None
    oa.step()
    want = _norm64([s["g"] for i, s in enumerate(a) if i != 3])
    assert abs(float(oa.grad_norm()) - want) <= TOL * want
