"""GPU: the non-finite guard.  Kernel level -- vg_adam_step_checked / vg_adam_step_dev_checked through the ctypes
binding and through optim.HipAdam(nonfinite_guard=True): which word comes up for which planted inf / NaN, that the
words are sticky and only ever ORed, and that p, m, v and the emitted bound are the unchecked step's bits.  Iteration
level -- a guarded trainer notices one inf pixel under graph replay and eagerly, `check_finite` names parameters of
every network, a checkpoint loaded in place brings the run back bit for bit, and the guard changes no result.

Non-finite values are planted as DATA (an inf written into a tensor); nothing here faults the device."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD, PARAM = 1, 2
CHUNK = 8192
# 30 tensors: two launches of 24.  1, 3: smaller than a vector / a wavefront; 8191, 8192, 8193: around one workgroup's chunk;
# 4 * 8192 + 5: five chunks, a ragged last one; tensor 6 is viewed at a one-element offset (the unaligned path)
SIZES = [1, 3, 8191, 8192, 8193, 4 * CHUNK + 5, 10007] + [257 + 613 * i for i in range(17)] + \
        [5, 2 * CHUNK + 3, 4099, 64, CHUNK, 777]
UNALIGNED = 6
PLANTS = {                                   # name -> (tensor, element)
    "first element": (5, 0),
    "last element of a vector body": (2, 8187),          # n = 8191: vectors cover [0, 8188)
    "scalar tail": (2, 8190),
    "last chunk": (5, 4 * CHUNK + 1),
    "tail of the last chunk": (5, 4 * CHUNK + 4),
    "second launch": (25, 2 * CHUNK - 1),
    "unaligned tensor": (UNALIGNED, 5000),
    "one-element tensor": (0, 0),
    "three-element tensor": (1, 2),
}
KINDS = {                                    # name -> (tensor planted in, value, expected word)
    "nan in g": ("g", float("nan"), GRAD | PARAM),       # m, then p = p - s * m / denom, turn NaN
    "inf in g": ("g", float("inf"), GRAD | PARAM),       # m = inf, v = inf: m / denom = inf / inf = NaN
    "-inf in g": ("g", float("-inf"), GRAD | PARAM),
    "p already inf": ("p", float("inf"), PARAM),         # finite g: p = inf - finite = inf, nothing non-finite was READ
}


def _state(seed=0):
    """p, g, m, v of the 30 tensors (a few steps in: m, v non-trivial), tensor `UNALIGNED`'s p one element off 16 bytes."""
    assert len(SIZES) == 30
    gen = torch.Generator().manual_seed(seed)
    st = []
    for i, n in enumerate(SIZES):
        p = torch.randn(n + 1, generator=gen).cuda()
        p = p[1:] if i == UNALIGNED else p[:n].clone()
        g = (torch.randn(n, generator=gen) * 0.1).cuda()
        m = (torch.randn(n, generator=gen) * 0.01).cuda()
        v = (torch.rand(n, generator=gen) * 1e-3).cuda()
        st.append([p, g, m, v])
    assert st[UNALIGNED][0].data_ptr() % 16 == 4 and st[0][0].data_ptr() % 16 == 0
    return st


def _clone(st):
    out = []
    for i, (p, g, m, v) in enumerate(st):
        if i == UNALIGNED:                   # keep the one-element offset
            buf = torch.empty(p.numel() + 1, device="cuda")
            buf[1:].copy_(p)
            p2 = buf[1:]
        else:
            p2 = p.clone()
        out.append([p2, g.clone(), m.clone(), v.clone()])
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lib_step(st, checked, dev_scalars, words=None, amax=None, step=3.0, null_flags=()):
    """One step through the C ABI.  ``words``: int32 device tensor, one per tensor (``null_flags``: entries passed as
    NULL); ``amax``: fp32 device tensor, one per tensor."""
    from disentangle_mlp_amd import _lib
    from disentangle_mlp_amd._lib import check
    from disentangle_mlp_amd.optim import _AdamTensor
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n = len(st)
    arr = (_AdamTensor * n)()
    for i, (p, g, m, v) in enumerate(st):
        arr[i] = _AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                             None if amax is None else amax[i:i + 1].data_ptr())
    flags = None
    if words is not None:
        flags = (ctypes.c_void_p * n)(*[None if i in null_flags else words.data_ptr() + 4 * i for i in range(n)])
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    if dev_scalars:
        scal = torch.zeros(2, device="cuda")
        check(lib.vg_adam_prepare(step, None, 0, lr, b1, b2, scal.data_ptr(), stream), "vg_adam_prepare")
        if checked:
            check(lib.vg_adam_step_dev_checked(arr, n, b1, b2, eps, scal.data_ptr(), flags, stream), "dev_checked")
        else:
            check(lib.vg_adam_step_dev(arr, n, b1, b2, eps, scal.data_ptr(), stream), "dev")
    else:
        bc1, bc2s = 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5
        if checked:
            check(lib.vg_adam_step_checked(arr, n, lr, b1, b2, eps, bc1, bc2s, flags, stream), "checked")
        else:
            check(lib.vg_adam_step(arr, n, lr, b1, b2, eps, bc1, bc2s, stream), "unchecked")
    torch.cuda.synchronize()


def _plant(st, kind, where):
    which, value, word = KINDS[kind]
    t, e = PLANTS[where]
    assert e < SIZES[t]
    st[t][{"p": 0, "g": 1}[which]][e] = value
    return t, word


def _same_bits(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        for j, name in enumerate(("p", "g", "m", "v")):
            assert torch.equal(_bits(x[j]), _bits(y[j])), (i, name)


@pytest.mark.parametrize("dev_scalars", [False, True], ids=["host-scalars", "device-scalars"])
def test_clean_step_leaves_every_word_alone_and_equals_the_unchecked_step(dev_scalars):
    base = _state()
    a, b = _clone(base), _clone(base)
    words = torch.full((30,), 0x10, dtype=torch.int32, device="cuda")      # the step only ever ORs
    am_a, am_b = torch.zeros(30, device="cuda"), torch.zeros(30, device="cuda")
    _lib_step(a, True, dev_scalars, words=words, amax=am_a)
    _lib_step(b, False, dev_scalars, amax=am_b)
    assert words.tolist() == [0x10] * 30
    _same_bits(a, b)
    assert torch.equal(_bits(am_a), _bits(am_b))
    assert all(float(am_a[i]) == float(a[i][0].abs().max()) for i in range(30))
    assert not torch.equal(a[0][0], base[0][0])                               # (it did step)
    # an independent reference for every code path (vectors, scalar tail, unaligned): the step in float64 from the fp32
    # scalars the kernel uses.  Each of p, m, v comes out of fewer than ten fp32 roundings (2^-24 relative each, on
    # operands no larger than the result's own scale here): 1e-5 relative leaves two orders of room and still sees any
    # element that was skipped, stepped twice or stepped with a neighbour's gradient.  Where a difference cancels (p0 next
    # to its update of at most ~5e-3, m0 next to its increment) the error is absolute: for m half an ulp of g - m0 (<= 0.6:
    # 3e-8) times 0.1 plus two roundings at the scale of the terms (<= 0.06: 2e-9 each), under 1e-8; for p half an ulp of
    # 5e-3 plus the update's relative error (5e-7 of 5e-3), under 1e-8
    lr, b1, b2, eps, step = 1e-3, 0.9, 0.999, 1e-8, 3.0
    omb1, omb2 = float(torch.tensor(1.0 - b1, dtype=torch.float32)), float(torch.tensor(1.0 - b2, dtype=torch.float32))
    b2f = float(torch.tensor(b2, dtype=torch.float32))
    ssz = float(torch.tensor(lr / (1.0 - b1 ** step), dtype=torch.float32))
    bc2s = float(torch.tensor((1.0 - b2 ** step) ** 0.5, dtype=torch.float32))
    epsf = float(torch.tensor(eps, dtype=torch.float32))
    for i, ((p0, g0, m0, v0), (p1, _, m1, v1)) in enumerate(zip(base, a)):
        p0, g0, m0, v0 = (t.double() for t in (p0, g0, m0, v0))
        m = m0 + omb1 * (g0 - m0)
        v = b2f * v0 + omb2 * g0 * g0
        p = p0 - ssz * (m / (v.sqrt() / bc2s + epsf))
        for name, want, got, atol in (("p", p, p1, 1e-8), ("m", m, m1, 1e-8), ("v", v, v1, 0.0)):
            assert torch.allclose(got.double(), want, rtol=1e-5, atol=atol), (i, name)
    # a NULL array and NULL entries: the same step
    c, d = _clone(base), _clone(base)
    _lib_step(c, True, dev_scalars, words=None)
    _lib_step(d, True, dev_scalars, words=words, null_flags=range(30))
    _same_bits(a, c)
    _same_bits(a, d)
    assert words.tolist() == [0x10] * 30


@pytest.mark.parametrize("dev_scalars", [False, True], ids=["host-scalars", "device-scalars"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_planted_element_raises_its_tensors_word_alone(kind, dev_scalars):
    base = _state(1)
    for where in PLANTS:
        a = _clone(base)
        t, word = _plant(a, kind, where)
        b = _clone(a)
        words = torch.zeros(30, dtype=torch.int32, device="cuda")
        am_a, am_b = torch.zeros(30, device="cuda"), torch.zeros(30, device="cuda")
        _lib_step(a, True, dev_scalars, words=words, amax=am_a)
        _lib_step(b, False, dev_scalars, amax=am_b)
        want = [0] * 30
        want[t] = word
        assert words.tolist() == want, (kind, where)
        _same_bits(a, b)                                     # the planted step too is the unchecked one, bit for bit
        assert torch.equal(_bits(am_a), _bits(am_b)), (kind, where)
        # detected, not skipped: the poisoned element was written
        assert not bool(torch.isfinite(a[t][0][PLANTS[where][1]]))
        # sticky across a clean step (of fresh, finite tensors on the same words); a NULL entry is not written
        c = _clone(base)
        _lib_step(c, True, dev_scalars, words=words)
        assert words.tolist() == want, (kind, where)
        words.zero_()
        d = _clone(base)
        _plant(d, kind, where)
        _lib_step(d, True, dev_scalars, words=words, null_flags=(t,))
        assert words.tolist() == [0] * 30, (kind, where)


def test_empty_tensors_are_skipped_and_their_words_untouched():
    base = _state(2)[:4]
    base.insert(2, [torch.empty(0, device="cuda") for _ in range(4)])
    base[3][1][7] = float("nan")
    words = torch.full((5,), 0x20, dtype=torch.int32, device="cuda")
    _lib_step(base, True, False, words=words)
    assert words.tolist() == [0x20, 0x20, 0x20, 0x20 | GRAD | PARAM, 0x20]


@pytest.mark.parametrize("capturable", [False, True], ids=["host-scalars", "device-scalars"])
def test_hip_adam_guard(capturable):
    from disentangle_mlp_amd.optim import HipAdam
    base = _state(3)

    def make(guard, st):
        ps = [torch.nn.Parameter(x[0]) for x in st]
        assert ps[UNALIGNED].data_ptr() % 16 == 4
        for p, x in zip(ps, st):
            p.grad = x[1]
        return ps, HipAdam(ps, lr=1e-3, capturable=capturable, nonfinite_guard=guard)

    pa, oa = make(True, _clone(base))
    pb, ob = make(False, _clone(base))
    words = oa.nonfinite_words()
    assert words.dtype == torch.int32 and words.shape == (30,) and words.is_cuda
    for _ in range(2):
        oa.step(), ob.step()
    assert oa.nonfinite() == {} and words.tolist() == [0] * 30

    def same():
        for x, y in zip(pa, pb):
            assert torch.equal(_bits(x.data), _bits(y.data))
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(oa.state[x][k]), _bits(ob.state[y][k]))
    same()
    for t, e, value, want in ((25, 2 * CHUNK - 1, float("nan"), GRAD | PARAM), (2, 8190, float("inf"), GRAD | PARAM)):
        pa[t].grad[e] = value
        pb[t].grad[e] = value
        oa.step(), ob.step()
        got = oa.nonfinite()
        assert len(got) == 1 and next(iter(got)) is pa[t] and got[pa[t]] == want
        same()
        # sticky: the gradient is finite again, the parameter is not -- its word keeps the gradient bit
        pa[t].grad[e] = 0.0
        pb[t].grad[e] = 0.0
        oa.step(), ob.step()
        assert oa.nonfinite_words() is words and words.tolist()[t] == want
        with torch.no_grad():                  # heal the parameter and the moments by hand, clear: clean again
            for ps, o in ((pa, oa), (pb, ob)):
                ps[t].data[e] = 0.5
                o.state[ps[t]]["exp_avg"][e] = 0.0
                o.state[ps[t]]["exp_avg_sq"][e] = 0.0
        oa.clear_nonfinite()
        assert words.tolist() == [0] * 30
        oa.step(), ob.step()
        assert oa.nonfinite() == {}
        same()
    # a parameter that is already inf under a finite gradient: PARAM only
    with torch.no_grad():
        pa[5].data[0] = float("inf")
    oa.step()
    assert {id(k): v for k, v in oa.nonfinite().items()} == {id(pa[5]): PARAM}
    oa.load_state_dict(oa.state_dict())
    assert oa.nonfinite_words() is words       # never replaced: a captured step writes there


# ---------------------------------------------------------------------------------------------- iteration level
def _batch(b=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(b, 3, 64, 64, generator=g) * 2 - 1).cuda()
    lat = [torch.randn(b, 128, generator=g).cuda() for _ in range(3)]
    return x, lat


def _weights(tr):
    sd = {}
    for a, net, opt in tr._guarded_optimizers():
        sd.update({f"{a}.{k}": v.detach().clone() for k, v in net.state_dict().items()})
        for i, st in opt.state_dict()["state"].items():      # (state_dict: the host's step counts follow the replays)
            sd.update({f"{a}.opt{i}.{k}": v.detach().clone() for k, v in st.items()})
    return sd


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert torch.equal(x, y) if not x.is_floating_point() else torch.equal(_bits(x.float()), _bits(y.float())), k


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_betavaegan_notices_an_inf_pixel_and_recovers_from_a_checkpoint(graph):
    from disentangle_mlp_amd import trainer as T
    from disentangle_mlp_amd.optim import HipAdam
    x, lat = _batch()
    steps = 4                                                # two eager warm-up iterations, the capture, one more replay
    tr = T.BetaVAEGANTrainer(beta=25.0, graph=graph)         # the default: guarded
    un = T.BetaVAEGANTrainer(beta=25.0, graph=graph, nonfinite_guard=False)
    assert tr.nonfinite_guard and isinstance(tr.optimizerD, HipAdam) and tr.optimizerD.nonfinite_guard
    assert tr.optimizerEG.nonfinite_guard and not un.nonfinite_guard and not un.optimizerD.nonfinite_guard
    for _ in range(steps):
        tr.step(x, *lat)
        un.step(x, *lat)
    if graph:
        assert len(tr._graphs) == 1 and tr.graph and len(un._graphs) == 1            # replaying, no fallback
        cap = next(iter(tr._graphs.values()))
    else:
        assert not tr._graphs
    assert tr.check_finite() is None
    assert tr.iteration == steps
    _assert_same(_weights(tr), _weights(un))                 # the guard changes no result
    ck = copy.deepcopy(tr.checkpoint(1))
    ref = {k: v.clone() for k, v in un.step(x, *lat).items()}          # the clean next step, in the unpoisoned trainer
    ref_w = _weights(un)
    # one inf pixel, one more step
    bad = x.clone()
    bad[3, 1, 17, 40] = float("inf")
    tr.step(bad, *lat)
    with pytest.raises(T.NonFiniteError) as e:
        tr.check_finite()
    nets = {n.split(".")[0] for n, _ in e.value.found}
    assert nets == {"netEG", "netD"}
    assert all(k in ("grad", "param", "grad+param") for _, k in e.value.found)
    named = {f"{a}.{k}" for a, net, _ in tr._guarded_optimizers() for k, _ in net.named_parameters()}
    assert {n for n, _ in e.value.found} <= named
    assert (e.value.first_iteration, e.value.last_iteration) == (steps, steps + 1)
    with pytest.raises(T.NonFiniteError):                    # sticky until the state is restored
        tr.check_finite()
    # back to the checkpoint, in place: the same capture replays, clean, with the unpoisoned trainer's bits
    tr.load_in_place(ck)
    out = {k: v.clone() for k, v in tr.step(x, *lat).items()}
    assert tr.check_finite() is None
    if graph:
        assert len(tr._graphs) == 1 and next(iter(tr._graphs.values())) is cap
    for k in ref:
        assert torch.equal(_bits(out[k].float()), _bits(ref[k].float())), k
    _assert_same(_weights(tr), ref_w)


def test_load_in_place_rewrites_the_pack_buffers_the_captured_graph_reads():
    """The captured phase 1 reads the discriminator's packs from buffers whose addresses the graph holds; `load_in_place`
    re-packs them from the recorded plan.  70 other filters packed in between (another trainer, a test's throw-away
    weights) must not make it write anywhere else: a pack buffer belongs to its weight object for life.  The step on
    another batch before the load is what makes stale buffers visible -- without it they hold the checkpoint's packs.
    With the address-keyed cache this replaced, more than 64 entries made the next scope clear the cache, so that the load
    packed into new buffers while the replay read the old ones: so the code read; that failure was never run."""
    from disentangle_mlp_amd import ops
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    tr, twin = T.BetaVAEGANTrainer(beta=25.0, graph=True), T.BetaVAEGANTrainer(beta=25.0, graph=True)
    for _ in range(4):                                       # two eager warm-up iterations, the capture, one more replay
        tr.step(x, *lat)
        twin.step(x, *lat)
    assert len(tr._graphs) == 1 and len(twin._graphs) == 1
    cap = next(iter(tr._graphs.values()))
    _assert_same(_weights(tr), _weights(twin))
    ck = copy.deepcopy(tr.checkpoint(1))
    x2, lat2 = _batch(seed=12)
    tr.step(x2, *lat2)                                       # the weights, and the packs, move on
    g = torch.Generator().manual_seed(13)
    xs = torch.randn(1, 16, 8, 8, generator=g).cuda()
    for _ in range(70):
        with ops.packed_filter_scope():
            ops.conv5x5_fwd(xs, (torch.randn(16, 16, 5, 5, generator=g) * 0.1).cuda(), None, 1)
    tr.load_in_place(ck)
    out = {k: v.clone() for k, v in tr.step(x, *lat).items()}
    ref = {k: v.clone() for k, v in twin.step(x, *lat).items()}
    assert len(tr._graphs) == 1 and next(iter(tr._graphs.values())) is cap           # the same capture replayed
    for k in ref:
        assert torch.equal(_bits(out[k].float()), _bits(ref[k].float())), k
    _assert_same(_weights(tr), _weights(twin))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("which", ["vae", "gan"])
def test_vae_and_gan_trainers_notice_an_inf_pixel(which, graph):
    from disentangle_mlp_amd import trainer as T
    x, lat = _batch()
    tr = T.VAETrainer(graph=graph) if which == "vae" else T.GANTrainer(graph=graph)
    assert tr.nonfinite_guard
    for _ in range(4):
        tr.step(x, lat[0])
    assert len(tr._graphs) == (1 if graph else 0) and tr.graph == graph
    assert tr.iteration == 4                                 # eager iterations and replays count alike
    # bits in a word that are not the guard's are not its business
    tr._guarded_optimizers()[0][2].nonfinite_words()[0] |= 0x10
    assert tr.check_finite() is None
    bad = x.clone()
    bad[0, 0, 0, 0] = float("inf")
    tr.step(bad, lat[0])
    assert len(tr._graphs) == (1 if graph else 0)            # graph: the poisoned step was a replay
    with pytest.raises(T.NonFiniteError) as e:
        tr.check_finite()
    assert {n.split(".")[0] for n, _ in e.value.found} == ({"model"} if which == "vae" else {"netG", "netD"})
    assert (e.value.first_iteration, e.value.last_iteration) == (4, 5)
    tr.clear_nonfinite()                                     # (the words; the weights stay poisoned)
    for _, _, opt in tr._guarded_optimizers():
        assert opt.nonfinite_words().tolist() == [0] * len(opt.nonfinite_words())
