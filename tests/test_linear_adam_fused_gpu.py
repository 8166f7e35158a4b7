"""GPU: the weight gradient of a big Linear layer and its Adam step in one kernel (vg_linear_wgrad_adam, _dev).

The reference is always the pair the fused entry replaces, run in the same process on clones of the same state:
``vg_gemm_nt_f16x3`` in the weight gradient's orientation into a scratch gradient, then ``vg_adam_step_checked`` /
``vg_adam_step_dev_checked`` on it (bound word zeroed in front, as HipAdam does).  There is no tolerance: p, m, v, the
amax word, the flag word and ``g_out`` are compared as 32-bit patterns (so a NaN compares too, and -0 is not +0).

Shapes (N, K, reduction M) are the smallest at which the kernel can go wrong: one tile and one stage; ragged tiles in both
directions; a row length that is no multiple of 32 with 3, 4 and 8 stages (both tails of the three-slot register ring);
several tiles each way.  An inf is planted as DATA; nothing here faults the device."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
BAD_ARG = -1
SHAPES = [(128, 128, 32), (160, 288, 64), (256, 132, 96), (256, 132, 128), (256, 132, 256), (384, 256, 128)]
STALE_BOUND = 7.0      # what the weight's bound word holds when the fused entry is called: it must zero the word itself


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lib():
    from disentangle_mlp_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _State:
    """p, m, v of one (N, K) weight with its bound and flag words."""

    def __init__(self, N, K, seed):
        gen = torch.Generator().manual_seed(seed)
        self.p = torch.randn(N, K, generator=gen).cuda()
        self.m = torch.zeros(N, K, device="cuda")
        self.v = torch.zeros(N, K, device="cuda")
        self.amax = torch.full((1,), STALE_BOUND, device="cuda")
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def clone(self):
        c = object.__new__(_State)
        for k in ("p", "m", "v", "amax", "flag"):
            setattr(c, k, getattr(self, k).clone())
        return c

    def assert_same(self, other, what):
        for k in ("p", "m", "v", "amax", "flag"):
            assert torch.equal(_bits(getattr(self, k)), _bits(getattr(other, k))), f"{what}: {k} differs"


def _operands(N, K, M, seed, wide=True):
    """gy (M, N), x (M, K) and their bound words; ``wide``: the gradient's rows span 1e-8 .. 1e2."""
    gen = torch.Generator().manual_seed(1000 + seed)
    gy = torch.randn(M, N, generator=gen)
    if wide:
        gy = gy * torch.logspace(-8, 2, N)[None, :]
    x = torch.randn(M, K, generator=gen)
    gy, x = gy.cuda(), x.cuda()
    return gy, x, gy.abs().max().reshape(1), x.abs().max().reshape(1)


def _scalars(step):
    from disentangle_mlp_amd._lib import check
    scal = torch.zeros(2, device="cuda")
    check(_lib().vg_adam_prepare(float(step), None, 0, LR, B1, B2, scal.data_ptr(), _stream()), "vg_adam_prepare")
    return scal


def _pair(st, gy, x, ga, xa, step, dev):
    """The parent's two launches; returns the scratch gradient."""
    from disentangle_mlp_amd._lib import check
    from disentangle_mlp_amd.optim import _AdamTensor
    lib = _lib()
    (M, N), K = gy.shape, x.shape[1]
    g = torch.empty(N, K, device="cuda")
    check(lib.vg_gemm_nt_f16x3(gy.data_ptr(), x.data_ptr(), None, g.data_ptr(), N, K, M, 1, N, 1, K, ga.data_ptr(),
                               xa.data_ptr(), None, 0, _stream()), "vg_gemm_nt_f16x3")
    st.amax.zero_()
    arr = (_AdamTensor * 1)(_AdamTensor(st.p.data_ptr(), g.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), st.p.numel(),
                                        st.amax.data_ptr()))
    flags = (ctypes.c_void_p * 1)(st.flag.data_ptr())
    if dev:
        scal = _scalars(step)
        check(lib.vg_adam_step_dev_checked(arr, 1, B1, B2, EPS, scal.data_ptr(), flags, _stream()), "dev_checked")
    else:
        check(lib.vg_adam_step_checked(arr, 1, LR, B1, B2, EPS, 1.0 - B1 ** step, (1.0 - B2 ** step) ** 0.5, flags,
                                       _stream()), "checked")
    torch.cuda.synchronize()
    return g


def _fused(st, gy, x, ga, xa, step, dev, g_out=None):
    """The fused entry; returns its status."""
    lib = _lib()
    (M, N), K = gy.shape, x.shape[1]
    gp = None if g_out is None else g_out.data_ptr()
    head = (gy.data_ptr(), x.data_ptr(), M, N, K, ga.data_ptr(), xa.data_ptr(), st.p.data_ptr(), st.m.data_ptr(),
            st.v.data_ptr(), st.amax.data_ptr(), st.flag.data_ptr())
    if dev:
        scal = _scalars(step)
        rc = lib.vg_linear_wgrad_adam_dev(*head, B1, B2, EPS, scal.data_ptr(), gp, _stream())
    else:
        rc = lib.vg_linear_wgrad_adam(*head, LR, B1, B2, EPS, 1.0 - B1 ** step, (1.0 - B2 ** step) ** 0.5, gp, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("step0", [1, 1000])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_is_the_pair_bit_for_bit(shape, step0, dev):
    N, K, M = shape
    ref = _State(N, K, seed=N + K + M)
    fus = ref.clone()
    for i in range(3):                                   # three consecutive steps: m and v are not zero
        gy, x, ga, xa = _operands(N, K, M, seed=i)
        g = _pair(ref, gy, x, ga, xa, step0 + i, dev)
        g_out = torch.full((N, K), float("nan"), device="cuda")
        fus.amax.fill_(STALE_BOUND)
        assert _fused(fus, gy, x, ga, xa, step0 + i, dev, g_out) == 0
        assert torch.equal(_bits(g_out), _bits(g)), f"step {i}: g_out differs"
        fus.assert_same(ref, f"step {i}")
    assert int(ref.flag) == 0 and float(ref.amax) > 0.0


def test_gradient_is_not_stored_without_g_out():
    N, K, M = 160, 288, 64
    ref = _State(N, K, seed=5)
    fus = ref.clone()
    gy, x, ga, xa = _operands(N, K, M, seed=3)
    _pair(ref, gy, x, ga, xa, 4, False)
    assert _fused(fus, gy, x, ga, xa, 4, False) == 0
    fus.assert_same(ref, "no g_out")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_planted_inf_raises_the_same_bits(dev):
    """One inf in gy (ordinary data): the same flag bits and the same p, m, v as the pair."""
    N, K, M = 160, 288, 64
    ref = _State(N, K, seed=9)
    fus = ref.clone()
    gy, x, _, xa = _operands(N, K, M, seed=1, wide=False)
    gy[3, 5] = float("inf")
    ga = gy.abs().max().reshape(1)
    g = _pair(ref, gy, x, ga, xa, 2, dev)
    g_out = torch.zeros(N, K, device="cuda")
    assert _fused(fus, gy, x, ga, xa, 2, dev, g_out) == 0
    assert int(ref.flag) & 1, "the pair must have seen the non-finite gradient"
    assert torch.equal(_bits(g_out), _bits(g))
    fus.assert_same(ref, "planted inf")


@pytest.mark.parametrize("shape", [(128, 130, 32), (128, 128, 48), (128, 128, 512)],
                         ids=["rows-not-16B", "reduction-48", "ksplit-2"])
def test_refused_before_any_launch(shape):
    N, K, M = shape
    if M == 512:
        assert _lib().vg_gemm_nt_f16x3_workspace_bytes(N, K, M) > 0      # the reduction is split for this shape
    st = _State(N, K, seed=2)
    before = st.clone()
    gy, x, ga, xa = _operands(N, K, M, seed=0)
    for dev in (False, True):
        assert _fused(st, gy, x, ga, xa, 1, dev) == BAD_ARG
    st.assert_same(before, "refused call")


def test_unaligned_state_is_refused():
    N, K, M = 128, 128, 32
    st = _State(N, K, seed=2)
    buf = torch.zeros(N * K + 1, device="cuda")
    st.m = buf[1:].view(N, K)
    gy, x, ga, xa = _operands(N, K, M, seed=0)
    assert _fused(st, gy, x, ga, xa, 1, False) == BAD_ARG


def test_two_replays_of_the_dev_form():
    """A captured (vg_adam_prepare on the device counter, fused step) pair, replayed twice, against two eager pairs."""
    from disentangle_mlp_amd._lib import check
    N, K, M = 256, 132, 128
    lib = _lib()
    ref = _State(N, K, seed=11)
    fus = ref.clone()
    gy, x, ga, xa = _operands(N, K, M, seed=2)
    _lib()                                               # (loaded outside the capture)
    step_dev = torch.full((1,), 6.0, dtype=torch.float64, device="cuda")
    scal = torch.zeros(2, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        check(lib.vg_adam_prepare(0.0, step_dev.data_ptr(), 1, LR, B1, B2, scal.data_ptr(), _stream()), "prepare")
        check(lib.vg_linear_wgrad_adam_dev(gy.data_ptr(), x.data_ptr(), M, N, K, ga.data_ptr(), xa.data_ptr(),
                                           fus.p.data_ptr(), fus.m.data_ptr(), fus.v.data_ptr(), fus.amax.data_ptr(),
                                           fus.flag.data_ptr(), B1, B2, EPS, scal.data_ptr(), None, _stream()), "fused")
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _pair(ref, gy, x, ga, xa, 7 + i, True)
        fus.assert_same(ref, f"replay {i}")
    assert float(step_dev) == 8.0
