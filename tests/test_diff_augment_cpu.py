"""CPU: the differentiable augmentation's reference (tests/_augment_refs.py) is consistent with itself -- its autograd
gradient is the explicit transpose formula the kernel implements, its integer mappings hold at every edge --, the
keyword is parsed and refused as documented, and the header, the binding and the library agree on the three entry
points.  No GPU."""
import math

import numpy as np
import pytest
import torch

import _augment_refs as R
from test_cabi_cpu import declared_symbols

NAN, INF = float("nan"), float("inf")
NEW = ("vg_diff_augment_workspace_bytes", "vg_diff_augment_fwd", "vg_diff_augment_bwd")


# ---- the reference against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", sorted(R.POLICIES))
@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 7, 5), (4, 16, 24)])
def test_autograd_of_the_reference_is_the_transpose_formula(policy, shape):
    g = torch.Generator().manual_seed(100 * policy + shape[1])
    C, H, W = shape
    u = torch.cat([torch.rand(6, 8, generator=g), R.extreme_rows(0.5)])
    B = u.shape[0]
    x = (2 * torch.rand(B, C, H, W, generator=g, dtype=torch.float64) - 1).requires_grad_()
    gy = 2 * torch.rand(B, C, H, W, generator=g, dtype=torch.float64) - 1
    for p in (1.0, 0.5):
        y = R.augment(x, u, policy, p)
        gx, = torch.autograd.grad(y, x, gy)
        want = R.transpose(gy, u, policy, p)
        assert float((gx - want).abs().max()) <= 1e-14, (policy, shape, p)
        # affine in x: A x = fwd(x) - fwd(0), and <gy, A x> = <A^T gy, x>
        ax = y.detach() - R.augment(torch.zeros_like(x), u, policy, p)
        assert abs(float((gy * ax).sum() - (want * x.detach()).sum())) <= 1e-11


def test_colour_mean_is_the_mean_of_x_plus_b():
    """Saturation keeps every pixel's channel mean: the contrast step's m is mean(x) + b, which the kernel uses."""
    g = torch.Generator().manual_seed(3)
    x = 2 * torch.rand(3, 9, 6, generator=g, dtype=torch.float64) - 1
    u = torch.rand(8, generator=g)
    b, s, c = R.factors(u)
    x1 = x + b
    xbar = x1.mean(dim=0, keepdim=True)
    x2 = (x1 - xbar) * s + xbar
    assert abs(float(x2.mean() - (x.mean() + b))) <= 1e-15


def test_closed_gate_and_p_zero_are_copies():
    g = torch.Generator().manual_seed(4)
    x = torch.rand(5, 3, 8, 8, generator=g, dtype=torch.float64)
    u = torch.rand(5, 8, generator=g)
    assert torch.equal(R.augment(x, u, 7, 0.0), x) and torch.equal(R.transpose(x, u, 7, 0.0), x)
    u[:, 7] = 0.5
    assert torch.equal(R.augment(x, u, 7, 0.5), x)                # u7 == p: closed
    u[:, 7] = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert not torch.equal(R.augment(x, u, 7, 0.5), x)


# ---- the integer mappings at their edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 5, 7, 8, 16, 24, 64])
def test_shift_mapping_at_every_edge(size):
    r = R.radius(size)
    n = 2 * r + 1
    assert r == math.floor(size / 8 + 0.5)
    assert R.shift_of(0.0, size) == -r and R.shift_of(R.ALMOST_ONE, size) == r
    seen = set()
    for u in R.edges(n):
        t = R.shift_of(u, size)
        prod = np.float32(u) * np.float32(n)                      # the ONE fp32 product the contract names
        assert t == min(int(math.floor(float(prod))), n - 1) - r and -r <= t <= r
        seen.add(t)
    assert seen == set(range(-r, r + 1))                          # every shift is reached, none beyond
    # crossing k / n moves the shift from k - 1 to k.  Above it is k; just below, the ONE fp32 product may round up to k
    # exactly (it is within half an ulp of k): then floor gives k -- what the product says is what counts, asserted above
    for k in range(1, n):
        t = np.float32(k) / np.float32(n)
        lo, hi = float(np.nextafter(t, np.float32(0))), float(np.nextafter(t, np.float32(1)))
        assert R.shift_of(hi, size) == k - r and R.shift_of(lo, size) in (k - 1 - r, k - r)
        assert R.shift_of(float(np.float32(k - 0.5) / np.float32(n)), size) == k - 1 - r


@pytest.mark.parametrize("size", [2, 5, 7, 8, 16, 24, 64])
def test_cut_mapping_at_every_edge(size):
    k, n = R.cut_size(size), R.cut_count(size)
    assert k == math.floor(size / 2 + 0.5) and n == size + 1 - k % 2
    assert {5: (3, 5), 7: (4, 8)}.get(size, (k, n)) == (k, n)    # an odd and an even cut size
    assert R.pick(0.0, n) == 0 and R.pick(R.ALMOST_ONE, n) == n - 1
    centres = set()
    for u in R.edges(n):
        o = R.pick(u, n)
        first, last = R.cut_range(u, size)
        centres.add(o)
        assert 0 <= o <= n - 1
        assert (first, last) == (max(o - k // 2, 0), min(o - k // 2 + k - 1, size - 1)) and 0 <= first <= last <= size - 1
    assert centres == set(range(n))
    for j in range(1, n):
        t = np.float32(j) / np.float32(n)
        assert R.pick(float(np.nextafter(t, np.float32(1))), n) == j          # (just below: j - 1, or j where the product rounds up)
        assert R.pick(float(np.nextafter(t, np.float32(0))), n) in (j - 1, j)
        assert R.pick(float(np.float32(j - 0.5) / np.float32(n)), n) == j - 1
    # centre 0 cuts rows 0 .. k - k // 2 - 1, centre n - 1 cuts through the last row
    assert R.cut_range(0.0, size) == (0, k - k // 2 - 1)
    assert R.cut_range(R.ALMOST_ONE, size)[1] == size - 1


def test_geometry_small_case_by_hand():
    """(3, 1, 8, 8) of the GPU test: r = 1, k = 4, n = 9."""
    assert (R.radius(8), R.cut_size(8), R.cut_count(8)) == (1, 4, 9)
    u = [0, 0, 0, 0.0, R.ALMOST_ONE, 0.5, 0.0, 0]                  # t_r = -1, t_c = +1; rows 2..5 (o = 4), cols 0..1 (o = 0)
    t_r, t_c, keep = R.geometry(u, 8, 8, 6)
    assert (t_r, t_c) == (-1, 1)
    want = torch.ones(8, 8, dtype=torch.bool)
    want[0, :] = False            # source row -1
    want[:, 7] = False            # source column 8
    want[2:6, 0:2] = False        # the cut
    assert torch.equal(keep, want)
    dropped = R.dropped_sources(u, 8, 8, 6)
    assert bool(dropped[7, :].all()) and bool(dropped[:, 0].all())          # shifted out of the frame
    assert bool(dropped[1:5, 1:3].all()) and int(dropped.sum()) == 8 + 7 + 8      # ... and under the cut (output 2..5 x 0..1)


# ---- keyword parsing -----------------------------------------------------------------------------------------------------------
def test_policy_and_probability_parsing():
    from disentangle_mlp_amd import ops
    assert ops.augment_policy("color,translation,cutout") == 7 == ops.augment_policy(" cutout , color,translation")
    assert ops.augment_policy("translation") == 2 and ops.augment_policy("cutout,color") == 5 and ops.augment_policy(6) == 6
    for bits, names in R.POLICIES.items():
        assert ops.augment_policy(names) == bits
    for bad in ("colour", "color,flip", "rotation"):
        with pytest.raises(ValueError, match="unknown policy"):
            ops.augment_policy(bad)
    for bad in ("", " , ", ","):
        with pytest.raises(ValueError, match="names no transform"):
            ops.augment_policy(bad)
    for bad in (0, 8, -1):
        with pytest.raises(ValueError, match="1..7"):
            ops.augment_policy(bad)
    for bad in (None, 1.0, ["color"], True):
        with pytest.raises(TypeError, match="policy"):
            ops.augment_policy(bad)
    assert ops.augment_probability(0) == 0.0 and ops.augment_probability(1) == 1.0 and ops.augment_probability(0.25) == 0.25
    for bad in (-0.01, 1.01, NAN, INF, -INF):
        with pytest.raises(ValueError, match=r"p must be in \[0, 1\]"):
            ops.augment_probability(bad)
    with pytest.raises(TypeError, match="p must be a number"):
        ops.augment_probability("half")


def test_trainer_keyword():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="VAETrainer has no discriminator: diff_augment does not apply"):
        T.VAETrainer(device="cpu", diff_augment="color")
    for cls, sets in ((T.BetaVAEGANTrainer, 4), (T.GANTrainer, 3)):
        for bad in ("colour", "", ("color,flip", 1.0)):
            with pytest.raises(ValueError, match="diff_augment"):
                cls(device="cpu", diff_augment=bad)
        for bad in (("color", -0.1), ("color", 1.5), ("color", NAN), ("color", INF)):
            with pytest.raises(ValueError, match=r"p must be in \[0, 1\]"):
                cls(device="cpu", diff_augment=bad)
        for bad in (7, ("color",), ("color", 1.0, 2), (7, 1.0), ("color", "often"), ("color", None)):
            with pytest.raises(TypeError, match="diff_augment"):
                cls(device="cpu", diff_augment=bad)
        plain = cls(device="cpu")
        full = cls(device="cpu", diff_augment="cutout,color, translation")
        half = cls(device="cpu", diff_augment=("translation,cutout", 0.5))
        assert plain._augment is None and not hasattr(plain, "augment_generator")
        assert full._augment == ("color,translation,cutout", 7, 1.0) and half._augment == ("translation,cutout", 6, 0.5)
        assert cls._augment_sets == sets
        # part of the capture key -- and without the keyword the key is what it was
        keys = {plain._host_state_key(), full._host_state_key(), half._host_state_key()}
        assert len(keys) == 3 and len(full._host_state_key()) == len(plain._host_state_key()) + 1
        assert cls(device="cpu", diff_augment=("color,cutout,translation", 1))._host_state_key() == full._host_state_key()
        assert set(full.checkpoint(0)) == set(plain.checkpoint(0))              # no checkpoint key
        assert full._latents == plain._latents
        assert [d.name for d in plain._drawn()] == list(plain._latents)
        assert [(d.name, d.dist) for d in full._drawn()][-1] == ("augment", "uniform")
        assert all(d.dist == "normal" for d in full._drawn()[:-1])
        u = full.draw_augment(5)
        assert u.shape == (sets, 5, 8) and u.dtype == torch.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
        with pytest.raises(TypeError, match="diff_augment"):
            plain.draw_augment(5)
        with pytest.raises(TypeError, match="augment= belongs to diff_augment, which is off"):
            plain.step(torch.zeros(2, 3, 64, 64), augment=u)
        with pytest.raises(ValueError, match="augment must be a float32 tensor of shape"):
            full._with_augment((None,) * len(full._latents), torch.zeros(sets, 4, 8), 5)


def test_streams_are_separate_and_seeded_per_rank():
    """The latents are bit for bit what they are without the option; the uniforms differ from rank to rank."""
    from disentangle_mlp_amd import trainer as T
    plain, full = T.GANTrainer(device="cpu", seed=5), T.GANTrainer(device="cpu", seed=5, diff_augment="color")
    a = plain._draw((None,), 4)
    b = full._draw((None, None), 4)
    assert len(a) == 1 and len(b) == 2 and torch.equal(a[0], b[0])
    assert torch.equal(plain._draw((None,), 4)[0], full._draw((None, None), 4)[0])       # ... and on the next iteration
    g0, g1, g0b = (T._augment_generator("cpu", 5, r) for r in (0, 1, 0))
    u0, u1, u0b = (torch.rand(3, 4, 8, generator=g) for g in (g0, g1, g0b))
    assert torch.equal(u0, u0b) and not torch.equal(u0, u1)
    assert T._augment_generator("cpu", 5, 0).initial_seed() != T._latent_generator("cpu", 5, 0).initial_seed()


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    from disentangle_mlp_amd import functional as F, ops
    x, u = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8)
    for fn in (ops.diff_augment_fwd, ops.diff_augment_bwd):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, u, 7, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.diff_augment(x, u)
    with pytest.raises(ValueError, match="unknown policy"):
        F.diff_augment(x, u, policy="flip")
    with pytest.raises(ValueError, match="p must be in"):
        F.diff_augment(x, u, p=2.0)
    assert F.diff_augment_uniforms(4, "cpu").shape == (4, 8) and F.diff_augment_uniforms(4, "cpu", sets=3).shape == (3, 4, 8)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    import ctypes
    from disentangle_mlp_amd import _lib, build
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
    raw = ctypes.CDLL(build.build(verbose=False))
    for name in NEW:
        assert getattr(raw, name) is not None
    assert _lib.load().vg_version() == _lib.ABI_VERSION == 7          # only added: the version stays


def test_host_side_validation():
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    q = lib.vg_diff_augment_workspace_bytes
    # one fp64 slot per (image, chunk of 4096 elements), rounded up to 256 bytes
    assert q(1, 3, 64, 64) == 256 and q(128, 3, 64, 64) == 128 * 3 * 8 and q(64, 3, 256, 256) == 64 * 48 * 8
    assert q(2, 3, 7, 5) == 256
    for bad in ((0, 3, 64, 64), (1, 0, 64, 64), (1, 5, 64, 64), (1, 3, 1, 64), (1, 3, 64, 1), (1, 4, 32768, 32768)):
        assert q(*bad) == 0, bad
    a = 4096                                                          # made-up, aligned addresses: every call below is refused on the host
    for fn in (lib.vg_diff_augment_fwd, lib.vg_diff_augment_bwd):
        assert fn(None, a, 2 * a, 1, 3, 64, 64, 7, 1.0, 3 * a, 256, None) == -1
        assert fn(a, None, 2 * a, 1, 3, 64, 64, 7, 1.0, 3 * a, 256, None) == -1
        assert fn(a, a, None, 1, 3, 64, 64, 7, 1.0, 3 * a, 256, None) == -1
        assert fn(None, None, None, 1, 3, 64, 64, 7, 1.0, None, 0, None) == -1
        assert fn(a, a, a, 1, 3, 64, 64, 2, 1.0, None, 0, None) == -1                   # in place
        for dims in ((0, 3, 64, 64), (1, 0, 64, 64), (1, 5, 64, 64), (1, 3, 1, 64), (1, 3, 64, 1)):
            assert fn(a, a, 2 * a, *dims, 7, 1.0, 3 * a, 1 << 20, None) == -1, dims
        for policy in (0, 8, -1):
            assert fn(a, a, 2 * a, 1, 3, 64, 64, policy, 1.0, 3 * a, 256, None) == -1
        for p in (-0.5, 1.5, NAN):
            assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, p, 3 * a, 256, None) == -1
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, 1.0, None, 0, None) == -1               # colour needs the workspace
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, 1.0, 3 * a + 4, 256, None) == -1           # ... 8-byte aligned
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, 1.0, 3 * a, 255, None) == -2               # ... and large enough
        assert fn(a, a, 2 * a, 128, 3, 64, 64, 5, 1.0, 3 * a, 128 * 3 * 8 - 1, None) == -2
