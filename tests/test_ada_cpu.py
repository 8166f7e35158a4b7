"""CPU: adaptive discriminator augmentation -- the NumPy restatement of the controller against
itself, and the host logic of the feature.

The first block (``test_restatement_*``) exercises tests/_ada_refs.py alone: those cases pass with or without the feature
-- they pin down the reference the GPU tests compare the kernel with.  Everything behind it needs the feature: the
keyword, the capture key, the checkpoint key, the wrappers' refusals and the new symbols of the C ABI."""
import math

import numpy as np
import pytest
import torch

import _ada_refs as A
from test_cabi_cpu import declared_symbols

NAN, INF = float("nan"), float("inf")
NEW = ("vg_diff_augment_fwd_dev", "vg_diff_augment_bwd_dev", "vg_ada_update")
F32 = np.float32


# ---- the restatement against itself (passes with or without the feature) -----------------------------------------------------
def test_restatement_clamps_at_both_ends():
    st = A.state(0.9)
    st = A.update(st, [1.0] * 8, 0.0, 0.6, 1 / 64, 1)                    # r_t = 1 > target: p = min(0.9 + 8/64, 1)
    assert st["p"] == F32(1.0) and st["rt"] == F32(1.0) and st["adjustments"] == 1
    st = A.update(st, [1.0] * 8, 0.0, 0.6, 1 / 64, 1)
    assert st["p"] == F32(1.0)
    st = A.state(0.1)
    st = A.update(st, [-1.0] * 8, 0.0, 0.6, 1 / 64, 1)                   # r_t = -1 < target: p = max(0.1 - 8/64, 0)
    assert st["p"] == F32(0.0) and st["rt"] == F32(-1.0)
    assert (st["sign_sum"], st["count"], st["calls"]) == (0, 0, 0)


def test_restatement_tie_leaves_p_unchanged():
    st = A.update(A.state(0.3), [1.0, 1.0, 1.0, -1.0], 0.0, 0.5, 1 / 64, 1)      # r_t = 2/4 == target
    assert st["rt"] == F32(0.5) and st["p"] == F32(0.3) and st["adjustments"] == 1
    # ... also where count * rate overflows: a tie never meets the step
    st = A.update(A.state(0.3), [1.0, 1.0, 1.0, -1.0], 0.0, 0.5, 3e38, 1)
    assert st["p"] == F32(0.3)


def test_restatement_nan_ties_and_signed_zeros():
    assert A.signs([NAN, NAN, 1.0], 0.0) == 1                           # a NaN adds 0 ...
    st = A.update(A.state(0.5), [NAN, NAN, 1.0, 1.0], 0.0, 0.6, 1 / 64, 1)
    assert st["rt"] == F32(0.5) and st["p"] == F32(0.5) - F32(4 / 64)     # ... and is counted: r_t = 2/4 < 0.6
    assert A.signs([0.0, -0.0], 0.0) == 0 and A.signs([0.0, -0.0], -0.0) == 0      # +-0 tie with a threshold of either sign
    assert A.signs([INF, -INF, INF], 0.5) == 1
    lo, at, hi = A.neighbours(0.5)
    assert A.signs([lo, at, hi, hi], 0.5) == 1
    lo, at, hi = A.neighbours(0.0)                                       # the smallest subnormals on both sides of 0
    assert lo < 0 < hi and A.signs([lo, at, hi, lo], 0.0) == -1


def test_restatement_ragged_count_and_intervals():
    # interval 4, batches 8, 8, 8, 5: the step is count * rate = 29 / 64, exact for the ragged last batch
    st = A.state(0.0)
    for k, n in enumerate((8, 8, 8, 5)):
        assert st["calls"] == k and st["adjustments"] == 0
        st = A.update(st, [1.0] * n, 0.0, 0.6, 1 / 64, 4)
    assert st["p"] == F32(29 / 64) and st["adjustments"] == 1 and st["calls"] == 0
    # interval 1: every call adjusts
    st = A.state(0.0)
    for k in range(3):
        st = A.update(st, [1.0] * 4, 0.0, 0.6, 1 / 64, 1)
        assert st["adjustments"] == k + 1 and st["p"] == F32((k + 1) * 4 / 64)
    # an inexact product: 7 * 0.001 is rounded once, then the sum is rounded once -- not the FMA's single rounding
    st = A.update(A.state(0.3), [1.0] * 7, 0.0, 0.6, 0.001, 1)
    assert st["p"] == F32(0.3) + F32(7.0) * F32(0.001)
    assert np.array_equal(A.words(st)[[1, 2, 3, 6, 7]], np.zeros(5, dtype=np.int32)) and A.words(st)[5] == 1


# ---- the keyword ------------------------------------------------------------------------------------------------------------
def test_keyword_parsing_and_refusals():
    from disentangle_mlp_amd import trainer as T
    assert T._parse_ada(None) is None and T._parse_ada(False) is None
    assert T._parse_ada(True) == (0.6, 1.0 / 500000.0, 4) == T._parse_ada({})
    assert T._parse_ada(dict(target=0.5, kimg=0.064, interval=2)) == (0.5, 1 / 64, 2)
    for bad in ("yes", 1, 0.6, ("color", 0.5), dict(rate=1.0), dict(target="high"), dict(interval=2.5), dict(interval=True),
                dict(kimg=None)):
        with pytest.raises(TypeError, match="ada"):
            T._parse_ada(bad)
    for bad in (dict(target=NAN), dict(target=INF), dict(target=1.0), dict(target=-1.0), dict(kimg=0), dict(kimg=-1),
                dict(kimg=NAN), dict(kimg=INF), dict(kimg=1e-320), dict(interval=0), dict(interval=-3)):
        with pytest.raises(ValueError, match="ada"):
            T._parse_ada(bad)
    with pytest.raises(TypeError, match="VAETrainer has no discriminator: ada does not apply"):
        T.VAETrainer(device="cpu", ada=True)
    for cls in (T.BetaVAEGANTrainer, T.GANTrainer):
        with pytest.raises(ValueError, match="ada adapts the probability of diff_augment"):
            cls(device="cpu", ada=True)
        with pytest.raises(ValueError, match="ada"):
            cls(device="cpu", diff_augment="color", ada=dict(kimg=0))


def test_start_value_state_and_capture_key():
    from disentangle_mlp_amd import ops, trainer as T
    for cls in (T.BetaVAEGANTrainer, T.GANTrainer):
        plain = cls(device="cpu")
        fixed = cls(device="cpu", diff_augment=("color,cutout", 0.25))
        bare = cls(device="cpu", diff_augment="color,cutout", ada=True)
        at = cls(device="cpu", diff_augment=("color,cutout", 0.25), ada=dict(interval=2, kimg=0.064))
        off = cls(device="cpu", diff_augment=("color,cutout", 0.25), ada=None)
        # off: nothing is there, and the key is exactly the fixed-p form
        for tr in (plain, fixed, off):
            assert tr.ada is None and tr._ada_state is None and tr.augment_p is None
            assert "ada_state" not in tr.checkpoint(0)
            with pytest.raises(TypeError, match="construct with ada="):
                tr.ada_report()
        assert off._host_state_key() == fixed._host_state_key()
        assert ("color,cutout", 5, 0.25) in fixed._host_state_key()
        assert not any(isinstance(k, tuple) and k and k[0] == "ada" for k in fixed._host_state_key())
        assert len(fixed._host_state_key()) == len(plain._host_state_key()) + 1
        # on: a bare policy starts at 0 (not the fixed-p default 1), a pair at its p0
        assert bare.ada == dict(target=0.6, rate=1.0 / 500000.0, interval=4) and at.ada == dict(target=0.6, rate=1 / 64, interval=2)
        assert float(bare.augment_p) == 0.0 and float(at.augment_p) == 0.25
        assert bare.augment_p.dtype == torch.float32 and bare.augment_p.shape == (1,)
        assert bare.augment_p.data_ptr() == bare._ada_state.data_ptr()                  # a view of word 0
        assert bare._ada_state.dtype == torch.int32 and bare._ada_state.shape == (8,)
        assert at.ada_report() == dict(p=0.25, sign_sum=0, count=0, calls=0, rt=0.0, adjustments=0)
        # the key: the policy and the controller's frozen arguments -- p is not in it
        key = at._host_state_key()
        assert ("color,cutout", 5) in key and ("ada", 0.6, 1 / 64, 2) in key and ("color,cutout", 5, 0.25) not in key
        assert len(key) == len(plain._host_state_key()) + 2
        other_p0 = cls(device="cpu", diff_augment=("color,cutout", 0.75), ada=dict(interval=2, kimg=0.064))
        assert other_p0._host_state_key() == key                                        # p0 is state, not a launch argument
        assert cls(device="cpu", diff_augment=("color,cutout", 0.25), ada=dict(interval=3, kimg=0.064))._host_state_key() != key
        assert bare._host_state_key() != key and fixed._host_state_key() != key
        # the draws are those of diff_augment
        assert [d.name for d in at._drawn()] == [d.name for d in fixed._drawn()]
    st = ops.ada_state("cpu", 0.5)
    assert st.tolist() == [0x3F000000, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match=r"p must be in \[0, 1\]"):
        ops.ada_state("cpu", 1.5)


def test_checkpoint_round_trip_on_the_cpu():
    from disentangle_mlp_amd import trainer as T
    words = torch.tensor(A.words(dict(p=F32(0.375), sign_sum=-5, count=24, calls=3, rt=F32(-0.25), adjustments=7)))
    kw = dict(device="cpu", diff_augment=("translation", 0.5), ada=dict(interval=4))
    a = T.BetaVAEGANTrainer(**kw)
    a._ada_state.copy_(words)
    ck = a.checkpoint(3)
    assert ck["ada_state"].device.type == "cpu" and ck["ada_state"].dtype == torch.int32
    a._ada_state.zero_()
    assert torch.equal(ck["ada_state"], words)                                          # a copy, not a view of the live words
    b = T.BetaVAEGANTrainer(**kw)
    buffer, view = b._ada_state, b.augment_p
    assert b.load(ck) == 3
    assert b._ada_state is buffer and b.augment_p is view and torch.equal(buffer, words)      # restored into the existing buffer
    assert b.ada_report() == dict(p=0.375, sign_sum=-5, count=24, calls=3, rt=-0.25, adjustments=7)
    # a checkpoint without the key loads and keeps the current state
    old = {k: v for k, v in ck.items() if k != "ada_state"}
    b._ada_state[5] = 9
    assert b.load(old) == 3 and b.ada_report()["adjustments"] == 9
    # a trainer without the keyword ignores the key
    c = T.BetaVAEGANTrainer(device="cpu", diff_augment=("translation", 0.5))
    assert c.load(ck) == 3 and c._ada_state is None
    with pytest.raises(ValueError, match="ada_state"):
        b.load(dict(ck, ada_state=torch.zeros(8)))
    # GANTrainer: the same key, the same restore
    g = T.GANTrainer(**kw)
    g._ada_state.copy_(words)
    gck = g.checkpoint(1)
    assert torch.equal(gck["ada_state"], words)
    h = T.GANTrainer(**kw)
    buffer = h._ada_state
    assert h.load(gck) == 1 and h._ada_state is buffer and torch.equal(buffer, words)
    h._ada_state[5] = 9
    assert h.load({k: v for k, v in gck.items() if k != "ada_state"}) == 1 and h.ada_report()["adjustments"] == 9


# ---- the wrappers -----------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments():
    from disentangle_mlp_amd import functional as Fn, ops
    st, d = ops.ada_state("cpu", 0.0), torch.zeros(4)
    with pytest.raises(ValueError, match="interval must be >= 1"):
        ops.ada_update(d, st, interval=0)
    with pytest.raises(ValueError, match=r"interval \* B must stay below 2\^31"):
        ops.ada_update(d, st, interval=1 << 29)
    for kw in (dict(target=NAN), dict(target=INF), dict(rate=-1e-6), dict(rate=NAN), dict(rate=INF), dict(threshold=NAN)):
        with pytest.raises(ValueError, match="ada_update"):
            ops.ada_update(d, st, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ada_update(d, st)
    for bad in (torch.zeros(8), torch.zeros(7, dtype=torch.int32), None):
        with pytest.raises(RuntimeError, match="int32 tensor of 8 words"):
            ops.ada_update(d, bad)
    assert ops.ada_read(st) == dict(p=0.0, sign_sum=0, count=0, calls=0, rt=0.0, adjustments=0)
    # p as a tensor: one fp32 word on the images' device (a CPU image is refused before that, as ever)
    x, u = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8)
    for fn in (ops.diff_augment_fwd, ops.diff_augment_bwd):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, u, 7, torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.diff_augment(x, u, p=torch.zeros(1))
    for bad in (torch.zeros(2), torch.zeros(1, dtype=torch.float64), torch.zeros(1)):
        with pytest.raises(RuntimeError, match="ONE float32 word"):
            ops._augment_word(bad, torch.device("cpu"))


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
    header = open(build.INCLUDE + "/vaegan_hip.h").read()
    assert "typedef struct vg_ada_state" in header and "must not change between a forward and its backward" in header


def test_host_side_validation():
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    a = 4096                                                          # made-up, aligned addresses: every call below is refused on the host
    for fn in (lib.vg_diff_augment_fwd_dev, lib.vg_diff_augment_bwd_dev):
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, None, 3 * a, 256, None) == -1           # no word
        assert fn(None, a, 2 * a, 1, 3, 64, 64, 7, 4 * a, 3 * a, 256, None) == -1
        assert fn(a, a, a, 1, 3, 64, 64, 2, 4 * a, None, 0, None) == -1                 # in place
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 8, 4 * a, 3 * a, 256, None) == -1
        assert fn(a, a, 2 * a, 1, 5, 64, 64, 7, 4 * a, 3 * a, 256, None) == -1
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, 4 * a, None, 0, None) == -1             # colour needs the workspace
        assert fn(a, a, 2 * a, 1, 3, 64, 64, 7, 4 * a, 3 * a, 255, None) == -2
    up = lib.vg_ada_update
    ok = dict(d=a, B=8, threshold=0.0, target=0.6, rate=1e-6, interval=4, state=2 * a)
    for change in (dict(d=None), dict(state=None), dict(state=2 * a + 2), dict(B=0), dict(B=-1), dict(interval=0),
                   dict(interval=-1), dict(target=NAN), dict(target=INF), dict(target=-INF), dict(rate=NAN), dict(rate=INF),
                   dict(rate=-1e-6), dict(threshold=NAN)):
        k = dict(ok, **change)
        assert up(k["d"], k["B"], k["threshold"], k["target"], k["rate"], k["interval"], k["state"], None) == -1, change
    assert math.isclose(1.0 / (500 * 1000), 2e-6)
